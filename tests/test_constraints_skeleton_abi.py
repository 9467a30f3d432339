"""CPU: dp_optimize_constrained_skeleton (include/dragposer_constraints.h) and dp_optimize_terms_skeleton (include/dragposer_terms.h), the
constrained and term-table optimise loops with per-frame skeletons -- headers, binding, exports, argument checks, the kernels' register
and LDS budget and the Python refusals.  No compute call is made here (the GPU side is tests/test_hip_constraints_skeleton.py)."""
import ctypes as C
import os
import re
import types

import pytest
import torch

import __graft_entry__ as G
from dragposer_amd import _lib
from test_build_quality import _kernel_notes  # (the flags __graft_entry__ compiles each unit with)
from test_terms_abi import _good_terms, _table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONS_HDR = os.path.join(ROOT, "include", "dragposer_constraints.h")
TERMS_HDR = os.path.join(ROOT, "include", "dragposer_terms.h")
SKEL_HDR = os.path.join(ROOT, "include", "dragposer_skeleton.h")
W_SKEL_BYTES = 68 * 4  # dp_cons_skel.h: W_SKEL_PAD, the [22][3] area of a wave's block padded to 16 bytes; 8 waves per workgroup
NAMES = ("dp_optimize_constrained_skeleton", "dp_optimize_terms_skeleton")


def test_headers_declare_the_skeleton_forms_and_the_library_exports_them():
    for hdr, sym, table in ((CONS_HDR, NAMES[0], _lib.CONSTRAINT_SYMBOLS), (TERMS_HDR, NAMES[1], _lib.TERM_SYMBOLS)):
        text = open(hdr).read()
        assert sym in set(re.findall(r"^int\s+(dp_\w+)\s*\(", text, flags=re.M)) and sym in table
        assert '#include "dragposer_skeleton.h"' in text
        assert sym in open(SKEL_HDR).read()  # (the skeleton header names the per-frame form)
        assert hasattr(_lib.load(), sym)
    assert "dp_cons_skel.hip" in G.HIP_SOURCES


def _args():
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    b = _lib.DpBatch(n_frames=4, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
    prm = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
    r = _lib.DpResult()
    r.z = p
    return buf, p, b, prm, r


def _own(which, p):
    """a well-formed dp_constraints / dp_terms, and what it keeps alive"""
    if which == 0:
        c = _lib.DpConstraints(w_feet_floor=1.0, w_head_hips_forward=2.0)
        c.global_pos = p
        return c, None
    arr = _table(_good_terms())
    return _lib.DpTerms(n_terms=5, terms=C.cast(arr, C.c_void_p), global_pos=p), arr


def _host_ctx(lib):
    ctx = C.c_void_p()
    assert lib.dp_debug_host_ctx(C.byref(ctx)) == _lib.DP_OK and ctx.value  # a context with no device behind it
    return ctx


@pytest.mark.parametrize("which", (0, 1))
def test_argument_errors_are_refused_before_any_device_is_touched(which):
    lib = _lib.load()
    fn = getattr(lib, NAMES[which])
    buf, p, b, prm, r = _args()
    own, keep = _own(which, p)
    good = _lib.DpSkeletonIn(offsets=p.value, stride=66)
    assert fn(None, C.byref(b), C.byref(prm), C.byref(own), C.byref(good), C.byref(r), None) == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    try:
        def call(batch=C.byref(b), params=C.byref(prm), ext=C.byref(own), sk=C.byref(good), res=C.byref(r)):
            rc = fn(ctx, batch, params, ext, sk, res, None)
            return rc, lib.dp_last_error(ctx).decode()

        # what the plain call refuses
        for kw in (dict(batch=None), dict(params=None), dict(ext=None), dict(res=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and "NULL" in msg and NAMES[which] in msg, kw
        bad_own = type(own)()
        bad_own.struct_size = 8
        rc, msg = call(ext=C.byref(bad_own))
        assert rc == _lib.DP_ERR_INVALID and "struct_size" in msg
        # the skeleton: NULL, NULL offsets, the stride, struct_size / reserved0
        rc, msg = call(sk=None)
        assert rc == _lib.DP_ERR_INVALID and "skeleton is NULL" in msg and NAMES[which] in msg
        rc, msg = call(sk=C.byref(_lib.DpSkeletonIn(stride=66)))
        assert rc == _lib.DP_ERR_INVALID and "offsets is NULL" in msg
        for stride in (1, 3, 65, 67, -66, 132):
            rc, msg = call(sk=C.byref(_lib.DpSkeletonIn(offsets=p.value, stride=stride)))
            assert rc == _lib.DP_ERR_INVALID and "stride" in msg, stride
        for size, rsv in ((0, 0), (8, 0), (C.sizeof(good) - 5, 0), (5000, 0), (C.sizeof(good), 3)):
            bad = _lib.DpSkeletonIn(offsets=p.value, stride=66)
            bad.struct_size, bad.reserved0 = size, rsv
            rc, msg = call(sk=C.byref(bad))
            assert rc == _lib.DP_ERR_INVALID and "dp_skeleton_in.struct_size" in msg, (size, rsv)
        # the order the headers state: the entry point's own struct before the skeleton's, the skeleton's before the batch
        bad_sk = _lib.DpSkeletonIn(offsets=p.value, stride=5)
        rc, msg = call(ext=C.byref(bad_own), sk=C.byref(bad_sk))
        assert rc == _lib.DP_ERR_INVALID and "dp_skeleton_in" not in msg and "struct_size" in msg
        bad_b = _lib.DpBatch(n_frames=0, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
        rc, msg = call(batch=C.byref(bad_b), sk=C.byref(bad_sk))
        assert rc == _lib.DP_ERR_INVALID and "stride" in msg
        rc, msg = call(batch=C.byref(bad_b))
        assert rc == _lib.DP_ERR_INVALID and "stride" not in msg
        # well-formed, either stride: refused only because there is no device
        for stride in (0, 66):
            rc, msg = call(sk=C.byref(_lib.DpSkeletonIn(offsets=p.value, stride=stride)))
            assert rc == _lib.DP_ERR_DEVICE and NAMES[which] in msg, (stride, rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del keep, buf


@pytest.mark.parametrize("which", (0, 1))
def test_the_test_only_library_declines(which):
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    ctx = _host_ctx(lib)
    try:
        buf, p, b, prm, r = _args()
        own, keep = _own(which, p)
        sk = _lib.DpSkeletonIn(offsets=p.value, stride=66)
        fn = getattr(lib, NAMES[which])
        fn.argtypes = getattr(_lib.load(), NAMES[which]).argtypes
        assert fn(ctx, C.byref(b), C.byref(prm), C.byref(own), C.byref(sk), C.byref(r), None) == _lib.DP_ERR_UNSUPPORTED
    finally:
        lib.dp_destroy(ctx)


def test_skeleton_kernels_keep_the_budget_and_the_plain_kernels_their_numbers(tmp_path):
    plain = _kernel_notes("dp_cons.hip", tmp_path)
    assert len(plain) == 2, list(plain)
    (_, pc), = [(k, v) for k, v in plain.items() if "dp_cons_kernel" in k]
    (_, pt), = [(k, v) for k, v in plain.items() if "dp_terms_kernel" in k]
    assert (pc["lds"], pt["lds"]) == (70832, 74288)  # dp_cons.h's two static_asserts, DESIGN.md section 13
    for n in (pc, pt):
        assert n["vspill"] == 0 and n["scratch"] == 0 and n["vgpr"] + n["agpr"] <= 256, n
    skel = _kernel_notes("dp_cons_skel.hip", tmp_path)
    assert len(skel) == 2, list(skel)
    (nc, sc), = [(k, v) for k, v in skel.items() if "dp_cons_skel_kernel" in k]
    (nt, st), = [(k, v) for k, v in skel.items() if "dp_terms_skel_kernel" in k]
    for name, n, p in ((nc, sc, pc), (nt, st, pt)):
        assert n["vspill"] == 0 and n["scratch"] == 0, (name, n)
        assert n["lds"] == p["lds"] + 8 * W_SKEL_BYTES, (name, n)  # one [22][3] area per wave, 8 waves
        assert n["lds"] <= 160 * 1024, (name, n)
        # the unified register file: 512 per SIMD lane, so at most 256 for two waves per SIMD, as the plain kernels
        assert n["vgpr"] + n["agpr"] <= 256, (name, n)


def _fake_opt():
    from dragposer_amd.optimizer import LatentOptimizer

    fake = types.SimpleNamespace(device=torch.device("cpu"))  # (no library, no context: reaching a launch would raise AttributeError)
    fake._skeleton = lambda *a: LatentOptimizer._skeleton(fake, *a)
    return fake


BAD_OFFSETS = (torch.zeros(66), torch.zeros(7, 22, 3), torch.zeros(8, 21, 3), torch.zeros(1, 8, 22, 3), torch.zeros(22, 3, dtype=torch.float64),
               torch.zeros(8, 3, 22).transpose(1, 2))


def test_optimize_constrained_and_terms_refuse_bad_offsets_before_any_launch():
    from dragposer_amd import Constraints, Terms
    from dragposer_amd.optimizer import LatentOptimizer

    fake = _fake_opt()
    a = (torch.zeros(8, 24), torch.zeros(8, 24), torch.zeros(8, 4), torch.zeros(8, 22, 3), torch.zeros(8, 22, 9), torch.zeros(8, 22, 2),
         torch.zeros(8, 22, dtype=torch.uint8))
    for bad in BAD_OFFSETS:
        with pytest.raises(ValueError, match="offsets"):
            LatentOptimizer.optimize_constrained(fake, *a, Constraints.reference(), offsets=bad)
        with pytest.raises(ValueError, match="offsets"):
            LatentOptimizer.optimize_terms(fake, *a, Terms(), offsets=bad)
    for fn, ext in ((LatentOptimizer.optimize_constrained, Constraints.reference()), (LatentOptimizer.optimize_terms, Terms())):
        with pytest.raises(TypeError):
            fn(fake, *a, ext, offsets=[[0.0] * 3] * 22)
        with pytest.raises(AttributeError):  # well-formed offsets go on to the library, which the fake does not have
            fn(fake, *a, ext, offsets=torch.zeros(8, 22, 3))

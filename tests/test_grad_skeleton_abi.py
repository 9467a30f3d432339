"""CPU: dp_forward_vjp_skeleton (include/dragposer_grad.h), the vector-Jacobian product of decode + FK with per-frame skeletons -- header,
binding, exports, argument checks, the kernel's register budget and the Python refusals.  No compute call is made here (the GPU side is
tests/test_hip_vjp_skeleton.py)."""
import ctypes as C
import os
import re
import types

import pytest
import torch

import __graft_entry__ as G
from dragposer_amd import _lib
from test_build_quality import _kernel_notes  # (the flags __graft_entry__ compiles each unit with)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "dragposer_grad.h")
SKEL_HDR = os.path.join(ROOT, "include", "dragposer_skeleton.h")


def test_header_declares_the_skeleton_vjp_and_the_library_exports_it():
    text = open(HDR).read()
    declared = set(re.findall(r"^int\s+(dp_\w+)\s*\(", text, flags=re.M))
    assert "dp_forward_vjp_skeleton" in declared and "dp_forward_vjp_skeleton" in _lib.GRAD_SYMBOLS
    assert '#include "dragposer_skeleton.h"' in text
    assert "dp_forward_vjp_skeleton" in open(SKEL_HDR).read()  # (the skeleton header names the per-frame form)
    lib = _lib.load()
    assert hasattr(lib, "dp_forward_vjp_skeleton")
    assert "dp_vjp_skel.hip" in G.HIP_SOURCES and G.EXTRA_FLAGS["dp_vjp_skel.hip"] == G.EXTRA_FLAGS["dp_vjp.hip"]


def _host_ctx(lib):
    ctx = C.c_void_p()
    assert lib.dp_debug_host_ctx(C.byref(ctx)) == _lib.DP_OK and ctx.value  # a context with no device behind it
    return ctx


def test_argument_errors_are_refused_before_any_device_is_touched():
    lib = _lib.load()
    g = _lib.DpGradIn()
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    good = _lib.DpSkeletonIn(offsets=p.value, stride=66)
    rc = lib.dp_forward_vjp_skeleton(None, 1, p, p, C.byref(good), C.byref(g), p, None, None, None, None)
    assert rc == _lib.DP_ERR_INVALID and b"ctx is NULL" in lib.dp_last_error(None)
    ctx = _host_ctx(lib)
    try:
        def call(n=4, z=p, cur=p, sk=C.byref(good), gr=C.byref(g), dz=p, doff=p):
            rc = lib.dp_forward_vjp_skeleton(ctx, n, z, cur, sk, gr, dz, p, doff, p, None)
            return rc, lib.dp_last_error(ctx).decode()

        # what dp_forward_vjp refuses
        for n in (0, -3):
            rc, msg = call(n=n)
            assert rc == _lib.DP_ERR_INVALID and "n_frames" in msg
        for kw in (dict(z=None), dict(cur=None), dict(gr=None), dict(dz=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and "NULL" in msg, kw
        for size, res in ((0, 0), (8, 0), (C.sizeof(g) - 1, 0), (5000, 0), (C.sizeof(g), 7)):
            bad = _lib.DpGradIn()
            bad.struct_size, bad.reserved0 = size, res
            rc, msg = call(gr=C.byref(bad))
            assert rc == _lib.DP_ERR_INVALID and "dp_grad_in.struct_size" in msg, (size, res)
        # what take_skeleton refuses
        rc, msg = call(sk=None)
        assert rc == _lib.DP_ERR_INVALID and "skeleton is NULL" in msg
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
        # well-formed (doffsets optional, either stride): refused only because there is no device
        for stride in (0, 66):
            for doff in (p, None):
                rc, msg = call(sk=C.byref(_lib.DpSkeletonIn(offsets=p.value, stride=stride)), doff=doff)
                assert rc == _lib.DP_ERR_DEVICE and "dp_forward_vjp_skeleton" in msg, (stride, doff, rc, msg)
    finally:
        lib.dp_destroy(ctx)


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    ctx = _host_ctx(lib)
    try:
        g = _lib.DpGradIn()
        buf = (C.c_float * 4096)()
        p = C.cast(buf, C.c_void_p)
        sk = _lib.DpSkeletonIn(offsets=p.value, stride=66)
        assert lib.dp_forward_vjp_skeleton(ctx, 4, p, p, C.byref(sk), C.byref(g), p, None, p, None, None) == _lib.DP_ERR_UNSUPPORTED
    finally:
        lib.dp_destroy(ctx)


def test_skeleton_vjp_kernel_keeps_the_budget(tmp_path):
    notes = _kernel_notes("dp_vjp_skel.hip", tmp_path)
    (name, n), = notes.items()
    assert "dp_vjp_skel_kernel" in name and "dp_vjp_kernel" not in name
    assert n["vspill"] == 0 and n["scratch"] == 0, (name, n)
    assert n["lds"] <= 64 * 1024, (name, n)
    # vgpr_count is the unified register file of the wave (architected VGPRs up to the accumulation offset, then the AGPRs): at most
    # 512 keeps one wave per SIMD, as dp_vjp_kernel
    assert n["agpr"] <= n["vgpr"] <= 512, (name, n)
    plain, = [v for k, v in _kernel_notes("dp_vjp.hip", tmp_path).items() if "dp_vjp_kernel" in k]
    assert n["lds"] == plain["lds"] + 3 * 22 * 64 * 4  # (one more lane-private column: the frame's bones)


def _fake_opt():
    from dragposer_amd.optimizer import LatentOptimizer

    fake = types.SimpleNamespace(device=torch.device("cpu"))  # (no library, no context: reaching a launch would raise AttributeError)
    fake._skeleton = lambda *a: LatentOptimizer._skeleton(fake, *a)
    return fake


def test_forward_vjp_refuses_bad_offsets_before_any_launch():
    from dragposer_amd.optimizer import LatentOptimizer

    fake = _fake_opt()
    z, cr = torch.zeros(8, 24), torch.zeros(8, 4)
    for bad in (torch.zeros(66), torch.zeros(7, 22, 3), torch.zeros(8, 21, 3), torch.zeros(1, 8, 22, 3), torch.zeros(22, 3, dtype=torch.float64),
                torch.zeros(8, 3, 22).transpose(1, 2)):
        with pytest.raises(ValueError):
            LatentOptimizer.forward_vjp(fake, z, cr, {}, offsets=bad)
    with pytest.raises(ValueError, match="doffsets"):
        LatentOptimizer.forward_vjp(fake, z, cr, {}, doffsets=True)  # (a gradient of offsets that were not passed)
    with pytest.raises(ValueError, match="doffsets"):  # (a preallocated result of the wrong shape)
        LatentOptimizer.forward_vjp(fake, z, cr, {}, offsets=torch.zeros(22, 3), out={"doffsets": torch.zeros(22, 3)})


def test_decode_fk_refuses_bad_offsets_before_any_launch():
    from dragposer_amd.autograd import decode_fk

    z, cr = torch.zeros(8, 24), torch.zeros(8, 4)
    for bad in (torch.zeros(66), torch.zeros(7, 22, 3), torch.zeros(8, 22, 2), torch.zeros(1, 8, 22, 3)):
        with pytest.raises(ValueError, match="offsets"):
            decode_fk(None, z, cr, offsets=bad)
    with pytest.raises(TypeError):
        decode_fk(None, z, cr, offsets=[[0.0] * 3] * 22)

"""CPU: dp_optimize_sequence_ar (include/dragposer_latent_ar.h), dp_optimize_sequence_holds with the pull term's target formed inside the
launch -- header, binding, exports, the order of dp_latent_ar's refusals on a context without a device, the test-only library's refusal,
what the Python layer refuses, and the kernel's register and LDS budget.  No compute call is made here (the GPU side is
tests/test_hip_latent_ar.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as G
from dragposer_amd import _lib
from test_build_quality import _kernel_notes  # (the flags __graft_entry__ compiles each unit with)
from test_holds_abi import _holds, _terms
from test_sequence_constraints_abi import _args, _host_ctx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "dragposer_latent_ar.h")
NAME = "dp_optimize_sequence_ar"
FIELDS = ("struct_size", "reserved0", "order", "coeffs", "bias", "trace")
AR_LDS = 76464 + 8 * 4 * 4 * 24  # dp_cons_ar.h: AR_LDS_BYTES = dp_cons_hold.h's + WPB waves * MAX_AR_ORDER rows * 24 floats


def test_header_declares_the_call_and_the_library_exports_it():
    text = open(HDR).read()
    assert re.findall(r"^int\s+(dp_\w+)\s*\(", text, flags=re.M) == [NAME] == list(_lib.LATENT_AR_SYMBOLS)
    assert hasattr(_lib.load(), NAME)
    assert "dp_cons_ar.hip" in G.HIP_SOURCES
    assert G.EXTRA_FLAGS.get("dp_cons_ar.hip") == G.EXTRA_FLAGS.get("dp_cons_hold.hip")
    assert G.SCHED_OVERRIDE.get("dp_cons_ar.hip", "x") == G.SCHED_OVERRIDE.get("dp_cons_hold.hip", "x")


def test_layout_and_defaults_match_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "ar.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_latent_ar.h"\nint main(void) {\n'
                   'printf("%zu %d\\n", sizeof(dp_latent_ar), DP_MAX_AR_ORDER);\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_latent_ar, {f}));\n' for f in FIELDS)
                   + 'dp_latent_ar r = DP_LATENT_AR_INIT;\n'
                   'printf("%u %u %d %d %d %d\\n", r.struct_size, r.reserved0, r.order, r.coeffs != 0, r.bias != 0, r.trace != 0);\nreturn 0; }\n')
    exe = tmp_path / "ar"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    assert [int(x) for x in lines[0].split()] == [C.sizeof(_lib.DpLatentAR), _lib.DP_MAX_AR_ORDER] == [40, 4]
    assert [int(x) for x in lines[1:7]] == [getattr(_lib.DpLatentAR, f).offset for f in FIELDS]
    r = _lib.DpLatentAR()
    assert [int(x) for x in lines[-1].split()] == [r.struct_size, 0, 0, 0, 0, 0]
    assert (r.reserved0, r.order, r.coeffs, r.bias, r.trace) == (0, 0, None, None, None)


def _ar(p, order=2, trace=None):
    return _lib.DpLatentAR(order=order, coeffs=p, bias=p, trace=trace)


def _frames(p, z_tgt=None, n_steps=3):
    return _lib.DpSeqFrames(n_steps=n_steps, tgt_pos=p, tgt_rot=p, tgt_root=None, w=p, tracked=p, z_tgt=z_tgt, z_tgt_step=0, z_tgt_seq=0)


def test_refusals_come_in_the_documented_order_before_any_device_is_touched():
    lib = _lib.load()
    fn = getattr(lib, NAME)
    buf, p, _, prm, st, adj, res = _args()
    fr = _frames(p)
    own, keep = _terms()
    hs, keep_h = _holds(p)
    ar = _ar(p)
    assert fn(None, 4, p, C.byref(fr), C.byref(prm), C.byref(own), C.byref(hs), C.byref(ar), None, C.byref(st), C.byref(adj), C.byref(res), None,
              None) == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    try:
        def call(n=4, latent=p, frames=C.byref(fr), params=C.byref(prm), ext=C.byref(own), holds=C.byref(hs), ar=C.byref(ar), sk=None,
                 state=C.byref(st), step=C.byref(adj), out=C.byref(res), extra=None):
            rc = fn(ctx, n, latent, frames, params, ext, holds, ar, sk, state, step, out, extra, None)
            return rc, lib.dp_last_error(ctx).decode()

        for kw in (dict(n=0), dict(latent=None), dict(frames=None), dict(params=None), dict(ext=None), dict(ar=None), dict(state=None), dict(out=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and "NULL" in msg and NAME in msg, kw
        # dp_optimize_sequence_holds' stages first, then dp_latent_ar's in the header's order; each names what it refuses
        bad_prm = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
        bad_prm.struct_size = 8
        bad_res = _lib.DpSeqResults(hist_scratch=p)
        bad_res.reserved0 = 7
        bad_own = _lib.DpTerms()
        bad_own.struct_size = 8
        bad_hs, k2 = _holds(p)
        bad_hs.struct_size = 12
        bad_extra = _lib.DpSeqExtra()
        bad_extra.struct_size = 12
        bad_sk = _lib.DpSkeletonIn(offsets=p.value, stride=5)
        bad_adam = _lib.DpParams(n_iter=10, lr=-1.0, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
        size_ar = _ar(p, order=0)
        size_ar.struct_size = 12
        res_ar = _ar(p, order=0)
        res_ar.reserved0 = 1
        order_ar = _lib.DpLatentAR(order=5)               # (and NULL coeffs / bias: the order is refused first)
        null_ar = _lib.DpLatentAR(order=3, coeffs=p)      # (and longer than the short state's history below)
        short_st = _lib.DpSeqState(global_pos=p, global_rot=p, latent_buf=p, disp_buf=p, heights_buf=p, history=2, n_heights=0)
        long_ar = _ar(p, order=3)
        fr_z = _frames(p, z_tgt=p)
        ar_stages = [(dict(ar=C.byref(size_ar)), "dp_latent_ar.struct_size"), (dict(ar=C.byref(res_ar)), "reserved0"),
                     (dict(ar=C.byref(order_ar)), "dp_latent_ar.order 5 outside 1..4"),
                     (dict(ar=C.byref(null_ar), state=C.byref(short_st), frames=C.byref(fr_z)), "coeffs or bias is NULL"),
                     (dict(ar=C.byref(long_ar), state=C.byref(short_st), frames=C.byref(fr_z)), "shorter than dp_latent_ar.order 3"),
                     (dict(frames=C.byref(fr_z)), "z_tgt must be NULL")]
        for kw, word in ar_stages:
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and word in msg and NAME in msg, (word, msg)
        early = [(dict(params=C.byref(bad_prm)), "dp_params.struct_size"), (dict(out=C.byref(bad_res)), "dp_seq_results.struct_size"),
                 (dict(ext=C.byref(bad_own)), "dp_terms.struct_size"), (dict(holds=C.byref(bad_hs)), "dp_holds.struct_size"),
                 (dict(extra=C.byref(bad_extra)), "dp_seq_extra.struct_size"), (dict(sk=C.byref(bad_sk)), "dp_skeleton_in.stride"),
                 (dict(frames=C.byref(_frames(p, n_steps=0))), "n_steps must be positive"), (dict(params=C.byref(bad_adam)), "Adam")]
        for kw, word in early:  # ... each before every fault of dp_latent_ar
            for kw_ar, _ in ar_stages[:3]:
                rc, msg = call(**{**kw_ar, **kw})
                assert rc == _lib.DP_ERR_INVALID and word in msg and NAME in msg, (word, msg)
        # well-formed: refused only because there is no device -- no dp_holds, none in it, no terms, every order up to the history, a trace
        no_terms = _lib.DpTerms()
        h0 = _lib.DpHolds()
        st4 = _lib.DpSeqState(global_pos=p, global_rot=p, latent_buf=p, disp_buf=p, heights_buf=p, history=4, n_heights=0)
        for kw in (dict(), dict(holds=None), dict(holds=C.byref(h0)), dict(ext=C.byref(no_terms), holds=None), dict(ar=C.byref(_ar(p, 1))),
                   dict(ar=C.byref(_ar(p, 4)), state=C.byref(st4)), dict(ar=C.byref(_ar(p, 2, trace=p))),
                   dict(sk=C.byref(_lib.DpSkeletonIn(offsets=p.value, stride=66))), dict(extra=C.byref(_lib.DpSeqExtra())), dict(step=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_DEVICE and NAME in msg, (kw, rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del keep, keep_h, buf, k2


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    ctx = _host_ctx(lib)
    try:
        buf, p, _, prm, st, adj, res = _args()
        fr = _frames(p)
        own, keep = _terms()
        ar = _ar(p)
        rc = lib.dp_optimize_sequence_ar(ctx, 4, p, C.byref(fr), C.byref(prm), C.byref(own), None, C.byref(ar), None, C.byref(st), C.byref(adj),
                                         C.byref(res), None, None)
        assert rc == _lib.DP_ERR_UNSUPPORTED and "test-only" in lib.dp_last_error(ctx).decode()
    finally:
        lib.dp_destroy(ctx)


def test_python_refuses_what_does_not_go_with_a_predictor():
    import types

    import torch

    from dragposer_amd import Constraints, LatentAR
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.optimizer import LatentOptimizer
    from dragposer_amd.temporal import HISTORY

    fake = types.SimpleNamespace(device=torch.device("cpu"))  # (no library, no context: reaching a launch would raise AttributeError)
    T, S = 3, 2

    def a(z_tgt, H=60):
        return (torch.zeros(S, 24), torch.zeros(T, S, 22, 3), torch.zeros(T, S, 22, 9), None, torch.zeros(S, 22, 2), torch.zeros(S, 22, dtype=torch.uint8),
                z_tgt, (0, 24), torch.zeros(S, 3), torch.zeros(S, 4), torch.zeros(S, H, 24), torch.zeros(S, H, 3), torch.zeros(S, H, 2), (4, 8))

    cv = LatentAR.constant_velocity()
    with pytest.raises(ValueError, match="pass z_tgt=None"):
        LatentOptimizer.optimize_sequence(fake, *a(torch.zeros(S, 24)), ar=cv)
    with pytest.raises(ValueError, match="pass terms="):
        LatentOptimizer.optimize_sequence(fake, *a(None), ar=cv, constraints=Constraints.reference())
    with pytest.raises(ValueError, match="fewer than ar.order = 2"):
        LatentOptimizer.optimize_sequence(fake, *a(None, H=1), ar=cv)
    with pytest.raises(ValueError, match="belongs to ar="):
        LatentOptimizer.optimize_sequence(fake, *a(torch.zeros(S, 24)), z_tgt_trace=torch.zeros(T, S, 24))
    assert HISTORY >= _lib.DP_MAX_AR_ORDER  # (so DragPose's "order > HISTORY" can only come from a shorter history than the shipped one)
    drag = types.SimpleNamespace(temporal=object())
    for fn in (DragPose.run_frames, DragPose.run):
        with pytest.raises(ValueError, match="two sources"):
            fn(drag, None, None, None, None, ar=cv)


def test_the_kernel_keeps_the_budget(tmp_path):
    notes = _kernel_notes("dp_cons_ar.hip", tmp_path)
    (name, n), = notes.items()
    assert "dp_terms_ar_seq_kernel" in name
    assert n["lds"] == AR_LDS == 79536 and 2 * n["lds"] <= 160 * 1024  # two workgroups fit a CU's LDS
    assert n["vspill"] == 0 and n["scratch"] == 0, n
    # the unified register file: 512 per SIMD lane, so at most 256 for two waves per SIMD, as the other sequence kernels
    assert n["vgpr"] + n["agpr"] <= 256, n

"""CPU: dp_optimize_sequence_gaps (include/dragposer_gaps.h), dp_optimize_sequence_ar for trackers that drop out and come back -- header,
binding, exports, the order of dp_gaps' refusals on a context without a device (with `ar` given and NULL), the test-only library's refusal,
what the Python layer refuses, and both kernels' register and LDS budget.  No compute call is made here (the GPU side is
tests/test_hip_gaps.py)."""
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
from test_latent_ar_abi import AR_LDS, _ar, _frames
from test_sequence_constraints_abi import _args, _host_ctx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "dragposer_gaps.h")
NAME = "dp_optimize_sequence_gaps"
FIELDS = ("struct_size", "reserved0", "max_hold", "decay", "state", "present", "trace")
HOLD_LDS = 76464  # dp_cons_hold.h: HD_LDS_BYTES


def test_header_declares_the_call_and_the_library_exports_it():
    text = open(HDR).read()
    assert re.findall(r"^int\s+(dp_\w+)\s*\(", text, flags=re.M) == [NAME] == list(_lib.GAP_SYMBOLS)
    assert hasattr(_lib.load(), NAME)
    assert "dp_cons_gap.hip" in G.HIP_SOURCES
    assert G.EXTRA_FLAGS.get("dp_cons_gap.hip") == G.EXTRA_FLAGS.get("dp_cons_ar.hip")
    assert G.SCHED_OVERRIDE.get("dp_cons_gap.hip", "x") == G.SCHED_OVERRIDE.get("dp_cons_ar.hip", "x")
    for name, value in (("DP_STATUS_TRACKER_HELD", 16), ("DP_STATUS_TRACKER_LOST", 32), ("DP_STATUS_NO_TRACKER", 64)):
        assert re.search(rf"#define {name} {value}\b", text) and getattr(_lib, name) == value
    base = open(os.path.join(ROOT, "include", "dragposer.h")).read()  # the bits are new: none collides with dragposer.h's
    assert sorted(int(v) for v in re.findall(r"#define DP_STATUS_\w+ (\d+)", base)) == [1, 2, 4, 8]


def test_layout_and_defaults_match_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "gaps.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_gaps.h"\nint main(void) {\n'
                   'printf("%zu %d %d\\n", sizeof(dp_gaps), DP_GAP_STATE_FLOATS, DP_GAP_MAX_HOLD);\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_gaps, {f}));\n' for f in FIELDS)
                   + 'dp_gaps g = DP_GAPS_INIT;\n'
                   'printf("%u %u %d %g %d %d %d\\n", g.struct_size, g.reserved0, g.max_hold, g.decay, g.state != 0, g.present != 0, g.trace != 0);\n'
                   'return 0; }\n')
    exe = tmp_path / "gaps"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    assert [int(x) for x in lines[0].split()] == [C.sizeof(_lib.DpGaps), _lib.DP_GAP_STATE_FLOATS, _lib.DP_GAP_MAX_HOLD] == [40, 16, 65535]
    assert [int(x) for x in lines[1:8]] == [getattr(_lib.DpGaps, f).offset for f in FIELDS]
    g = _lib.DpGaps()
    assert lines[-1].split() == [str(g.struct_size), "0", "0", "1", "0", "0", "0"]
    assert (g.reserved0, g.max_hold, g.state, g.present, g.trace) == (0, 0, None, None, None)


def _gaps(p, max_hold=3, decay=0.7, state=True, present=None, trace=None):
    return _lib.DpGaps(max_hold=max_hold, decay=decay, state=p if state else None, present=present, trace=trace)


@pytest.mark.parametrize("with_ar", (True, False))
def test_refusals_come_in_the_documented_order_before_any_device_is_touched(with_ar):
    lib = _lib.load()
    fn = getattr(lib, NAME)
    buf, p, _, prm, st, adj, res = _args()
    fr = _frames(p, z_tgt=None if with_ar else p)
    own, keep = _terms()
    hs, keep_h = _holds(p)
    ar = _ar(p)
    ar_ref = C.byref(ar) if with_ar else None
    gs = _gaps(p)
    assert fn(None, 4, p, C.byref(fr), C.byref(prm), C.byref(own), C.byref(hs), ar_ref, C.byref(gs), None, C.byref(st), C.byref(adj), C.byref(res),
              None, None) == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    try:
        def call(n=4, latent=p, frames=C.byref(fr), params=C.byref(prm), ext=C.byref(own), holds=C.byref(hs), ar=ar_ref, gaps=C.byref(gs), sk=None,
                 state=C.byref(st), step=C.byref(adj), out=C.byref(res), extra=None):
            rc = fn(ctx, n, latent, frames, params, ext, holds, ar, gaps, sk, state, step, out, extra, None)
            return rc, lib.dp_last_error(ctx).decode()

        for kw in (dict(n=0), dict(latent=None), dict(frames=None), dict(params=None), dict(ext=None), dict(gaps=None), dict(state=None), dict(out=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and "NULL" in msg and NAME in msg, kw
        # dp_gaps' own stages in the header's order: each names what it refuses, with every later stage's fault present as well
        size_g = _gaps(p, max_hold=-1, decay=0.0, state=False)
        size_g.struct_size = 16
        res_g = _gaps(p, max_hold=-1, decay=0.0, state=False)
        res_g.reserved0 = 1
        gap_stages = [(size_g, "dp_gaps.struct_size"), (res_g, "reserved0"),
                      (_gaps(p, max_hold=-1, decay=0.0, state=False), "dp_gaps.max_hold -1 outside 0..65535"),
                      (_gaps(p, max_hold=65536, decay=2.0, state=False), "dp_gaps.max_hold 65536 outside 0..65535"),
                      (_gaps(p, decay=0.0, state=False), "dp_gaps.decay"), (_gaps(p, decay=1.0000001, state=False), "dp_gaps.decay"),
                      (_gaps(p, decay=float("nan"), state=False), "dp_gaps.decay"), (_gaps(p, decay=float("inf"), state=False), "dp_gaps.decay"),
                      (_gaps(p, decay=-0.5, state=False), "dp_gaps.decay"), (_gaps(p, state=False), "dp_gaps.state is NULL")]
        for g, word in gap_stages:
            rc, msg = call(gaps=C.byref(g))
            assert rc == _lib.DP_ERR_INVALID and word in msg and NAME in msg, (word, msg)
        # every earlier stage before each of dp_gaps' own
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
        early = [(dict(params=C.byref(bad_prm)), "dp_params.struct_size"), (dict(out=C.byref(bad_res)), "dp_seq_results.struct_size"),
                 (dict(ext=C.byref(bad_own)), "dp_terms.struct_size"), (dict(holds=C.byref(bad_hs)), "dp_holds.struct_size"),
                 (dict(extra=C.byref(bad_extra)), "dp_seq_extra.struct_size"), (dict(sk=C.byref(bad_sk)), "dp_skeleton_in.stride"),
                 (dict(frames=C.byref(_frames(p, z_tgt=fr.z_tgt, n_steps=0))), "n_steps must be positive"), (dict(params=C.byref(bad_adam)), "Adam")]
        if with_ar:  # dp_latent_ar's own, which dp_optimize_sequence_ar checks last
            size_ar = _ar(p, order=0)
            size_ar.struct_size = 12
            early += [(dict(ar=C.byref(size_ar)), "dp_latent_ar.struct_size"), (dict(ar=C.byref(_lib.DpLatentAR(order=5))), "dp_latent_ar.order 5"),
                      (dict(ar=C.byref(_lib.DpLatentAR(order=2, coeffs=p))), "coeffs or bias is NULL"),
                      (dict(frames=C.byref(_frames(p, z_tgt=p))), "z_tgt must be NULL")]
        else:        # without a predictor the targets are frames->z_tgt, required as in dp_optimize_sequence_holds
            early += [(dict(frames=C.byref(_frames(p, z_tgt=None))), "NULL input array")]
        for kw, word in early:
            for g, _ in gap_stages[:3] + gap_stages[4:5] + gap_stages[-1:]:
                rc, msg = call(**{"gaps": C.byref(g), **kw})
                assert rc == _lib.DP_ERR_INVALID and word in msg and NAME in msg, (word, msg)
        # well-formed: refused only because there is no device
        no_terms = _lib.DpTerms()
        for kw in (dict(), dict(holds=None), dict(holds=C.byref(_lib.DpHolds())), dict(ext=C.byref(no_terms), holds=None),
                   dict(gaps=C.byref(_gaps(p, max_hold=0, decay=1.0))), dict(gaps=C.byref(_gaps(p, max_hold=65535, decay=1e-30))),
                   dict(gaps=C.byref(_gaps(p, present=p, trace=p))), dict(sk=C.byref(_lib.DpSkeletonIn(offsets=p.value, stride=66))),
                   dict(extra=C.byref(_lib.DpSeqExtra())), dict(step=None)):
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
        own, keep = _terms()
        ar, gs = _ar(p), _gaps(p)
        for fr, ar_ref in ((_frames(p), C.byref(ar)), (_frames(p, z_tgt=p), None)):
            rc = lib.dp_optimize_sequence_gaps(ctx, 4, p, C.byref(fr), C.byref(prm), C.byref(own), None, ar_ref, C.byref(gs), None, C.byref(st),
                                               C.byref(adj), C.byref(res), None, None)
            assert rc == _lib.DP_ERR_UNSUPPORTED and "test-only" in lib.dp_last_error(ctx).decode()
    finally:
        lib.dp_destroy(ctx)


def test_python_refuses_what_does_not_go_with_gaps():
    import types

    import torch

    from dragposer_amd import Constraints, Gaps
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.optimizer import LatentOptimizer

    fake = types.SimpleNamespace(device=torch.device("cpu"))  # (no library, no context: reaching a launch would raise AttributeError)
    T, S = 3, 2
    a = (torch.zeros(S, 24), torch.zeros(T, S, 22, 3), torch.zeros(T, S, 22, 9), None, torch.zeros(S, 22, 2), torch.zeros(S, 22, dtype=torch.uint8),
         torch.zeros(S, 24), (0, 24), torch.zeros(S, 3), torch.zeros(S, 4), torch.zeros(S, 60, 24), torch.zeros(S, 60, 3), torch.zeros(S, 60, 2), (4, 8))
    state = torch.zeros(S, 22, 16)
    for kw in (dict(gap_state=state), dict(present=torch.ones(T, S, 22, dtype=torch.uint8)), dict(gap_trace=True)):
        with pytest.raises(ValueError, match="belong to gaps="):
            LatentOptimizer.optimize_sequence(fake, *a, **kw)
    with pytest.raises(ValueError, match="needs gap_state"):
        LatentOptimizer.optimize_sequence(fake, *a, gaps=Gaps(3, 0.7))
    with pytest.raises(ValueError, match="pass terms="):
        LatentOptimizer.optimize_sequence(fake, *a, gaps=Gaps(3, 0.7), gap_state=state, constraints=Constraints.reference())
    with pytest.raises(ValueError, match="Gaps: max_hold"):
        LatentOptimizer.optimize_sequence(fake, *a, gaps=Gaps(-1, 0.7), gap_state=state)
    with pytest.raises(ValueError, match="Gaps: decay"):
        LatentOptimizer.optimize_sequence(fake, *a, gaps=Gaps(3, 0.0), gap_state=state)
    drag = types.SimpleNamespace(temporal=None)
    for fn in (DragPose.run_frames, DragPose.run):
        with pytest.raises(ValueError, match="present belongs to gaps="):
            fn(drag, None, None, None, None, present=torch.ones(T, S, 6))
        with pytest.raises(ValueError, match="Gaps: decay"):
            fn(drag, None, None, None, None, gaps=Gaps(3, 2.0))


def test_both_kernels_keep_the_budget(tmp_path):
    """Neither kernel takes LDS beyond AR_LDS_BYTES: the one with the predictor has dp_terms_ar_seq_kernel's, exactly; the one without has no
    history area (DP_CONS_AR is off) and so dp_terms_hold_seq_kernel's, exactly, which is less.  No spill, no scratch, and at most 256
    registers, for two waves per SIMD as the other sequence kernels."""
    notes = _kernel_notes("dp_cons_gap.hip", tmp_path)
    assert len(notes) == 2
    by = {("ar" if "dp_terms_gap_ar_seq_kernel" in k else "plain"): v for k, v in notes.items()}
    assert any("dp_terms_gap_seq_kernel" in k for k in notes) and set(by) == {"ar", "plain"}
    assert by["ar"]["lds"] == AR_LDS == 79536 and by["plain"]["lds"] == HOLD_LDS <= AR_LDS
    for n in by.values():
        assert 2 * n["lds"] <= 160 * 1024  # two workgroups fit a CU's LDS
        assert n["vspill"] == 0 and n["scratch"] == 0, n
        assert n["vgpr"] + n["agpr"] <= 256, n

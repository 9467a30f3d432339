"""CPU: dp_optimize_sequence_tethers (include/dragposer_tethers.h), dp_optimize_sequence_gaps with joints tied to their own recent path --
header, binding, exports, the order of dp_tethers' refusals on a context without a device (with `ar` given and NULL), the test-only
library's refusal, what the Python layer refuses, and both kernels' register and LDS budget.  No compute call is made here (the GPU side
is tests/test_hip_tethers.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as G
from dragposer_amd import _lib
from test_build_quality import _kernel_notes  # (the flags __graft_entry__ compiles each unit with)
from test_gaps_abi import _gaps
from test_holds_abi import _holds
from test_latent_ar_abi import AR_LDS, _ar, _frames
from test_sequence_constraints_abi import _args, _host_ctx
from test_terms_abi import _good_terms, _table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "dragposer_tethers.h")
NAME = "dp_optimize_sequence_tethers"
TETHER_FIELDS = ("term", "alpha")
TETHERS_FIELDS = ("struct_size", "reserved0", "n_tethers", "tethers", "state", "trace")
HOLD_LDS = 76464            # dp_cons_hold.h: HD_LDS_BYTES
WPREV_LDS = 8 * 4 * 4 * 4   # dp_cons_tether.h: WPB waves * MAX_TETHERS * 4 floats of last world positions
HELD, KNEE, ELBOW = 2, 5, 6  # _rows(): the point-DISTANCE term test_holds_abi's hold refers to, and two more for tethers


def _rows():
    D = _lib.DP_TERM_DISTANCE
    return _good_terms() + [dict(type=D, joint_a=6, joint_b=-1, weight=0.6, p1=0.02), dict(type=D, joint_a=19, joint_b=-1, weight=0.8)]


def _terms(rows=None):
    rows = rows or _rows()
    arr = _table(rows)
    return _lib.DpTerms(n_terms=len(rows), terms=C.cast(arr, C.c_void_p)), arr


def _tethers(p, rows=((KNEE, 0.0), (ELBOW, 1.0)), state=True, trace=None):
    arr = (_lib.DpTether * max(1, len(rows)))(*[_lib.DpTether(term=t, alpha=a) for t, a in rows])
    return _lib.DpTethers(n_tethers=len(rows), tethers=C.cast(arr, C.c_void_p), state=p if state else None, trace=trace), arr


def test_header_declares_the_call_and_the_library_exports_it():
    text = open(HDR).read()
    assert re.findall(r"^int\s+(dp_\w+)\s*\(", text, flags=re.M) == [NAME] == list(_lib.TETHER_SYMBOLS)
    assert hasattr(_lib.load(), NAME)
    assert "dp_cons_tether.hip" in G.HIP_SOURCES
    assert G.EXTRA_FLAGS.get("dp_cons_tether.hip") == G.EXTRA_FLAGS.get("dp_cons_gap.hip")
    assert G.SCHED_OVERRIDE.get("dp_cons_tether.hip", "x") == G.SCHED_OVERRIDE.get("dp_cons_gap.hip", "x")
    assert re.search(r"#define DP_MAX_TETHERS 4\b", text) and _lib.DP_MAX_TETHERS == 4
    assert re.search(r"#define DP_TETHER_STATE_FLOATS 8\b", text) and _lib.DP_TETHER_STATE_FLOATS == 8


def test_header_states_the_equivalence_and_the_refusals():
    text = " ".join(re.sub(r"^ \* ?", "", open(HDR).read(), flags=re.M).split())  # (the comment's text, its line breaks and margin taken out)
    for phrase in ("Equivalence. The launch returns the bits of this per-frame composition: dp_optimize_terms[_skeleton]",
                   "then dp_sequence_advance, then the latent copy, then the update above",
                   "With n_tethers == 0 the call returns the bits of dp_optimize_sequence_gaps",
                   "W = gpn + (P_a - P_0)", "point = have != 0 ? W + alpha * (W - Wprev) : W", "|W_c| <= DP_INPUT_LIMIT",
                   "A step refused as bad state, which skips the loop, does not touch the state",
                   "live = 0 switches the term off for the first step", "neither read nor written",
                   "Refusals: dp_optimize_sequence_gaps' in its order", "then dp_tethers, after dp_gaps", "a bad struct_size or a non-zero reserved0",
                   "n_tethers outside 0..DP_MAX_TETHERS", "a NULL tethers or a NULL state with n_tethers > 0", "a term index out of range",
                   "a term another tether or a hold refers to", "an alpha that is not finite or outside [0, 1]",
                   "DP_ERR_UNSUPPORTED from a library built without the kernel",
                   "Not covered: dp_live_step and the plug-in, dp_optimize_sequence_constrained, the dp_w4 / dp_w16 kernels, joint-to-joint terms, "
                   "gradients through the tether"):
        assert phrase in text, phrase


def test_layouts_and_defaults_match_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "tethers.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_tethers.h"\nint main(void) {\n'
                   'printf("%zu %zu %d %d\\n", sizeof(dp_tether), sizeof(dp_tethers), DP_MAX_TETHERS, DP_TETHER_STATE_FLOATS);\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_tether, {f}));\n' for f in TETHER_FIELDS)
                   + "".join(f'printf("%zu\\n", offsetof(dp_tethers, {f}));\n' for f in TETHERS_FIELDS)
                   + 'dp_tethers t = DP_TETHERS_INIT;\n'
                   'printf("%u %u %d %d %d %d\\n", t.struct_size, t.reserved0, t.n_tethers, t.tethers != 0, t.state != 0, t.trace != 0);\nreturn 0; }\n')
    exe = tmp_path / "tethers"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    assert [int(x) for x in lines[0].split()] == [C.sizeof(_lib.DpTether), C.sizeof(_lib.DpTethers), _lib.DP_MAX_TETHERS,
                                                  _lib.DP_TETHER_STATE_FLOATS] == [8, 40, 4, 8]
    assert [int(x) for x in lines[1:3]] == [getattr(_lib.DpTether, f).offset for f in TETHER_FIELDS]
    assert [int(x) for x in lines[3:9]] == [getattr(_lib.DpTethers, f).offset for f in TETHERS_FIELDS]
    t = _lib.DpTethers()
    assert [int(x) for x in lines[-1].split()] == [t.struct_size, 0, 0, 0, 0, 0]
    assert (t.reserved0, t.n_tethers, t.tethers, t.state, t.trace) == (0, 0, None, None, None)


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
    ts, keep_t = _tethers(p)
    assert fn(None, 4, p, C.byref(fr), C.byref(prm), C.byref(own), C.byref(hs), ar_ref, C.byref(gs), C.byref(ts), None, C.byref(st), C.byref(adj),
              C.byref(res), None, None) == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    keeps = []
    try:
        def call(n=4, latent=p, frames=C.byref(fr), params=C.byref(prm), ext=C.byref(own), holds=C.byref(hs), ar=ar_ref, gaps=C.byref(gs),
                 tethers=C.byref(ts), sk=None, state=C.byref(st), step=C.byref(adj), out=C.byref(res), extra=None):
            rc = fn(ctx, n, latent, frames, params, ext, holds, ar, gaps, tethers, sk, state, step, out, extra, None)
            return rc, lib.dp_last_error(ctx).decode()

        def made(*a, **k):
            t, arr = _tethers(p, *a, **k)
            keeps.append((t, arr))
            return t

        for kw in (dict(n=0), dict(latent=None), dict(frames=None), dict(params=None), dict(ext=None), dict(gaps=None), dict(tethers=None),
                   dict(state=None), dict(out=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and "NULL" in msg and "tethers" in msg and NAME in msg, kw
        # dp_tethers' own stages in the header's order: each names what it refuses, with every later stage's fault present as well
        late = ((KNEE, 2.0),)  # (an alpha out of range: the last stage)
        size_t = made(late, state=False)
        size_t.struct_size = 16
        res_t = made(late, state=False)
        res_t.reserved0 = 1
        count_lo, count_hi = made(late, state=False), made(late, state=False)
        count_lo.n_tethers, count_hi.n_tethers = -1, 5
        no_arr = made(late, state=False)
        no_arr.tethers = None
        two_rows = _rows()
        stages = [(size_t, "dp_tethers.struct_size"), (res_t, "reserved0"), (count_lo, "dp_tethers.n_tethers -1 outside 0..4"),
                  (count_hi, "dp_tethers.n_tethers 5 outside 0..4"), (no_arr, "dp_tethers.tethers is NULL"), (made(late, state=False), "dp_tethers.state is NULL"),
                  (made(((-1, 2.0),)), "tether 0: term -1 outside the table of 7"), (made(((KNEE, 0.0), (7, 2.0))), "tether 1: term 7 outside the table of 7"),
                  (made(((0, 2.0),)), "tether 0: term 0 is not a DP_TERM_DISTANCE term"), (made(((1, 2.0),)), "tether 0: term 1 has a joint_b"),
                  (made(((KNEE, 2.0), (KNEE, 2.0))), "tether 0: alpha"), (made(((KNEE, 0.5), (KNEE, 2.0))), "tether 1: term 5 is already tethered by tether 0"),
                  (made(((ELBOW, 1.0), (HELD, 2.0))), "tether 1: term 2 is held by hold 0"),
                  (made(((KNEE, -0.25),)), "tether 0: alpha"), (made(((KNEE, 0.0), (ELBOW, 1.0000001))), "tether 1: alpha"),
                  (made(((KNEE, float("nan")),)), "tether 0: alpha"), (made(((KNEE, float("inf")),)), "tether 0: alpha")]
        for t, word in stages:
            rc, msg = call(tethers=C.byref(t))
            assert rc == _lib.DP_ERR_INVALID and word in msg and NAME in msg, (word, msg)
        pf_rows = _rows()
        pf_rows[KNEE] = dict(pf_rows[KNEE], per_frame=p.value)
        pf_own, pf_keep = _terms(pf_rows)
        rc, msg = call(ext=C.byref(pf_own), tethers=C.byref(made(late)))
        assert rc == _lib.DP_ERR_INVALID and "tether 0: term 5 has a per_frame array" in msg, msg
        # every earlier stage before each of dp_tethers' own: dp_gaps' last of all
        bad_prm = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
        bad_prm.struct_size = 8
        bad_own = _lib.DpTerms()
        bad_own.struct_size = 8
        bad_hs, k2 = _holds(p)
        bad_hs.struct_size = 12
        bad_adam = _lib.DpParams(n_iter=10, lr=-1.0, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
        early = [(dict(params=C.byref(bad_prm)), "dp_params.struct_size"), (dict(ext=C.byref(bad_own)), "dp_terms.struct_size"),
                 (dict(holds=C.byref(bad_hs)), "dp_holds.struct_size"), (dict(sk=C.byref(_lib.DpSkeletonIn(offsets=p.value, stride=5))), "dp_skeleton_in.stride"),
                 (dict(frames=C.byref(_frames(p, z_tgt=fr.z_tgt, n_steps=0))), "n_steps must be positive"), (dict(params=C.byref(bad_adam)), "Adam"),
                 (dict(gaps=C.byref(_gaps(p, max_hold=-1))), "dp_gaps.max_hold"), (dict(gaps=C.byref(_gaps(p, decay=0.0))), "dp_gaps.decay"),
                 (dict(gaps=C.byref(_gaps(p, state=False))), "dp_gaps.state is NULL")]
        if with_ar:
            early += [(dict(ar=C.byref(_lib.DpLatentAR(order=5))), "dp_latent_ar.order 5"), (dict(frames=C.byref(_frames(p, z_tgt=p))), "z_tgt must be NULL")]
        else:
            early += [(dict(frames=C.byref(_frames(p, z_tgt=None))), "NULL input array")]
        for kw, word in early:
            for t, _ in stages[:3] + stages[5:7] + stages[-1:]:
                rc, msg = call(**{"tethers": C.byref(t), **kw})
                assert rc == _lib.DP_ERR_INVALID and word in msg and NAME in msg, (word, msg)
        # well-formed: refused only because there is no device
        for kw in (dict(), dict(holds=None), dict(holds=C.byref(_lib.DpHolds())), dict(tethers=C.byref(_lib.DpTethers())),
                   dict(tethers=C.byref(made(((KNEE, 0.0), (ELBOW, 1.0)), trace=p))), dict(tethers=C.byref(made(((HELD, 0.5),))), holds=None),
                   dict(tethers=C.byref(made(((KNEE, 0.25),)))), dict(sk=C.byref(_lib.DpSkeletonIn(offsets=p.value, stride=66))),
                   dict(extra=C.byref(_lib.DpSeqExtra())), dict(step=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_DEVICE and NAME in msg, (kw, rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del keep, keep_h, keep_t, buf, k2, pf_keep, two_rows


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    ctx = _host_ctx(lib)
    try:
        buf, p, _, prm, st, adj, res = _args()
        own, keep = _terms()
        ar, gs = _ar(p), _gaps(p)
        ts, keep_t = _tethers(p)
        for fr, ar_ref in ((_frames(p), C.byref(ar)), (_frames(p, z_tgt=p), None)):
            rc = lib.dp_optimize_sequence_tethers(ctx, 4, p, C.byref(fr), C.byref(prm), C.byref(own), None, ar_ref, C.byref(gs), C.byref(ts), None,
                                                  C.byref(st), C.byref(adj), C.byref(res), None, None)
            assert rc == _lib.DP_ERR_UNSUPPORTED and "test-only" in lib.dp_last_error(ctx).decode()
    finally:
        lib.dp_destroy(ctx)


def test_the_plug_in_library_carries_no_tether_unit():
    """the unit goes into libdragposer_hip.so only (include/dragposer_tethers.h, Not covered)"""
    if shutil.which("nm") is None or not os.path.exists(G.UNITY_LIB):
        pytest.skip("no nm, or the plug-in library is not built")
    syms = lambda path: subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    assert "dp_launch_terms_tether_seq" in syms(G.LIB) and "dp_launch_terms_tether_seq" not in syms(G.UNITY_LIB)
    assert "dp_launch_terms_gap_seq" in syms(G.UNITY_LIB)


def test_python_refuses_what_does_not_go_with_tethers():
    import types

    import torch

    from dragposer_amd import Constraints, Gaps, Tether, Tethers
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.optimizer import LatentOptimizer
    from dragposer_amd.terms import Term, Terms

    fake = types.SimpleNamespace(device=torch.device("cpu"))  # (no library, no context: reaching a launch would raise AttributeError)
    T, S = 3, 2
    a = (torch.zeros(S, 24), torch.zeros(T, S, 22, 3), torch.zeros(T, S, 22, 9), None, torch.zeros(S, 22, 2), torch.zeros(S, 22, dtype=torch.uint8),
         torch.zeros(S, 24), (0, 24), torch.zeros(S, 3), torch.zeros(S, 4), torch.zeros(S, 60, 24), torch.zeros(S, 60, 3), torch.zeros(S, 60, 2), (4, 8))
    table = Terms([Term.distance(6, point=(0.0, 0.0, 0.0), hi=0.02)])
    te, state, gstate = Tethers([Tether(0)]), torch.zeros(S, 1, 8), torch.zeros(S, 22, 16)
    for kw in (dict(tether_state=state), dict(tether_trace=True)):
        with pytest.raises(ValueError, match="belong to tethers="):
            LatentOptimizer.optimize_sequence(fake, *a, **kw)
    with pytest.raises(ValueError, match="pass terms="):
        LatentOptimizer.optimize_sequence(fake, *a, tethers=te, tether_state=state)
    with pytest.raises(ValueError, match="pass terms="):
        LatentOptimizer.optimize_sequence(fake, *a, tethers=te, tether_state=state, constraints=Constraints.reference())
    with pytest.raises(ValueError, match="pass gaps="):
        LatentOptimizer.optimize_sequence(fake, *a, tethers=te, tether_state=state, terms=table)
    with pytest.raises(ValueError, match="needs tether_state"):
        LatentOptimizer.optimize_sequence(fake, *a, tethers=te, terms=table, gaps=Gaps(0, 1.0), gap_state=gstate)
    with pytest.raises(ValueError, match="tether 0: alpha"):
        LatentOptimizer.optimize_sequence(fake, *a, tethers=Tethers([Tether(0, 1.5)]), tether_state=state, terms=table, gaps=Gaps(0, 1.0), gap_state=gstate)
    with pytest.raises(ValueError, match="dp_live_step"):
        LatentOptimizer.optimize_sequence(fake, a[0], a[1][:1], a[2][:1], *a[3:], tethers=te, tether_state=state, terms=table, gaps=Gaps(0, 1.0),
                                          gap_state=gstate, live=True)
    drag = types.SimpleNamespace(temporal=None, S=S, device=torch.device("cpu"), tether_state=None)
    drag._tethers = types.MethodType(DragPose._tethers, drag)
    for fn in (DragPose.run_frames, DragPose.run):
        with pytest.raises(ValueError, match="pass terms="):
            fn(drag, None, None, None, None, tethers=te)
        with pytest.raises(ValueError, match="tether 0: term 3 outside"):
            fn(drag, None, None, None, None, tethers=Tethers([Tether(3)]), terms=table)
    with pytest.raises(ValueError, match="run_frames"):
        DragPose.run(drag, None, None, None, None, tethers=te, terms=table, live=True)


def test_both_kernels_keep_the_budget(tmp_path):
    """hipcc -S with the build's flags: each kernel's LDS is its gap kernel's and the 512 bytes of last world positions, two workgroups still
    fit a CU's 160 KiB; no spill, no scratch, no accumulator registers, at most 256 registers for two waves per SIMD"""
    notes = _kernel_notes("dp_cons_tether.hip", tmp_path)
    assert len(notes) == 2
    by = {("ar" if "dp_terms_tether_ar_seq_kernel" in k else "plain"): v for k, v in notes.items()}
    assert any("dp_terms_tether_seq_kernel" in k for k in notes) and set(by) == {"ar", "plain"}
    assert by["ar"]["lds"] == AR_LDS + WPREV_LDS == 80048 and by["plain"]["lds"] == HOLD_LDS + WPREV_LDS == 76976
    for n in by.values():
        assert 2 * n["lds"] <= 160 * 1024
        assert n["vspill"] == 0 and n["scratch"] == 0 and n["agpr"] == 0, n
        assert n["vgpr"] <= 256, n

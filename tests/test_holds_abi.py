"""CPU: dp_optimize_sequence_holds (include/dragposer_holds.h), dp_optimize_sequence_terms with joints held where they touched down --
header, binding, exports, the order of the argument refusals on a context without a device, every rule of a hold with its message, the
test-only library's refusal, Hold.check / Holds.check, and the kernel's register and LDS budget.  No compute call is made here (the GPU
side is tests/test_hip_holds.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as G
from dragposer_amd import _lib
from test_build_quality import _kernel_notes  # (the flags __graft_entry__ compiles each unit with)
from test_sequence_constraints_abi import _args, _host_ctx
from test_terms_abi import _good_terms, _table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "dragposer_holds.h")
NAME = "dp_optimize_sequence_holds"
HOLD_FIELDS = ("term", "level", "contact_lo", "contact_hi")
HOLDS_FIELDS = ("struct_size", "reserved0", "n_holds", "holds", "state", "trace")
HD_LDS = 76464  # dp_cons_hold.h: HD_LDS_BYTES (dp_cons_seq.h's table layout: a hold's state lives in its term's row of the wave's block)
POINT_TERM = 2  # _good_terms(): the point-DISTANCE term on joint 8


def test_header_declares_the_call_and_the_library_exports_it():
    text = open(HDR).read()
    assert re.findall(r"^int\s+(dp_\w+)\s*\(", text, flags=re.M) == [NAME] == list(_lib.HOLD_SYMBOLS)
    assert hasattr(_lib.load(), NAME)
    assert "dp_cons_hold.hip" in G.HIP_SOURCES
    assert G.EXTRA_FLAGS.get("dp_cons_hold.hip") == G.EXTRA_FLAGS.get("dp_cons_seq.hip")
    assert G.SCHED_OVERRIDE.get("dp_cons_hold.hip", "x") == G.SCHED_OVERRIDE.get("dp_cons_seq.hip", "x")


def test_hold_layouts_and_defaults_match_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "holds.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_holds.h"\nint main(void) {\n'
                   'printf("%zu %zu %d\\n", sizeof(dp_hold), sizeof(dp_holds), DP_MAX_HOLDS);\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_hold, {f}));\n' for f in HOLD_FIELDS)
                   + "".join(f'printf("%zu\\n", offsetof(dp_holds, {f}));\n' for f in HOLDS_FIELDS)
                   + 'dp_holds h = DP_HOLDS_INIT;\n'
                   'printf("%u %u %d %d %d %d\\n", h.struct_size, h.reserved0, h.n_holds, h.holds != 0, h.state != 0, h.trace != 0);\nreturn 0; }\n')
    exe = tmp_path / "holds"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    assert [int(x) for x in lines[0].split()] == [C.sizeof(_lib.DpHold), C.sizeof(_lib.DpHolds), _lib.DP_MAX_HOLDS]
    assert [int(x) for x in lines[1:5]] == [getattr(_lib.DpHold, f).offset for f in HOLD_FIELDS]
    assert [int(x) for x in lines[5:11]] == [getattr(_lib.DpHolds, f).offset for f in HOLDS_FIELDS]
    h = _lib.DpHolds()
    assert [int(x) for x in lines[-1].split()] == [h.struct_size, 0, 0, 0, 0, 0]
    assert (h.reserved0, h.n_holds, h.holds, h.state, h.trace) == (0, 0, None, None, None)


def _holds(p, rows=((POINT_TERM, 0.0, 0.02, 0.05),)):
    arr = (_lib.DpHold * max(1, len(rows)))(*[_lib.DpHold(term=t, level=lv, contact_lo=lo, contact_hi=hi) for t, lv, lo, hi in rows])
    return _lib.DpHolds(n_holds=len(rows), holds=C.cast(arr, C.c_void_p), state=p, trace=None), arr


def _terms(rows=None):
    arr = _table(rows or _good_terms())
    return _lib.DpTerms(n_terms=len(rows or _good_terms()), terms=C.cast(arr, C.c_void_p)), arr


def test_refusals_come_in_the_documented_order_before_any_device_is_touched():
    lib = _lib.load()
    fn = getattr(lib, NAME)
    buf, p, fr, prm, st, adj, res = _args()
    own, keep = _terms()
    hs, keep_h = _holds(p)
    assert fn(None, 4, p, C.byref(fr), C.byref(prm), C.byref(own), C.byref(hs), None, C.byref(st), C.byref(adj), C.byref(res), None, None) == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    try:
        def call(n=4, latent=p, frames=C.byref(fr), params=C.byref(prm), ext=C.byref(own), holds=C.byref(hs), sk=None, state=C.byref(st),
                 step=C.byref(adj), out=C.byref(res), extra=None):
            rc = fn(ctx, n, latent, frames, params, ext, holds, sk, state, step, out, extra, None)
            return rc, lib.dp_last_error(ctx).decode()

        for kw in (dict(n=0), dict(latent=None), dict(frames=None), dict(params=None), dict(ext=None), dict(holds=None), dict(state=None),
                   dict(out=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and "NULL" in msg and NAME in msg, kw
        # one bad argument of every stage; each names its struct
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
        bad_fr = _lib.DpSeqFrames(n_steps=0, tgt_pos=p, tgt_rot=p, w=p, tracked=p, z_tgt=p, z_tgt_seq=24)
        bad_adam = _lib.DpParams(n_iter=10, lr=-1.0, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
        stages = [(dict(params=C.byref(bad_prm)), "dp_params.struct_size"), (dict(out=C.byref(bad_res)), "dp_seq_results.struct_size"),
                  (dict(ext=C.byref(bad_own)), "dp_terms.struct_size"), (dict(holds=C.byref(bad_hs)), "dp_holds.struct_size"),
                  (dict(extra=C.byref(bad_extra)), "dp_seq_extra.struct_size"), (dict(sk=C.byref(bad_sk)), "dp_skeleton_in.stride"),
                  (dict(frames=C.byref(bad_fr)), "n_steps must be positive"), (dict(params=C.byref(bad_adam)), "Adam")]
        for i, (kw, word) in enumerate(stages):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and word in msg and NAME in msg, (kw, msg)
            # ... and is reported before every later stage's fault (bad_adam is well-formed up to Adam: it stands in for `params` there)
            later = {}
            for kw2, _ in stages[i + 1:]:
                later.update(kw2)
            if "params" in kw:
                later.pop("params", None)
            rc, msg = call(**{**later, **kw})
            assert rc == _lib.DP_ERR_INVALID and word in msg, (i, msg)
        # the rest of dp_holds' own rules, each with its message
        h2, k2 = _holds(p)
        h2.reserved0 = 1
        rc, msg = call(holds=C.byref(h2))
        assert rc == _lib.DP_ERR_INVALID and "dp_holds.struct_size" in msg and "reserved0" in msg
        for n in (-1, _lib.DP_MAX_HOLDS + 1):
            h2, k2 = _holds(p)
            h2.n_holds = n
            rc, msg = call(holds=C.byref(h2))
            assert rc == _lib.DP_ERR_INVALID and "n_holds" in msg and "0..4" in msg, msg
        h2, k2 = _holds(p)
        h2.holds = None
        rc, msg = call(holds=C.byref(h2))
        assert rc == _lib.DP_ERR_INVALID and "dp_holds.holds is NULL" in msg
        h2, k2 = _holds(p)
        h2.state = None
        rc, msg = call(holds=C.byref(h2))
        assert rc == _lib.DP_ERR_INVALID and "dp_holds.state is NULL" in msg
        for term in (-1, 5):
            h2, k2 = _holds(p, ((term, 0.0, 0.0, 0.1),))
            rc, msg = call(holds=C.byref(h2))
            assert rc == _lib.DP_ERR_INVALID and "hold 0" in msg and "outside the table" in msg, msg
        for term, word in ((0, "not a DP_TERM_DISTANCE"), (3, "not a DP_TERM_DISTANCE"), (1, "joint_b")):
            h2, k2 = _holds(p, ((POINT_TERM, 0.0, 0.0, 0.1), (term, 0.0, 0.0, 0.1)))
            rc, msg = call(holds=C.byref(h2))
            assert rc == _lib.DP_ERR_INVALID and "hold 1" in msg and word in msg, msg
        rows = _good_terms()
        rows[POINT_TERM] = dict(rows[POINT_TERM], per_frame=p.value)
        o2, k3 = _terms(rows)
        rc, msg = call(ext=C.byref(o2))
        assert rc == _lib.DP_ERR_INVALID and "hold 0" in msg and "per_frame" in msg, msg
        h2, k2 = _holds(p, ((POINT_TERM, 0.0, 0.0, 0.1), (POINT_TERM, 0.0, 0.0, 0.1)))
        rc, msg = call(holds=C.byref(h2))
        assert rc == _lib.DP_ERR_INVALID and "hold 1" in msg and "already held by hold 0" in msg, msg
        nan, inf = float("nan"), float("inf")
        for lv, lo, hi, word in ((nan, 0.0, 0.1, "non-finite"), (0.0, -inf, 0.1, "non-finite"), (0.0, 0.0, inf, "non-finite"),
                                 (0.0, 0.2, 0.1, "contact_lo is above contact_hi")):
            h2, k2 = _holds(p, ((POINT_TERM, lv, lo, hi),))
            rc, msg = call(holds=C.byref(h2))
            assert rc == _lib.DP_ERR_INVALID and "hold 0" in msg and word in msg, msg
        # the table's own rules come first, dp_seq_extra's after
        o2, k3 = _terms()
        o2.n_terms = 17
        h2, k2 = _holds(p, ((9, 0.0, 0.0, 0.1),))
        rc, msg = call(ext=C.byref(o2), holds=C.byref(h2))
        assert rc == _lib.DP_ERR_INVALID and "n_terms" in msg
        e = _lib.DpSeqExtra()
        e.row_step[3] = -4
        rc, msg = call(extra=C.byref(e))
        assert rc == _lib.DP_ERR_INVALID and "row_step[3]" in msg
        # well-formed: no hold, one (lo == hi), four on two point terms' worth of table; with a trace, a skeleton and an extra: refused only
        # because there is no device
        rows = _good_terms() + [dict(type=_lib.DP_TERM_DISTANCE, joint_a=j, joint_b=-1, weight=w) for j, w in ((4, 1.0), (3, 0.0), (7, 2.0))]
        o4, k4 = _terms(rows)
        h4, k5 = _holds(p, ((POINT_TERM, 0.0, 0.0, 0.1), (5, -0.9, 0.05, 0.05), (6, 0.0, 0.0, 0.0), (7, 1.0, -1.0, 1.0)))
        h0 = _lib.DpHolds()
        ht, k6 = _holds(p)
        ht.trace = p
        for kw in (dict(), dict(holds=C.byref(h0)), dict(ext=C.byref(o4), holds=C.byref(h4)), dict(holds=C.byref(ht)),
                   dict(sk=C.byref(_lib.DpSkeletonIn(offsets=p.value, stride=66))), dict(extra=C.byref(_lib.DpSeqExtra())), dict(step=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_DEVICE and NAME in msg, (kw, rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del keep, keep_h, buf


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    ctx = _host_ctx(lib)
    try:
        buf, p, fr, prm, st, adj, res = _args()
        own, keep = _terms()
        hs, keep_h = _holds(p)
        rc = lib.dp_optimize_sequence_holds(ctx, 4, p, C.byref(fr), C.byref(prm), C.byref(own), C.byref(hs), None, C.byref(st), C.byref(adj),
                                            C.byref(res), None, None)
        assert rc == _lib.DP_ERR_UNSUPPORTED and "test-only" in lib.dp_last_error(ctx).decode()
    finally:
        lib.dp_destroy(ctx)


def test_hold_check_raises_for_what_the_abi_refuses():
    import torch

    from dragposer_amd import Hold, Holds, Term, Terms

    ts = Terms([Term.plane(4, (0.0, 1.0, 0.0)), Term.distance(3, 7, hi=0.2), Term.distance(8, point=(0.0, 0.0, 0.0), drop_up=True),
                Term.distance(4, point=(0.0, 0.0, 0.0), per_frame=torch.zeros(2, 4))])
    Holds([Hold(2, 0.02, 0.05)]).check(ts)
    Holds([]).check(ts)
    Hold(2, 0.05, 0.05, level=-0.9).check(ts)
    for hold, word in ((Hold(2, 0.06, 0.05), "contact_lo is above"), (Hold(2, float("nan"), 0.05), "non-finite"),
                       (Hold(2, 0.0, float("inf")), "non-finite"), (Hold(2, 0.0, 0.1, level=float("inf")), "non-finite"),
                       (Hold(4, 0.0, 0.1), "outside the table"), (Hold(-1, 0.0, 0.1), "outside the table"), (Hold(0, 0.0, 0.1), "not a DISTANCE"),
                       (Hold(1, 0.0, 0.1), "joint_b"), (Hold(3, 0.0, 0.1), "per_frame")):
        with pytest.raises(ValueError, match=word):
            Holds([hold]).check(ts)
    with pytest.raises(ValueError, match="already held by hold 0"):
        Holds([Hold(2, 0.0, 0.1), Hold(2, 0.0, 0.2)]).check(ts)
    with pytest.raises(ValueError, match="at most 4"):
        Holds([Hold(2, 0.0, 0.1)] * 5).check(ts)


def test_python_refuses_holds_without_a_table():
    import types

    import torch

    from dragposer_amd import Constraints, Hold, Holds, Terms
    from dragposer_amd.optimizer import LatentOptimizer

    fake = types.SimpleNamespace(device=torch.device("cpu"))  # (no library, no context: reaching a launch would raise AttributeError)
    T, S = 3, 2
    a = (torch.zeros(S, 24), torch.zeros(T, S, 22, 3), torch.zeros(T, S, 22, 9), None, torch.zeros(S, 22, 2), torch.zeros(S, 22, dtype=torch.uint8),
         torch.zeros(S, 24), (0, 24), torch.zeros(S, 3), torch.zeros(S, 4), torch.zeros(S, 60, 24), torch.zeros(S, 60, 3), torch.zeros(S, 60, 2), (4, 8))
    hs = Holds([Hold(0, 0.0, 0.1)])
    with pytest.raises(ValueError, match="pass terms="):
        LatentOptimizer.optimize_sequence(fake, *a, holds=hs, hold_state=torch.zeros(S, 1, 4))
    with pytest.raises(ValueError, match="pass terms="):
        LatentOptimizer.optimize_sequence(fake, *a, constraints=Constraints.reference(), holds=hs, hold_state=torch.zeros(S, 1, 4))
    with pytest.raises(ValueError, match="belong to holds="):
        LatentOptimizer.optimize_sequence(fake, *a, terms=Terms(), hold_state=torch.zeros(S, 1, 4))
    with pytest.raises(ValueError, match="needs hold_state"):
        LatentOptimizer.optimize_sequence(fake, *a, terms=Terms(), holds=hs)


def test_the_hold_kernel_keeps_the_budget(tmp_path):
    notes = _kernel_notes("dp_cons_hold.hip", tmp_path)
    (name, n), = notes.items()
    assert "dp_terms_hold_seq_kernel" in name
    assert n["lds"] == HD_LDS
    assert n["vspill"] == 0 and n["scratch"] == 0, n
    # the unified register file: 512 per SIMD lane, so at most 256 for two waves per SIMD, as the other sequence kernels
    assert n["vgpr"] + n["agpr"] <= 256, n

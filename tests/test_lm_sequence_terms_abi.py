"""CPU: dp_optimize_sequence_lm_terms (include/dragposer_sequence_lm_terms.h) -- the header against the binding, the refusals on a context
without a device in the header's order, what the Python layers check before a launch, and dp_lm_seq_terms_kernel's register, scratch and LDS
budget.  No compute call is made here (the GPU side is tests/test_hip_lm_sequence_terms.py)."""
import ctypes as C
import os
import re
import types

import pytest

import __graft_entry__ as G
from dragposer_amd import LM, Term, Terms, _lib
from test_build_quality import _kernel_notes
from test_host_san import ROOT
from test_lm_sequence_abi import _pieces
from test_sequence_constraints_abi import _host_ctx

HDR = os.path.join(ROOT, "include", "dragposer_sequence_lm_terms.h")
SEQ_TERMS_LDS = 125456  # dp_lm_seq_terms.h: dp_lm.h's 121 488 + the table's 1 408 + 4 waves x 256 bytes of rows + 4 waves x 4 rows x 96 bytes of history
WHO = "dp_optimize_sequence_lm_terms"


def test_header_declares_the_call_and_the_library_exports_it():
    text = open(HDR).read()
    assert re.findall(r"^int\s+(dp_\w+)\s*\(", text, flags=re.M) == [WHO] == list(_lib.LM_SEQUENCE_TERMS_SYMBOLS)
    assert hasattr(_lib.load(), WHO)
    assert "dp_lm_seq_terms.hip" in G.HIP_SOURCES
    lds = re.search(r"SEQ_TERMS_LDS_BYTES == (\d+) &&", open(os.path.join(G.CSRC, "dp_lm_seq_terms.h")).read())
    assert int(lds.group(1)) == SEQ_TERMS_LDS == 121488 + 1408 + 4 * 256 + 4 * 4 * 96
    # the four LM headers agree on what is not covered: one sentence, the same in each
    inc = lambda name: open(os.path.join(ROOT, "include", name)).read()
    flat = lambda name: " ".join(inc(name).replace("*", " ").split())
    for name in ("dragposer_lm.h", "dragposer_lm_terms.h", "dragposer_sequence_lm.h", "dragposer_sequence_lm_terms.h"):
        assert flat(name).count("Not covered: ") == 1, name
        assert ("Not covered: points (include/dragposer_points.h), holds, gaps and tethers in the LM loss, per-frame skeletons, dp_live_step and "
                "the plug-in.") in flat(name), name
    for name in ("dragposer_lm.h", "dragposer_lm_terms.h", "dragposer_sequence_lm.h"):
        assert "dragposer_sequence_lm_terms.h" in inc(name), name  # the older headers point here


def _call(lib, ctx, p, frames, state, terms, prm=None, ar=None, step=None, res=None, extra=None, tx=None, null=(), n_seq=4):
    prm = prm if prm is not None else _lib.DpLmParams()
    step = step if step is not None else _lib.DpSeqStep(adjust_joint=0, adjust_target_joint=13, adjust_weight=0.5)
    res = res if res is not None else _lib.DpSeqResults(hist_scratch=p, pose_ret=p)
    extra = extra if extra is not None else _lib.DpSeqLmExtra(mu=p)
    ts, keep = terms
    rc = lib.dp_optimize_sequence_lm_terms(ctx, n_seq, None if "latent" in null else p, None if "frames" in null else C.byref(frames),
                                           None if "params" in null else C.byref(prm), None if "terms" in null else C.byref(ts),
                                           C.byref(ar) if ar is not None else None, None if "state" in null else C.byref(state),
                                           None if "adjust" in null else C.byref(step), None if "out" in null else C.byref(res),
                                           None if "extra" in null else C.byref(extra), C.byref(tx) if tx is not None else None, None)
    del keep
    return rc, (lib.dp_last_error(ctx).decode() if ctx else lib.dp_last_error(None).decode())


def test_refusals_come_in_the_documented_order_before_any_device_is_touched():
    lib = _lib.load()
    buf, p, frames, state, sized = _pieces()
    other = (C.c_float * 16)()
    q = C.cast(other, C.c_void_p)  # a pointer that is not state->global_pos
    good = Terms([Term.plane(4, (0, 1, 0)), Term.distance(3, 7, lo=0.1, hi=0.2)] * 8)  # (16 terms)

    def table(terms=good, gp=None, lt=None, **k):
        s, keep = terms.to_struct(4, None, gp, lt)
        for key, v in k.items():
            setattr(s, key, v)
        return s, keep

    rc, msg = _call(lib, None, p, frames(), state(), table())
    assert rc == _lib.DP_ERR_INVALID and WHO + ": ctx is NULL" in msg
    ctx = _host_ctx(lib)
    try:
        prm = lambda **k: sized(_lib.DpLmParams, **k)
        res = lambda **k: sized(_lib.DpSeqResults, **dict(dict(hist_scratch=p), **k))
        ext = lambda **k: sized(_lib.DpSeqLmExtra, **k)
        lar = lambda **k: sized(_lib.DpLatentAR, **dict(dict(order=2, coeffs=p, bias=p), **k))
        sx = lambda **k: sized(_lib.DpSeqExtra, **k)
        neg = sx()
        neg.row_step[15] = -4
        no_zt = frames(z_tgt=None)
        bad_term = Terms([Term.plane(4, (0, 1, 0))])
        bad_term.terms[0].joint_a = 22
        object.__setattr__(bad_term, "check", lambda: None)
        object.__setattr__(bad_term.terms[0], "check", lambda *a, **k: None)
        rc, msg = _call(lib, ctx, p, frames(), state(), table(), prm=prm(struct_size=4), n_seq=0)
        assert rc == _lib.DP_ERR_INVALID and "n_sequences must be positive" in msg
        for null in ("latent", "frames", "params", "terms", "state", "out"):
            rc, msg = _call(lib, ctx, p, frames(), state(), table(), prm=prm(n_steps=0), null=(null,))
            assert rc == _lib.DP_ERR_INVALID and "NULL latent, frames, params, terms, state or results" in msg, msg
        # each stage names what it refuses, with a later stage's fault present as well
        stages = [  # 1. dp_optimize_sequence_lm's order up to dp_seq_lm_extra
            (dict(prm=prm(struct_size=44, n_steps=0)), "dp_lm_params.struct_size is 44"),
            (dict(prm=prm(n_steps=0), res=res(struct_size=8)), "n_steps 0 outside 1..64"),
            (dict(prm=prm(mu0=5e6), res=res(struct_size=8)), "mu0 outside [mu_min, mu_max]"),
            (dict(res=res(struct_size=8), frames=frames(n_steps=0)), "dp_seq_results.struct_size is 8"),
            (dict(frames=frames(n_steps=0), res=res(hist_scratch=None)), "n_steps must be positive"),
            (dict(res=res(hist_scratch=None), state=state(history=0)), "NULL state array / hist_scratch"),
            (dict(state=state(_h0=22), step=_lib.DpSeqStep(adjust_joint=22)), "bad height joint"),
            (dict(step=_lib.DpSeqStep(adjust_joint=22), extra=ext(struct_size=8)), "bad joint adjustment"),
            (dict(extra=ext(struct_size=40), terms=table(n_terms=17)), "dp_seq_lm_extra.struct_size is 40"),
            (dict(extra=ext(reserved0=5), terms=table(struct_size=8)), "reserved0 5"),
            # 2. dp_terms and its table
            (dict(terms=table(struct_size=8), tx=sx(struct_size=8)), "dp_terms"),
            (dict(terms=table(gp=q), tx=sx(struct_size=8)), "dp_terms.global_pos must be NULL or dp_seq_state.global_pos"),
            (dict(terms=table(lt=p, n_terms=17), tx=sx(struct_size=8)), "dp_terms.loss_terms is one row per frame; a sequence launch writes dp_seq_extra.loss_terms"),
            (dict(terms=table(n_terms=17), tx=sx(struct_size=8)), "n_terms 17 outside 0..16"),
            (dict(terms=table(up_axis=3), tx=neg), "up_axis outside 0..2"),
            (dict(terms=table(bad_term), tx=neg), "term 0: joint_a 22 outside 0..21"),
            # 3. dp_seq_extra
            (dict(tx=sx(struct_size=8), ar=lar(struct_size=8)), "dp_seq_extra"),
            (dict(tx=sx(reserved0=3), ar=lar(struct_size=8)), "reserved0 3"),
            (dict(tx=neg, ar=lar(order=0)), "dp_seq_extra.row_step[15] is negative"),
            (dict(tx=sx(joint_pos=p), ar=lar(order=0)), "dp_seq_extra.joint_pos must be NULL here; the joint positions of every step go to dp_seq_lm_extra.joint_pos"),
            (dict(tx=sx(joint_pos=p), frames=no_zt), "dp_seq_lm_extra.joint_pos"),
            # 4. the predictor
            (dict(ar=lar(struct_size=32, order=0)), "dp_latent_ar.struct_size is 32"),
            (dict(ar=lar(order=5), state=state(history=2)), "dp_latent_ar.order 5 outside 1..4"),
            (dict(ar=lar(order=3), state=state(history=2)), "shorter than dp_latent_ar.order 3"),
            (dict(ar=lar()), "frames->z_tgt must be NULL"),                  # both
            (dict(frames=no_zt), "neither a predictor nor frames->z_tgt")]  # neither
        for kw, word in stages:
            kw = dict(kw)
            rc, msg = _call(lib, ctx, p, kw.pop("frames", frames()), kw.pop("state", state()), kw.pop("terms", table()), **kw)
            assert rc == _lib.DP_ERR_INVALID and word in msg and WHO in msg, (word, msg)
        # well-formed: refused only because there is no device.  global_pos NULL or the state's, every optional struct absent or empty,
        # loss_extra ignored, an empty table, either source of the targets
        held = sx(loss_terms=p, loss_extra=p)
        held.row_step[0], held.row_step[15] = 16, 0
        for kw in (dict(), dict(terms=table(gp=p)), dict(null=("extra",)), dict(null=("adjust",)), dict(tx=sx()), dict(tx=held),
                   dict(terms=table(Terms())), dict(frames=no_zt, ar=lar()), dict(frames=no_zt, ar=lar(order=4, trace=p), tx=held)):
            kw = dict(kw)
            rc, msg = _call(lib, ctx, p, kw.pop("frames", frames()), kw.pop("state", state()), kw.pop("terms", table()), **kw)
            assert rc == _lib.DP_ERR_DEVICE and WHO in msg and "no device image" in msg, (rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del buf, other


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    lib.dp_optimize_sequence_lm_terms.argtypes = _lib.load().dp_optimize_sequence_lm_terms.argtypes
    buf, p, frames, state, sized = _pieces()
    ctx = _host_ctx(lib)
    try:
        rc, msg = _call(lib, ctx, p, frames(), state(), Terms([Term.plane(4, (0, 1, 0))]).to_struct(4, None))
        assert rc == _lib.DP_ERR_UNSUPPORTED and "test-only" in msg and WHO in msg
        rc, msg = _call(lib, ctx, p, frames(z_tgt=None), state(), Terms().to_struct(4, None))  # (its argument checks come first)
        assert rc == _lib.DP_ERR_INVALID and "neither" in msg
    finally:
        lib.dp_destroy(ctx)
    del buf


def test_python_layers_check_before_a_launch():
    import torch

    from dragposer_amd import Constraints, Hold, Holds, Points
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.optimizer import LatentOptimizer

    table = Terms([Term.distance(4, 8, hi=0.3)])
    pts = Terms([Term.distance(4, 8, hi=0.3)], points=Points([]))
    opt = types.SimpleNamespace()  # (no library: reaching the launch's preparation raises AttributeError)
    with pytest.raises(ValueError, match="optimize_sequence_lm: a table with points does not go with the LM solver .*Not covered"):
        LatentOptimizer.optimize_sequence_lm(opt, *[None] * 14, terms=pts)
    with pytest.raises(ValueError, match="optimize_sequence_lm: loss_terms is an output of terms="):
        LatentOptimizer.optimize_sequence_lm(opt, *[None] * 14, loss_terms=torch.zeros(1))
    # in DragPose the table belongs to the solver, as the predictor does: LM(terms=), validated before the predictor
    assert LM().terms is None and LM(3, terms=table).check().terms is table
    assert [f for f in LM.__dataclass_fields__][-2:] == ["terms", "predictor"]
    assert bytes(LM(5, terms=table).to_struct(2.0, 0.5)) == bytes(LM(5).to_struct(2.0, 0.5))  # (not part of the C struct)
    with pytest.raises(ValueError, match="LM: terms must be a dragposer_amd.Terms, got list"):
        LM(terms=[]).check()
    with pytest.raises(ValueError, match="LM: a table with points does not go with the LM solver"):
        LM(terms=pts).check()
    with pytest.raises(ValueError, match="steps 0 outside"):  # (everything dp_optimize_lm would refuse comes first)
        LM(steps=0, terms=pts).check()
    with pytest.raises(ValueError, match="table with points"):  # (... and the predictor last)
        LM(terms=pts, predictor="hold").check()
    drag = types.SimpleNamespace(temporal=None, S=2, device=torch.device("cpu"), _skeleton=lambda offsets: None, _holds=lambda *a: None)
    for fn, who in ((DragPose.run, "run"), (DragPose.run_frames, "run_frames")):
        with pytest.raises(ValueError, match="LM: a table with points does not go with the LM solver"):
            fn(drag, None, None, None, None, solver=LM(terms=pts))
        for name, layer in (("terms", table), ("holds", Holds([Hold(0, 0.02, 0.05)])), ("constraints", Constraints.reference())):
            with pytest.raises(ValueError, match=f"DragPose.{who}: solver= does not go with {name}="):  # every layer stays refused beside solver=
                fn(drag, None, None, None, None, solver=LM(terms=table), **{name: layer})
    with pytest.raises(AttributeError):  # the solver's table is taken: the call gets past the checks
        DragPose.run_frames(drag, torch.zeros(3, 2, 6, 3), torch.zeros(3, 2, 6, 3, 3), None, None, solver=LM(terms=table))


def test_the_kernel_keeps_its_budget(tmp_path):
    """hipcc -S with the build's flags: one kernel in the unit, no spilled vector register, no scratch, the LDS figure the header states.
    As built: 256 vector + 222 accumulator registers (478 of the unified file's 512), 264 scalar registers spilled into lanes."""
    notes = _kernel_notes("dp_lm_seq_terms.hip", tmp_path)
    assert len(notes) == 1
    (name, n), = notes.items()
    assert "dp_lm_seq_terms_kernel" in name
    assert n["vspill"] == 0 and n["scratch"] == 0, n
    assert n["lds"] == SEQ_TERMS_LDS and n["lds"] <= 160 * 1024, n
    assert n["vgpr"] <= 512 and n["agpr"] <= 256, n  # (.vgpr_count is the unified file's total, accumulator half included; one wave per SIMD)

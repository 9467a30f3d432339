"""CPU: the whole-sequence Levenberg-Marquardt call (include/dragposer_sequence_lm.h) -- the header against the C compiler and the binding, the
refusals of dp_optimize_sequence_lm on a context without a device in the header's order, the test-only library's refusal, what LM(predictor=)
and DragPose.run_frames(solver=) check, and dp_lm_seq_kernel's register and LDS budget.  No compute call is made here (the GPU side is
tests/test_hip_lm_sequence.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import pytest

import __graft_entry__ as G
from dragposer_amd import LM, LatentAR, _lib
from test_build_quality import _kernel_notes
from test_host_san import ROOT
from test_sequence_constraints_abi import _host_ctx

HDR = os.path.join(ROOT, "include", "dragposer_sequence_lm.h")
EXTRA_FIELDS = ("struct_size", "reserved0", "mu", "mu_trace", "n_accepted", "loss0", "joint_pos")
SEQ_LDS = 123024  # dp_lm_seq.h: SEQ_LDS_BYTES = dp_lm.h's 121 488 + 4 waves x 4 rows x 96 bytes of predictor history


def test_header_declares_the_call_and_the_library_exports_it():
    text = open(HDR).read()
    assert re.findall(r"^int\s+(dp_\w+)\s*\(", text, flags=re.M) == ["dp_optimize_sequence_lm"] == list(_lib.LM_SEQUENCE_SYMBOLS)
    assert hasattr(_lib.load(), "dp_optimize_sequence_lm")
    assert "dp_lm_seq.hip" in G.HIP_SOURCES
    lds = re.search(r"static_assert\(SEQ_LDS_BYTES == (\d+)", open(os.path.join(G.CSRC, "dp_lm_seq.h")).read())
    assert int(lds.group(1)) == SEQ_LDS == 121488 + 4 * 4 * 96
    assert "dragposer_sequence_lm.h" in open(os.path.join(ROOT, "include", "dragposer_lm.h")).read()  # the older header points here


def test_layout_matches_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "lmseq.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_sequence_lm.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu\\n", sizeof(dp_seq_lm_extra), sizeof(dp_lm_params), sizeof(dp_latent_ar), sizeof(dp_seq_results));\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_seq_lm_extra, {f}));\n' for f in EXTRA_FIELDS)
                   + 'dp_seq_lm_extra e = DP_SEQ_LM_EXTRA_INIT;\n'
                   'printf("%u %u %d %d %d %d %d\\n", e.struct_size, e.reserved0, e.mu != 0, e.mu_trace != 0, e.n_accepted != 0, e.loss0 != 0, e.joint_pos != 0);\n'
                   'return 0; }\n')
    exe = tmp_path / "lmseq"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    assert [int(x) for x in lines[0].split()] == [C.sizeof(_lib.DpSeqLmExtra), C.sizeof(_lib.DpLmParams), C.sizeof(_lib.DpLatentAR),
                                                  C.sizeof(_lib.DpSeqResults)] == [48, 48, 40, 64]
    assert [int(x) for x in lines[1:8]] == [getattr(_lib.DpSeqLmExtra, f).offset for f in EXTRA_FIELDS] == [0, 4, 8, 16, 24, 32, 40]
    e = _lib.DpSeqLmExtra()
    assert [int(x) for x in lines[8].split()] == [e.struct_size, 0, 0, 0, 0, 0, 0] == [48, 0, 0, 0, 0, 0, 0]
    assert (e.reserved0, e.mu, e.mu_trace, e.n_accepted, e.loss0, e.joint_pos) == (0, None, None, None, None, None)


def _pieces():
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)

    def frames(**k):
        return _lib.DpSeqFrames(**dict(dict(n_steps=5, tgt_pos=p, tgt_rot=p, tgt_root=p, w=p, tracked=p, z_tgt=p, z_tgt_step=96, z_tgt_seq=24), **k))

    def state(**k):
        s = _lib.DpSeqState(**dict(dict(global_pos=p, global_rot=p, latent_buf=p, disp_buf=p, heights_buf=p, history=4, n_heights=2), **k))
        s.height_joints[0], s.height_joints[1] = k.get("_h0", 0), 4
        return s

    def sized(cls, **k):
        s = cls()
        for key, v in k.items():
            setattr(s, key, v)
        return s

    return buf, p, frames, state, sized


def _call(lib, ctx, p, frames, state, prm=None, ar=None, step=None, res=None, extra=None, null=(), n_seq=4):
    prm = prm if prm is not None else _lib.DpLmParams()
    step = step if step is not None else _lib.DpSeqStep(adjust_joint=0, adjust_target_joint=13, adjust_weight=0.5)
    res = res if res is not None else _lib.DpSeqResults(hist_scratch=p, pose_ret=p)
    extra = extra if extra is not None else _lib.DpSeqLmExtra(mu=p)
    rc = lib.dp_optimize_sequence_lm(ctx, n_seq, None if "latent" in null else p, None if "frames" in null else C.byref(frames),
                                     None if "params" in null else C.byref(prm), C.byref(ar) if ar is not None else None,
                                     None if "state" in null else C.byref(state), None if "adjust" in null else C.byref(step),
                                     None if "out" in null else C.byref(res), None if "extra" in null else C.byref(extra), None)
    return rc, (lib.dp_last_error(ctx).decode() if ctx else lib.dp_last_error(None).decode())


def test_refusals_come_in_the_documented_order_before_any_device_is_touched():
    lib = _lib.load()
    buf, p, frames, state, sized = _pieces()
    nan = float("nan")
    rc, msg = _call(lib, None, p, frames(), state())
    assert rc == _lib.DP_ERR_INVALID and "dp_optimize_sequence_lm: ctx is NULL" in msg
    ctx = _host_ctx(lib)
    try:
        prm = lambda **k: sized(_lib.DpLmParams, **k)
        res = lambda **k: sized(_lib.DpSeqResults, **dict(dict(hist_scratch=p), **k))
        ext = lambda **k: sized(_lib.DpSeqLmExtra, **k)
        lar = lambda **k: sized(_lib.DpLatentAR, **dict(dict(order=2, coeffs=p, bias=p), **k))
        no_zt = frames(z_tgt=None)
        rc, msg = _call(lib, ctx, p, frames(), state(), prm=prm(struct_size=4), n_seq=0)
        assert rc == _lib.DP_ERR_INVALID and "n_sequences must be positive" in msg
        for null in ("latent", "frames", "params", "state", "out"):
            rc, msg = _call(lib, ctx, p, frames(), state(), prm=prm(n_steps=0), null=(null,))
            assert rc == _lib.DP_ERR_INVALID and "NULL latent, frames, params, state or results" in msg, msg
        # each stage names what it refuses, with a later stage's fault present as well
        stages = [(dict(prm=prm(struct_size=44, n_steps=0)), "dp_lm_params.struct_size is 44"),
                  (dict(prm=prm(struct_size=5000), res=res(struct_size=8)), "dp_lm_params.struct_size is 5000"),
                  (dict(prm=prm(n_steps=0, lambda_rot=nan), res=res(struct_size=8)), "n_steps 0 outside 1..64"),
                  (dict(prm=prm(n_steps=65), res=res(struct_size=8)), "n_steps 65 outside 1..64"),
                  (dict(prm=prm(lambda_tmp=-1.0, mu_down=2.0)), "lambda_rot or lambda_tmp"),
                  (dict(prm=prm(mu0=nan, mu_down=2.0)), "is not finite"),
                  (dict(prm=prm(mu_down=1.0, mu_up=1.0)), "mu_down must lie in (0, 1)"),
                  (dict(prm=prm(mu_up=1.0, mu_min=2.0, mu_max=1.0)), "mu_up must be greater than 1"),
                  (dict(prm=prm(mu_min=2.0, mu_max=1.0, mu0=5.0)), "0 < mu_min <= mu_max"),
                  (dict(prm=prm(mu0=5e6), res=res(struct_size=8)), "mu0 outside [mu_min, mu_max]"),
                  (dict(res=res(struct_size=8), frames=frames(n_steps=0)), "dp_seq_results.struct_size is 8"),
                  (dict(res=res(reserved0=2), frames=frames(n_steps=0)), "reserved0 2"),
                  (dict(frames=frames(n_steps=0), res=res(hist_scratch=None)), "n_steps must be positive"),
                  (dict(frames=frames(tgt_rot=None), res=res(hist_scratch=None)), "NULL input array"),
                  (dict(frames=frames(tracked=None), state=state(history=0)), "NULL input array"),
                  (dict(res=res(hist_scratch=None), state=state(history=0)), "NULL state array / hist_scratch"),
                  (dict(state=state(latent_buf=None, history=0)), "NULL state array / hist_scratch"),
                  (dict(state=state(history=0, _h0=22)), "history / n_heights out of range"),
                  (dict(state=state(n_heights=9)), "history / n_heights out of range"),
                  (dict(state=state(_h0=22), step=_lib.DpSeqStep(adjust_joint=22)), "bad height joint"),
                  (dict(step=_lib.DpSeqStep(adjust_joint=22), extra=ext(struct_size=8)), "bad joint adjustment"),
                  (dict(step=_lib.DpSeqStep(adjust_joint=3, adjust_target_joint=-1), extra=ext(struct_size=8)), "bad joint adjustment"),
                  (dict(extra=ext(struct_size=40), frames=no_zt), "dp_seq_lm_extra.struct_size is 40"),
                  (dict(extra=ext(reserved0=5), ar=lar(struct_size=8)), "reserved0 5"),
                  (dict(ar=lar(struct_size=32, order=0)), "dp_latent_ar.struct_size is 32"),
                  (dict(ar=lar(reserved0=1, order=0)), "reserved0 1"),
                  (dict(ar=lar(order=0, coeffs=None)), "dp_latent_ar.order 0 outside 1..4"),
                  (dict(ar=lar(order=5), state=state(history=2)), "dp_latent_ar.order 5 outside 1..4"),
                  (dict(ar=lar(coeffs=None), state=state(history=1)), "dp_latent_ar.coeffs or bias is NULL"),
                  (dict(ar=lar(bias=None), state=state(history=1)), "dp_latent_ar.coeffs or bias is NULL"),
                  (dict(ar=lar(order=3), state=state(history=2)), "shorter than dp_latent_ar.order 3"),
                  (dict(ar=lar()), "frames->z_tgt must be NULL"),                      # both
                  (dict(frames=no_zt), "neither a predictor nor frames->z_tgt")]      # neither
        for kw, word in stages:
            kw = dict(kw)
            rc, msg = _call(lib, ctx, p, kw.pop("frames", frames()), kw.pop("state", state()), **kw)
            assert rc == _lib.DP_ERR_INVALID and word in msg and "dp_optimize_sequence_lm" in msg, (word, msg)
        # well-formed, with either source of the targets, with and without the optional structs: refused only because there is no device
        for kw in (dict(), dict(null=("extra",)), dict(null=("adjust",)), dict(extra=_lib.DpSeqLmExtra()), dict(frames=no_zt, ar=lar()),
                   dict(frames=no_zt, ar=lar(order=4, trace=p)), dict(prm=prm(n_steps=64, early_stop=1, stop_eps_pos=1e-4), n_seq=1),
                   dict(step=_lib.DpSeqStep(adjust_joint=-1, adjust_target_joint=99))):
            kw = dict(kw)
            rc, msg = _call(lib, ctx, p, kw.pop("frames", frames()), kw.pop("state", state()), **kw)
            assert rc == _lib.DP_ERR_DEVICE and "dp_optimize_sequence_lm" in msg and "no device image" in msg, (rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del buf


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    lib.dp_optimize_sequence_lm.argtypes = _lib.load().dp_optimize_sequence_lm.argtypes
    buf, p, frames, state, sized = _pieces()
    ctx = _host_ctx(lib)
    try:
        rc, msg = _call(lib, ctx, p, frames(), state())
        assert rc == _lib.DP_ERR_UNSUPPORTED and "test-only" in msg and "dp_optimize_sequence_lm" in msg
        rc, msg = _call(lib, ctx, p, frames(), state(), prm=sized(_lib.DpLmParams, n_steps=0))  # (its argument checks come first)
        assert rc == _lib.DP_ERR_INVALID
        rc, msg = _call(lib, ctx, p, frames(z_tgt=None), state())
        assert rc == _lib.DP_ERR_INVALID and "neither" in msg
    finally:
        lib.dp_destroy(ctx)
    del buf


def test_lm_predictor_is_validated_last_and_is_not_part_of_the_struct():
    hold = LatentAR.hold()
    assert LM().predictor is None and LM(3, predictor=hold).check().predictor is hold
    assert [f for f in LM.__dataclass_fields__][-1] == "predictor"
    with pytest.raises(ValueError, match="predictor must be a dragposer_amd.LatentAR, got str"):
        LM(predictor="hold").check()
    with pytest.raises(ValueError, match="steps 0 outside"):  # (everything dp_optimize_lm would refuse comes first)
        LM(steps=0, predictor="hold").check()
    with pytest.raises(ValueError, match="mu0 outside"):
        LM(mu0=1e7, predictor=object()).check()
    a, b = LM(5, predictor=hold).to_struct(2.0, 0.5), LM(5).to_struct(2.0, 0.5)
    assert bytes(a) == bytes(b) and C.sizeof(a) == 48


def test_dragpose_checks_around_the_solver():
    import torch

    from dragposer_amd.drag_pose import DragPose

    # (no library, no context: reaching the launch's preparation raises AttributeError, which is how this test knows a call got past the checks)
    drag = types.SimpleNamespace(temporal=None, S=2, device=torch.device("cpu"), _skeleton=lambda offsets: None)
    with pytest.raises(AttributeError):  # target_root= is taken now
        DragPose.run_frames(drag, torch.zeros(3, 2, 6, 3), torch.zeros(3, 2, 6, 3, 3), None, None, target_root=torch.zeros(3, 2, 3), solver=LM())
    with pytest.raises(ValueError, match="DragPose.run_frames: solver= does not go with ar="):  # the predictor belongs to the solver
        DragPose.run_frames(drag, None, None, None, None, solver=LM(predictor=LatentAR.hold()), ar=LatentAR.hold())
    with pytest.raises(ValueError, match="predictor must be a dragposer_amd.LatentAR"):
        DragPose.run_frames(drag, None, None, None, None, solver=LM(predictor=3))
    with_temporal = types.SimpleNamespace(temporal=object(), S=2, device=torch.device("cpu"), _skeleton=lambda offsets: None)
    for fn, who in ((DragPose.run, "run"), (DragPose.run_frames, "run_frames")):
        with pytest.raises(ValueError, match=f"DragPose.{who}: ar= and a temporal model are two sources"):
            fn(with_temporal, None, None, None, None, solver=LM(predictor=LatentAR.hold()))
    other = types.SimpleNamespace(temporal=None, S=2, device=torch.device("cpu"), _skeleton=lambda offsets: offsets)
    with pytest.raises(ValueError, match="DragPose.run_frames: solver= runs on the context's skeleton only"):
        DragPose.run_frames(other, None, None, None, None, solver=LM(), offsets=torch.ones(22, 3))


def test_the_kernel_keeps_its_budget(tmp_path):
    """hipcc -S with the build's flags: no spilled vector register, no scratch, and the LDS figure the header states, within a CU's 160 KB"""
    notes = _kernel_notes("dp_lm_seq.hip", tmp_path)
    assert len(notes) == 1
    (name, n), = notes.items()
    assert "dp_lm_seq_kernel" in name
    assert n["vspill"] == 0 and n["scratch"] == 0, n
    assert n["lds"] == SEQ_LDS and n["lds"] <= 160 * 1024, n
    assert n["vgpr"] <= 512 and n["agpr"] <= 256, n  # (.vgpr_count is the unified file's total, accumulator half included; one wave per SIMD)

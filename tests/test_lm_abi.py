"""CPU: the Levenberg-Marquardt call (include/dragposer_lm.h) -- the header against the C compiler and the binding, the refusals of
dp_optimize_lm on a context without a device in the header's order, the test-only library's refusal, what LM.check() and
DragPose.run(solver=...) refuse, and dp_lm_kernel's register and LDS budget.  No compute call is made here (the GPU side is
tests/test_hip_lm.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as G
from dragposer_amd import LM, _lib
from test_build_quality import _kernel_notes
from test_host_san import ROOT
from test_sequence_constraints_abi import _host_ctx

HDR = os.path.join(ROOT, "include", "dragposer_lm.h")
PARAMS_FIELDS = ("struct_size", "n_steps", "lambda_rot", "lambda_tmp", "mu0", "mu_up", "mu_down", "mu_min", "mu_max", "early_stop", "stop_eps_pos",
                 "stop_eps_rot")
EXTRA_FIELDS = ("struct_size", "reserved0", "mu", "n_accepted", "loss0")
LM_LDS = 121488  # dp_lm.h: LDS_BYTES


def test_header_declares_the_call_and_the_library_exports_it():
    text = open(HDR).read()
    assert re.findall(r"^int\s+(dp_\w+)\s*\(", text, flags=re.M) == ["dp_optimize_lm"] == list(_lib.LM_SYMBOLS)
    assert hasattr(_lib.load(), "dp_optimize_lm")
    assert re.search(r"#define DP_LM_MAX_STEPS 64\b", text) and _lib.DP_LM_MAX_STEPS == 64
    assert "dp_lm.hip" in G.HIP_SOURCES
    lds = re.search(r"static_assert\(LDS_BYTES == (\d+)", open(os.path.join(G.CSRC, "dp_lm.h")).read())
    assert int(lds.group(1)) == LM_LDS


def test_layout_and_defaults_match_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "lm.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_lm.h"\nint main(void) {\n'
                   'printf("%zu %zu %d\\n", sizeof(dp_lm_params), sizeof(dp_lm_extra), DP_LM_MAX_STEPS);\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_lm_params, {f}));\n' for f in PARAMS_FIELDS)
                   + "".join(f'printf("%zu\\n", offsetof(dp_lm_extra, {f}));\n' for f in EXTRA_FIELDS)
                   + 'dp_lm_params p = DP_LM_PARAMS_INIT;\ndp_lm_extra e = DP_LM_EXTRA_INIT;\n'
                   'printf("%u %d %d\\n", p.struct_size, p.n_steps, p.early_stop);\n'
                   'printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\\n", p.lambda_rot, p.lambda_tmp, p.mu0, p.mu_up, p.mu_down, p.mu_min, p.mu_max, '
                   'p.stop_eps_pos, p.stop_eps_rot);\n'
                   'printf("%u %u %d %d %d\\n", e.struct_size, e.reserved0, e.mu != 0, e.n_accepted != 0, e.loss0 != 0);\nreturn 0; }\n')
    exe = tmp_path / "lm"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    assert [int(x) for x in lines[0].split()] == [C.sizeof(_lib.DpLmParams), C.sizeof(_lib.DpLmExtra), _lib.DP_LM_MAX_STEPS] == [48, 32, 64]
    n = len(PARAMS_FIELDS)
    assert [int(x) for x in lines[1:1 + n]] == [getattr(_lib.DpLmParams, f).offset for f in PARAMS_FIELDS] == list(range(0, 48, 4))
    assert [int(x) for x in lines[1 + n:1 + n + 5]] == [getattr(_lib.DpLmExtra, f).offset for f in EXTRA_FIELDS] == [0, 4, 8, 16, 24]
    p, e, d = _lib.DpLmParams(), _lib.DpLmExtra(), LM()
    assert [int(x) for x in lines[-3].split()] == [p.struct_size, p.n_steps, p.early_stop] == [48, 3, 0] and d.steps == 3
    f32 = lambda x: C.c_float(x).value
    floats = [f32(float(x)) for x in lines[-2].split()]  # (%.9g round-trips a float)
    assert floats == [p.lambda_rot, p.lambda_tmp, p.mu0, p.mu_up, p.mu_down, p.mu_min, p.mu_max, p.stop_eps_pos, p.stop_eps_rot]
    assert floats[2:7] == [f32(d.mu0), f32(d.mu_up), f32(d.mu_down), f32(d.mu_min), f32(d.mu_max)] == [f32(1e-2), 4.0, f32(1.0 / 3.0), f32(1e-6), 1e6]
    assert [int(x) for x in lines[-1].split()] == [e.struct_size, 0, 0, 0, 0] and (e.reserved0, e.mu, e.n_accepted, e.loss0) == (0, None, None, None)


def test_refusals_come_in_the_documented_order_before_any_device_is_touched():
    lib = _lib.load()
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    batch = _lib.DpBatch(n_frames=4, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
    out = _lib.DpResult(z=p)
    nan, inf = float("nan"), float("inf")

    def call(ctx, params=None, extra=None, result=None, b=batch, null=()):
        prm = params if params is not None else _lib.DpLmParams()
        ex = extra if extra is not None else _lib.DpLmExtra(mu=p)
        rs = result if result is not None else out
        rc = lib.dp_optimize_lm(ctx, None if "batch" in null else C.byref(b), None if "params" in null else C.byref(prm), C.byref(rs),
                                None if "extra" in null else C.byref(ex), None)
        return rc, (lib.dp_last_error(ctx).decode() if ctx else "")

    assert call(None)[0] == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    try:
        for null in ("batch", "params"):
            rc, msg = call(ctx, null=(null,))
            assert rc == _lib.DP_ERR_INVALID and "NULL batch or params" in msg, msg

        def prm(**k):
            s = _lib.DpLmParams()
            for key, v in k.items():
                setattr(s, key, v)
            return s

        def ext(**k):
            s = _lib.DpLmExtra(mu=p)
            for key, v in k.items():
                setattr(s, key, v)
            return s

        small = _lib.DpResult(z=p)
        small.struct_size = 8
        bad_batch = _lib.DpBatch(n_frames=0, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
        # each stage names what it refuses, with a later stage's fault present as well
        stages = [(dict(params=prm(struct_size=44, n_steps=0)), "dp_lm_params.struct_size is 44"),
                  (dict(params=prm(struct_size=5000, n_steps=0)), "dp_lm_params.struct_size is 5000"),
                  (dict(result=small, params=prm(n_steps=0)), "dp_result.struct_size"),
                  (dict(extra=ext(struct_size=24), params=prm(n_steps=0)), "dp_lm_extra.struct_size is 24"),
                  (dict(extra=ext(reserved0=1), params=prm(n_steps=0)), "reserved0 1"),
                  (dict(params=prm(n_steps=0, lambda_rot=nan)), "n_steps 0 outside 1..64"),
                  (dict(params=prm(n_steps=65, lambda_rot=nan)), "n_steps 65 outside 1..64"),
                  (dict(params=prm(lambda_rot=nan, mu_down=2.0)), "lambda_rot or lambda_tmp"),
                  (dict(params=prm(lambda_tmp=-1.0, mu_down=2.0)), "lambda_rot or lambda_tmp"),
                  (dict(params=prm(mu0=nan, mu_down=2.0)), "is not finite"),
                  (dict(params=prm(mu_max=inf, mu_down=2.0)), "is not finite"),
                  (dict(params=prm(stop_eps_rot=nan, mu_down=2.0)), "is not finite"),
                  (dict(params=prm(mu_down=1.0, mu_up=1.0)), "mu_down must lie in (0, 1)"),
                  (dict(params=prm(mu_down=0.0, mu_up=1.0)), "mu_down must lie in (0, 1)"),
                  (dict(params=prm(mu_up=1.0, mu_min=2.0, mu_max=1.0)), "mu_up must be greater than 1"),
                  (dict(params=prm(mu_min=2.0, mu_max=1.0, mu0=5.0)), "0 < mu_min <= mu_max"),
                  (dict(params=prm(mu_min=0.0, mu0=5e6)), "0 < mu_min <= mu_max"),
                  (dict(params=prm(mu0=5e6), b=bad_batch), "mu0 outside [mu_min, mu_max]"),
                  (dict(params=prm(mu0=1e-7), b=bad_batch), "mu0 outside [mu_min, mu_max]"),
                  (dict(b=bad_batch), "n_frames must be positive"),
                  (dict(b=_lib.DpBatch(n_frames=4, z0=p, z_tgt=None, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)), "NULL input array")]
        for kw, word in stages:
            rc, msg = call(ctx, **kw)
            assert rc == _lib.DP_ERR_INVALID and word in msg and "dp_optimize_lm" in msg, (word, msg)
        # well-formed, with and without the extra struct: refused only because there is no device
        for kw in (dict(), dict(null=("extra",)), dict(extra=_lib.DpLmExtra()), dict(params=prm(n_steps=64, early_stop=1, stop_eps_pos=1e-4))):
            rc, msg = call(ctx, **kw)
            assert rc == _lib.DP_ERR_DEVICE and "dp_optimize_lm" in msg and "no device image" in msg, (rc, msg)
    finally:
        lib.dp_destroy(ctx)
    del buf


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    lib.dp_optimize_lm.argtypes = _lib.load().dp_optimize_lm.argtypes
    ctx = _host_ctx(lib)
    try:
        buf = (C.c_float * 4096)()
        p = C.cast(buf, C.c_void_p)
        batch = _lib.DpBatch(n_frames=4, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
        out, prm = _lib.DpResult(z=p), _lib.DpLmParams()
        rc = lib.dp_optimize_lm(ctx, C.byref(batch), C.byref(prm), C.byref(out), None, None)
        assert rc == _lib.DP_ERR_UNSUPPORTED and "test-only" in lib.dp_last_error(ctx).decode()
        prm.n_steps = 0  # (its argument checks come first)
        assert lib.dp_optimize_lm(ctx, C.byref(batch), C.byref(prm), C.byref(out), None, None) == _lib.DP_ERR_INVALID
    finally:
        lib.dp_destroy(ctx)


def test_lm_check_refuses_what_the_library_would():
    LM().check()
    LM(steps=64, mu0=1.0, mu_min=1.0, mu_max=1.0).check()
    for kw, word in ((dict(steps=0), "steps 0 outside 1..64"), (dict(steps=65), "steps 65 outside 1..64"), (dict(steps=2.5), "outside 1..64"),
                     (dict(mu0=float("nan")), "mu0 is not finite"), (dict(mu_max=float("inf")), "mu_max is not finite"),
                     (dict(mu_down=1.0), r"mu_down must lie in \(0, 1\)"), (dict(mu_down=0.0), "mu_down must lie"), (dict(mu_up=1.0), "mu_up must be greater than 1"),
                     (dict(mu_min=0.0), "0 < mu_min <= mu_max"), (dict(mu_min=2.0, mu_max=1.0), "0 < mu_min <= mu_max"),
                     (dict(mu0=1e7), r"mu0 outside \[mu_min, mu_max\]"), (dict(mu0=1e-7), "mu0 outside")):
        with pytest.raises(ValueError, match=word):
            LM(**kw).check()
    s = LM(5, stop_eps_pos=1e-3).to_struct(2.0, 0.5, stop_eps_pos=1e-4, stop_eps_rot=1e-2)
    assert (s.n_steps, s.lambda_rot, s.lambda_tmp, s.early_stop) == (5, 2.0, 0.5, 1) and s.struct_size == C.sizeof(_lib.DpLmParams)
    assert s.stop_eps_pos == C.c_float(1e-3).value and s.stop_eps_rot == C.c_float(1e-2).value  # (the LM's own threshold wins)


def test_dragpose_refuses_the_solver_with_any_other_layer():
    import types

    import torch

    from dragposer_amd import Constraints, Gaps, Hold, Holds, Term, Terms, Tether, Tethers
    from dragposer_amd.drag_pose import DragPose

    drag = types.SimpleNamespace(temporal=None, S=2, device=torch.device("cpu"))  # (no library, no context: reaching a launch would raise AttributeError)
    table = Terms([Term.distance(4, 8, hi=0.3)])
    layers = dict(constraints=Constraints.reference(), terms=table, holds=Holds([Hold(0, 0.02, 0.05)]), ar=object(), gaps=Gaps(0, 1.0),
                  tethers=Tethers([Tether(0)]))
    for fn, who in ((DragPose.run, "run"), (DragPose.run_frames, "run_frames")):
        for name, value in layers.items():
            with pytest.raises(ValueError, match=f"DragPose.{who}: solver= does not go with {name}="):
                fn(drag, None, None, None, None, solver=LM(), **{name: value})
    with pytest.raises(ValueError, match="DragPose.run: solver= does not go with live="):
        DragPose.run(drag, None, None, None, None, solver=LM(), live=True)
    with pytest.raises(ValueError, match="steps 0 outside"):
        DragPose.run(drag, None, None, None, None, solver=LM(steps=0))
    other = types.SimpleNamespace(temporal=None, S=2, device=torch.device("cpu"), _skeleton=lambda offsets: offsets)
    with pytest.raises(ValueError, match="solver= runs on the context's skeleton only"):
        DragPose.run(other, None, None, None, None, solver=LM(), offsets=torch.ones(22, 3))


def test_the_kernel_keeps_its_budget(tmp_path):
    """hipcc -S with the build's flags: no spilled vector register, no scratch, and the LDS figure the header states"""
    notes = _kernel_notes("dp_lm.hip", tmp_path)
    assert len(notes) == 1
    (name, n), = notes.items()
    assert "dp_lm_kernel" in name
    assert n["vspill"] == 0 and n["scratch"] == 0, n
    assert n["lds"] == LM_LDS and n["lds"] <= 160 * 1024, n
    assert n["vgpr"] <= 512 and n["agpr"] <= 256, n  # (.vgpr_count is the unified file's total, accumulator half included; one wave per SIMD: dp_lm.h)

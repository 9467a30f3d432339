"""CPU: the constrained entry point of include/dragposer_constraints.h -- header, binding, exports, argument checks and the kernel's
register and LDS budget.  No compute call is made here (the GPU side is tests/test_hip_constraints.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as G
from dragposer_amd import _lib
from test_build_quality import _kernel_notes  # (the flags __graft_entry__ compiles each unit with)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "dragposer_constraints.h")
FIELDS = ("struct_size", "reserved0", "w_feet_floor", "w_head_hips_forward", "w_head_hips_colinear", "w_hips_feet_colinear", "floor_joints",
          "foot_joints", "head_joint", "hips_joint", "up_axis", "floor_one_sided", "floor_level", "fwd_axis", "fwd_threshold", "fwd_margin",
          "feet_radius", "global_pos", "loss_extra")
LDS_BUDGET = 70832  # dp_cons.h: LDS_BYTES, DESIGN.md section 13


def test_header_declares_the_constraint_symbols_and_the_library_exports_them():
    declared = set(re.findall(r"^int\s+(dp_\w+)\s*\(", open(HDR).read(), flags=re.M))
    assert declared == set(_lib.CONSTRAINT_SYMBOLS)
    assert not set(_lib.CONSTRAINT_SYMBOLS) & (set(_lib.PUBLIC_SYMBOLS) | set(_lib.GRAD_SYMBOLS))
    lib = _lib.load()
    for sym in declared:
        assert hasattr(lib, sym), sym
    assert "dp_cons.hip" in G.HIP_SOURCES


def test_constraints_layout_and_defaults_match_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "cons.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_constraints.h"\nint main(void) {\n'
                   'printf("%zu\\n", sizeof(dp_constraints));\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_constraints, {f}));\n' for f in FIELDS)
                   + 'dp_constraints c = DP_CONSTRAINTS_INIT;\n'
                   'printf("%u %u %g %g %g %g %d %d %d %d %d %d %d %d %g %g %g %g %g %g %g %d %d\\n", c.struct_size, c.reserved0, c.w_feet_floor,'
                   ' c.w_head_hips_forward, c.w_head_hips_colinear, c.w_hips_feet_colinear, c.floor_joints[0], c.floor_joints[1], c.foot_joints[0],'
                   ' c.foot_joints[1], c.head_joint, c.hips_joint, c.up_axis, c.floor_one_sided, c.floor_level, c.fwd_axis[0], c.fwd_axis[1],'
                   ' c.fwd_axis[2], c.fwd_threshold, c.fwd_margin, c.feet_radius, c.global_pos != 0, c.loss_extra != 0);\nreturn 0; }\n')
    exe = tmp_path / "cons"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    assert lines[:-1] == [str(C.sizeof(_lib.DpConstraints))] + [str(getattr(_lib.DpConstraints, f).offset) for f in FIELDS]
    c = _lib.DpConstraints()  # the binding's defaults are the header's
    want = [c.struct_size, 0, 0, 0, 0, 0, 4, 8, 3, 7, 13, 0, 1, 0, 0, 0, 0, 1, 0.5, 0.2, 0.2, 0, 0]
    assert [float(x) for x in lines[-1].split()] == pytest.approx([float(x) for x in want])
    assert (tuple(c.floor_joints), tuple(c.foot_joints), c.head_joint, c.hips_joint, c.up_axis) == ((4, 8), (3, 7), 13, 0, 1)


def test_python_constraints_defaults():
    from dragposer_amd import Constraints

    c = Constraints()
    assert (c.w_feet_floor, c.w_head_hips_forward, c.w_head_hips_colinear, c.w_hips_feet_colinear) == (0, 0, 0, 0)
    r = Constraints.reference()
    assert (r.w_feet_floor, r.w_head_hips_forward, r.w_head_hips_colinear, r.w_hips_feet_colinear) == (1, 1, 1, 1)
    s = r.to_struct()
    assert (tuple(s.floor_joints), tuple(s.foot_joints), s.head_joint, s.hips_joint, s.up_axis, s.floor_one_sided) == ((4, 8), (3, 7), 13, 0, 1, 0)
    with pytest.raises(ValueError):
        Constraints(w_feet_floor=-1.0).to_struct()


def _args():
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    b = _lib.DpBatch(n_frames=1, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
    prm = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
    r = _lib.DpResult()
    r.z = p
    return buf, p, b, prm, r


def test_argument_errors_are_refused_before_any_device_is_touched():
    lib = _lib.load()
    buf, p, b, prm, r = _args()
    c = _lib.DpConstraints()
    assert lib.dp_optimize_constrained(None, C.byref(b), C.byref(prm), C.byref(c), C.byref(r), None) == _lib.DP_ERR_INVALID
    ctx = C.c_void_p()
    assert lib.dp_debug_host_ctx(C.byref(ctx)) == _lib.DP_OK and ctx.value  # a context with no device behind it
    try:
        def call(batch=C.byref(b), params=C.byref(prm), cons=None, res=C.byref(r), **fields):
            cc = _lib.DpConstraints()
            cc.global_pos = p
            for k, v in fields.items():
                if k in ("floor_joints", "foot_joints", "fwd_axis"):
                    getattr(cc, k)[:] = v
                else:
                    setattr(cc, k, v)
            rc = lib.dp_optimize_constrained(ctx, batch, params, C.byref(cc) if cons is None else cons, res, None)
            return rc, lib.dp_last_error(ctx).decode()

        for kw in (dict(batch=None), dict(params=None), dict(res=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and "NULL" in msg, kw
        assert lib.dp_optimize_constrained(ctx, C.byref(b), C.byref(prm), None, C.byref(r), None) == _lib.DP_ERR_INVALID
        for size, res in ((0, 0), (8, 0), (C.sizeof(_lib.DpConstraints) - 1, 0), (5000, 0), (C.sizeof(_lib.DpConstraints), 3)):
            bad = _lib.DpConstraints()
            bad.struct_size, bad.reserved0 = size, res
            rc, msg = call(cons=C.byref(bad))
            assert rc == _lib.DP_ERR_INVALID and "struct_size" in msg, (size, res)
        bad_r = _lib.DpResult()
        bad_r.struct_size = 8
        assert call(res=C.byref(bad_r))[0] == _lib.DP_ERR_INVALID
        for kw in (dict(floor_joints=(4, 22)), dict(floor_joints=(-1, 8)), dict(foot_joints=(3, 99)), dict(head_joint=22), dict(hips_joint=-1)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and "joint index" in msg, kw
        for up in (-1, 3):
            rc, msg = call(up_axis=up)
            assert rc == _lib.DP_ERR_INVALID and "up_axis" in msg
        for name in ("w_feet_floor", "w_head_hips_forward", "w_head_hips_colinear", "w_hips_feet_colinear"):
            for x in (-1.0, float("nan"), float("inf")):
                rc, msg = call(**{name: x})
                assert rc == _lib.DP_ERR_INVALID and "weight" in msg, (name, x)
        rc, msg = call(w_feet_floor=1.0, global_pos=None)
        assert rc == _lib.DP_ERR_INVALID and "global_pos" in msg
        rc, msg = call(w_head_hips_colinear=1.0, global_pos=None)  # (no floor term: global_pos is not read)
        assert rc == _lib.DP_ERR_DEVICE, (rc, msg)
        rc, msg = call(w_feet_floor=1.0, w_head_hips_forward=2.0)  # well-formed: refused only because there is no device
        assert rc == _lib.DP_ERR_DEVICE, (rc, msg)
    finally:
        lib.dp_destroy(ctx)


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    ctx = C.c_void_p()
    assert lib.dp_debug_host_ctx(C.byref(ctx)) == _lib.DP_OK
    try:
        buf, p, b, prm, r = _args()
        c = _lib.DpConstraints()
        assert lib.dp_optimize_constrained(ctx, C.byref(b), C.byref(prm), C.byref(c), C.byref(r), None) == _lib.DP_ERR_UNSUPPORTED
    finally:
        lib.dp_destroy(ctx)


def test_constrained_kernel_keeps_its_register_and_lds_budget(tmp_path):
    notes = _kernel_notes("dp_cons.hip", tmp_path)
    (name, n), = [(k, v) for k, v in notes.items() if "dp_cons_kernel" in k]
    assert n["vspill"] == 0 and n["scratch"] == 0, (name, n)
    assert n["lds"] <= LDS_BUDGET, (name, n)

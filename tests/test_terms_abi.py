"""CPU: the term-table entry point of include/dragposer_terms.h -- header, binding, exports, argument checks, the Python mirror of those
checks, and the table kernel's register and LDS budget.  No compute call is made here (the GPU side is tests/test_hip_terms.py)."""
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
HDR = os.path.join(ROOT, "include", "dragposer_terms.h")
TERM_FIELDS = ("type", "joint_a", "joint_b", "flags", "weight", "point", "dir", "axis_a", "axis_b", "p0", "p1", "per_frame")
TERMS_FIELDS = ("struct_size", "reserved0", "n_terms", "up_axis", "terms", "global_pos", "loss_terms")
LDS_BUDGET = 76 * 1024  # dp_cons.h: LDS_BYTES_T, DESIGN.md section 13


def test_header_declares_the_term_symbols_and_the_library_exports_them():
    declared = set(re.findall(r"^int\s+(dp_\w+)\s*\(", open(HDR).read(), flags=re.M))
    assert declared == set(_lib.TERM_SYMBOLS)
    assert not set(_lib.TERM_SYMBOLS) & (set(_lib.PUBLIC_SYMBOLS) | set(_lib.GRAD_SYMBOLS) | set(_lib.CONSTRAINT_SYMBOLS))
    lib = _lib.load()
    for sym in declared:
        assert hasattr(lib, sym), sym
    src = open(G.__file__).read()
    assert "_lib.TERM_SYMBOLS" in src  # build()'s export check


def test_terms_layout_and_defaults_match_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "terms.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_terms.h"\nint main(void) {\n'
                   'printf("%zu %zu\\n", sizeof(dp_term), sizeof(dp_terms));\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_term, {f}));\n' for f in TERM_FIELDS)
                   + "".join(f'printf("%zu\\n", offsetof(dp_terms, {f}));\n' for f in TERMS_FIELDS)
                   + 'dp_term t = DP_TERM_INIT;\ndp_terms s = DP_TERMS_INIT;\n'
                   'printf("%d %d %d %d %g %g %g %g %g %g %g %g %g %g %g %g %g %g %g %d\\n", t.type, t.joint_a, t.joint_b, t.flags, t.weight,'
                   ' t.point[0], t.point[1], t.point[2], t.dir[0], t.dir[1], t.dir[2], t.axis_a[0], t.axis_a[1], t.axis_a[2], t.axis_b[0],'
                   ' t.axis_b[1], t.axis_b[2], t.p0, t.p1, t.per_frame != 0);\n'
                   'printf("%u %u %d %d %d %d %d\\n", s.struct_size, s.reserved0, s.n_terms, s.up_axis, s.terms != 0, s.global_pos != 0,'
                   ' s.loss_terms != 0);\n'
                   'printf("%d %d %d %d %d %d\\n", DP_MAX_TERMS, DP_TERM_PLANE, DP_TERM_DISTANCE, DP_TERM_ALIGN, DP_TERM_ONE_SIDED,'
                   ' DP_TERM_DROP_UP);\nreturn 0; }\n')
    exe = tmp_path / "terms"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    assert lines[0].split() == [str(C.sizeof(_lib.DpTerm)), str(C.sizeof(_lib.DpTerms))]
    offs = [str(getattr(_lib.DpTerm, f).offset) for f in TERM_FIELDS] + [str(getattr(_lib.DpTerms, f).offset) for f in TERMS_FIELDS]
    assert lines[1:1 + len(offs)] == offs
    t, s = _lib.DpTerm(), _lib.DpTerms()  # the binding's defaults are the header's
    want_t = [t.type, t.joint_a, t.joint_b, t.flags, t.weight, *t.point, *t.dir, *t.axis_a, *t.axis_b, t.p0, t.p1, 0]
    assert [float(x) for x in lines[-3].split()] == pytest.approx([float(x) for x in want_t])
    assert (t.joint_b, tuple(t.dir), tuple(t.axis_a)) == (-1, (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    assert [int(x) for x in lines[-2].split()] == [s.struct_size, 0, 0, 1, 0, 0, 0]
    assert [int(x) for x in lines[-1].split()] == [_lib.DP_MAX_TERMS, _lib.DP_TERM_PLANE, _lib.DP_TERM_DISTANCE, _lib.DP_TERM_ALIGN,
                                                   _lib.DP_TERM_ONE_SIDED, _lib.DP_TERM_DROP_UP]


def _args():
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    b = _lib.DpBatch(n_frames=1, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
    prm = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
    r = _lib.DpResult()
    r.z = p
    return buf, p, b, prm, r


def _good_terms():
    """one well-formed term of each shape (every field a refusal case below changes)"""
    P, D, A = _lib.DP_TERM_PLANE, _lib.DP_TERM_DISTANCE, _lib.DP_TERM_ALIGN
    return [dict(type=P, joint_a=4, weight=1.0, dir=(0.0, 1.0, 0.0), flags=_lib.DP_TERM_ONE_SIDED),
            dict(type=D, joint_a=3, joint_b=7, weight=2.0, p0=0.1, p1=0.3, flags=_lib.DP_TERM_DROP_UP),
            dict(type=D, joint_a=8, joint_b=-1, weight=0.5, point=(0.1, 0.0, 0.2)),
            dict(type=A, joint_a=13, joint_b=0, weight=1.0, axis_a=(0.0, 0.0, 1.0), axis_b=(0.0, 0.0, 1.0), p0=0.5, p1=-0.3),
            dict(type=A, joint_a=13, joint_b=-1, weight=1.0, axis_a=(1.0, 0.0, 0.0), dir=(0.6, 0.0, 0.8))]


def _table(rows):
    arr = (_lib.DpTerm * max(1, len(rows)))(*[_lib.DpTerm() for _ in rows])  # (DP_TERM_INIT's defaults in every element)
    for i, row in enumerate(rows):
        for k, v in row.items():
            if k in ("point", "dir", "axis_a", "axis_b"):
                getattr(arr[i], k)[:] = v
            else:
                setattr(arr[i], k, v)
    return arr


# (the term index, the field changes) -> refused; every entry of the header's list
BAD_TERMS = [
    (0, dict(type=0)), (0, dict(type=4)), (0, dict(flags=4)), (1, dict(flags=-1)),
    (0, dict(joint_a=22)), (0, dict(joint_a=-1)), (1, dict(joint_b=22)), (1, dict(joint_b=-2)), (0, dict(joint_b=5)),
    (0, dict(weight=-1.0)), (1, dict(weight=float("nan"))), (3, dict(weight=float("inf"))),
    (2, dict(point=(0.0, float("nan"), 0.0))), (3, dict(axis_b=(float("inf"), 0.0, 0.0))), (1, dict(p1=float("inf"))),
    (3, dict(p1=float("nan"))), (1, dict(p0=-0.1)), (1, dict(p0=0.5, p1=0.3)), (3, dict(p0=-0.5)),
    (0, dict(dir=(0.0, 1.001, 0.0))), (0, dict(dir=(0.0, 0.0, 0.0))), (4, dict(dir=(0.6, 0.0, 0.7))),
    (3, dict(axis_a=(0.0, 0.0, 0.0))), (3, dict(axis_b=(0.0, 0.0, 0.0))),
]


def test_argument_errors_are_refused_before_any_device_is_touched():
    lib = _lib.load()
    buf, p, b, prm, r = _args()
    arr = _table(_good_terms())
    good = _lib.DpTerms(n_terms=5, terms=C.cast(arr, C.c_void_p), global_pos=p)
    assert lib.dp_optimize_terms(None, C.byref(b), C.byref(prm), C.byref(good), C.byref(r), None) == _lib.DP_ERR_INVALID
    ctx = C.c_void_p()
    assert lib.dp_debug_host_ctx(C.byref(ctx)) == _lib.DP_OK and ctx.value  # a context with no device behind it
    try:
        def call(batch=C.byref(b), params=C.byref(prm), terms=None, res=C.byref(r)):
            rc = lib.dp_optimize_terms(ctx, batch, params, C.byref(good) if terms is None else terms, res, None)
            return rc, lib.dp_last_error(ctx).decode()

        for kw in (dict(batch=None), dict(params=None), dict(res=None)):
            rc, msg = call(**kw)
            assert rc == _lib.DP_ERR_INVALID and "NULL" in msg, kw
        assert lib.dp_optimize_terms(ctx, C.byref(b), C.byref(prm), None, C.byref(r), None) == _lib.DP_ERR_INVALID
        for size, res in ((0, 0), (8, 0), (C.sizeof(_lib.DpTerms) - 1, 0), (5000, 0), (C.sizeof(_lib.DpTerms), 3)):
            bad = _lib.DpTerms(n_terms=5, terms=C.cast(arr, C.c_void_p), global_pos=p)
            bad.struct_size, bad.reserved0 = size, res
            rc, msg = call(terms=C.byref(bad))
            assert rc == _lib.DP_ERR_INVALID and "struct_size" in msg, (size, res)
        bad_r = _lib.DpResult()
        bad_r.struct_size = 8
        assert call(res=C.byref(bad_r))[0] == _lib.DP_ERR_INVALID
        for n in (-1, 17):
            big = _table(_good_terms() * 4)
            rc, msg = call(terms=C.byref(_lib.DpTerms(n_terms=n, terms=C.cast(big, C.c_void_p), global_pos=p)))
            assert rc == _lib.DP_ERR_INVALID and "n_terms" in msg, n
        rc, msg = call(terms=C.byref(_lib.DpTerms(n_terms=2, terms=None, global_pos=p)))
        assert rc == _lib.DP_ERR_INVALID and "NULL terms" in msg
        for up in (-1, 3):
            rc, msg = call(terms=C.byref(_lib.DpTerms(n_terms=5, up_axis=up, terms=C.cast(arr, C.c_void_p), global_pos=p)))
            assert rc == _lib.DP_ERR_INVALID and "up_axis" in msg
        for i, change in BAD_TERMS:
            rows = _good_terms()
            rows[i].update(change)
            a2 = _table(rows)
            rc, msg = call(terms=C.byref(_lib.DpTerms(n_terms=5, terms=C.cast(a2, C.c_void_p), global_pos=p)))
            assert rc == _lib.DP_ERR_INVALID and f"term {i}" in msg, (i, change, rc, msg)
        for i in (0, 2):  # an active PLANE or point-DISTANCE term needs global_pos
            rows = _good_terms()
            for k in (0, 2):
                if k != i:
                    rows[k]["weight"] = 0.0
            a2 = _table(rows)
            rc, msg = call(terms=C.byref(_lib.DpTerms(n_terms=5, terms=C.cast(a2, C.c_void_p), global_pos=None)))
            assert rc == _lib.DP_ERR_INVALID and "global_pos" in msg, i
        rows = _good_terms()
        rows[0]["weight"] = rows[2]["weight"] = 0.0  # (inactive: global_pos is not read) and a world ALIGN whose dir a row replaces
        rows[4].update(dir=(0.0, 0.0, 0.0), per_frame=p)
        a2 = _table(rows)
        rc, msg = call(terms=C.byref(_lib.DpTerms(n_terms=5, terms=C.cast(a2, C.c_void_p), global_pos=None)))
        assert rc == _lib.DP_ERR_DEVICE, (rc, msg)
        empty = _lib.DpTerms(n_terms=0, terms=None)
        assert call(terms=C.byref(empty))[0] == _lib.DP_ERR_DEVICE
        bad_b = _lib.DpBatch(n_frames=0, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
        assert call(batch=C.byref(bad_b))[0] == _lib.DP_ERR_INVALID  # (what dp_optimize refuses)
        bad_p = _lib.DpParams(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=0.0, lambda_rot=1.0)
        assert call(params=C.byref(bad_p))[0] == _lib.DP_ERR_INVALID
        rc, msg = call()  # well-formed: refused only because there is no device
        assert rc == _lib.DP_ERR_DEVICE, (rc, msg)
    finally:
        lib.dp_destroy(ctx)


def test_python_validation_mirrors_the_library():
    """Terms.check raises ValueError exactly where the library returns DP_ERR_INVALID (the same BAD_TERMS table)"""
    from dragposer_amd import Term, Terms

    def term(row):
        t = Term(type=row.get("type", 1), joint_a=row.get("joint_a", 0))
        for k, v in row.items():
            setattr(t, k, tuple(v) if isinstance(v, tuple) else v)
        return t

    Terms([term(r) for r in _good_terms()]).check()
    for i, change in BAD_TERMS:
        rows = _good_terms()
        rows[i].update(change)
        with pytest.raises(ValueError, match=f"term {i}"):
            Terms([term(r) for r in rows]).check()
    with pytest.raises(ValueError):
        Terms([term(_good_terms()[0])] * 17).check()
    with pytest.raises(ValueError):
        Terms([], up_axis=3).check()
    with pytest.raises(ValueError):
        Term.distance(3, 7, point=(0.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        Term.align(13, (0, 0, 1))


def test_from_constraints_maps_the_four_terms():
    from dragposer_amd import Constraints, Terms
    from dragposer_amd.terms import ALIGN, DISTANCE, DROP_UP, ONE_SIDED, PLANE

    t = Terms.from_constraints(Constraints.reference(w_feet_floor=3.0, floor_one_sided=True, floor_level=0.02))
    assert [x.type for x in t.terms] == [ALIGN, DISTANCE, PLANE, PLANE, DISTANCE, DISTANCE] and t.up_axis == 1
    fw, hc, f0, f1, d0, d1 = t.terms
    assert (fw.joint_a, fw.joint_b, fw.flags, fw.p0, fw.p1, fw.axis_a, fw.axis_b) == (13, 0, DROP_UP, 0.5, 0.2, (0, 0, 1), (0, 0, 1))
    assert (hc.joint_a, hc.joint_b, hc.flags, hc.p0, hc.p1) == (13, 0, DROP_UP, 0.0, 0.0)
    assert [(f.joint_a, f.weight, f.flags, f.dir, f.point) for f in (f0, f1)] == [(j, 1.5, ONE_SIDED, (0, 1, 0), (0, 0.02, 0)) for j in (4, 8)]
    assert [(d.joint_a, d.joint_b, d.flags, d.p0, d.p1) for d in (d0, d1)] == [(0, j, DROP_UP, 0.0, 0.2) for j in (3, 7)]
    assert len(Terms.from_constraints(Constraints(w_head_hips_colinear=1.0))) == 1
    assert len(Terms.from_constraints(Constraints())) == 0
    t.check()


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    ctx = C.c_void_p()
    assert lib.dp_debug_host_ctx(C.byref(ctx)) == _lib.DP_OK
    try:
        buf, p, b, prm, r = _args()
        s = _lib.DpTerms(n_terms=0, terms=None)
        assert lib.dp_optimize_terms(ctx, C.byref(b), C.byref(prm), C.byref(s), C.byref(r), None) == _lib.DP_ERR_UNSUPPORTED
    finally:
        lib.dp_destroy(ctx)


def test_table_kernel_keeps_its_register_and_lds_budget(tmp_path):
    """no spill, no scratch, LDS within 76 KB and at most 256 registers (2 waves per SIMD, as the four-term kernel)"""
    notes = _kernel_notes("dp_cons.hip", tmp_path)
    (name, n), = [(k, v) for k, v in notes.items() if "dp_terms_kernel" in k]
    assert n["vspill"] == 0 and n["scratch"] == 0, (name, n)
    assert n["lds"] <= LDS_BUDGET, (name, n)
    assert n["vgpr"] + n["agpr"] <= 256, (name, n)

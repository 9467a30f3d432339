"""CPU: terms on weighted joint combinations (include/dragposer_points.h) -- dragposer_amd.Point / Points and what Terms.check accepts
with them, the header against the C compiler and the binding, the unit's build flags, the three kernels' register and LDS budget, the
refusals of the three entry points on a context without a device, and what the Python layer refuses.  No compute call is made here (the
GPU side is tests/test_hip_points.py, the sanitized walk tests/points_san/main.cpp, run by tests/test_host_san.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as G
from dragposer_amd import Point, Points, _lib
from dragposer_amd.terms import Term, Terms
from test_build_quality import _kernel_notes  # (the flags __graft_entry__ compiles each unit with)
from test_host_san import ROOT
from test_sequence_constraints_abi import _args, _host_ctx
from test_latent_ar_abi import _frames
from test_terms_abi import _table

HDR = os.path.join(ROOT, "include", "dragposer_points.h")
NAMES = ("dp_optimize_terms_points", "dp_optimize_terms_points_skeleton", "dp_optimize_sequence_terms_points")
POINTS_FIELDS = ("struct_size", "reserved0", "n_points", "reserved1", "coeff")
TERMS_LDS, SKEL_TERMS_LDS = 74288, 76464   # dp_cons.h: LDS_BYTES_T; dp_cons_skel.h: SK_LDS_BYTES_T
POINTS_LDS = 4 * 22 * 4 + 8 * 4 * 4 * 4   # dp_cons_points.h: the coefficient table and WPB waves' areas of MAX_POINTS positions


# ---------------------------------------------------------------------------------------------- Python: Point, Points, Terms.check
def test_point_constructors():
    assert Point({4: 0.5, 8: 0.5}).coeffs == Point.midpoint(4, 8).coeffs
    assert Point.midpoint(4, 8).coeffs[4] == 0.5 and sum(Point.midpoint(4, 8).coeffs) == 1.0
    assert Point.midpoint(3, 3).coeffs[3] == 1.0
    assert Point([0.0] * 21 + [1.0]).coeffs[21] == 1.0
    c = Point.centroid()
    assert len(c.coeffs) == 22 and all(abs(m - 1.0 / 22.0) < 1e-15 for m in c.coeffs)
    masses = [float(j + 1) for j in range(22)]
    c = Point.centroid(masses)
    assert abs(sum(c.coeffs) - 1.0) < 1e-12 and abs(c.coeffs[21] / c.coeffs[0] - 22.0) < 1e-9
    for bad in ([1.0] * 21, [1.0] * 23):
        with pytest.raises(ValueError):
            Point(bad)
    with pytest.raises(ValueError):
        Point({22: 1.0})
    with pytest.raises(ValueError):
        Point.centroid([0.0] * 22)
    with pytest.raises(ValueError):
        Point.centroid([1.0] * 21 + [-1.0])
    with pytest.raises(ValueError):
        Point.centroid([1.0] * 21)


def test_points_accept_and_refuse_what_the_header_states():
    ps = Points([Point.centroid(), Point.midpoint(4, 8), {17: 0.5, 21: 0.5}, Point({13: 1.0})])
    ps.check()
    assert len(ps) == 4 and [ps.joint(k) for k in range(4)] == [22, 23, 24, 25]
    with pytest.raises(ValueError):
        ps.joint(4)
    Points([]).check()
    Points([Point({4: 0.50004, 8: 0.5})]).check()  # (a sum within 1e-4)
    with pytest.raises(ValueError, match="at most 4"):
        Points([Point.centroid()] * 5).check()
    with pytest.raises(ValueError, match="point 1: a coefficient is not finite"):
        Points([Point.centroid(), Point({4: float("nan"), 8: 0.5})]).check()
    with pytest.raises(ValueError, match="point 0: a coefficient is not finite"):
        Points([Point({4: float("inf")})]).check()
    for coeffs in ({4: 0.5, 8: 0.5003}, {4: 0.5}, {}):
        with pytest.raises(ValueError, match="point 2: the coefficients sum to"):
            Points([Point.centroid(), Point.midpoint(4, 8), Point(coeffs)]).check()
    s, keep = ps.to_struct()
    assert s.n_points == 4 and s.reserved0 == 0 and s.reserved1 == 0 and s.struct_size == C.sizeof(_lib.DpPoints)
    assert list(keep) == [C.c_float(m).value for p in ps.points for m in p.coeffs]
    s, keep = Points([]).to_struct()
    assert s.n_points == 0 and s.coeff is None


def test_terms_check_takes_point_indices_for_plane_and_distance_only():
    ps = Points([Point.centroid(), Point.midpoint(4, 8)])
    good = [Term.distance(22, 23, hi=0.1, drop_up=True), Term.distance(23, 4, lo=0.05, hi=0.2), Term.distance(22, 22),
            Term.distance(23, point=(0.0, 0.0, 0.0)), Term.plane(23, (0.0, 1.0, 0.0), one_sided=True), Term.distance(3, 22)]
    table = Terms(good, points=ps)
    table.check()
    assert table.has_points and not Terms(good[:0]).has_points and Terms([], points=Points([])).has_points
    assert Terms(good, 1, ps).points is ps  # (the third positional argument)
    assert table.frames(0, 1).points is ps
    for t in good:  # the same terms without the points, and a bare Term.check(), keep today's bound
        with pytest.raises(ValueError, match="outside"):
            Terms([t]).check()
        with pytest.raises(ValueError, match="outside"):
            t.check()
    with pytest.raises(ValueError, match="joint_a 22 outside 0..21"):
        Term(type=_lib.DP_TERM_DISTANCE, joint_a=22, joint_b=0).check()
    for bad, word in ((Term.distance(24, 0), "term 0: joint_a 24 outside 0..23"), (Term.distance(0, 24), "term 0: joint_b 24 outside -1..23"),
                      (Term.plane(26, (0.0, 1.0, 0.0)), "joint_a 26 outside 0..23"),
                      (Term.align(22, (0.0, 0.0, 1.0), dir=(0.0, 1.0, 0.0)), "an ALIGN term cannot name a point"),
                      (Term.align(13, (0.0, 0.0, 1.0), 23, (0.0, 0.0, 1.0)), "an ALIGN term cannot name a point")):
        with pytest.raises(ValueError, match=word):
            Terms([bad], points=ps).check()
    with pytest.raises(ValueError, match="point 0: the coefficients sum to"):
        Terms([], points=Points([Point({4: 0.4})])).check()


def test_python_refuses_what_does_not_go_with_points():
    import types

    import torch

    from dragposer_amd import Gaps, Hold, Holds, Tether, Tethers
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.optimizer import LatentOptimizer

    fake = types.SimpleNamespace(device=torch.device("cpu"))  # (no library, no context: reaching a launch would raise AttributeError)
    T, S = 1, 2
    a = (torch.zeros(S, 24), torch.zeros(T, S, 22, 3), torch.zeros(T, S, 22, 9), None, torch.zeros(S, 22, 2), torch.zeros(S, 22, dtype=torch.uint8),
         torch.zeros(S, 24), (0, 24), torch.zeros(S, 3), torch.zeros(S, 4), torch.zeros(S, 60, 24), torch.zeros(S, 60, 3), torch.zeros(S, 60, 2), (4, 8))
    table = Terms([Term.distance(22, point=(0.0, 0.0, 0.0), hi=0.02)], points=Points([Point.midpoint(4, 8)]))
    layers = dict(holds=Holds([Hold(0, 0.02, 0.05)]), gaps=Gaps(0, 1.0), ar=object(), tethers=Tethers([Tether(0)]))
    for name, value in layers.items():
        with pytest.raises(ValueError, match=f"points does not go with {name}="):
            LatentOptimizer.optimize_sequence(fake, *a, terms=table, **{name: value})
    with pytest.raises(ValueError, match="points does not go with live="):
        LatentOptimizer.optimize_sequence(fake, *a, terms=table, live=True)
    drag = types.SimpleNamespace(temporal=None, S=S, device=torch.device("cpu"))
    for fn, who in ((DragPose.run_frames, "run_frames"), (DragPose.run, "run")):
        for name, value in layers.items():
            with pytest.raises(ValueError, match=f"DragPose.{who}: a table with points does not go with {name}="):
                fn(drag, None, None, None, None, terms=table, **{name: value})
    with pytest.raises(ValueError, match="DragPose.run: a table with points does not go with live="):
        DragPose.run(drag, None, None, None, None, terms=table, live=True)


# ---------------------------------------------------------------------------------------------- the header, the binding, the build
def test_header_declares_the_calls_and_the_library_exports_them():
    text = open(HDR).read()
    assert re.findall(r"^int\s+(dp_\w+)\s*\(", text, flags=re.M) == list(NAMES) == list(_lib.POINT_SYMBOLS)
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name)
    assert re.search(r"#define DP_MAX_POINTS 4\b", text) and _lib.DP_MAX_POINTS == 4
    assert "dp_cons_points.hip" in G.HIP_SOURCES
    assert G.EXTRA_FLAGS.get("dp_cons_points.hip") == G.EXTRA_FLAGS.get("dp_cons_gap.hip")
    assert G.SCHED_OVERRIDE.get("dp_cons_points.hip", "x") == G.SCHED_OVERRIDE.get("dp_cons_gap.hip", "x")


def test_header_states_the_contract():
    text = " ".join(re.sub(r"^ \* ?", "", open(HDR).read(), flags=re.M).split())  # (the comment's text, its line breaks and margin taken out)
    for phrase in ("P_(22+k) = sum_j m_k[j] P_j", "W_(22+k) = g + P_(22+k)", "joint_a and joint_b of a DP_TERM_PLANE or DP_TERM_DISTANCE term may be 22 + k",
                   "dL/dP_j += m_k[j] * dL/dP_(22+k)", "s = fmaf(m_k[j], P_j, s) for j = 0 .. 21 in that order",
                   "a UNIT point (one coefficient 1, the others 0) gives the bits of the same term naming that joint directly",
                   "n_points = 0 included", "The coefficients are HOST data", "no new per-frame status",
                   "a bad struct_size or a non-zero reserved0 or reserved1", "n_points outside 0..DP_MAX_POINTS", "a NULL coeff with n_points > 0",
                   "a coefficient that is not finite", "differs from 1 by more than 1e-4", "joint_a or joint_b is >= 22 + n_points",
                   "a DP_TERM_ALIGN term naming a point", "after what dp_terms refuses and before the skeleton struct",
                   "DP_ERR_UNSUPPORTED from a library built without the kernel",
                   "Not in holds / tethers / gaps / the latent predictor / dp_live_step / the plug-in"):
        assert phrase in text, phrase


def test_layout_and_defaults_match_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "points.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dragposer_points.h"\nint main(void) {\n'
                   'printf("%zu %d\\n", sizeof(dp_points), DP_MAX_POINTS);\n'
                   + "".join(f'printf("%zu\\n", offsetof(dp_points, {f}));\n' for f in POINTS_FIELDS)
                   + 'dp_points p = DP_POINTS_INIT;\n'
                   'printf("%u %u %d %d %d\\n", p.struct_size, p.reserved0, p.n_points, p.reserved1, p.coeff != 0);\nreturn 0; }\n')
    exe = tmp_path / "points"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    assert [int(x) for x in lines[0].split()] == [C.sizeof(_lib.DpPoints), _lib.DP_MAX_POINTS] == [24, 4]
    assert [int(x) for x in lines[1:6]] == [getattr(_lib.DpPoints, f).offset for f in POINTS_FIELDS] == [0, 4, 8, 12, 16]
    p = _lib.DpPoints()
    assert [int(x) for x in lines[-1].split()] == [p.struct_size, 0, 0, 0, 0]
    assert (p.reserved0, p.n_points, p.reserved1, p.coeff) == (0, 0, 0, None)


def test_the_plug_in_library_carries_no_points_unit():
    """the unit goes into libdragposer_hip.so (and the test-only library, which holds every unit but its own dp_host.o) only"""
    if shutil.which("nm") is None or not os.path.exists(G.UNITY_LIB):
        pytest.skip("no nm, or the plug-in library is not built")
    syms = lambda path: subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    for launcher in ("dp_launch_terms_points", "dp_launch_terms_points_skel", "dp_launch_terms_points_seq"):  # (C++ names: mangled)
        assert launcher in syms(G.LIB) and launcher not in syms(G.UNITY_LIB)
    assert "dp_launch_terms_gap_seq" in syms(G.UNITY_LIB)


def test_the_three_kernels_keep_the_budget(tmp_path):
    """hipcc -S with the build's flags: each kernel's LDS is its table kernel's plus the coefficient table and the waves' areas (864
    bytes), two workgroups still fit a CU's 160 KiB; no spill, no scratch, no accumulator registers, at most 256 registers for two waves
    per SIMD"""
    notes = _kernel_notes("dp_cons_points.hip", tmp_path)
    assert len(notes) == 3
    pick = lambda word: [v for k, v in notes.items() if word in k]
    plain, skel, seq = pick("dp_terms_points_kernel"), pick("dp_terms_points_skel_kernel"), pick("dp_terms_points_seq_kernel")
    assert len(plain) == len(skel) == len(seq) == 1
    assert POINTS_LDS == 864
    assert plain[0]["lds"] == TERMS_LDS + POINTS_LDS == 75152
    assert skel[0]["lds"] == seq[0]["lds"] == SKEL_TERMS_LDS + POINTS_LDS == 77328
    for n in notes.values():
        assert 2 * n["lds"] <= 160 * 1024
        assert n["vspill"] == 0 and n["scratch"] == 0 and n["agpr"] == 0, n
        assert n["vgpr"] <= 256, n


# ---------------------------------------------------------------------------------------------- refusals on a context without a device
def _rows():
    D, P, A = _lib.DP_TERM_DISTANCE, _lib.DP_TERM_PLANE, _lib.DP_TERM_ALIGN
    return [dict(type=D, joint_a=22, joint_b=23, weight=2.0, p1=0.1, flags=_lib.DP_TERM_DROP_UP), dict(type=P, joint_a=23, weight=1.0),
            dict(type=D, joint_a=24, joint_b=-1, weight=0.5), dict(type=D, joint_a=4, joint_b=23, weight=1.0, p0=0.05, p1=0.2),
            dict(type=A, joint_a=13, joint_b=0, weight=1.0)]


def _terms(p, rows=None, seq=False):
    rows = rows if rows is not None else _rows()
    arr = _table(rows)
    return _lib.DpTerms(n_terms=len(rows), terms=C.cast(arr, C.c_void_p), global_pos=None if seq else p), arr


def _points(rows=None, **k):
    rows = rows if rows is not None else [Point.centroid().coeffs, Point.midpoint(4, 8).coeffs, Point.midpoint(17, 21).coeffs]
    arr = (C.c_float * max(1, 22 * len(rows)))(*[m for r in rows for m in r])
    s = _lib.DpPoints(n_points=len(rows), coeff=C.cast(arr, C.c_void_p) if rows else None)
    for key, v in k.items():
        setattr(s, key, v)
    return s, arr


@pytest.mark.parametrize("which", (0, 1, 2))
def test_refusals_come_in_the_documented_order_before_any_device_is_touched(which):
    lib = _lib.load()
    fn = getattr(lib, NAMES[which])
    buf, p, _, prm, st, adj, res = _args()
    fr = _frames(p, z_tgt=p)
    batch = _lib.DpBatch(n_frames=4, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
    out = _lib.DpResult(z=p)
    keeps = []

    def call(ctx, terms=None, points=None, params=None, stride=66, null_points=False):
        t, ta = terms if terms is not None else _terms(p, seq=which == 2)
        q, qa = points if points is not None else _points()
        keeps.append((t, ta, q, qa))
        prm_ref = C.byref(params if params is not None else prm)
        q_ref = None if null_points else C.byref(q)
        sk = _lib.DpSkeletonIn(offsets=p.value, stride=stride)
        if which == 0:
            rc = fn(ctx, C.byref(batch), prm_ref, C.byref(t), q_ref, C.byref(out), None)
        elif which == 1:
            rc = fn(ctx, C.byref(batch), prm_ref, C.byref(t), q_ref, C.byref(sk), C.byref(out), None)
        else:
            rc = fn(ctx, 4, p, C.byref(fr), prm_ref, C.byref(t), q_ref, C.byref(sk), C.byref(st), C.byref(adj), C.byref(res), None, None)
        return rc, (lib.dp_last_error(ctx).decode() if ctx else "")

    assert call(None)[0] == _lib.DP_ERR_INVALID
    ctx = _host_ctx(lib)
    try:
        rc, msg = call(ctx, null_points=True)
        assert rc == _lib.DP_ERR_INVALID and "NULL" in msg and "points" in msg and NAMES[which] in msg
        nan_row, off_row = list(Point.midpoint(4, 8).coeffs), list(Point.midpoint(4, 8).coeffs)
        nan_row[7], off_row[4] = float("nan"), 0.6
        cen = Point.centroid().coeffs
        align_rows = _rows()
        align_rows[4] = dict(align_rows[4], joint_a=22)
        far_rows = _rows()
        far_rows[2] = dict(far_rows[2], joint_a=25)
        # each stage names what it refuses, with a later stage's fault present as well
        stages = [(dict(points=_points(struct_size=16, n_points=-1)), "dp_points.struct_size"),
                  (dict(points=_points(reserved0=1, n_points=-1)), "reserved0"),
                  (dict(points=_points(reserved1=1, n_points=-1)), "dp_points.reserved1"),
                  (dict(points=_points(n_points=-1, coeff=None)), "dp_points.n_points -1 outside 0..4"),
                  (dict(points=_points(n_points=5, coeff=None)), "dp_points.n_points 5 outside 0..4"),
                  (dict(points=_points(coeff=None), terms=_terms(p, far_rows, which == 2)), "dp_points.coeff is NULL"),
                  (dict(points=_points([cen, nan_row, off_row])), "point 1: the coefficient of joint 7 is not finite"),
                  (dict(points=_points([cen, off_row, cen]), terms=_terms(p, far_rows, which == 2)), "point 1: the coefficients sum to"),
                  (dict(terms=_terms(p, far_rows[:4] + align_rows[4:], which == 2)), "term 2: index 25 names a point, and dp_points has 3"),
                  (dict(points=_points([])), "term 0: index 23 names a point, and dp_points has 0"),
                  (dict(terms=_terms(p, align_rows, which == 2), params=_lib.DpParams(n_iter=10, lr=-1.0, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)),
                   "term 4: an ALIGN term names a point")]
        for kw, word in stages:
            rc, msg = call(ctx, **kw)
            assert rc == _lib.DP_ERR_INVALID and word in msg and NAMES[which] in msg, (word, msg)
        # what dp_terms refuses comes first; the skeleton struct and Adam come after
        high = _rows()
        high[0] = dict(high[0], joint_a=26)
        rc, msg = call(ctx, terms=_terms(p, high, which == 2), points=_points(n_points=-1))
        assert rc == _lib.DP_ERR_INVALID and "term 0: joint_a 26 outside 0..25" in msg, msg
        if which:
            rc, msg = call(ctx, points=_points(n_points=-1), stride=5)
            assert rc == _lib.DP_ERR_INVALID and "dp_points.n_points" in msg, msg
            rc, msg = call(ctx, stride=5)
            assert rc == _lib.DP_ERR_INVALID and "dp_skeleton_in.stride" in msg, msg
        rc, msg = call(ctx, params=_lib.DpParams(n_iter=10, lr=-1.0, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0))
        assert rc == _lib.DP_ERR_INVALID and "Adam" in msg, msg
        # well-formed: refused only because there is no device
        four = [cen, Point.midpoint(4, 8).coeffs, Point.midpoint(17, 21).coeffs, Point({13: 1.0}).coeffs]
        for kw in (dict(), dict(points=_points([]), terms=_terms(p, _rows()[4:], which == 2)), dict(points=_points([]), terms=_terms(p, [], which == 2)),
                   dict(points=_points(four), terms=_terms(p, far_rows, which == 2))):
            rc, msg = call(ctx, **kw)
            assert rc == _lib.DP_ERR_DEVICE and NAMES[which] in msg, (rc, msg)
        # the existing entry points keep refusing index 22
        t, ta = _terms(p, seq=which == 2)
        if which == 0:
            rc = lib.dp_optimize_terms(ctx, C.byref(batch), C.byref(prm), C.byref(t), C.byref(out), None)
        elif which == 1:
            rc = lib.dp_optimize_terms_skeleton(ctx, C.byref(batch), C.byref(prm), C.byref(t), C.byref(_lib.DpSkeletonIn(offsets=p.value, stride=66)), C.byref(out), None)
        else:
            rc = lib.dp_optimize_sequence_terms(ctx, 4, p, C.byref(fr), C.byref(prm), C.byref(t), None, C.byref(st), C.byref(adj), C.byref(res), None, None)
        assert rc == _lib.DP_ERR_INVALID and "term 0: joint_a 22 outside 0..21" in lib.dp_last_error(ctx).decode()
    finally:
        lib.dp_destroy(ctx)
    del keeps, buf


def test_the_test_only_library_declines():
    if not os.path.exists(G.REF8_LIB):
        pytest.skip("test-only library not built")
    lib = _lib.load(G.REF8_LIB)
    ctx = _host_ctx(lib)
    try:
        buf, p, _, prm, st, adj, res = _args()
        batch = _lib.DpBatch(n_frames=4, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
        out = _lib.DpResult(z=p)
        t, ta = _terms(p)
        q, qa = _points()
        rc = lib.dp_optimize_terms_points(ctx, C.byref(batch), C.byref(prm), C.byref(t), C.byref(q), C.byref(out), None)
        assert rc == _lib.DP_ERR_UNSUPPORTED and "test-only" in lib.dp_last_error(ctx).decode()
    finally:
        lib.dp_destroy(ctx)

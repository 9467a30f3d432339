"""GPU (MI355X): dp_optimize_constrained_skeleton (include/dragposer_constraints.h) and dp_optimize_terms_skeleton
(include/dragposer_terms.h) -- the constrained and term-table optimise loops with per-frame skeletons (dp_cons_skel.hip) -- bit for bit
against the plain calls on one context per skeleton, at the batch sizes where one-frame-per-wave, eight-waves-per-workgroup can go wrong
(1, 8, 9, 37), on another tree, with refused rows, for repeatability and graph capture, and against the real reference's run with one
skeleton per frame (tests/golden/cons_skel*.npz, tools/make_constraint_goldens.py)."""
import os

import numpy as np
import pytest
import torch

import constraints_oracle as CO
import test_hip_constraints as HC  # (helpers; its tests are not collected from here)
from oracle import ref_torch as R
from test_hip_skeleton import MODES, _raw, _skeletons
from test_hip_terms import _rows

pytestmark = pytest.mark.gpu
OUTS = HC.OUTS
EXTRA = {"cons": "loss_extra", "terms": "loss_terms"}
SIZES = (1, 8, 9, 37)  # a lone wave; a full workgroup; one wave into the second; several workgroups, the last one ragged
DEV = "cuda:0"


@pytest.fixture(scope="module")
def xsens():
    """the shipped model: one context with its own skeleton (the mixed launches), one per skeleton (the plain calls they must equal)"""
    from dragposer_amd.optimizer import LatentOptimizer

    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    skels = _skeletons(np.asarray(_raw()["offsets"], np.float32))
    return LatentOptimizer(device=DEV), [LatentOptimizer(device=DEV, arrays=_raw(offsets=s)) for s in skels], skels


def _inputs(B, seed):
    from dragposer_amd.optimizer import to_device_batch

    b, gp = HC._inputs(R.OracleModel(), B, seed=seed)
    return to_device_batch(b, DEV), torch.from_numpy(gp).to(DEV)


def _table(B, head=13):
    """PLANE, DISTANCE and ALIGN, each once from the table alone and once with per-frame rows (s = 0 on every third frame)"""
    from dragposer_amd import Term, Terms

    s = 0.5 ** 0.5
    return Terms([Term.plane(4, (0, 1, 0), (0, 0.02, 0), weight=3.0, one_sided=True),
                  Term.plane(8, (s, s, 0), (0.0, -0.8, 0.0), weight=1.5, per_frame=_rows(B, (0.0, -0.8, 0.0), DEV, 1)),
                  Term.distance(3, 7, lo=0.1, hi=0.3, weight=2.0, drop_up=True),
                  Term.distance(21, point=(0.3, 0.5, 0.2), hi=0.2, weight=0.5, per_frame=_rows(B, (0.3, 0.5, 0.2), DEV, 2)),
                  Term.align(head, (0, 0, 1), 0, (0, 0, 1), threshold=0.5, margin=0.2, drop_up=True),
                  Term.align(head, (1, 0, 0), dir=(0.6, 0.0, 0.8), weight=1.0, per_frame=_rows(B, (0.6, 0.0, 0.8), DEV, 3))])


def _take(terms, rows):
    from dragposer_amd import Term, Terms

    return Terms([Term(**{**t.__dict__, "per_frame": None if t.per_frame is None else t.per_frame[rows].contiguous()}) for t in terms.terms],
                 terms.up_axis)


def _call(opt, which, d, gp, ext, mode, offsets=None, rows=None, **kw):
    """the launch of `which` on frames `rows` (all of them when None): ext = a Constraints or a Terms"""
    if rows is not None:
        d, gp = {k: v[rows].contiguous() for k, v in d.items()}, gp[rows].contiguous()
        ext = _take(ext, rows) if which == "terms" else ext
    if which == "cons":
        return opt.optimize_constrained(**d, constraints=ext, global_pos=gp, lambda_tmp=0.02, offsets=offsets, **MODES[mode], **kw)
    return opt.optimize_terms(**d, terms=ext, global_pos=gp, lambda_tmp=0.02, offsets=offsets, **MODES[mode], **kw)


def _ext(which, B, cons=None, head=13):
    from dragposer_amd import Constraints

    return (cons or Constraints.reference()) if which == "cons" else _table(B, head)


def _mixed(skels, B):
    """[B,22,3]: frame f takes skeleton f % 4 -- every workgroup holds all four"""
    idx = np.arange(B) % len(skels)
    return torch.from_numpy(np.stack([skels[k] for k in idx])).to(DEV), idx


def _assert_equal(got, want, names, rows=None):
    for n in names:
        a = got[n] if rows is None else got[n][rows]
        assert a.shape == want[n].shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                        want[n].view(torch.int32) if a.dtype == torch.float32 else want[n]), n


def _mixed_equals_one_context_per_skeleton(main, refs, skels, which, mode, B, seed, **ext_kw):
    d, gp = _inputs(B, seed)
    ext = _ext(which, B, **ext_kw)
    off, idx = _mixed(skels, B)
    got = _call(main, which, d, gp, ext, mode, offsets=off)
    for k, ref in enumerate(refs):
        if not (idx == k).any():
            continue
        rows = torch.from_numpy(np.nonzero(idx == k)[0]).to(DEV)
        want = _call(ref, which, d, gp, ext, mode, rows=rows)
        torch.cuda.synchronize()
        _assert_equal(got, want, OUTS + (EXTRA[which],), rows)
    assert int(got["status"].abs().sum()) == 0
    assert bool(torch.isfinite(got[EXTRA[which]]).all())
    assert B < 8 or float(got[EXTRA[which]].abs().sum()) > 0.0  # (the terms are active; a lone frame may satisfy all of them)


@pytest.mark.parametrize("mode", ["fixed", "early", "long"])
@pytest.mark.parametrize("which", ["cons", "terms"])
def test_mixed_batch_equals_one_context_per_skeleton(xsens, which, mode):
    """every output of the frames given skeleton X, the extra losses, iters and status included, carries the bits of the plain call on a
    context created with X"""
    main, refs, skels = xsens
    for B in SIZES:
        _mixed_equals_one_context_per_skeleton(main, refs, skels, which, mode, B, seed=30 + B)


@pytest.mark.parametrize("which", ["cons", "terms"])
def test_one_skeleton_for_the_launch_and_the_contexts_own(xsens, which):
    main, refs, skels = xsens
    B = 37
    d, gp = _inputs(B, seed=5)
    ext = _ext(which, B)
    names = OUTS + (EXTRA[which],)
    for mode in ("fixed", "early"):
        want = _call(refs[3], which, d, gp, ext, mode)
        _assert_equal(_call(main, which, d, gp, ext, mode, offsets=torch.from_numpy(skels[3]).to(DEV)), want, names)  # stride 0
        own = _call(main, which, d, gp, ext, mode)
        _assert_equal(_call(main, which, d, gp, ext, mode, offsets=torch.from_numpy(skels[0]).to(DEV)), own, names)
        _assert_equal(_call(main, which, d, gp, ext, mode, offsets=torch.from_numpy(skels[0]).to(DEV).expand(B, 22, 3).contiguous()), own, names)
        assert not torch.equal(own["pos"], want["pos"])  # (the other skeleton does change the answer)


@pytest.mark.parametrize("which", ["cons", "terms"])
def test_mixed_batch_on_another_tree(which):
    """tests/test_hip_topology.py's arms_at_two_levels: other parents, joints with several children; the joints of the terms named as in
    tests/test_hip_constraints.py::test_other_skeleton"""
    from dragposer_amd import Constraints
    from dragposer_amd.optimizer import LatentOptimizer
    from test_hip_topology import TREES, _model_arrays

    tree = "arms_at_two_levels"
    raw = _model_arrays(TREES[tree], seed=len(tree))
    skels = _skeletons(np.asarray(raw["offsets"], np.float32))
    main = LatentOptimizer(device=DEV, arrays=raw)
    refs = [LatentOptimizer(device=DEV, arrays={**raw, "offsets": s}) for s in skels]
    cons = Constraints(w_feet_floor=1.0, w_head_hips_forward=1.0, w_head_hips_colinear=1.0, w_hips_feet_colinear=1.0, head_joint=12,
                       hips_joint=0, floor_joints=(4, 8), foot_joints=(3, 7))
    try:
        for mode, B in (("fixed", 37), ("early", 9)):
            _mixed_equals_one_context_per_skeleton(main, refs, skels, which, mode, B, seed=3, head=12, **(dict(cons=cons) if which == "cons" else {}))
    finally:
        for o in [main] + refs:
            o.close()


@pytest.mark.parametrize("which", ["cons", "terms"])
def test_a_refused_skeleton_row_poisons_its_own_frame_only(xsens, which):
    from dragposer_amd import _lib

    main, _, skels = xsens
    B = 19
    d, gp = _inputs(B, seed=21)
    ext = _ext(which, B)
    off, _ = _mixed(skels, B)
    bad = off.clone()
    bad[5, 7, 1] = float("nan")
    bad[12, 1, 0] = 1e5           # beyond DP_INPUT_LIMIT (a root child's bone)
    bad[3, 0, :] = float("nan")   # row 0 is never read: frame 3 stays clean
    names = OUTS + (EXTRA[which],)
    for mode in ("fixed", "early"):
        clean = _call(main, which, d, gp, ext, mode, offsets=off)
        got = _call(main, which, d, gp, ext, mode, offsets=bad)
        torch.cuda.synchronize()
        keep = torch.ones(B, dtype=torch.bool, device=DEV)
        keep[5] = keep[12] = False
        _assert_equal({n: got[n][keep] for n in names}, {n: clean[n][keep] for n in names}, names)  # frame 3 and the wave neighbours included
        assert int(clean["status"].abs().sum()) == 0
        for f in (5, 12):
            assert got["status"][f].item() == _lib.DP_STATUS_NONFINITE_RESULT | _lib.DP_STATUS_BAD_STATE
            assert got["iters"][f].item() == (1 if mode == "early" else MODES[mode]["n_iter"])  # (as for a refused z0 / cur_rot)
            for n in names:
                if n not in ("iters", "status"):
                    assert bool(torch.isnan(got[n][f]).all()), (n, f)


@pytest.mark.parametrize("which", ["cons", "terms"])
def test_two_launches_and_a_replayed_graph_give_the_same_bits(xsens, which):
    main, _, skels = xsens
    B = 37
    d, gp = _inputs(B, seed=4)
    ext = _ext(which, B)
    off, _ = _mixed(skels, B)
    names = OUTS + (EXTRA[which],)
    a = _call(main, which, d, gp, ext, "early", offsets=off)
    _assert_equal(_call(main, which, d, gp, ext, "early", offsets=off), a, names)
    out = {k: torch.full_like(v, -1) for k, v in a.items()}
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):  # (a first launch outside the capture)
        _call(main, which, d, gp, ext, "early", offsets=off, out=out, outputs=tuple(out))
    torch.cuda.current_stream(DEV).wait_stream(s)
    for v in out.values():
        v.fill_(-1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _call(main, which, d, gp, ext, "early", offsets=off, out=out, outputs=tuple(out))
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal(out, a, names)


_ORACLE = {}


def _oracle_frame(name, g, f, es, tmp):
    """the fp64 oracle (tests/constraints_oracle.py) on the frames of golden `name` that share frame f's skeleton, on a model saved with
    that skeleton: computed once per file and skeleton, for the mechanism check of an excepted frame -> (its result, f's row in it)"""
    from dragposer_amd import Constraints

    k = f % 4  # (make_goldens.skeleton_set: frame b takes skeleton b % 4)
    rows = np.arange(k, len(g["z0"]), 4)
    assert np.array_equal(g["offsets"][rows], np.broadcast_to(g["offsets"][k], (len(rows), 22, 3)))
    if (name, k) not in _ORACLE:
        path = os.path.join(str(tmp), f"{name}_{k}.npz")
        np.savez(path, **_raw(offsets=g["offsets"][k]))
        sub = {key: np.asarray(g[key])[rows] for key in ("z0", "z_tgt", "cur_rot", "tgt_pos", "tgt_rot", "w", "tracked")}
        _ORACLE[name, k] = CO.optimize_constrained(R.OracleModel(path, dtype=torch.float64), sub, Constraints.reference(), g["global_pos"][rows],
                                                   g["meta"]["n_iter"], lam_tmp=0.02, **es)
    return _ORACLE[name, k], int(f // 4)


@pytest.mark.parametrize("which", ["cons", "terms"])
@pytest.mark.parametrize("name", ["cons_skel", "cons_skel_es"])
def test_reference_block_with_per_frame_skeletons_against_the_reference_goldens(xsens, golden_dir, tmp_path_factory, name, which):
    """Constraints.reference() (and the same block written as a table) with offsets= one skeleton per frame, against the real DragPose.run
    with its `# Additional Losses` block on and run(offsets=<that frame's skeleton>) -- the bars of
    tests/test_hip_constraints.py::test_reference_block_against_the_reference_goldens: 0.05 mm per frame, mean 0.002 mm, losses to rtol
    2e-3, equal iteration counts.  Excepted: a frame whose fp64 oracle trajectory passes within 1e-5 of a switch, or (early stop) takes
    a stop decision within rounding of its threshold -- at most two per file, capped at 5 mm.  On the CPU that oracle matches the
    reference's run on every frame of both files (0.0019 mm at the most, equal counts), so the reference itself uses none of the two."""
    from dragposer_amd import Constraints, Terms
    from dragposer_amd.optimizer import to_device_batch

    main = xsens[0]
    g = R.load_golden(os.path.join(golden_dir, f"{name}.npz"))
    mt = g["meta"]
    es = HC.ES if mt["early_stop"] else {}
    cons = Constraints.reference()
    gp = torch.from_numpy(np.ascontiguousarray(g["global_pos"], dtype=np.float32)).to(DEV)
    off = torch.from_numpy(np.ascontiguousarray(g["offsets"], dtype=np.float32)).to(DEV)
    kw = dict(global_pos=gp, n_iter=mt["n_iter"], lambda_tmp=mt["lambda_tmp"], offsets=off, **es)
    if which == "cons":
        out = main.optimize_constrained(**to_device_batch(g, DEV), constraints=cons, **kw)
    else:
        out = main.optimize_terms(**to_device_batch(g, DEV), terms=Terms.from_constraints(cons), **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert (out["status"] == 0).all()
    err = np.linalg.norm(out["pos"] - g["pos"], axis=-1).max(1) * 1000.0
    print(f"{name}/{which}: max {err.max():.5f} mm, mean {err.mean():.6f} mm, iteration counts differing on {(out['iters'] != g['iters']).sum()} frames")
    exc = set()
    tmp = tmp_path_factory.getbasetemp()
    for f in np.nonzero((err > 0.05) | (out["iters"] != g["iters"]))[0]:
        ref, r = _oracle_frame(name, g, int(f), es, tmp)
        lo, hi = sorted((int(out["iters"][f]), int(g["iters"][f])))
        assert ref["kink"][r] < 1e-5 or (es and HC.near_stop_any(ref, r, lo, hi, es)), (f, err[f], out["iters"][f], g["iters"][f], ref["kink"][r])
        exc.add(int(f))
    assert len(exc) <= 2 and err.max() <= 5.0, (sorted(exc), err.max())
    ok = np.ones(len(err), dtype=bool)
    ok[list(exc)] = False
    assert np.array_equal(out["iters"][ok], g["iters"][ok])
    assert err[ok].mean() <= 0.002, err[ok].mean()
    idx = np.arange(len(err)), g["iters"] - 1
    np.testing.assert_allclose(out["loss"][ok], g["loss_hist"][idx][ok], rtol=2e-3, atol=1e-8)
    np.testing.assert_allclose(out[EXTRA[which]][ok].sum(1), g["extra_hist"][idx][ok], rtol=2e-3, atol=1e-7)

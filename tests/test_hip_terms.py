"""GPU (MI355X): dp_optimize_terms (include/dragposer_terms.h) -- a table of user-defined terms in one launch -- against
dp_optimize_constrained (empty table, the reference block as a table), the reference goldens, the fp64 restatement (tests/terms_oracle.py)
for each type and flag with per-frame rows, the decode_fk + torch.optim.Adam loop, another skeleton, for isolation, determinism and
graph capture, and through DragPose.run.  The bars and the kink rule are tests/test_hip_constraints.py's."""
import warnings

import numpy as np
import pytest
import torch

import terms_oracle as TO
import test_hip_constraints as HC  # (helpers and cases; its tests are not collected from here)
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu
OUTS = HC.OUTS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def opts(dev):
    from dragposer_amd.optimizer import LatentOptimizer

    return {"fp32": LatentOptimizer(device=dev), "bf16": LatentOptimizer(device=dev, weight_dtype="bf16")}


def _run(opt, b, gp, terms, dev, **kw):
    from dragposer_amd.optimizer import to_device_batch

    d = to_device_batch(b, dev)
    out = opt.optimize_terms(**d, terms=terms, global_pos=torch.from_numpy(gp).to(dev), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _twin(model, b, gp, terms, frames, n_iter, **kw):
    sub = {k: np.asarray(v)[frames] for k, v in b.items() if k in ("z0", "z_tgt", "cur_rot", "tgt_pos", "tgt_rot", "w", "tracked")}
    sub["z0"] = sub["z0"].astype(np.float64) + 1e-7
    return TO.optimize_terms(model, sub, _sub_terms(terms, frames), np.asarray(gp)[frames], n_iter, lam_tmp=0.02, **kw)["pos"]


def _sub_terms(terms, frames):
    from dragposer_amd import Term, Terms

    ts = []
    for t in terms.terms:
        d = dict(t.__dict__)
        if t.per_frame is not None:
            d["per_frame"] = t.per_frame.detach().cpu()[frames]
        ts.append(Term(**d))
    return Terms(ts, terms.up_axis)


def _rows(B, vec, dev, seed, scale=1.0, noise=0.05):
    """[B,4] fp32 device rows: vec + noise, s in [0, scale) with every third frame at s = 0"""
    g = torch.Generator().manual_seed(seed)
    v = torch.as_tensor(vec, dtype=torch.float32).expand(B, 3) + noise * torch.randn(B, 3, generator=g)
    s = scale * torch.rand(B, 1, generator=g) * (torch.arange(B) % 3 != 0).unsqueeze(1)
    return torch.cat([v, s], 1).contiguous().to(dev)


ES = HC.ES


@pytest.mark.parametrize("early", [False, True])
def test_empty_table_is_the_zero_weight_constrained_kernel(opts, dev, early):
    from dragposer_amd import Constraints, Terms

    model = R.OracleModel()
    b, gp = HC._inputs(model, 512, seed=21)
    kw = dict(n_iter=100, **ES) if early else dict(n_iter=50)
    got = _run(opts["fp32"], b, gp, Terms(), dev, lambda_tmp=0.02, **kw)
    ref = HC._run(opts["fp32"], b, gp, Constraints(), dev, lambda_tmp=0.02, **kw)
    assert got["loss_terms"].shape == (512, 0)
    same = all(np.array_equal(got[k], ref[k], equal_nan=True) for k in OUTS)
    if not same:  # (expected bit-identical: the same code with no term; otherwise held to the bars)
        warnings.warn("empty table: not bit-identical to dp_optimize_constrained with zero weights")
        err = np.linalg.norm(got["pos"] - ref["pos"], axis=-1).max(1) * 1000.0
        assert (err > 0.05).sum() <= 2 and err.max() < 5.0, np.sort(err)[-4:]
    assert (got["status"] == 0).all()


@pytest.mark.parametrize("name", ["cons_s1", "cons_es"])
def test_reference_table_against_the_reference_goldens(opts, dev, golden_dir, name):
    """Terms.from_constraints(Constraints.reference()) against the real DragPose.run with its `# Additional Losses` block on, with the
    bars of test_hip_constraints.py::test_reference_block_against_the_reference_goldens"""
    import os

    import constraints_oracle as CO
    from dragposer_amd import Constraints, Terms
    from dragposer_amd.optimizer import to_device_batch

    g = R.load_golden(os.path.join(golden_dir, f"{name}.npz"))
    mt = g["meta"]
    n_iter = mt["n_iter"]
    es = ES if mt["early_stop"] else {}
    cons = Constraints.reference()
    gpd = torch.from_numpy(np.ascontiguousarray(g["global_pos"], dtype=np.float32)).to(dev)
    out = opts["fp32"].optimize_terms(**to_device_batch(g, dev), terms=Terms.from_constraints(cons), global_pos=gpd, n_iter=n_iter,
                                      lambda_tmp=mt["lambda_tmp"], **es)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert (out["status"] == 0).all()
    ref = CO.optimize_constrained(R.OracleModel(dtype=torch.float64), g, cons, g["global_pos"], n_iter, lam_tmp=0.02, **es)
    err = np.linalg.norm(out["pos"] - g["pos"], axis=-1).max(1) * 1000.0
    exc = set()
    for f in np.nonzero((err > 0.05) | (out["iters"] != g["iters"]))[0]:
        lo, hi = sorted((int(out["iters"][f]), int(g["iters"][f])))
        assert ref["kink"][f] < 1e-5 or (es and HC.near_stop_any(ref, f, lo, hi, es)), (f, err[f], out["iters"][f], g["iters"][f], ref["kink"][f])
        exc.add(int(f))
    assert len(exc) <= 2 and err.max() <= 5.0, (sorted(exc), err.max())
    ok = np.ones(len(err), dtype=bool)
    ok[list(exc)] = False
    assert np.array_equal(out["iters"][ok], g["iters"][ok])
    assert err[ok].mean() <= 0.002, err[ok].mean()
    idx = np.arange(len(err)), g["iters"] - 1
    np.testing.assert_allclose(out["loss"][ok], g["loss_hist"][idx][ok], rtol=2e-3, atol=1e-8)
    np.testing.assert_allclose(out["loss_terms"][ok].sum(1), g["extra_hist"][idx][ok], rtol=2e-3, atol=1e-7)


@pytest.mark.parametrize("wd", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(HC.TERMS))
def test_table_follows_dp_optimize_constrained(opts, dev, case, wd):
    from dragposer_amd import Constraints, Terms

    model = R.OracleModel()
    b, gp = HC._inputs(model, 512, seed=40 + len(case))
    cons = Constraints(**HC.TERMS[case])
    a = HC._run(opts[wd], b, gp, cons, dev, n_iter=30, lambda_tmp=0.02)
    t = _run(opts[wd], b, gp, Terms.from_constraints(cons), dev, n_iter=30, lambda_tmp=0.02)
    assert (t["status"] == 0).all() and (t["iters"] == 30).all()
    err = np.linalg.norm(t["pos"] - a["pos"], axis=-1).max(1) * 1000.0
    assert (err > 0.05).sum() <= 2 and err.max() < 5.0, np.sort(err)[-4:]
    ok = err <= 0.05
    np.testing.assert_allclose(t["loss_terms"][ok].sum(1), a["loss_extra"][ok].sum(1), rtol=2e-3,
                               atol=1e-6 * max(1.0, np.abs(a["loss_extra"]).max()))


def _cases(B, dev):
    from dragposer_amd import Term, Terms

    s = 0.5 ** 0.5
    return {
        "plane_one_sided": Terms([Term.plane(4, (0, 1, 0), (0, 0.02, 0), weight=3.0, one_sided=True)]),  # (feet near world y = 0)
        "plane_tilted_rows": Terms([Term.plane(8, (s, s, 0), (0.0, -0.8, 0.0), weight=1.5, per_frame=_rows(B, (0.0, -0.8, 0.0), dev, 1))]),
        "band": Terms([Term.distance(3, 7, lo=0.3, hi=0.5, weight=3.0), Term.distance(13, 0, lo=0.1, hi=0.2, drop_up=True)], up_axis=2),
        "point_distance_rows": Terms([Term.distance(21, point=(0.3, 0.2, 0.1), lo=0.05, hi=0.1, weight=2.0,
                                                    per_frame=_rows(B, (0.3, 0.2, 0.1), dev, 2, scale=2.0))]),
        "world_align_rows": Terms([Term.align(13, (0, 0, 1), dir=(1, 0, 0), threshold=0.1, margin=0.1, weight=1.2, drop_up=True,
                                              per_frame=_rows(B, (0.0, 0.0, 1.0), dev, 3))]),
        "same_joint": Terms([Term.distance(5, 5, hi=0.0), Term.align(9, (1, 0, 0), 9, (0, 1, 0), margin=0.3, weight=2.0),
                             Term.align(17, (1, 0, 0), 21, (0, 1, 0), margin=-0.2, weight=0.7)]),
    }


@pytest.mark.parametrize("case", ["plane_one_sided", "plane_tilted_rows", "band", "point_distance_rows", "world_align_rows", "same_joint"])
def test_each_type_against_the_fp64_oracle(opts, dev, case):
    model = R.OracleModel(dtype=torch.float64)
    B = 1024
    b, gp = HC._inputs(model, B, seed=60 + len(case))
    terms = _cases(B, dev)[case]
    ref = TO.optimize_terms(model, b, terms, gp, 30, lam_tmp=0.02)
    got = _run(opts["fp32"], b, gp, terms, dev, n_iter=30, lambda_tmp=0.02)
    assert (got["status"] == 0).all() and (got["iters"] == 30).all()
    ok = HC._compare(got, ref, twin=lambda fr: _twin(model, b, gp, terms, fr, 30))
    lt, lr_ = got["loss_terms"][ok], ref["loss_terms"][ok]
    np.testing.assert_allclose(lt, lr_, rtol=2e-3, atol=1e-6 * max(1.0, np.abs(lr_).max()))
    assert np.abs(ref["loss_terms"]).sum() > 0.0
    for i, t in enumerate(terms.terms):  # a frame at s = 0 has the term off
        if t.per_frame is not None:
            off = (t.per_frame[:, 3] == 0).cpu().numpy()
            assert (got["loss_terms"][off, i] == 0).all()


def CUSTOM():
    """a hand above a table, the knees apart, the head facing +x (tools/time_terms.py's custom table)"""
    from dragposer_amd import Term, Terms

    return Terms([Term.plane(17, (0, 1, 0), (0, -0.2, 0), weight=2.0, one_sided=True),
                  Term.distance(2, 6, lo=0.25, hi=10.0, weight=4.0, drop_up=True),
                  Term.align(13, (0, 0, 1), dir=(1, 0, 0), threshold=0.2, margin=0.0, weight=0.5, drop_up=True)])


def test_custom_table_equals_the_decode_fk_adam_loop(opts, dev):
    from dragposer_amd import decode_fk
    from dragposer_amd.optimizer import to_device_batch

    opt = opts["fp32"]
    model = R.OracleModel()
    b, gp = HC._inputs(model, 512, seed=8)
    d = to_device_batch(b, dev)
    g = torch.from_numpy(gp).to(dev)
    terms = CUSTOM()
    n_iter, lam = 30, 0.02
    got = opt.optimize_terms(**d, terms=terms, global_pos=g, n_iter=n_iter, lambda_tmp=lam)
    z = d["z0"].clone().requires_grad_()
    adam = torch.optim.Adam([z], lr=1e-2)
    trk = d["tracked"].float()
    E = trk.sum(1)
    for _ in range(n_iter):
        o = decode_fk(opt, z, d["cur_rot"], outputs=("pos", "rot"))
        lp = (((o["pos"] - d["tgt_pos"]) ** 2).sum(-1) * d["w"][..., 0] * trk).sum(1) / (3.0 * E)
        lr_ = (((o["rot"] - d["tgt_rot"]) ** 2).sum(-1) * d["w"][..., 1] * trk).sum(1) / (9.0 * E)
        lt = lam * ((z - d["z_tgt"]) ** 2).mean(1)
        ex, _ = TO.term_values(terms, o["pos"], o["rot"].reshape(-1, 22, 3, 3), g)
        adam.zero_grad()
        (lp + lr_ + lt + ex.sum(1)).sum().backward()
        adam.step()
    torch.cuda.synchronize()
    assert ex.abs().sum().item() > 0.0
    err = np.linalg.norm(o["pos"].detach().cpu().numpy() - got["pos"].cpu().numpy(), axis=-1).max(1) * 1000.0
    assert (err > 0.05).sum() <= 2 and err.max() < 5.0, np.sort(err)[-4:]
    np.testing.assert_allclose(got["z"].cpu().numpy()[err <= 0.05], z.detach().cpu().numpy()[err <= 0.05], atol=2e-4)


def test_early_stop_counts_the_table(opts, dev):
    model = R.OracleModel(dtype=torch.float64)
    b, gp = HC._inputs(model, 256, seed=77)
    terms = CUSTOM()
    ref = TO.optimize_terms(model, b, terms, gp, 100, lam_tmp=0.02, **ES)
    got = _run(opts["fp32"], b, gp, terms, dev, n_iter=100, lambda_tmp=0.02, **ES)
    ok = HC._compare(got, ref)
    same = got["iters"][ok] == ref["iters"][ok]
    assert same.mean() > 0.99, (np.nonzero(~same)[0], got["iters"][ok][~same], ref["iters"][ok][~same])
    ref0 = TO.optimize_terms(model, b, type(terms)(), gp, 100, lam_tmp=0.02, **ES)  # the terms change where frames stop
    assert (ref0["iters"] != ref["iters"]).any()


def test_other_skeleton(dev, tmp_path):
    from dragposer_amd import Term, Terms
    from dragposer_amd.optimizer import LatentOptimizer
    from test_hip_topology import TREES, _model_arrays

    tree = "arms_at_two_levels"
    raw = _model_arrays(TREES[tree], seed=len(tree))
    path = str(tmp_path / "model.npz")
    np.savez(path, **raw)
    model = R.OracleModel(path, dtype=torch.float64)
    opt = LatentOptimizer(device=dev, arrays=raw)
    B = 256
    b, gp = HC._inputs(model, B, seed=3)
    terms = Terms([Term.plane(4, (0, 1, 0), (0, 0, 0), weight=1.0, one_sided=True), Term.distance(3, 7, lo=0.2, hi=0.4, weight=2.0),
                   Term.align(12, (0, 0, 1), 0, (0, 0, 1), threshold=0.5, margin=0.2, drop_up=True),
                   Term.distance(8, point=(0.1, 0.0, 0.1), hi=0.05, per_frame=_rows(B, (0.1, 0.0, 0.1), dev, 4))])
    ref = TO.optimize_terms(model, b, terms, gp, 20, lam_tmp=0.02)
    got = _run(opt, b, gp, terms, dev, n_iter=20, lambda_tmp=0.02)
    HC._compare(got, ref)


def test_bad_rows_isolation_determinism_and_graph_capture(opts, dev):
    from dragposer_amd import _lib
    from dragposer_amd.optimizer import to_device_batch

    opt = opts["fp32"]
    model = R.OracleModel()
    B = 200
    b, gp = HC._inputs(model, B, seed=4)
    d = to_device_batch(b, dev)
    g = torch.from_numpy(gp).to(dev)
    terms = _cases(B, dev)["point_distance_rows"]
    terms.terms += CUSTOM().terms
    rows = terms.terms[0].per_frame
    kw = dict(n_iter=60, lambda_tmp=0.02, **ES)
    a = opt.optimize_terms(**d, terms=terms, global_pos=g, **kw)
    a2 = opt.optimize_terms(**d, terms=terms, global_pos=g, **kw)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], a2[k]), k
    assert (a["status"] == 0).all()
    good = rows.clone()
    rows[5, 1] = float("nan")
    rows[7, 3] = -1.0
    rows[9, 0] = float("inf")
    rows[3, 3] = 0.0  # (s = 0: the term is off for that frame)
    c = opt.optimize_terms(**d, terms=terms, global_pos=g, **kw)
    torch.cuda.synchronize()
    keep = torch.ones(B, dtype=torch.bool, device=dev)
    keep[[3, 5, 7, 9]] = False
    for k in a:
        assert torch.equal(c[k][keep], a[k][keep]), k
    st = c["status"].cpu().numpy()
    for f in (5, 7, 9):
        assert st[f] == _lib.DP_STATUS_NONFINITE_RESULT | _lib.DP_STATUS_BAD_TARGETS, (f, st[f])
        assert torch.isnan(c["z"][f]).all() and torch.isnan(c["loss"][f]).all() and torch.isnan(c["loss_terms"][f]).all()
    assert st[3] == 0 and c["loss_terms"][3, 0].item() == 0.0
    rows.copy_(good)
    # captured and replayed: the replay reads the rows' contents of replay time
    out = {k: torch.full_like(v, -1) for k, v in a.items()}
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        opt.optimize_terms(**d, terms=terms, global_pos=g, out=out, outputs=tuple(out), **kw)
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.optimize_terms(**d, terms=terms, global_pos=g, out=out, outputs=tuple(out), **kw)
    for v in out.values():
        v.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(out[k], a[k]), k
    rows[:, 1] += 0.3  # new contents, same storage
    fresh = opt.optimize_terms(**d, terms=terms, global_pos=g, **kw)
    graph.replay()
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(out[k], fresh[k]), k
    assert not torch.equal(fresh["pos"], a["pos"])
    rows.copy_(good)


def _seq_run(g, opt, dz=0.0, t_end=None, per_frame=None, **kw):
    """DragPose over the seq6 fixture as test_hip_constraints.py::test_dragpose_run_with_constraints drives it; `per_frame(t, dp)` is
    called before frame t.  -> (poses [T,S,88], gpos [T,S,3], foot world positions [T,S,3] or None, statuses)"""
    from dragposer_amd.drag_pose import DragPose
    from test_temporal import _load_temporal

    mt, cfg = g["meta"], g["meta"]["cfg"]
    K, T = mt["K"], mt["T"] if t_end is None else t_end
    ja = tuple(cfg["joint_adjustment_indices"]) if cfg["enable_joint_adjustment"] else None
    dp = DragPose(opt, _load_temporal(g), g["means_latent"], g["stds_latent"], n_sequences=K)
    dp.set_initial_state(np.asarray(g["z0"], np.float32) + np.float32(dz), np.zeros((K, 3), np.float32), g["init_rot"], g["init_heights"])
    ps, gs, ws, st = [], [], [], []
    for t in range(T):
        if per_frame is not None:
            per_frame(t, dp)
        g0 = dp.current_global_pos.clone()
        pose, gpos = dp.run(g["tgt_pos"][t], g["tgt_rot"][t], g["mask_idx"], g["weights"], offsets=opt.host_model.arrays["offsets"],
                            stop_eps_pos=0.01 * 0.01, stop_eps_rot=0.01, max_iter=100, min_loss_incr=0.00001, learning_rate=1e-2,
                            lambda_rot=1, lambda_temporal=cfg["lambda_temporal"], temporal_future_window=cfg["temporal_future_window"],
                            joint_adjustment_indices=ja, joint_adjustment_weight=cfg["joint_adjustment_weight"], **kw)
        ps.append(pose.cpu().numpy().copy())
        gs.append(gpos.cpu().numpy().copy())
        if "joint_pos" in dp.last:
            ws.append((g0 + dp.last["joint_pos"][:, 4]).cpu().numpy().copy())
        st.append(dp.last["status"].cpu().numpy().copy() if "status" in dp.last else None)
    return np.stack(ps), np.stack(gs), (np.stack(ws) if ws else None), st


def test_dragpose_run_with_terms(dev, golden_dir):
    import os

    from dragposer_amd import Constraints, Term, Terms
    from dragposer_amd.optimizer import LatentOptimizer

    g = R.load_golden(os.path.join(golden_dir, "seq6.npz"))
    K, T = g["meta"]["K"], g["meta"]["T"]
    opt = LatentOptimizer(device=dev)
    cons = Constraints.reference()
    with pytest.raises(ValueError):
        _seq_run(g, opt, t_end=1, constraints=cons, terms=Terms())
    _, g_plain, _, _ = _seq_run(g, opt)
    _, g_twin, _, _ = _seq_run(g, opt, dz=1e-7)
    p_c, g_c, _, _ = _seq_run(g, opt, constraints=cons)
    p_t, g_t, _, st = _seq_run(g, opt, terms=Terms.from_constraints(cons))
    assert np.isfinite(p_t).all() and np.isfinite(g_t).all() and all(int(s.max()) == 0 for s in st)
    dg = np.abs(g_t - g_c).reshape(T, -1).max(1) * 1000.0
    tw = np.maximum.accumulate(np.abs(g_twin - g_plain).reshape(T, -1).max(1) * 1000.0)
    assert (dg <= 2.0 * tw + 0.05).all(), (np.nonzero(dg > 2.0 * tw + 0.05)[0][:5], dg.max(), tw.max())

    # a foot lock: joint 4 pinned (a point-DISTANCE soft pin) where it was at frame t0, on for frames t0+1 .. t1, off elsewhere
    t0, t1 = T // 4, T // 4 + max(4, T // 4)
    rows = torch.zeros(K, 4, device=dev)
    lock = Terms([Term.distance(4, point=(0.0, 0.0, 0.0), hi=0.0, weight=50.0, per_frame=rows)])
    free_poses, _, w_free, _ = _seq_run(g, opt, terms=Terms([Term.distance(4, point=(0.0, 0.0, 0.0), hi=0.0, weight=0.0)]))
    pinned = {}

    def per_frame(t, dp):
        if t == t0 + 1:
            pinned["at"] = torch.from_numpy(w_free[t0]).to(dev)
        on = t0 < t <= t1
        rows[:, :3] = pinned["at"] if on else 0.0
        rows[:, 3] = 1.0 if on else 0.0

    _, _, w_lock, st = _seq_run(g, opt, terms=lock, per_frame=per_frame)
    assert all(int(s.max()) == 0 for s in st) and np.isfinite(w_lock).all()
    drift_lock = np.linalg.norm(w_lock[t0 + 1:t1 + 1] - w_free[t0], axis=-1).max()
    drift_free = np.linalg.norm(w_free[t0 + 1:t1 + 1] - w_free[t0], axis=-1).max()
    assert drift_lock < (0.5 if drift_free > 0.02 else 1.0) * drift_free, (drift_lock, drift_free)
    np.testing.assert_array_equal(w_lock[:t0 + 1], w_free[:t0 + 1])  # (rows off: the same frames, bit for bit)

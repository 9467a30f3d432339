"""GPU (MI355X): terms on weighted joint combinations (include/dragposer_points.h) -- dp_optimize_terms_points and its skeleton and
sequence forms.  Unit points against the same terms naming the joints (bit for bit, at one, two and three workgroups, with early stop,
with per-frame and single skeletons), true combinations against the fp64 restatement (tests/points_oracle.py) with
tests/test_hip_constraints.py's bars, the decode_fk + torch.optim.Adam loop, run_frames against per-frame run() across a prediction
(bit for bit), determinism, a refused per-frame row, graph capture, and what the Python layer refuses."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import points_oracle as PO
import terms_oracle as TO
import test_hip_constraints as HC  # (helpers and bars; its tests are not collected from here)
import test_hip_terms as HT
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu
ES = HC.ES
FEET, HANDS, HEAD = (4, 8), (17, 21), 13
MASSES = [1.0 + 0.5 * ((3 * j) % 7) for j in range(22)]  # non-uniform, every joint in it


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def opts(dev):
    from dragposer_amd.optimizer import LatentOptimizer

    return {"fp32": LatentOptimizer(device=dev)}


def balance(radius=0.1, weight=3.0, lo=0.0, masses=MASSES):
    """the centre of mass horizontally within `radius` of the midpoint of the feet -> (the term on indices 22 and 23, its two points)"""
    from dragposer_amd import Point, Term

    return Term.distance(22, 23, lo=lo, hi=radius, weight=weight, drop_up=True), [Point.centroid(masses), Point.midpoint(*FEET)]


# ------------------------------------------------------------------------------------------------ 1. unit points are the joints
def _direct(B, dev, rows=True):
    """test_hip_terms' CUSTOM() table plus a joint-joint and a point-DISTANCE term (with per-frame rows): PLANE / DISTANCE on joints 17, 2, 6, 21"""
    from dragposer_amd import Term, Terms

    pf = HT._rows(B, (0.3, 0.2, 0.1), dev, 2, scale=2.0) if rows else None
    return Terms(HT.CUSTOM().terms + [Term.distance(6, 17, lo=0.2, hi=0.6, weight=1.5),
                                      Term.distance(21, point=(0.3, 0.2, 0.1), lo=0.05, hi=0.1, weight=2.0, per_frame=pf)])


def _as_unit_points(table):
    """every PLANE / DISTANCE joint of `table` renamed to a unit point: four points, indices 22..25"""
    from dragposer_amd import Point, Points, Terms
    from dragposer_amd.terms import ALIGN

    joints = sorted({j for t in table.terms if t.type != ALIGN for j in (t.joint_a, t.joint_b) if j >= 0})
    assert joints == [2, 6, 17, 21]
    idx = {j: 22 + k for k, j in enumerate(joints)}
    ren = lambda t: t if t.type == ALIGN else replace(t, joint_a=idx[t.joint_a], joint_b=idx.get(t.joint_b, -1))
    return Terms([ren(t) for t in table.terms], table.up_axis, Points([Point({j: 1.0}) for j in joints]))


def _both(opt, B, dev, seed, offsets=None, **kw):
    from dragposer_amd.optimizer import to_device_batch

    b, gp = HC._inputs(R.OracleModel(), B, seed=seed)
    d, g = to_device_batch(b, dev), torch.from_numpy(gp).to(dev)
    direct = _direct(B, dev)
    a = opt.optimize_terms(**d, terms=direct, global_pos=g, lambda_tmp=0.02, offsets=offsets, **kw)
    u = opt.optimize_terms(**d, terms=_as_unit_points(direct), global_pos=g, lambda_tmp=0.02, offsets=offsets, **kw)
    torch.cuda.synchronize()
    return a, u


@pytest.mark.parametrize("early", (False, True), ids=("fixed", "early"))
@pytest.mark.parametrize("B", (1, 9, 17))
def test_unit_points_are_the_joints_bit_for_bit(opts, dev, B, early):
    """B = 1, 9, 17 with 8 waves per workgroup: a lone wave, a second workgroup holding one frame, a third"""
    a, u = _both(opts["fp32"], B, dev, 90 + B, **(dict(n_iter=60, **ES) if early else dict(n_iter=30)))
    assert set(a) == set(u) and "loss_terms" in a
    for k in a:
        assert torch.equal(a[k], u[k]), k
    assert int(a["status"].max()) == 0 and float(a["loss_terms"].abs().sum()) > 0.0
    if early and B > 1:
        assert int(a["iters"].min()) < 60


@pytest.mark.parametrize("per_frame", (True, False), ids=("per_frame", "single"))
def test_unit_points_with_skeletons(opts, dev, per_frame):
    opt, B = opts["fp32"], 17
    own = torch.from_numpy(opt.host_model.arrays["offsets"]).to(dev).reshape(22, 3).contiguous()
    scale = torch.tensor([1.0, 0.93, 1.06], device=dev)[torch.arange(B, device=dev) % 3]
    offsets = (own[None] * scale[:, None, None]).contiguous() if per_frame else (own * 1.04).contiguous()
    a, u = _both(opt, B, dev, 77, offsets=offsets, n_iter=30)
    plain, _ = _both(opt, B, dev, 77, n_iter=30)
    for k in a:
        assert torch.equal(a[k], u[k]), k
    assert int(a["status"].max()) == 0 and not torch.equal(a["pos"], plain["pos"])  # (the bones are in use)


def test_a_table_without_points_is_dp_optimize_terms(opts, dev):
    """through the new entry point with n_points = 0, and with a point no term names"""
    from dragposer_amd import Point, Points, Terms
    from dragposer_amd.optimizer import to_device_batch

    opt, B = opts["fp32"], 17
    b, gp = HC._inputs(R.OracleModel(), B, seed=12)
    d, g = to_device_batch(b, dev), torch.from_numpy(gp).to(dev)
    direct = _direct(B, dev)
    calls = []
    inner = opt.lib.dp_optimize_terms_points
    a = opt.optimize_terms(**d, terms=direct, global_pos=g, lambda_tmp=0.02, n_iter=60, **ES)
    for pts in (Points([]), Points([Point.centroid(MASSES)])):
        table = Terms(direct.terms, direct.up_axis, pts)
        assert table.has_points
        opt.lib.dp_optimize_terms_points = lambda *x: (calls.append(len(pts)), inner(*x))[1]
        try:
            n = opt.optimize_terms(**d, terms=table, global_pos=g, lambda_tmp=0.02, n_iter=60, **ES)
        finally:
            opt.lib.dp_optimize_terms_points = inner
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], n[k]), (len(pts), k)
    assert calls == [0, 1]


# ------------------------------------------------------------------------------------------------ 2. true combinations against fp64
B2, N2 = 256, 30
# a seed per case: the fp64 oracle's own fp32 twin stays within test_hip_constraints._compare's bars at it (checked on the CPU with
# tools/points_seeds.py, which runs exactly the comparison below with the fp32 oracle in the kernel's place)
SEEDS = {"balance": 101, "hands_rows": 102, "plane_midpoint": 103, "member_joint": 104, "same_point": 105}


def cases(B, dev):
    """-> {name: (table, the index of the term under test)}.  Each point has more than two member joints, so that the gradient of its term
    reaches more than two: the hands' and the feet's midpoints are taken over both joints of each hand (16, 17 / 20, 21) and each foot
    (3, 4 / 7, 8)."""
    from dragposer_amd import Point, Points, Term, Terms

    bal, bal_pts = balance(radius=0.1, weight=3.0, lo=0.03)
    hands = Point({16: 0.15, 17: 0.35, 20: 0.15, 21: 0.35})
    feet = Point({3: 0.25, 4: 0.25, 7: 0.25, 8: 0.25})
    com = Point.centroid(MASSES)
    return {
        "balance": (Terms([bal], 1, Points(bal_pts)), 0),
        "hands_rows": (Terms([Term.distance(22, point=(0.3, 0.2, 0.1), lo=0.05, hi=0.1, weight=2.0,
                                            per_frame=HT._rows(B, (0.3, 0.2, 0.1), dev, 2, scale=2.0))], 1, Points([hands])), 0),
        "plane_midpoint": (Terms([Term.plane(22, (0, 1, 0), (0, 0.1, 0), weight=3.0, one_sided=True)], 1, Points([feet])), 0),
        "member_joint": (Terms([Term.distance(22, HEAD, lo=0.2, hi=0.3, weight=2.0)], 1, Points([com])), 0),
        "same_point": (Terms([Term.distance(22, 22, lo=0.0, hi=0.1, weight=5.0)], 1, Points([com])), 0),
    }


def _sub_terms(terms, frames):
    sub = HT._sub_terms(terms, frames)
    return type(terms)(sub.terms, terms.up_axis, terms.points)


def oracle_twin(model, b, gp, terms, frames, n_iter):
    sub = {k: np.asarray(v)[frames] for k, v in b.items() if k in ("z0", "z_tgt", "cur_rot", "tgt_pos", "tgt_rot", "w", "tracked")}
    sub["z0"] = sub["z0"].astype(np.float64) + 1e-7
    return PO.optimize_terms(model, sub, _sub_terms(terms, frames), np.asarray(gp)[frames], n_iter, lam_tmp=0.02)["pos"]


def compare(got, ref, model, b, gp, terms, i):
    """test_each_type_against_the_fp64_oracle's comparison: _compare, unchanged, and rtol = 2e-3 on loss_terms"""
    ok = HC._compare(got, ref, twin=lambda fr: oracle_twin(model, b, gp, terms, fr, N2))
    lt, lr_ = got["loss_terms"][ok], ref["loss_terms"][ok]
    np.testing.assert_allclose(lt, lr_, rtol=2e-3, atol=1e-6 * max(1.0, np.abs(lr_).max()))
    return ok


@pytest.mark.parametrize("case", list(SEEDS))
def test_true_combinations_against_the_fp64_oracle(opts, dev, case):
    model = R.OracleModel(dtype=torch.float64)
    b, gp = HC._inputs(model, B2, seed=SEEDS[case])
    terms, i = cases(B2, dev)[case]
    ref = PO.optimize_terms(model, b, terms, gp, N2, lam_tmp=0.02)
    got = HT._run(opts["fp32"], b, gp, terms, dev, n_iter=N2, lambda_tmp=0.02)
    assert (got["status"] == 0).all() and (got["iters"] == N2).all()
    compare(got, ref, model, b, gp, terms, i)
    off = HT._run(opts["fp32"], b, gp, type(terms)([replace(terms.terms[i], weight=0.0)], terms.up_axis, terms.points), dev, n_iter=N2, lambda_tmp=0.02)
    if case == "same_point":  # V - V: the value and the gradient are exactly 0
        assert (got["loss_terms"] == 0).all() and (ref["loss_terms"] == 0).all()
        for k in ("z", "pos", "rot", "loss", "pose"):
            assert np.array_equal(got[k], off[k]), k
        return
    assert got["loss_terms"][:, i].sum() > 0.0 and ref["loss_terms"][:, i].sum() > 0.0
    pos, rot = torch.from_numpy(ref["pos"]), torch.from_numpy(ref["rot"]).reshape(B2, 22, 3, 3)
    reach = PO.joints_reached(terms, i, pos, rot, torch.from_numpy(gp).double()).numpy()
    assert reach.max() > 2 and (reach[ref["loss_terms"][:, i] > 0] > 2).all(), reach
    assert not np.array_equal(got["z"], off["z"])  # the term moves the solution
    for t in terms.terms:  # a frame at s = 0 has the term off
        if t.per_frame is not None:
            assert (got["loss_terms"][(t.per_frame[:, 3] == 0).cpu().numpy(), i] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. the decode_fk + Adam loop
def test_balance_table_equals_the_decode_fk_adam_loop(opts, dev):
    """test_hip_terms.test_custom_table_equals_the_decode_fk_adam_loop with the balance term added in PyTorch; its bars"""
    from dragposer_amd import Points, Terms, decode_fk
    from dragposer_amd.optimizer import to_device_batch

    opt = opts["fp32"]
    b, gp = HC._inputs(R.OracleModel(), 128, seed=8)
    d = to_device_batch(b, dev)
    g = torch.from_numpy(gp).to(dev)
    bal, pts = balance(radius=0.1, weight=3.0)
    terms = Terms(HT.CUSTOM().terms + [bal], 1, Points(pts))
    n_iter, lam = 30, 0.02
    got = opt.optimize_terms(**d, terms=terms, global_pos=g, n_iter=n_iter, lambda_tmp=lam)
    z = d["z0"].clone().requires_grad_()
    adam = torch.optim.Adam([z], lr=1e-2)
    trk = d["tracked"].float()
    E = trk.sum(1)
    M = PO.coeff_matrix(terms.points, torch.float32, dev)
    for _ in range(n_iter):
        o = decode_fk(opt, z, d["cur_rot"], outputs=("pos", "rot"))
        lp = (((o["pos"] - d["tgt_pos"]) ** 2).sum(-1) * d["w"][..., 0] * trk).sum(1) / (3.0 * E)
        lr_ = (((o["rot"] - d["tgt_rot"]) ** 2).sum(-1) * d["w"][..., 1] * trk).sum(1) / (9.0 * E)
        lt = lam * ((z - d["z_tgt"]) ** 2).mean(1)
        ex, _ = TO.term_values(Terms(terms.terms[:-1]), o["pos"], o["rot"].reshape(-1, 22, 3, 3), g)
        u = torch.einsum("j,bjc->bc", M[0] - M[1], o["pos"])[:, [0, 2]]  # the balance term, written out: h(com - support), up = y
        bt = bal.weight * torch.relu((u ** 2).sum(-1) - bal.p1 ** 2)
        adam.zero_grad()
        (lp + lr_ + lt + ex.sum(1) + bt).sum().backward()
        adam.step()
    torch.cuda.synchronize()
    assert ex.abs().sum().item() > 0.0 and bt.sum().item() > 0.0
    err = np.linalg.norm(o["pos"].detach().cpu().numpy() - got["pos"].cpu().numpy(), axis=-1).max(1) * 1000.0
    assert (err > 0.05).sum() <= 2 and err.max() < 5.0, np.sort(err)[-4:]
    np.testing.assert_allclose(got["z"].cpu().numpy()[err <= 0.05], z.detach().cpu().numpy()[err <= 0.05], atol=2e-4)


# ------------------------------------------------------------------------------------------------ 4. sequences
def test_run_frames_equals_the_loop_of_run_across_a_prediction():
    """S = 3, T = 20, a seeded predictor with window 8: run_frames(terms=<with points>, offsets=<per sequence>) cuts 8 / 8 / 4, each one
    call of optimize_sequence through dp_optimize_sequence_terms_points, and equals per-frame run() on poses, positions, counts and the
    whole state.  The table: the balance term and the hands' midpoint pinned to [T,S,4] rows."""
    from dragposer_amd import Point, Points, Term, Terms
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.temporal import TemporalPredictor
    from test_hip_sequence_constraints import HJ, _clip, _opt, _row

    S, T = 3, 20
    c, opt = _clip(S, T), _opt()
    bal, pts = balance(radius=0.05, weight=3.0)
    rows = c.rows.clone()
    rows[5, 1, 3] = 0.0  # (one frame of one sequence with the pin off)
    table = Terms([bal, Term.distance(24, point=(0.0, 0.0, 0.0), lo=0.0, hi=0.05, weight=1.5, per_frame=rows)], 1,
                  Points(pts + [Point.midpoint(*HANDS)]))
    own = torch.from_numpy(opt.host_model.arrays["offsets"]).to(opt.device).reshape(22, 3).contiguous()
    mixed = (own[None] * torch.tensor([1.0, 0.95, 1.05], device=opt.device)[:, None, None]).contiguous()
    torch.manual_seed(5)
    predictor = TemporalPredictor(n_encoder_layers=1, n_decoder_layers=1, dim_feedforward=16)
    idx = np.array(R.TRACK6)
    wts = np.array([R.W6[j] for j in R.TRACK6], np.float32)
    kw = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2, max_iter=10, min_loss_incr=1e-5, learning_rate=1e-2, lambda_rot=1, lambda_temporal=0.02,
              temporal_future_window=8, height_indices=HJ, joint_adjustment_indices=(0, 3), joint_adjustment_weight=0.5, offsets=mixed)
    dps = []
    for _ in range(2):
        dp = DragPose(opt, predictor, np.zeros(24), np.ones(24), n_sequences=S, native_temporal=True)
        dp.set_initial_state(c.z0, np.zeros((S, 3), np.float32), c.rot0, c.heights0)
        dps.append(dp)
    a, b = dps
    tp, tR = c.tgt_pos[:, :, idx], c.tgt_rot[:, :, idx].reshape(T, S, -1, 3, 3)
    pa, ga, ia, la = [], [], [], []
    frame_calls = []
    inner = opt.lib.dp_optimize_terms_points_skeleton
    opt.lib.dp_optimize_terms_points_skeleton = lambda *x: (frame_calls.append(1), inner(*x))[1]
    try:
        for t in range(T):
            frame = table.frames(t, t + 1)
            pose, gpos = a.run(tp[t], tR[t], idx, wts, terms=Terms([_row(x) for x in frame.terms], 1, table.points), **kw)
            pa.append(pose.clone()); ga.append(gpos.clone()); ia.append(a.last["iters"].clone()); la.append(a.last["loss_terms"].clone())
    finally:
        opt.lib.dp_optimize_terms_points_skeleton = inner
    calls, seq_calls = [], []
    seq, inner_seq = opt.optimize_sequence, opt.lib.dp_optimize_sequence_terms_points
    opt.optimize_sequence = lambda *x, **k: (calls.append((int(x[1].shape[0]), k["terms"].has_points, k.get("offsets") is not None)), seq(*x, **k))[1]
    opt.lib.dp_optimize_sequence_terms_points = lambda *x: (seq_calls.append(1), inner_seq(*x))[1]
    try:
        pb, gb, ib = b.run_frames(tp, tR, idx, wts, terms=table, **kw)
    finally:
        del opt.optimize_sequence
        opt.lib.dp_optimize_sequence_terms_points = inner_seq
    torch.cuda.synchronize()
    assert calls == [(8, True, True), (8, True, True), (4, True, True)] and len(seq_calls) == 3 and len(frame_calls) == T
    assert torch.equal(torch.stack(pa), pb) and torch.equal(torch.stack(ga), gb) and torch.equal(torch.stack(ia), ib)
    assert torch.equal(torch.stack(la), b.last_terms)
    for attr in ("latent", "current_global_pos", "current_global_rot", "latent_buffer", "displacement_buffer", "heights_buffer", "target_latent_buffer"):
        assert torch.equal(getattr(a, attr), getattr(b, attr)), attr
    assert bool(torch.isfinite(pb).all()) and int(b.last_status.max()) == 0
    assert float(b.last_terms[..., 0].sum()) > 0.0 and float(b.last_terms[..., 1].sum()) > 0.0 and float(b.last_terms[5, 1, 1]) == 0.0
    assert int(ib.min()) < int(ib.max())  # the early stop ends frames at different counts


# ------------------------------------------------------------------------------------------------ 5. misc
def test_bad_rows_isolation_determinism_and_graph_capture(opts, dev):
    from dragposer_amd import _lib
    from dragposer_amd.optimizer import to_device_batch

    opt, B = opts["fp32"], 40
    b, gp = HC._inputs(R.OracleModel(), B, seed=4)
    d, g = to_device_batch(b, dev), torch.from_numpy(gp).to(dev)
    terms, _ = cases(B, dev)["hands_rows"]
    bal, pts = balance()
    terms = type(terms)(terms.terms + [replace(bal, joint_a=23, joint_b=24)], 1, type(terms.points)(terms.points.points + pts))
    rows = terms.terms[0].per_frame
    kw = dict(n_iter=60, lambda_tmp=0.02, **ES)
    a = opt.optimize_terms(**d, terms=terms, global_pos=g, **kw)
    a2 = opt.optimize_terms(**d, terms=terms, global_pos=g, **kw)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], a2[k]), k
    assert (a["status"] == 0).all() and float(a["loss_terms"][:, 0].sum()) > 0.0 and float(a["loss_terms"][:, 1].sum()) > 0.0
    good = rows.clone()
    rows[5, 1] = float("nan")
    rows[7, 3] = -1.0
    rows[9, 0] = float("inf")
    c = opt.optimize_terms(**d, terms=terms, global_pos=g, **kw)
    torch.cuda.synchronize()
    keep = torch.ones(B, dtype=torch.bool, device=dev)
    keep[[5, 7, 9]] = False
    for k in a:
        assert torch.equal(c[k][keep], a[k][keep]), k
    st = c["status"].cpu().numpy()
    for f in (5, 7, 9):
        assert st[f] == _lib.DP_STATUS_NONFINITE_RESULT | _lib.DP_STATUS_BAD_TARGETS, (f, st[f])
        assert torch.isnan(c["z"][f]).all() and torch.isnan(c["loss"][f]).all() and torch.isnan(c["loss_terms"][f]).all()
    rows.copy_(good)
    # captured and replayed: the coefficients travel in the launch, the rows are read at replay time
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


def test_dragpose_refuses_the_sequence_layers_with_points(dev):
    from dragposer_amd import Gaps, Hold, Holds, Points, Tether, Tethers, Terms
    from dragposer_amd.drag_pose import DragPose
    from test_hip_sequence_constraints import _clip, _opt

    c = _clip(3, 2)
    bal, pts = balance()
    table = Terms([bal], 1, Points(pts))
    dp = DragPose(_opt(), None, np.zeros(24), np.ones(24), n_sequences=3)
    dp.set_initial_state(c.z0, np.zeros((3, 3), np.float32), c.rot0, c.heights0)
    idx = np.array(R.TRACK6)
    wts = np.array([R.W6[j] for j in R.TRACK6], np.float32)
    tp, tR = c.tgt_pos[0][:, idx], c.tgt_rot[0][:, idx].reshape(3, -1, 3, 3)
    for name, value in (("holds", Holds([Hold(0, 0.02, 0.05)])), ("gaps", Gaps(0, 1.0)), ("ar", object()), ("tethers", Tethers([Tether(0)])),
                        ("live", True)):
        with pytest.raises(ValueError, match="points"):
            dp.run(tp, tR, idx, wts, terms=table, **{name: value})

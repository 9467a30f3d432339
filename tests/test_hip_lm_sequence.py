"""GPU (MI355X): dp_optimize_sequence_lm (include/dragposer_sequence_lm.h) -- dp_optimize_lm's frame with the step loop of a sequence on the
device -- against the per-frame composition the header names, done by hand: optimize_lm with the carried latent, global rotation and mu and
the step's (shifted) targets, then sequence_advance, then the latent copy.  The same arithmetic in the same order: every comparison is bit
for bit (NaN where NaN); no tolerance is involved.  Then the faults the contract names, and the two routes through DragPose."""
import functools
import os
import types

import numpy as np
import pytest
import torch

import lm_oracle as LO
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu

T, H = 7, 4
HJ = (0, 4, 8, 13, 17, 21)
ADJ = (0, 13, 0.5)  # (joint 13 carries a tracker in the 6- and the 3-tracker recipe)
LAM = 0.02
EPS = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2)
OUT_KEYS = ("pose_ret", "pos_ret", "world_rot", "iters", "loss", "status", "scratch", "mu_trace", "n_accepted", "loss0", "joint_pos")
STATE_KEYS = ("latent", "gpos", "grot", "lbuf", "dbuf", "hbuf", "mu")
BAD_STATE, BAD_TARGETS, NONFINITE = 2, 4, 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _opt(dtype="fp32"):
    from dragposer_amd.optimizer import LatentOptimizer

    return LatentOptimizer(device="cuda:0", weight_dtype=dtype)


def _lms():
    from dragposer_amd import LM

    return {"six": LM(steps=6, early_stop=False), "three": LM(3)}


@functools.lru_cache(maxsize=None)
def _clip(recipe, S):
    """T x S frames of the recipe (seed 11) as a clip of S sequences: targets and z_tgt rows [T,S], the trackers of the first S frames held for
    all steps, the first S frames' warm start and rotation, a target root trajectory and a start position of its own draw"""
    m64 = R.OracleModel(dtype=torch.float64)
    kw = dict(trackers=3 if recipe[0] == "3" else 6)
    b = LO.warm_inputs(m64, T * S, seed=11, **kw) if recipe.endswith("warm") else R.synth_inputs(m64, T * S, seed=11, **kw)
    d = "cuda:0"
    t = lambda k, *shape: torch.from_numpy(np.ascontiguousarray(b[k])).to(d).reshape(*shape).contiguous()
    g = torch.Generator(device="cpu").manual_seed(17 + S)
    return types.SimpleNamespace(
        S=S, tgt_pos=t("tgt_pos", T, S, 22, 3), tgt_rot=t("tgt_rot", T, S, 22, 9), z_tgt=t("z_tgt", T, S, 24), w=t("w", T, S, 22, 2)[0].contiguous(),
        tracked=t("tracked", T, S, 22)[0].contiguous(), z0=t("z0", T, S, 24)[0].contiguous(), grot=t("cur_rot", T, S, 4)[0].contiguous(),
        gpos=(0.5 * torch.randn(S, 3, generator=g)).to(d), root=torch.cumsum(0.02 * torch.randn(T, S, 3, generator=g), dim=0).to(d),
        lbuf=(0.3 * torch.randn(S, H, 24, generator=g)).to(d), dbuf=(0.01 * torch.randn(S, H, 3, generator=g)).to(d),
        hbuf=torch.rand(S, H, len(HJ), generator=g).to(d))


def _state(c, mu0=1e-2):
    return types.SimpleNamespace(latent=c.z0.clone(), gpos=c.gpos.clone(), grot=c.grot.clone(), lbuf=c.lbuf.clone(), dbuf=c.dbuf.clone(),
                                 hbuf=c.hbuf.clone(), mu=torch.full((c.S,), mu0, device=c.z0.device))


@functools.lru_cache(maxsize=None)
def _ar(K):
    from dragposer_amd import LatentAR

    if K == 1:
        return LatentAR.hold()
    A = np.random.default_rng(23).uniform(-0.49, 0.49, (K, 24, 24)) / np.sqrt(24.0 * K)  # a fixed random A, |A| < 0.5
    assert np.abs(A).max() < 0.5
    return LatentAR(A, 0.05 * np.random.default_rng(24).standard_normal(24))


def _per_frame(opt, c, st, lm, t0=0, n=T, ar=None, root=True, adj=ADJ, tgt_pos=None, z_tgt=None):
    """the composition, frame by frame on the host -> the outputs of frames t0 .. t0 + n (with the z_tgt rows used); st is advanced in place"""
    S, d = c.S, opt.device
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    z_tgt = c.z_tgt if z_tgt is None else z_tgt
    o = {k: [] for k in OUT_KEYS + ("z_tgt",)}
    nan = torch.full((S, 24), float("nan"), device=d)
    for t in range(t0, t0 + n):
        zt = ar.predict(st.lbuf) if ar is not None else z_tgt[t].contiguous()
        tp = (tgt_pos[t] + (c.root[t] - st.gpos).unsqueeze(1)).contiguous() if root else tgt_pos[t]
        fr = opt.optimize_lm(st.latent, zt, st.grot, tp, c.tgt_rot[t], c.w, c.tracked, lm=lm, lambda_rot=1.0, lambda_tmp=LAM, mu=st.mu, **EPS)
        pose, pos = torch.empty(S, 88, device=d), torch.empty(S, 3, device=d)
        opt.sequence_advance(fr, st.gpos, st.grot, st.lbuf, st.dbuf, st.hbuf, HJ, pose_ret=pose, pos_ret=pos, adjust=adj,
                             tgt_pos=tp if adj is not None else None)
        st.latent.copy_(fr["z"])
        bad_state = (fr["status"] & BAD_STATE) != 0  # (such a step used no target: the header's NaN row)
        for k, v in (("pose_ret", pose), ("pos_ret", pos), ("world_rot", fr["world_rot"]), ("iters", fr["iters"]), ("loss", fr["loss"]),
                     ("status", fr["status"]), ("scratch", torch.cat((st.lbuf[:, -1], st.dbuf[:, -1], st.hbuf[:, -1]), dim=1)), ("mu_trace", st.mu),
                     ("n_accepted", fr["n_accepted"]), ("loss0", fr["loss0"]), ("joint_pos", fr["pos"]),
                     ("z_tgt", torch.where(bad_state[:, None], nan, zt))):
            o[k].append(v.clone())
    return {k: torch.stack(v) for k, v in o.items()}


def _launch(opt, c, st, lm, t0=0, n=T, ar=None, root=True, adj=ADJ, tgt_pos=None, z_tgt=None, strides=None, outputs=None, null_mu=False):
    """one launch over frames t0 .. t0 + n -> its outputs; st is advanced in place"""
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    sl = slice(t0, t0 + n)
    scratch = torch.empty(n, c.S, 24 + 3 + len(HJ), device=opt.device)
    if ar is not None:
        zt, strides = None, (0, 0)
    elif z_tgt is not None:
        zt = z_tgt
    else:
        zt, strides = c.z_tgt[sl].contiguous(), (c.S * 24, 24)
    o = opt.optimize_sequence_lm(st.latent, tgt_pos[sl].contiguous(), c.tgt_rot[sl].contiguous(), c.root[sl].contiguous() if root else None, c.w,
                                 c.tracked, zt, strides, st.gpos, st.grot, st.lbuf, st.dbuf, st.hbuf, HJ, lm=lm, lambda_rot=1.0, lambda_tmp=LAM,
                                 mu=None if null_mu else st.mu, ar=ar, adjust=adj, scratch=scratch, z_tgt_trace=True if ar is not None else None,
                                 outputs=outputs, **EPS)
    o["scratch"] = scratch
    if ar is not None:
        o["z_tgt"] = o.pop("z_tgt_trace")
    return o


def _same(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return bool(torch.equal(a, b))
    return bool(torch.equal(torch.isnan(a), torch.isnan(b))) and bool(torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)))


def _assert_same(got, exp, keys, what=""):
    get = (lambda x, k: x[k]) if isinstance(exp, dict) else getattr
    bad = [k for k in keys if not _same(get(got, k), get(exp, k))]
    assert not bad, (what, bad)


def _cat(a, b):
    return {k: torch.cat((a[k], b[k])) for k in a if k != "mu"}


VARIANTS = {"root_adjust": dict(), "plain": dict(root=False, adj=None), "ar1": dict(ar=1), "ar2": dict(ar=2, adj=None)}


def _case(recipe, S, which, variant, dtype="fp32"):
    opt, c, lm = _opt(dtype), _clip(recipe, S), _lms()[which]
    kw = dict(VARIANTS[variant])
    if "ar" in kw:
        kw["ar"] = _ar(kw["ar"])
    keys = OUT_KEYS + (("z_tgt",) if "ar" in kw else ())
    est = _state(c)
    exp = _per_frame(opt, c, est, lm, **kw)
    gst = _state(c)
    got = _launch(opt, c, gst, lm, **kw)
    cst = _state(c)
    chained = _cat(_launch(opt, c, cst, lm, 0, 3, **kw), _launch(opt, c, cst, lm, 3, 4, **kw))
    torch.cuda.synchronize()
    what = (recipe, S, which, variant, dtype)
    _assert_same(got, exp, keys, what)
    _assert_same(gst, est, STATE_KEYS, what)
    _assert_same(chained, exp, keys, what + ("3 + 4",))
    _assert_same(cst, est, STATE_KEYS, what + ("3 + 4",))
    assert int(exp["status"].max()) == 0 and bool(torch.isfinite(exp["pose_ret"]).all())
    assert _same(got["scratch"][-H:, :, :24], gst.lbuf.transpose(0, 1))  # the second launch appended what the steps handed over
    return exp


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("which", ["six", "three"])
@pytest.mark.parametrize("recipe", ["6cold", "6warm", "3cold", "3warm"])
def test_one_launch_equals_the_composition(dev, recipe, which, S):
    """S = 1 (one wave alone) and S = 5 (two workgroups, the second partly filled), T = 7 in one launch and as 3 + 4 steps, with tgt_root and the
    joint adjustment: every per-step output, the whole state, mu and its trace"""
    exp = _case(recipe, S, which, "root_adjust")
    if S == 5:  # the clip is not a vacuous one: trials are rejected and accepted, and the damping moves and is carried
        assert bool((exp["n_accepted"] < exp["iters"]).any()) and bool((exp["n_accepted"] > 0).any())
        mt = exp["mu_trace"]
        moved = [(mt[:, s] != 1e-2).any() and (mt[1:, s] != mt[:-1, s]).any() for s in range(S)]
        assert any(bool(m) for m in moved)


@pytest.mark.parametrize("variant", ["plain", "ar1", "ar2"])
@pytest.mark.parametrize("which", ["six", "three"])
@pytest.mark.parametrize("recipe", ["6cold", "3warm"])
def test_variants_equal_the_composition(dev, recipe, which, variant):
    """without tgt_root and joint adjustment; with the predictor of order 1 (hold) and 2 (a fixed random A): also the z_tgt row every step used"""
    exp = _case(recipe, 5, which, variant)
    if variant != "plain":
        assert bool((exp["loss"][..., 2] > 0).any())             # the pull term is in the loss
        assert not torch.equal(exp["z_tgt"][1], exp["z_tgt"][0])  # the targets move with the sequence


def test_a_strided_target_buffer(dev):
    """z_tgt rows of a [S][window + 1][24] buffer, strides (24, (window + 1) * 24), as run_frames hands them over"""
    opt, c, lm, window = _opt(), _clip("6cold", 5), _lms()["three"], 9
    buf = torch.zeros(5, window + 1, 24, device=dev)
    buf[:, 2:2 + T] = c.z_tgt.transpose(0, 1)
    est, gst = _state(c), _state(c)
    exp = _per_frame(opt, c, est, lm)
    got = _launch(opt, c, gst, lm, z_tgt=buf[:, 2:], strides=(24, (window + 1) * 24))
    torch.cuda.synchronize()
    _assert_same(got, exp, OUT_KEYS)
    _assert_same(gst, est, STATE_KEYS)


def test_null_outputs_a_bf16_context_and_two_launches(dev):
    opt, c, lm = _opt(), _clip("3cold", 5), _lms()["six"]
    wst = _state(c)
    whole = _launch(opt, c, wst, lm)
    again_st = _state(c)
    again = _launch(opt, c, again_st, lm)
    torch.cuda.synchronize()
    _assert_same(again, whole, OUT_KEYS)      # no atomics: two calls, identical bits
    _assert_same(again_st, wst, STATE_KEYS)
    for names in (("pose_ret",), ("iters", "mu_trace"), ("loss0", "status"), ("loss", "joint_pos", "world_rot"), ("pos_ret", "n_accepted"), ()):
        st = _state(c)
        part = _launch(opt, c, st, lm, outputs=names)
        torch.cuda.synchronize()
        assert set(part) == set(names) | {"scratch", "mu"}
        _assert_same(part, whole, names + ("scratch",), names)
        _assert_same(st, wst, STATE_KEYS, names)
    st = _state(c)  # mu = NULL: every sequence starts at mu0, the damping is carried inside the launch and not returned
    part = _launch(opt, c, st, lm, null_mu=True)
    torch.cuda.synchronize()
    _assert_same(part, whole, OUT_KEYS, "mu NULL")
    assert bool((st.mu == 1e-2).all())
    _case("6warm", 5, "three", "root_adjust", dtype="bf16")
    _case("3cold", 5, "six", "ar2", dtype="bf16")


def test_a_captured_launch_replayed_with_mu_advancing(dev):
    """one launch of 3 steps captured into a graph and replayed twice: latent, state and mu are read and written at replay time, so the second
    replay continues from the first -- the bits of two eager launches on the same frames"""
    opt, c, lm = _opt(), _clip("6cold", 5), _lms()["three"]
    est = _state(c)
    e1 = _launch(opt, c, est, lm, 0, 3)
    mu1 = est.mu.clone()
    e2 = _launch(opt, c, est, lm, 0, 3)
    torch.cuda.synchronize()
    assert not torch.equal(mu1, torch.full_like(mu1, 1e-2)) and not torch.equal(est.mu, mu1)
    gst = _state(c)
    init = {k: getattr(gst, k).clone() for k in STATE_KEYS}
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        o = _launch(opt, c, gst, lm, 0, 3)  # (warm-up, and the launch's output tensors)
    torch.cuda.current_stream(dev).wait_stream(s)
    outs = {k: o[k] for k in OUT_KEYS if k != "scratch"}
    args = dict(lm=lm, lambda_rot=1.0, lambda_tmp=LAM, mu=gst.mu, adjust=ADJ, scratch=o["scratch"], **EPS, **outs)
    tp, tr, root, zt = c.tgt_pos[:3].contiguous(), c.tgt_rot[:3].contiguous(), c.root[:3].contiguous(), c.z_tgt[:3].contiguous()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.optimize_sequence_lm(gst.latent, tp, tr, root, c.w, c.tracked, zt, (c.S * 24, 24), gst.gpos, gst.grot, gst.lbuf, gst.dbuf, gst.hbuf, HJ, **args)
    for k, v in init.items():
        getattr(gst, k).copy_(v)
    for exp, mu in ((e1, mu1), (e2, est.mu)):
        for k in OUT_KEYS:
            o[k].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(o, exp, OUT_KEYS)
        assert torch.equal(gst.mu, mu)
    _assert_same(gst, est, STATE_KEYS)


def _fault_checks(got, gst, clean, cst, keys, t_bad, s_bad=1):
    st = got["status"].cpu()
    assert int(st[t_bad, s_bad]) == BAD_TARGETS | NONFINITE
    assert bool((st[t_bad + 1:, s_bad] == (BAD_STATE | NONFINITE)).all()) and bool((st[:t_bad, s_bad] == 0).all())
    assert bool((got["iters"][t_bad:, s_bad] == 0).all()) and bool((got["n_accepted"][t_bad:, s_bad] == 0).all())
    assert bool(torch.isfinite(got["pose_ret"][t_bad, s_bad]).all())                # the warm start's pose
    assert bool(torch.isfinite(got["joint_pos"][t_bad, s_bad]).all()) and bool(torch.isfinite(got["world_rot"][t_bad, s_bad]).all())
    assert bool(torch.isnan(got["scratch"][t_bad, s_bad, :24]).all())                # a NaN z: the history row and the carried latent
    assert bool(torch.isnan(got["loss"][t_bad:, s_bad]).all()) and bool(torch.isnan(got["loss0"][t_bad:, s_bad]).all())
    for k in ("pose_ret", "pos_ret", "world_rot", "joint_pos", "scratch"):
        assert bool(torch.isnan(got[k][t_bad + 1:, s_bad]).all()), k            # every later step: results NaN
    mu_before = got["mu_trace"][t_bad - 1, s_bad] if t_bad > 0 else torch.tensor(1e-2, device=got["mu_trace"].device)
    assert bool((got["mu_trace"][t_bad:, s_bad] == mu_before).all()) and bool(gst.mu[s_bad] == mu_before)  # mu untouched
    assert bool(torch.isnan(gst.latent[s_bad]).all()) and bool(torch.isnan(gst.gpos[s_bad]).all()) and bool(torch.isnan(gst.grot[s_bad]).all())
    rest = [s for s in range(got["status"].shape[1]) if s != s_bad]
    for k in keys:  # the other sequences: the bits of the launch without the fault
        assert _same(got[k][:, rest], clean[k][:, rest]), k
    for k in STATE_KEYS:
        assert _same(getattr(gst, k)[rest], getattr(cst, k)[rest]), k


def test_a_nan_tracker_sample(dev):
    """a NaN tracker sample at step 2 of sequence 1 of 5: that step DP_STATUS_BAD_TARGETS, every later one DP_STATUS_BAD_STATE, mu untouched,
    the other four sequences bit-equal to the clean launch -- and all of it the bits of the composition"""
    opt, c, lm = _opt(), _clip("6cold", 5), _lms()["six"]
    cst = _state(c)
    clean = _launch(opt, c, cst, lm)
    tp = c.tgt_pos.clone()
    tp[2, 1, 17, 1] = float("nan")
    gst, est = _state(c), _state(c)
    got = _launch(opt, c, gst, lm, tgt_pos=tp)
    exp = _per_frame(opt, c, est, lm, tgt_pos=tp)
    torch.cuda.synchronize()
    _assert_same(got, exp, OUT_KEYS)
    _assert_same(gst, est, STATE_KEYS)
    _fault_checks(got, gst, clean, cst, OUT_KEYS, 2)


def test_a_predictor_row_beyond_the_input_limit(dev):
    """A_1 = 1.2 I on a history row of 9e3: the row the predictor forms is beyond DP_INPUT_LIMIT and is refused like any z_tgt row"""
    from dragposer_amd import LatentAR

    opt, c, lm = _opt(), _clip("3warm", 5), _lms()["three"]
    ar = LatentAR(1.2 * np.eye(24, dtype=np.float32))
    cst = _state(c)
    clean = _launch(opt, c, cst, lm, ar=ar)
    gst, est = _state(c), _state(c)
    for st in (gst, est):
        st.lbuf[1, -1, 5] = 9.0e3
    got = _launch(opt, c, gst, lm, ar=ar)
    exp = _per_frame(opt, c, est, lm, ar=ar)
    torch.cuda.synchronize()
    keys = OUT_KEYS + ("z_tgt",)
    _assert_same(got, exp, keys)
    _assert_same(gst, est, STATE_KEYS)
    assert float(got["z_tgt"][0, 1, 5]) > 1.0e4 and bool(torch.isnan(got["z_tgt"][1:, 1]).all())
    _fault_checks(got, gst, clean, cst, keys, 0)


# ---------------------------------------------------------------------------------------------------- through DragPose
@functools.lru_cache(maxsize=None)
def _bvh_clip():
    import argparse

    from dragposer_amd import eval_drag
    from dragposer_amd.encoder import PoseEncoder
    from dragposer_amd.model import DEFAULT_MODEL, load_model_arrays
    from dragposer_amd.optimizer import LatentOptimizer

    clip = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "example_clip.bvh")
    raw = load_model_arrays(DEFAULT_MODEL, skeleton_bvh=clip)
    opt = LatentOptimizer(device="cuda:0", arrays=raw)
    cfg = dict(eval_drag.DEFAULT_CONFIG)
    q = eval_drag.prepare_file(argparse.Namespace(max_frames=12, drop=None, initial_latent=None), clip, opt, PoseEncoder(arrays=raw).to(opt.device), cfg, raw)
    mask_idx = np.nonzero(np.asarray(cfg["mask"]))[0]
    weights = np.asarray(cfg["weights"], np.float32)[mask_idx]
    ja = tuple(cfg["joint_adjustment_indices"]) if cfg["enable_joint_adjustment"] else None
    kw = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2, lambda_rot=1, temporal_future_window=0, height_indices=eval_drag.HEIGHT_INDICES,
              joint_adjustment_indices=ja, joint_adjustment_weight=cfg["joint_adjustment_weight"])
    return opt, q, mask_idx, weights, kw


def _fresh(opt, q):
    from dragposer_amd.drag_pose import DragPose

    dp = DragPose(opt, None, np.zeros(24, np.float32), np.ones(24, np.float32), n_sequences=1)
    dp.set_initial_state(q["z0"], q["m"]["global_pos"][0][None], q["m"]["global_rot"][0][None], q["m"]["heights"][0][None])
    return dp


def test_dragpose_run_frames_with_target_root(dev):
    """12 frames of tests/data/example_clip.bvh: run_frames(solver=LM(3), target_root=) equals the loop over run(solver=) that shifts the targets by
    hand (eval_drag's frame loop)"""
    from dragposer_amd import LM

    opt, q, mask_idx, weights, kw = _bvh_clip()
    solver, n = LM(3), 12
    loop, whole = _fresh(opt, q), _fresh(opt, q)
    poses, gposs, iters, status, losses, jpos = [], [], [], [], [], []
    for t in range(n):
        tp = q["tp_rel"][t][None] + (q["gpos"][t] - loop.current_global_pos).unsqueeze(1)
        pose, gpos = loop.run(tp, q["tR"][t][None], mask_idx, weights, solver=solver, lambda_temporal=0.0, **kw)
        for lst, v in ((poses, pose), (gposs, gpos), (iters, loop.last["iters"]), (status, loop.last["status"]), (losses, loop.last["loss"]),
                       (jpos, loop.last["joint_pos"])):
            lst.append(v.clone())
    ps, gs, its = whole.run_frames(q["tp_rel"][:n].reshape(n, 1, -1, 3), q["tR"][:n].reshape(n, 1, -1, 3, 3), mask_idx, weights,
                                   target_root=q["gpos"][:n].reshape(n, 1, 3), solver=solver, lambda_temporal=0.0, **kw)
    torch.cuda.synchronize()
    assert torch.equal(ps, torch.stack(poses)) and torch.equal(gs, torch.stack(gposs)) and torch.equal(its, torch.stack(iters))
    assert torch.equal(whole.last_status, torch.stack(status)) and int(whole.last_status.max()) == 0
    assert torch.equal(whole.last_loss, torch.stack(losses)) and torch.equal(whole.last_joint_pos, torch.stack(jpos))
    assert torch.equal(whole.lm_mu, loop.lm_mu) and torch.equal(whole.latent, loop.latent)
    for k in ("current_global_pos", "current_global_rot", "latent_buffer", "displacement_buffer", "heights_buffer"):
        assert torch.equal(getattr(whole, k), getattr(loop, k)), k


def test_dragpose_with_the_solvers_predictor(dev):
    """run_frames(solver=LM(3, predictor=LatentAR.hold())) is one launch for all frames, weighed by lambda_temporal; run() with the same solver
    is its one-step launch: the same bits"""
    from dragposer_amd import LM, LatentAR

    opt, q, mask_idx, weights, kw = _bvh_clip()
    solver, n = LM(3, predictor=LatentAR.hold()), 12
    loop, whole = _fresh(opt, q), _fresh(opt, q)
    tps, poses, gposs, ztg = [], [], [], []
    for t in range(n):
        tp = q["tp_rel"][t][None] + (q["gpos"][t] - loop.current_global_pos).unsqueeze(1)
        tps.append(tp.clone())
        pose, gpos = loop.run(tp, q["tR"][t][None], mask_idx, weights, solver=solver, lambda_temporal=0.05, **kw)
        poses.append(pose.clone())
        gposs.append(gpos.clone())
        ztg.append(loop.last["z_tgt"].clone())
        assert float(loop.last["loss"][0, 2]) >= 0.0
    ps, gs, its = whole.run_frames(torch.stack(tps), q["tR"][:n].reshape(n, 1, -1, 3, 3), mask_idx, weights, solver=solver, lambda_temporal=0.05, **kw)
    torch.cuda.synchronize()
    assert torch.equal(ps, torch.stack(poses)) and torch.equal(gs, torch.stack(gposs))
    assert torch.equal(whole.last_z_tgt, torch.stack(ztg)) and torch.equal(whole.lm_mu, loop.lm_mu) and torch.equal(whole.latent, loop.latent)
    assert bool((whole.last_loss[..., 2] > 0).any())  # the pull is weighed in
    assert torch.equal(whole.last_z_tgt[1:, 0], whole.latent_buffer[0, -n:-1])  # hold: each target is the row the step before left

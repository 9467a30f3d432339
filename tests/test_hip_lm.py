"""GPU (MI355X): dp_optimize_lm (include/dragposer_lm.h) -- Levenberg-Marquardt steps on the matrix pipe -- against the fp64 oracle
(tests/lm_oracle.py): one step (the latent within 4 x the fp32 oracle's own deviation from the fp64 one, the accept flag, the forward results
at the kernel's own latent), several steps (the loss never rises; the total loss against the oracle's; iters under early_stop), the edges
(a singular A, lambda_rot = 0, a bf16 context, determinism, mu = NULL, graph capture), the status word, and through DragPose.run."""
import functools
import os

import numpy as np
import pytest
import torch

import lm_oracle as LO
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu
RECIPES = ("6cold", "6warm", "3cold", "3warm")
MARGIN = 1e-3  # a step whose oracle margin |L' - L| / L is below this may be decided either way


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def opts(dev):
    from dragposer_amd.optimizer import LatentOptimizer

    return {"fp32": LatentOptimizer(device=dev), "bf16": LatentOptimizer(device=dev, weight_dtype="bf16")}


@functools.lru_cache(maxsize=None)
def _models():
    return R.OracleModel(dtype=torch.float64), R.OracleModel(dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _inputs(recipe, B):
    """6cold / 6warm / 3cold / 3warm / mcold / mwarm (mixed 1-6 trackers per frame), seed 11"""
    m64 = _models()[0]
    kw = dict(trackers=3 if recipe[0] == "3" else 6, mixed=recipe[0] == "m")
    return LO.warm_inputs(m64, B, seed=11, **kw) if recipe.endswith("warm") else R.synth_inputs(m64, B, seed=11, **kw)


def _mus(B):
    return np.asarray([1e-4, 1e-2, 1.0], np.float32)[np.random.default_rng(5).integers(0, 3, B)]


def _run(opt, b, dev, mu=None, **kw):
    from dragposer_amd.optimizer import to_device_batch

    d = to_device_batch(b, dev)
    out = opt.optimize_lm(**d, mu=torch.from_numpy(mu.copy()).to(dev) if mu is not None else None, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _sub(b, n):
    return {k: np.asarray(v)[:n] for k, v in b.items()}


def _forward_bars(got, b, z, loss, lam_rot=1.0, lam_tmp=0.02, model=None):
    """pos / rot (with `got`) and loss (with `loss`) of the kernel against the fp64 oracle's forward pass at the kernel's own latent: the
    project's forward bars"""
    ref = LO.forward_np(model or _models()[0], z.astype(np.float64), b, lam_rot, lam_tmp)
    if "pos" in got:
        err_mm = np.linalg.norm(got["pos"] - ref["pos"], axis=-1).max() * 1000.0
        print(f"  forward: max joint error {err_mm:.5f} mm, max |rot| error {np.abs(got['rot'] - ref['rot']).max():.2e}")
        assert err_mm < 0.05, err_mm
        assert np.abs(got["rot"] - ref["rot"]).max() < 2e-5
    if loss is not None:
        big = np.abs(ref["loss"]) > 1e-9
        rel = np.abs(loss - ref["loss"])[big] / np.abs(ref["loss"])[big]
        print(f"  forward: max relative loss error {rel.max() if big.any() else 0.0:.2e}, max absolute {np.abs(loss - ref['loss']).max():.2e}")
        np.testing.assert_allclose(loss, ref["loss"], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("B", [41, 1])
@pytest.mark.parametrize("recipe", RECIPES + ("mcold", "mwarm"))
def test_one_step_against_the_fp64_oracle(opts, dev, recipe, B):
    m64, m32 = _models()
    b = _sub(_inputs(recipe, 41), B)
    mu = _mus(41)[:B]
    ref = LO.lm(m64, b, 1, mu=mu.astype(np.float64))
    r32 = LO.lm(m32, b, 1, mu=mu)
    got = _run(opts["fp32"], b, dev, mu=mu, lm=_lm(1, early_stop=False))
    bar = max(4.0 * np.abs(r32["z"] - ref["z"]).max(), 1e-6)
    dz = np.abs(got["z"] - ref["z"]).max()
    print(f"{recipe} B={B}: kernel max |dz| {dz:.3e}, fp32 oracle {np.abs(r32['z'] - ref['z']).max():.3e}, bar {bar:.3e}, "
          f"smallest oracle margin {np.nanmin(ref['margin']):.3e}, accepted {int(ref['accepted'].sum())}/{B}")
    sure = ref["margin"][:, 0] >= MARGIN
    np.testing.assert_array_equal(got["n_accepted"][sure], ref["n_accepted"][sure])
    assert (got["status"] == 0).all() and (got["iters"] == 1).all()
    same = got["n_accepted"] == ref["n_accepted"]
    assert np.abs(got["z"] - ref["z"])[same].max() <= bar, (dz, bar)
    np.testing.assert_array_equal(got["z"], got["z_pre"])
    np.testing.assert_allclose(got["mu"], ref["mu"][...], rtol=1e-6)
    _forward_bars(got, b, got["z"], None)


@pytest.mark.parametrize("B", [41, 1])
@pytest.mark.parametrize("recipe", RECIPES + ("mcold", "mwarm"))
def test_one_step_losses_at_the_kernels_own_latents(opts, dev, recipe, B):
    """loss0 and loss against the fp64 oracle's forward pass at z0 and at the kernel's own returned z, to the forward bar of
    tests/test_hip_parity.py (rtol 1e-5, atol 1e-9).  The kernel reports both from a pass in double on its fp32 weights (dp_lm.hip): the
    fp32 pass that decides the steps places a joint to 1e-7 .. 1e-6 m, near the solution a residual is millimetres, and its loss was up to
    5.6e-5 off (the fp32 oracle itself: 2.9e-5 and 4.3e-5 on the warm recipes).  Measured with the pass in double: loss0 within 8.2e-6 (3 warm,
    the weights' own rounding to fp32 once folded), 3.8e-6 (6 warm), under 1e-6 on the cold recipes."""
    b = _sub(_inputs(recipe, 41), B)
    mu = _mus(41)[:B]
    got = _run(opts["fp32"], b, dev, mu=mu, lm=_lm(1, early_stop=False))
    print(f"{recipe} B={B}:")
    _forward_bars({}, b, np.asarray(b["z0"]), got["loss0"])
    _forward_bars({}, b, got["z"], got["loss"])


def _lm(steps, **kw):
    from dragposer_amd import LM

    return LM(steps=steps, **kw)


@pytest.mark.parametrize("steps", [4, 8])
@pytest.mark.parametrize("recipe", RECIPES)
def test_several_steps(opts, dev, recipe, steps):
    m64, m32 = _models()
    b = _inputs(recipe, 64)
    ref, r32 = LO.lm(m64, b, steps), LO.lm(m32, b, steps)
    got = _run(opts["fp32"], b, dev, lm=_lm(steps, early_stop=False))
    assert (got["status"] == 0).all() and (got["iters"] == steps).all()
    assert (got["loss"].sum(1) <= got["loss0"].sum(1)).all()
    tot, want = got["loss"].sum(1).astype(np.float64), ref["loss"].sum(1)
    pair = np.abs(r32["loss"].sum(1) - want) / want
    rel = np.abs(tot - want) / want
    bar = 4.0 * pair.max()
    out = int((rel > bar).sum())
    print(f"{recipe} {steps} steps: kernel max rel loss difference {rel.max():.3e} (median {np.median(rel):.3e}), fp32 oracle pair max {pair.max():.3e}, "
          f"bar {bar:.3e}, frames beyond {out}/64, accepted mean {got['n_accepted'].mean():.2f} (oracle {ref['n_accepted'].mean():.2f})")
    assert out <= 0.01 * len(rel), (np.sort(rel)[-4:], bar)
    # early stop: iters equal the oracle's wherever no step's margin was below the bar
    eps = dict(stop_eps_pos=float(np.median(want)) * 0.5, stop_eps_rot=float(np.median(want)) * 0.5)
    ref_e = LO.lm(m64, b, steps, early_stop=True, **eps)
    got_e = _run(opts["fp32"], b, dev, lm=_lm(steps, early_stop=True), **eps)
    sure = ~(ref_e["ran"] & (ref_e["margin"] < MARGIN)).any(1)
    print(f"  early stop: oracle iters histogram {np.bincount(ref_e['iters'], minlength=steps + 1).tolist()}, compared on {int(sure.sum())}/64 frames")
    np.testing.assert_array_equal(got_e["iters"][sure], ref_e["iters"][sure])
    assert (got_e["loss"].sum(1) <= got_e["loss0"].sum(1)).all()


def test_singular_normal_equations_are_solved_by_the_damping_alone(opts, dev):
    b = {k: np.array(v) for k, v in _inputs("6warm", 16).items()}
    b["tracked"][:] = 0
    b["tracked"][:, 13] = 1
    b["w"][:] = 0
    b["w"][:, 13, 0] = 5.0  # one position-only tracker: 3 rows for 24 unknowns
    got = _run(opts["fp32"], b, dev, lm=_lm(4, early_stop=False), lambda_tmp=0.0)
    assert (got["status"] == 0).all()
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    assert (got["loss"].sum(1) <= got["loss0"].sum(1)).all()
    _forward_bars(got, b, got["z"], None, lam_tmp=0.0)


def test_lambda_rot_zero_and_a_bf16_context(opts, dev):
    m64 = _models()[0]
    b = _inputs("6cold", 41)
    ref = LO.lm(m64, b, 2, lam_rot=0.0)
    got = _run(opts["fp32"], b, dev, lm=_lm(2, early_stop=False), lambda_rot=0.0)
    assert (got["status"] == 0).all() and (got["loss"][:, 1] == 0).all()
    rel = np.abs(got["loss"].sum(1) - ref["loss"].sum(1)) / ref["loss"].sum(1)
    print(f"lambda_rot 0: max rel loss difference to the oracle {rel.max():.3e}")
    assert np.median(rel) < 1e-3
    _forward_bars(got, b, got["z"], None, lam_rot=0.0)
    mb = R.OracleModel(dtype=torch.float64, weight_rounding="bf16")
    refb = LO.lm(mb, b, 2)
    gotb = _run(opts["bf16"], b, dev, lm=_lm(2, early_stop=False))
    relb = np.abs(gotb["loss"].sum(1) - refb["loss"].sum(1)) / refb["loss"].sum(1)
    print(f"bf16 context: max rel loss difference to the bf16-rounded oracle {relb.max():.3e}")
    assert (gotb["status"] == 0).all() and np.median(relb) < 1e-3
    _forward_bars(gotb, b, gotb["z"], None, model=mb)


def test_deterministic_mu_null_and_graph_capture(opts, dev):
    from dragposer_amd.optimizer import to_device_batch

    opt = opts["fp32"]
    b = _inputs("3cold", 41)
    a = _run(opt, b, dev, lm=_lm(3))
    c = _run(opt, b, dev, lm=_lm(3))
    filled = _run(opt, b, dev, mu=np.full(41, 1e-2, np.float32), lm=_lm(3))
    for k in a:
        np.testing.assert_array_equal(a[k], c[k], err_msg=k)
        np.testing.assert_array_equal(a[k], filled[k], err_msg=k)
    d = to_device_batch(b, dev)
    out = opt.allocate_outputs(41)
    out.update(n_accepted=torch.empty(41, dtype=torch.int32, device=dev), loss0=torch.empty(41, 3, device=dev))
    mu = torch.full((41,), 1e-2, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        opt.optimize_lm(**d, lm=_lm(3), mu=mu, out=out, outputs=tuple(out))
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.optimize_lm(**d, lm=_lm(3), mu=mu, out=out, outputs=tuple(out))
    for v in out.values():
        v.fill_(-1)
    mu.fill_(1e-2)
    graph.replay()
    torch.cuda.synchronize()
    for k in out:
        np.testing.assert_array_equal(out[k].cpu().numpy(), a[k], err_msg=k)
    np.testing.assert_array_equal(mu.cpu().numpy(), a["mu"])


def test_status(opts, dev):
    from dragposer_amd import _lib

    opt = opts["fp32"]
    b = {k: np.array(v) for k, v in _inputs("6cold", 9).items()}
    clean = _run(opt, b, dev, lm=_lm(3))
    bad = {k: v.copy() for k, v in b.items()}
    bad["tgt_pos"][4, 13, 1] = np.nan
    got = _run(opt, bad, dev, lm=_lm(3))
    assert got["status"][4] == _lib.DP_STATUS_BAD_TARGETS | _lib.DP_STATUS_NONFINITE_RESULT
    assert np.isnan(got["z"][4]).all() and np.isnan(got["loss"][4]).all() and got["iters"][4] == 0
    assert np.isfinite(got["pos"][4]).all()  # (the warm start's pose)
    rest = np.arange(9) != 4
    for k in clean:
        np.testing.assert_array_equal(got[k][rest], clean[k][rest], err_msg=k)
    state = {k: v.copy() for k, v in b.items()}
    state["z0"][2, 5] = np.inf
    got = _run(opt, state, dev, lm=_lm(3))
    assert got["status"][2] == _lib.DP_STATUS_BAD_STATE | _lib.DP_STATUS_NONFINITE_RESULT and np.isnan(got["pos"][2]).all()
    rest = np.arange(9) != 2
    for k in clean:
        np.testing.assert_array_equal(got[k][rest], clean[k][rest], err_msg=k)
    skew = {k: v.copy() for k, v in b.items()}
    skew["tgt_rot"][6, 13] *= 1.05  # not a rotation: reported, the element-wise loss is computed as given
    got = _run(opt, skew, dev, lm=_lm(3))
    assert got["status"][6] == _lib.DP_STATUS_TARGET_NOT_ROTATION and (got["status"][rest & (np.arange(9) != 6)] == 0).all()
    assert np.isfinite(got["z"][6]).all() and got["loss"][6].sum() <= got["loss0"][6].sum()
    ref = LO.forward_np(_models()[0], got["z"][[6]].astype(np.float64), _sub_frames(skew, [6]))
    np.testing.assert_allclose(got["loss"][[6]], ref["loss"], rtol=2e-3, atol=1e-8)  # (the element-wise loss on the matrix as given)


def _sub_frames(b, frames):
    return {k: np.asarray(v)[frames] for k, v in b.items()}


def test_dragpose_run_with_the_lm_solver(dev):
    """12 frames of tests/data/example_clip.bvh (eval_drag's own preparation, 6 trackers) through DragPose.run(solver=LM(3)): frame by frame the
    bits of optimize_lm + sequence_advance composed by hand; lm_mu carries over and is reset when a sequence begins; run_frames(solver=) gives
    the same bits"""
    import argparse

    from dragposer_amd import LM, eval_drag
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.encoder import PoseEncoder
    from dragposer_amd.model import DEFAULT_MODEL, load_model_arrays
    from dragposer_amd.optimizer import LatentOptimizer

    clip = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "example_clip.bvh")
    raw = load_model_arrays(DEFAULT_MODEL, skeleton_bvh=clip)
    opt = LatentOptimizer(device=dev, arrays=raw)
    cfg = dict(eval_drag.DEFAULT_CONFIG)
    T = 12
    q = eval_drag.prepare_file(argparse.Namespace(max_frames=T, drop=None, initial_latent=None), clip, opt, PoseEncoder(arrays=raw).to(dev), cfg, raw)
    mask_idx = np.nonzero(np.asarray(cfg["mask"]))[0]
    weights = np.asarray(cfg["weights"], np.float32)[mask_idx]
    ja = tuple(cfg["joint_adjustment_indices"]) if cfg["enable_joint_adjustment"] else None
    solver = LM(3)
    kw = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2, lambda_rot=1, lambda_temporal=0.0, temporal_future_window=0, height_indices=eval_drag.HEIGHT_INDICES,
              joint_adjustment_indices=ja, joint_adjustment_weight=cfg["joint_adjustment_weight"])

    def fresh():
        dp = DragPose(opt, None, np.zeros(24, np.float32), np.ones(24, np.float32), n_sequences=1)
        dp.set_initial_state(q["z0"], q["m"]["global_pos"][0][None], q["m"]["global_rot"][0][None], q["m"]["heights"][0][None])
        return dp

    dp, hand = fresh(), fresh()
    poses, gposs, mus, tps = [], [], [], []
    for t in range(T):
        assert (dp.lm_mu is None) == (t == 0)
        tp = q["tp_rel"][t][None] + (q["gpos"][t] - dp.current_global_pos).unsqueeze(1)  # (eval_drag's frame loop)
        tps.append(tp.clone())
        pose, gpos = dp.run(tp, q["tR"][t][None], mask_idx, weights, solver=solver, **kw)
        # the same frame composed by hand on a second operator
        trk = hand._trackers(mask_idx, weights)
        hand._temporal_targets(0)
        trk["tgt_pos"].index_copy_(1, trk["mj"], tp.reshape(1, -1, 3))
        trk["tgt_rot"].index_copy_(1, trk["mj"], q["tR"][t].reshape(1, -1, 9))
        if hand.lm_mu is None:
            hand.lm_mu = torch.full((1,), solver.mu0, device=dev)
        fr = opt.optimize_lm(hand.latent, hand.target_latent_buffer[:, hand.current_index].contiguous(), hand.current_global_rot, trk["tgt_pos"],
                             trk["tgt_rot"], trk["w"], trk["tracked"], lm=solver, lambda_rot=1.0, lambda_tmp=0.0, mu=hand.lm_mu,
                             stop_eps_pos=kw["stop_eps_pos"], stop_eps_rot=kw["stop_eps_rot"])
        hp, hg = torch.empty(1, 88, device=dev), torch.empty(1, 3, device=dev)
        adjust = (int(ja[0]), int(trk["mj_host"][ja[1]]), float(cfg["joint_adjustment_weight"])) if ja is not None else None
        opt.sequence_advance(fr, hand.current_global_pos, hand.current_global_rot, hand.latent_buffer, hand.displacement_buffer,
                             hand.heights_buffer, tuple(int(h) for h in eval_drag.HEIGHT_INDICES), pose_ret=hp, pos_ret=hg, adjust=adjust,
                             tgt_pos=trk["tgt_pos"] if adjust is not None else None)
        hand.latent.copy_(fr["z"])
        assert torch.equal(pose, hp) and torch.equal(gpos, hg) and torch.equal(dp.lm_mu, hand.lm_mu), t
        assert torch.equal(dp.latent, hand.latent) and torch.equal(dp.current_global_pos, hand.current_global_pos)
        assert torch.equal(dp.last["iters"], fr["iters"]) and (dp.last["status"] == 0).all()
        assert (dp.last["loss"].sum(1) <= dp.last["loss0"].sum(1)).all()
        poses.append(pose.clone())
        gposs.append(gpos.clone())
        mus.append(dp.lm_mu.clone())
    assert any(not torch.equal(m, torch.full((1,), solver.mu0, device=dev)) for m in mus)  # (the damping moved, and is carried)
    whole = fresh()
    ps, gs, its = whole.run_frames(torch.stack(tps), torch.stack([q["tR"][t][None] for t in range(T)]).reshape(T, 1, -1, 3, 3), mask_idx, weights,
                                   solver=solver, **kw)
    assert torch.equal(ps, torch.stack(poses)) and torch.equal(gs, torch.stack(gposs)) and torch.equal(whole.lm_mu, mus[-1])
    whole.set_initial_state(q["z0"], q["m"]["global_pos"][0][None], q["m"]["global_rot"][0][None], q["m"]["heights"][0][None])
    assert whole.lm_mu is None  # (reset when a sequence begins)

"""CPU: the Levenberg-Marquardt oracle (tests/lm_oracle.py) in fp64 -- the loss never increases, and the claims the README makes about
steps against Adam iterations (oracle.ref_torch.optimize, the reference's solver) on recipe S, 256 frames, seed 11, lambda_rot 1,
lambda_tmp 0.02: warm (z0 = z_src + 0.05 N(0,1), z_tgt = z0) 2 steps are at or below Adam-50's loss on at least 90 % of the frames with 6
and with 3 trackers; cold (the recipe's own z0) with 6 trackers 8 steps are.  Then the conditions the inputs of tests/test_hip_lm_paths.py
(GPU) were chosen for: every_joint_inputs' one-step margins on three trees, the two problems whose rejections are certain, the mu_min recipe."""
import functools

import numpy as np
import pytest
import torch

import lm_oracle as LO
from oracle import ref_torch as R

B = 256


@functools.lru_cache(maxsize=None)
def _case(trackers, warm):
    model = R.OracleModel(dtype=torch.float64)
    b = LO.warm_inputs(model, B, trackers=trackers, seed=11) if warm else R.synth_inputs(model, B, trackers=trackers, seed=11)
    adam = R.optimize(model, b["z0"], b["z_tgt"], b["cur_rot"], b["tgt_pos"], b["tgt_rot"], b["w"], b["tracked"], 50, lam_tmp=0.02)
    return adam["loss"].sum(1), LO.lm(model, b, 8)


@pytest.mark.parametrize("trackers,warm,steps", [(6, True, 2), (3, True, 2), (6, False, 8)])
def test_steps_against_adam_50(trackers, warm, steps):
    adam50, lm = _case(trackers, warm)
    hist = lm["loss_hist"]
    share = float((hist[:, steps] <= adam50).mean())
    print(f"{trackers} trackers, {'warm' if warm else 'cold'}: median loss Adam-50 {np.median(adam50):.3e}, LM "
          + ", ".join(f"{k} steps {np.median(hist[:, k]):.3e}" for k in (1, 2, 4, 8)) + f"; {steps} steps at or below Adam-50 on {share:.1%}")
    assert share >= 0.90, share


@pytest.mark.parametrize("trackers,warm", [(6, True), (3, True), (6, False)])
def test_the_loss_never_increases(trackers, warm):
    lm = _case(trackers, warm)[1]
    hist = lm["loss_hist"]
    assert np.isfinite(hist).all() and (np.diff(hist, axis=1) <= 0).all()
    np.testing.assert_array_equal(lm["iters"], 8)
    np.testing.assert_array_equal(lm["n_accepted"], lm["accepted"].sum(1))
    np.testing.assert_allclose(lm["loss"].sum(1), hist[:, -1], rtol=1e-12)
    np.testing.assert_allclose(lm["loss0"].sum(1), hist[:, 0], rtol=1e-12)


def test_early_stop_and_the_damping_bounds():
    model = R.OracleModel(dtype=torch.float64)
    b = LO.warm_inputs(model, 32, trackers=6, seed=11)
    full = LO.lm(model, b, 6)
    eps = float(np.median(full["loss"].sum(1)))
    early = LO.lm(model, b, 6, early_stop=True, stop_eps_pos=eps, stop_eps_rot=eps)
    assert (early["iters"] <= full["iters"]).all() and (early["iters"] < 6).any()
    stopped = early["iters"] < 6
    assert ((early["loss"][stopped, 0] <= eps) & (early["loss"][stopped, 1] <= eps)).all()
    # a step that cannot be accepted: mu climbs to mu_max and, with early_stop, the frame ends after a rejection there
    stuck = LO.lm(model, b, 12, early_stop=True, mu_down=0.5, mu_up=10.0, mu_max=1e-1, mu0=1e-2, mu_min=1e-2,
                  mu=np.full(32, 1e-2))
    assert (stuck["mu"] <= 1e-1).all() and (stuck["mu"] >= 1e-2).all()
    f32 = LO.lm(R.OracleModel(dtype=torch.float32), b, 2)
    assert f32["z"].dtype == np.float32 and np.abs(f32["z"] - LO.lm(model, b, 2)["z"]).max() < 1e-3


# ---- the conditions that tests/test_hip_lm_paths.py (GPU) relies on, checked here without a GPU
MARGIN = 1e-3  # tests/test_hip_lm.py: a step whose oracle margin is below this may be decided either way


@functools.lru_cache(maxsize=None)
def _tree_models(name):
    """(fp64 oracle model, fp32 oracle model) of the shipped tree ("xsens") or of one of tests/test_hip_topology.py's"""
    if name == "xsens":
        return R.OracleModel(dtype=torch.float64), R.OracleModel(dtype=torch.float32)
    import tempfile

    from test_hip_topology import TREES, _model_arrays

    with tempfile.TemporaryDirectory() as tmp:
        return LO.tree_models(_model_arrays(TREES[name], seed=len(name)), tmp + "/model.npz")


def _mus(B):  # (tests/test_hip_lm.py's)
    return np.asarray([1e-4, 1e-2, 1.0], np.float32)[np.random.default_rng(5).integers(0, 3, B)]


EVERY_JOINT_CASES = [("xsens", True), ("xsens", False), ("arms_at_two_levels", False), ("four_limbs_on_one_joint", False)]


@pytest.mark.parametrize("tree,warm", EVERY_JOINT_CASES)
def test_every_joint_inputs_leave_no_frame_out(tree, warm):
    """the builder's layout, and the one-step margins: every frame decided by at least 0.05, fp32 and fp64 oracle agreeing on every flag"""
    m64, m32 = _tree_models(tree)
    b = LO.every_joint_inputs(m64, warm)
    trk = b["tracked"]
    assert trk.shape == (28, 22) and np.array_equal(trk[:22], np.eye(22, dtype=np.uint8)) and trk[22].all()
    assert trk[23:].sum(1).tolist() == [7, 9, 11, 15, 21]
    perm = np.random.default_rng(3).permutation(22)
    assert all(set(np.nonzero(trk[23 + i])[0]) == set(perm[:n]) for i, n in enumerate((7, 9, 11, 15, 21)))
    on = trk.astype(bool)
    assert (b["w"][~on] == 0).all() and (b["tgt_pos"][~on] == 0).all() and (b["tgt_rot"][~on] == 0).all()
    assert (b["w"][on][:, 0] >= 1).all() and (b["w"][on] <= 10).all() and (b["w"][on][:, 1] >= 0.01).all()
    par = m64.parents
    interior = [j for j in range(1, 22) if j in par[1:]]  # (joints with a child: tests/test_hip_lm.py's recipes track the root and chain ends only)
    assert len(interior) >= 15 and all(trk[j].sum() == 1 and trk[j, j] for j in interior)
    ref = LO.forward_np(m64, b["z_src"].astype(np.float64), b, 1.0, 0.0)  # (the targets are the tree's own FK of z_src)
    assert np.abs(ref["pos"][on] - b["tgt_pos"][on]).max() < 1e-6 and np.abs(ref["rot"][on] - b["tgt_rot"][on]).max() < 1e-6
    mu = _mus(28)
    r64, r32 = LO.lm(m64, b, 1, mu=mu.astype(np.float64)), LO.lm(m32, b, 1, mu=mu)
    print(f"{tree} {'warm' if warm else 'cold'}: accepted {int(r64['accepted'].sum())}/28, smallest margin {r64['margin'].min():.3e} (fp32 "
          f"{r32['margin'].min():.3e}), oracle pair max |dz| {np.abs(r32['z'] - r64['z']).max():.3e}")
    assert r64["margin"].min() >= 0.05 and r32["margin"].min() >= 0.05
    np.testing.assert_array_equal(r64["accepted"], r32["accepted"])


def test_a_wrong_row_of_an_interior_joint_would_be_noticed():
    """the rotation rows of joint 10 (interior: no recipe of tests/test_hip_lm.py tracks it) zeroed in J: the one-step latent of the frames
    that track it moves by far more than the bar it is held to"""
    m64, m32 = _tree_models("xsens")
    assert 10 in m64.parents[1:] and 10 not in R.TRACK6
    b = LO.every_joint_inputs(m64, True)
    mu = _mus(28)
    r64, r32 = LO.lm(m64, b, 1, mu=mu.astype(np.float64)), LO.lm(m32, b, 1, mu=mu)
    bar = max(4.0 * np.abs(r32["z"] - r64["z"]).max(), 1e-6)

    def hook(J):
        J = J.clone()
        J[:, 66 + 90:66 + 99] = 0.0
        return J

    bad = LO.lm(m64, b, 1, mu=mu.astype(np.float64), jac_hook=hook)
    moved = np.abs(bad["z"] - r64["z"]).max(1)
    tracks10 = b["tracked"][:, 10] != 0
    print(f"dG_10/dz zeroed: frame 10 moves by {moved[10]:.3e}, the frames that track joint 10 by {moved[tracks10].min():.3e} .. "
          f"{moved[tracks10].max():.3e}, the others by {moved[~tracks10].max():.3e}; bar {bar:.3e} ({moved[10] / bar:.0f} x)")
    assert (moved[~tracks10] == 0).all() and moved[10] > 100.0 * bar
    assert (moved[tracks10 & r64["accepted"][:, 0]] > bar).all()


@pytest.mark.parametrize("problem", ["zero", "at_target"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_rejections_that_are_certain(problem, dtype):
    """both problems in both oracles: five rejections take mu 0.01 -> 10 = mu_max, the sixth is at mu_max and ends the frame"""
    model = R.OracleModel(dtype=dtype)
    b, lam_tmp = (LO.zero_problem if problem == "zero" else LO.at_target_problem)(model, 9)
    kw = dict(lam_tmp=lam_tmp, mu_max=10.0, stop_eps_pos=-1.0, stop_eps_rot=-1.0)
    r = LO.lm(model, b, 12, early_stop=True, **kw)
    np.testing.assert_array_equal(r["iters"], 6)
    np.testing.assert_array_equal(r["n_accepted"], 0)
    assert (r["mu"] == 10.0).all() and np.array_equal(r["z"], b["z0"].astype(r["z"].dtype))
    assert (r["loss"] == 0).all() and (r["loss0"] == 0).all()
    full = LO.lm(model, b, 12, early_stop=False, **kw)
    np.testing.assert_array_equal(full["iters"], 12)
    assert (full["mu"] == 10.0).all() and (full["n_accepted"] == 0).all() and np.array_equal(full["z"], r["z"])


def test_the_mu_min_recipe_is_accepted_twice_on_every_frame():
    m64 = R.OracleModel(dtype=torch.float64)
    b = LO.warm_inputs(m64, 41, trackers=6, seed=11)
    r = LO.lm(m64, b, 2, mu_min=5e-3)
    sure = (r["margin"] >= MARGIN).all(1)
    print(f"mu_min 5e-3, 6 warm, B = 41: accepted {r['n_accepted'].tolist()}, frames with both margins >= {MARGIN}: {int(sure.sum())}/41")
    np.testing.assert_array_equal(r["n_accepted"], 2)
    assert (r["mu"] == 5e-3).all() and int((~sure).sum()) <= 2

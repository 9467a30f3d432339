"""CPU: the Levenberg-Marquardt oracle (tests/lm_oracle.py) in fp64 -- the loss never increases, and the claims the README makes about
steps against Adam iterations (oracle.ref_torch.optimize, the reference's solver) on recipe S, 256 frames, seed 11, lambda_rot 1,
lambda_tmp 0.02: warm (z0 = z_src + 0.05 N(0,1), z_tgt = z0) 2 steps are at or below Adam-50's loss on at least 90 % of the frames with 6
and with 3 trackers; cold (the recipe's own z0) with 6 trackers 8 steps are."""
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

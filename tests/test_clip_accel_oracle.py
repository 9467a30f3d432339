"""CPU: the oracle of dp_optimize_clip_lm_accel (tests/clip_accel_oracle.py) against itself -- the block recursion with lower bandwidth 2
against a dense Cholesky of the whole sequence's matrix in fp64, the band matrix against the entries the header states, lambda_accel = 0 and
T <= 2 against tests/clip_lm_oracle.py, a constant-velocity sequence (which the term does not see), and the decision margins of the inputs
tests/test_hip_clip_accel.py runs (pinned here, so that the GPU test's "no sequence left out" rests on numbers a CPU run can reproduce)."""
import functools

import numpy as np
import pytest
import torch

import clip_accel_oracle as AO
import clip_lm_oracle as CO
import lm_oracle as LO
from oracle import ref_torch as R

MARGIN = 1e-3  # tests/test_hip_lm.py's: a step whose oracle margin is below this may be decided either way
SETTINGS = [(0.0, 0.5), (0.0, 50.0), (0.5, 5.0)]  # (lambda_smooth, lambda_accel) of the GPU tests


@functools.lru_cache(maxsize=None)
def _models():
    return R.OracleModel(dtype=torch.float64), R.OracleModel(dtype=torch.float32)


def test_the_band_matrix_has_the_entries_the_header_states():
    dd = lambda T: torch.diagonal(AO.band_matrix(T, 0.0, 1.0, torch.float64)).tolist()
    assert dd(1) == [0.0] and dd(2) == [0.0, 0.0] and dd(3) == [1.0, 4.0, 1.0] and dd(4) == [1.0, 5.0, 5.0, 1.0]
    assert dd(5) == [1.0, 5.0, 6.0, 5.0, 1.0] and dd(7) == [1.0, 5.0, 6.0, 6.0, 6.0, 5.0, 1.0]
    K = AO.band_matrix(7, 0.0, 1.0, torch.float64)
    assert torch.diagonal(K, -1).tolist() == [-2.0, -4.0, -4.0, -4.0, -4.0, -2.0] and torch.diagonal(K, -2).tolist() == [1.0] * 5
    assert torch.diagonal(AO.band_matrix(4, 0.0, 1.0, torch.float64), -1).tolist() == [-2.0, -4.0, -2.0]
    assert float(torch.tril(K, -3).abs().max()) == 0.0 and torch.equal(K, K.T)
    K = AO.band_matrix(5, 2.0, 0.0, torch.float64)  # the path Laplacian alone
    assert torch.diagonal(K).tolist() == [2.0, 4.0, 4.0, 4.0, 2.0] and torch.diagonal(K, -1).tolist() == [-2.0] * 4
    # (K Z)_t from the differences is K Z
    Z = torch.randn(7, 2, 24, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    both, _ = AO.coupling_gradient(Z, 0.3, 1.7)
    np.testing.assert_allclose(both.numpy(), torch.einsum("tu,usk->tsk", AO.band_matrix(7, 0.3, 1.7, torch.float64), Z).numpy(), atol=1e-13)


@pytest.mark.parametrize("S,T", [(1, 3), (1, 4), (2, 5), (3, 33)])
@pytest.mark.parametrize("mu", [1e-2, 1e-6])
def test_the_recursion_equals_a_dense_solve_in_fp64(S, T, mu):
    m64 = _models()[0]
    b = CO.clip_inputs(m64, S, T, trackers=6)
    worst = 0.0
    for ls, la in ((0.0, 0.5), (0.5, 50.0), (0.0, 500.0)):
        a = AO.clip_lm(m64, b, S, 1, ls, la, mu=np.full(S, mu))
        d = AO.clip_lm(m64, b, S, 1, ls, la, mu=np.full(S, mu), dense=True)
        assert a["solved"].all() and d["solved"].all()
        worst = max(worst, np.abs(a["delta"][0] - d["delta"][0]).max())
        np.testing.assert_array_equal(a["accepted"], d["accepted"])
    print(f"S={S} T={T} mu={mu:g}: recursion against the dense solve, max |difference| {worst:.2e}")
    assert worst <= 1e-9  # (measured: 1.2e-11 at worst, at lambda_accel 500 and mu 1e-6)


def test_lambda_accel_zero_is_the_first_difference_oracle():
    m64 = _models()[0]
    b = CO.clip_inputs(m64, 3, 9, trackers=3)
    for ls in (0.0, 0.5, 50.0):
        new, old = AO.clip_lm(m64, b, 3, 3, ls, 0.0), CO.clip_lm(m64, b, 3, 3, ls)
        for k in ("z", "loss", "mu", "loss_hist", "clip_loss"):
            np.testing.assert_allclose(new[k], old[k], rtol=0, atol=1e-12, err_msg=k)
        for k in ("n_accepted", "accepted", "solved"):
            np.testing.assert_array_equal(new[k], old[k], err_msg=k)
        assert (new["accel_loss"] == 0).all()


@pytest.mark.parametrize("T", [1, 2])
def test_two_frames_or_fewer_have_no_second_difference(T):
    m64 = _models()[0]
    b = CO.clip_inputs(m64, 4, T, trackers=3)
    for la in (0.5, 500.0):
        new, old = AO.clip_lm(m64, b, 4, 3, 0.7, la), CO.clip_lm(m64, b, 4, 3, 0.7)
        for k in ("z", "mu", "loss_hist", "clip_loss"):
            np.testing.assert_allclose(new[k], old[k], rtol=0, atol=1e-12, err_msg=k)
        np.testing.assert_array_equal(new["accepted"], old["accepted"])
        assert (new["accel_loss"] == 0).all()


def test_constant_velocity_costs_nothing():
    m64 = _models()[0]
    S, T = 2, 7
    b = {k: np.array(v) for k, v in CO.clip_inputs(m64, S, T, trackers=3).items()}
    z0 = b["z0"].reshape(T, S, 24).astype(np.float64)
    a, v = z0[0].copy(), 0.05 * (z0[1] - z0[0])
    z0 = a[None] + np.arange(T)[:, None, None] * v[None]  # z_t = a + b t, in double: fp32 rounding of the line would be seen
    Z = torch.as_tensor(z0, dtype=torch.float64)
    both, accel = AO.coupling_gradient(Z, 0.0, 50.0 / 24.0)
    assert float(AO.accel_coupling(Z, 50.0 / 24.0).max()) <= 1e-24 and float(accel.abs().max()) <= 1e-13 and torch.equal(both, accel)
    # and the first-difference term does see it
    assert float(CO.coupling(Z, 1.0).min()) > 0 and float(CO.laplacian_rows(Z).abs().max()) > 1e-3
    # so L_s at z0 is the frames' loss alone, whatever lambda_accel
    r = AO.clip_lm(m64, dict(b, z0=z0.reshape(S * T, 24)), S, 1, 0.0, 50.0)
    assert r["loss_hist"][:, 0] == pytest.approx(CO.clip_lm(m64, dict(b, z0=z0.reshape(S * T, 24)), S, 1, 0.0)["loss_hist"][:, 0], rel=1e-12)


def test_the_loss_never_increases_and_accel_loss_is_the_returned_latents():
    m64 = _models()[0]
    b = CO.clip_inputs(m64, 3, 9, trackers=3)
    for ls, la in SETTINGS:
        r = AO.clip_lm(m64, b, 3, 5, ls, la)
        h = r["loss_hist"]
        assert (np.diff(h, axis=1) <= 0).all() and ((np.diff(h, axis=1) < 0) == r["accepted"]).all()
        np.testing.assert_array_equal(h[:, -1], r["clip_loss"][:, 0])
        Z = torch.as_tensor(r["z"]).reshape(9, 3, 24)
        loss, _ = LO.forward(m64, torch.as_tensor(r["z"]), LO._conv(m64, b), 1.0, 0.02)
        tot, cp, ap = AO.totals(loss, Z, ls / 24.0, la / 24.0)
        np.testing.assert_allclose(r["clip_loss"], torch.stack((tot, cp), 1).numpy(), rtol=1e-12)
        np.testing.assert_allclose(r["accel_loss"], ap.numpy(), rtol=1e-12)
        assert (r["accel_loss"] > 0).all() and (r["accel_loss"] <= r["clip_loss"][:, 1]).all()


# the smallest decision margin of each GPU case in fp64 (warm recipe, seed 11, lambda_tmp 0.02), by setting (0, 0.5) / (0, 50) / (0.5, 5); the pins
# are those figures rounded down.  One step, 3 trackers, mu 1e-2 and 1e-6: 5.26e-2 is the smallest of all 48 cells ((2, 65) at (0, 0.5), mu 1e-6).
ONE_STEP_FLOOR = 5e-2
ONE_STEP_SHAPES = [(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (5, 7), (3, 33), (2, 65)]
# three steps from mu0, (S, T, trackers): measured 6.01e-2 3.31e-2 1.97e-2 / 3.64e-2 1.12e-2 4.03e-2 / 3.77e-2 3.53e-2 3.23e-2 / 2.31e-1 4.82e-2 5.31e-2 /
# 4.69e-3 2.09e-2 2.64e-2 / 7.04e-3 1.75e-2 6.06e-3 / 1.32e-2 3.51e-2 4.03e-2
THREE_STEPS = {(1, 4, 3): (6.0e-2, 3.3e-2, 1.9e-2), (1, 5, 3): (3.6e-2, 1.1e-2, 4.0e-2), (5, 7, 3): (3.7e-2, 3.5e-2, 3.2e-2), (3, 33, 3): (2.3e-1, 4.8e-2, 5.3e-2),
               (3, 33, 6): (4.6e-3, 2.0e-2, 2.6e-2), (5, 7, 6): (7.0e-3, 1.7e-2, 6.0e-3), (2, 65, 6): (1.3e-2, 3.5e-2, 4.0e-2)}
# the two cases the GPU file keeps out: (1, 3) 3 trackers at (0, 0.5): 9.04e-4, below MARGIN; (2, 65) 3 trackers at (0, 50): 1.046e-3, on the line
KEPT_OUT = {(1, 3, 3, 0.0, 0.5): (8.5e-4, 9.5e-4), (2, 65, 3, 0.0, 50.0): (1.0e-3, 1.1e-3)}


@pytest.mark.parametrize("S,T", ONE_STEP_SHAPES)
def test_one_step_margins_of_the_gpu_tests_inputs(S, T):
    m64, m32 = _models()
    b = CO.clip_inputs(m64, S, T, trackers=3)
    low, dev = [], []
    for ls, la in SETTINGS:
        for mu in (1e-2, 1e-6):
            r, r32 = (AO.clip_lm(m, b, S, 1, ls, la, mu=np.full(S, mu)) for m in (m64, m32))
            np.testing.assert_array_equal(r32["accepted"], r["accepted"])
            low.append(r["margin"].min())
            dev.append(np.abs(r32["z"] - r["z"]).max())
    print(f"({S}, {T}): smallest one-step margin {min(low):.3e}; the fp32 oracle's deviation {min(dev):.2e} .. {max(dev):.2e}")
    assert min(low) >= ONE_STEP_FLOOR > MARGIN
    assert max(dev) <= 1.2e-3  # (what "fp32 at lambda_accel <= 50" means in the header: 1.05e-3 at worst, (3, 33) at (0, 50) with mu 1e-6)


@pytest.mark.parametrize("case", sorted(THREE_STEPS))
def test_three_step_margins_of_the_gpu_tests_inputs(case):
    m64, m32 = _models()
    S, T, trackers = case
    b = CO.clip_inputs(m64, S, T, trackers=trackers)
    low = []
    for (ls, la), pin in zip(SETTINGS, THREE_STEPS[case]):
        r, r32 = (AO.clip_lm(m, b, S, 3, ls, la) for m in (m64, m32))
        np.testing.assert_array_equal(r32["accepted"], r["accepted"])  # (fp32 and fp64 decide alike)
        assert (np.diff(r["loss_hist"], axis=1) <= 0).all()
        low.append(r["margin"].min())
        assert r["margin"].min() >= pin > MARGIN, (ls, la, r["margin"].min())
    print(f"{case}: smallest margins at (0, 0.5) / (0, 50) / (0.5, 5): {low[0]:.3e} {low[1]:.3e} {low[2]:.3e}")


@pytest.mark.parametrize("case", sorted(KEPT_OUT))
def test_margins_of_the_two_cases_the_gpu_tests_keep_out(case):
    m64 = _models()[0]
    S, T, trackers, ls, la = case
    r = AO.clip_lm(m64, CO.clip_inputs(m64, S, T, trackers=trackers), S, 3, ls, la)
    lo, hi = KEPT_OUT[case]
    print(f"{case}: smallest margin {r['margin'].min():.3e}")
    assert lo <= r["margin"].min() <= hi


def test_infill_from_the_velocity_at_the_start_of_the_gap():
    m64, m32 = _models()
    S, T = 2, 9
    b = CO.infill_inputs(m64, S, T, keep=(0, 1, T - 1))
    r, r32 = (AO.clip_lm(m, b, S, 3, 0.0, 5.0, lam_tmp=0.0) for m in (m64, m32))
    first = CO.clip_lm(m64, b, S, 3, 5.0, lam_tmp=0.0)
    assert r["solved"].all() and (r["n_accepted"] == 3).all()
    np.testing.assert_array_equal(r32["accepted"], r["accepted"])
    inner = np.abs(r["z"] - first["z"]).reshape(T, S, 24)[2:T - 1].max(axis=(1, 2))
    print(f"in-fill (2, 9) lambda_accel 5: smallest margin {r['margin'].min():.3e}, fp32 oracle max |dz| {np.abs(r32['z'] - r['z']).max():.2e}, "
          f"interior frames against the first-difference solve {inner.min():.3e} .. {inner.max():.3e}")
    assert r["margin"].min() >= 0.1 and inner.min() > 1e-2  # (the GPU test's bar is of the order of 4e-5)
    # without either coupling a frame without data rejects every trial; the second-difference term alone makes the matrix definite
    none = AO.clip_lm(m64, b, S, 1, 0.0, 0.0, lam_tmp=0.0)
    assert not none["solved"].any()

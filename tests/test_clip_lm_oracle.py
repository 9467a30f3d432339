"""CPU: the oracle of dp_optimize_clip_lm (tests/clip_lm_oracle.py) against itself -- the block recursion against a dense Cholesky of the whole
sequence's matrix in fp64, the loss that never rises, T = 1 against tests/lm_oracle.py, the certain rejection, the in-fill case, and the
decision margins of the inputs tests/test_hip_clip_lm.py runs (pinned here, so that the GPU test's claim about which sequences are compared
rests on numbers a CPU run can reproduce)."""
import functools

import numpy as np
import pytest
import torch

import clip_lm_oracle as CO
import lm_oracle as LO
from oracle import ref_torch as R

MARGIN = 1e-3  # tests/test_hip_lm.py's: a step whose oracle margin is below this may be decided either way


@functools.lru_cache(maxsize=None)
def _models():
    return R.OracleModel(dtype=torch.float64), R.OracleModel(dtype=torch.float32)


@pytest.mark.parametrize("S,T", [(1, 1), (1, 2), (2, 3), (1, 33), (1, 130)])
@pytest.mark.parametrize("mu", [1e-2, 1e-6])
def test_the_recursion_equals_a_dense_solve_in_fp64(S, T, mu):
    m64 = _models()[0]
    b = CO.clip_inputs(m64, S, T, trackers=6)
    worst = 0.0
    for ls in (0.5, 5.0, 50.0):
        a = CO.clip_lm(m64, b, S, 1, ls, mu=np.full(S, mu))
        d = CO.clip_lm(m64, b, S, 1, ls, mu=np.full(S, mu), dense=True)
        assert a["solved"].all() and d["solved"].all()
        worst = max(worst, np.abs(a["delta"][0] - d["delta"][0]).max())
        np.testing.assert_array_equal(a["accepted"], d["accepted"])
    print(f"S={S} T={T} mu={mu:g}: recursion against the dense solve, max |difference| {worst:.2e}")
    assert worst <= 1e-10


def test_the_loss_never_increases_and_the_history_is_the_kept_loss():
    m64 = _models()[0]
    b = CO.clip_inputs(m64, 3, 9, trackers=3)
    for ls in (0.0, 0.5, 50.0):
        r = CO.clip_lm(m64, b, 3, 5, ls)
        h = r["loss_hist"]
        assert (np.diff(h, axis=1) <= 0).all()
        assert ((np.diff(h, axis=1) < 0) == r["accepted"]).all()
        np.testing.assert_array_equal(h[:, -1], r["clip_loss"][:, 0])
        # the returned pair is the loss of the returned latents
        t = LO._conv(m64, b)
        loss, _ = LO.forward(m64, torch.as_tensor(r["z"]), t, 1.0, 0.02)
        tot, cp = CO.totals(loss, torch.as_tensor(r["z"]).reshape(9, 3, 24), ls / 24.0)
        np.testing.assert_allclose(r["clip_loss"], torch.stack((tot, cp), 1).numpy(), rtol=1e-12)
        assert (r["clip_loss"][:, 1] == 0).all() == (ls == 0.0)


def test_one_frame_is_the_per_frame_problem():
    m64 = _models()[0]
    b = CO.clip_inputs(m64, 7, 1, trackers=3)
    ref = LO.lm(m64, b, 3)
    for ls in (0.0, 3.0):
        got = CO.clip_lm(m64, b, 7, 3, ls)
        np.testing.assert_allclose(got["z"], ref["z"], rtol=0, atol=1e-12)
        np.testing.assert_array_equal(got["n_accepted"], ref["n_accepted"])
        np.testing.assert_allclose(got["mu"], ref["mu"], rtol=1e-15)
        np.testing.assert_allclose(got["loss_hist"], ref["loss_hist"], rtol=1e-12)


def test_without_coupling_the_frames_decouple_but_the_decision_is_the_sequences():
    m64 = _models()[0]
    b = CO.clip_inputs(m64, 2, 4, trackers=6)
    one = CO.clip_lm(m64, b, 2, 1, 0.0)
    per = LO.lm(m64, b, 1)
    A, g = LO.normal_equations(m64, torch.as_tensor(b["z0"], dtype=torch.float64), LO._conv(m64, b), 1.0, 0.02)
    H = A + 1e-2 * (A * torch.eye(24, dtype=torch.float64))
    delta = torch.linalg.solve(H, -g[..., None])[..., 0].numpy()
    np.testing.assert_allclose(one["delta"][0], delta, rtol=0, atol=1e-10)
    assert one["n_accepted"].tolist() == [1, 1] and per["n_accepted"].tolist() == [1] * 8


def test_a_frame_without_data_and_without_coupling_rejects_every_trial():
    for m in _models():
        b = {k: np.array(v) for k, v in CO.clip_inputs(m, 2, 5, trackers=6).items()}
        w = b["w"].reshape(5, 2, 22, 2)
        w[2, 1] = 0  # frame 2 of sequence 1: A_t = 0 exactly with lambda_tmp = 0
        r = CO.clip_lm(m, dict(b, w=w.reshape(10, 22, 2)), 2, 3, 0.0, lam_tmp=0.0)
        assert not r["solved"][1].any() and r["solved"][0].all()
        assert r["n_accepted"][1] == 0 and r["n_accepted"][0] > 0
        assert r["mu"][1] == pytest.approx(1e-2 * 4.0 ** 3) and np.isinf(r["margin"][1]).all()
        np.testing.assert_array_equal(r["z"][1::2], b["z0"][1::2])


def test_infill_frames_follow_their_neighbours():
    m64, m32 = _models()
    b = CO.infill_inputs(m64, 2, 9, keep=(0, 4, 8))
    r = CO.clip_lm(m64, b, 2, 3, 5.0, lam_tmp=0.0)
    r32 = CO.clip_lm(m32, b, 2, 3, 5.0, lam_tmp=0.0)
    assert r["solved"].all() and r["n_accepted"].min() >= 1
    print(f"in-fill (2, 9): loss history {r['loss_hist'].tolist()}, smallest margin {r['margin'].min():.3e}, fp32 oracle max |dz| {np.abs(r32['z'] - r['z']).max():.2e}")
    np.testing.assert_array_equal(r32["accepted"], r["accepted"])
    assert r["margin"].min() >= MARGIN
    # a frame without data moves only through the coupling: after the first accepted step it lies nearer the mean of its neighbours
    Z0, Z = b["z0"].reshape(9, 2, 24).astype(np.float64), r["z"].reshape(9, 2, 24)
    gap = lambda A: np.linalg.norm(A[1:-1] - 0.5 * (A[:-2] + A[2:]), axis=-1)
    free = [1, 2, 3, 5, 6, 7]
    assert (gap(Z)[np.array(free) - 1] < gap(Z0)[np.array(free) - 1]).all()


# (S, T), trackers -> the smallest decision margin over 3 steps and lambda_smooth in {0, 0.5, 5}, measured in fp64 (warm recipe, seed 11, mu0 1e-2,
# lambda_tmp 0.02): (5, 7) 3 trackers 2.32e-2, (3, 33) 3 trackers 1.98e-2, (3, 33) 6 trackers 1.59e-2; (5, 7) 6 trackers 1.7e-5 .. 8.0e-4, below MARGIN
PINNED = {((5, 7), 3): 1.98e-2, ((3, 33), 3): 1.98e-2, ((3, 33), 6): 1.58e-2}


@pytest.mark.parametrize("shape", [(5, 7), (3, 33)])
@pytest.mark.parametrize("trackers", [3, 6])
def test_margins_of_the_gpu_tests_inputs(shape, trackers):
    m64, m32 = _models()
    S, T = shape
    b = CO.clip_inputs(m64, S, T, trackers=trackers)
    low = []
    for ls in (0.0, 0.5, 5.0):
        r, r32 = CO.clip_lm(m64, b, S, 3, ls), CO.clip_lm(m32, b, S, 3, ls)
        np.testing.assert_array_equal(r32["accepted"], r["accepted"])  # (fp32 and fp64 decide alike in all twelve cells)
        assert (np.diff(r["loss_hist"], axis=1) <= 0).all()
        low.append(r["margin"].min())
    print(f"{shape} {trackers} trackers: smallest margins at lambda_smooth 0 / 0.5 / 5: {low[0]:.3e} {low[1]:.3e} {low[2]:.3e}")
    if (shape, trackers) in PINNED:
        assert min(low) >= PINNED[(shape, trackers)] > MARGIN  # these cases leave no sequence out: they carry the GPU test's claim
    else:
        assert 1.5e-5 <= min(low) and max(low) <= 9e-4  # every cell of this case has a step below MARGIN

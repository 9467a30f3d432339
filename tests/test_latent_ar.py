"""CPU: dragposer_amd.LatentAR -- the closed forms, predict()'s stated fp32 order, the least-squares fit and its windows, files, and what
the constructor refuses.  The launch that evaluates the same arithmetic on the device is tests/test_hip_latent_ar.py."""
import numpy as np
import pytest
import torch

from dragposer_amd import LatentAR


def _tracks(n=40, T=14, seed=3):
    """noise-free tracks of a known stable order-2 model, each from a random start: -> (tracks, A [2,24,24], c, the companion matrix's
    spectral radius)"""
    g = np.random.default_rng(seed)
    A1 = 0.5 * np.eye(24) + g.standard_normal((24, 24)) * 0.08
    A2 = -0.2 * np.eye(24) + g.standard_normal((24, 24)) * 0.05
    c = 0.1 * g.standard_normal(24)
    out = []
    for _ in range(n):
        z = [g.standard_normal(24), g.standard_normal(24)]
        for _ in range(2, T):
            z.append(c + A1 @ z[-1] + A2 @ z[-2])
        out.append(np.array(z))
    comp = np.block([[A1, A2], [np.eye(24), np.zeros((24, 24))]])
    return out, np.stack([A1, A2]), c, float(np.abs(np.linalg.eigvals(comp)).max())


def _buffer(S=5, H=7, seed=0):
    return torch.randn(S, H, 24, generator=torch.Generator().manual_seed(seed))


def test_hold_returns_the_newest_row_bit_for_bit():
    lb = _buffer()
    ar = LatentAR.hold()
    assert ar.order == 1 and torch.equal(ar.predict(lb), lb[:, -1])
    assert torch.equal(ar.predict(lb[0]), lb[0, -1])          # [H,24] -> [24]
    assert torch.equal(ar.predict(lb[:, -1:]), lb[:, -1])     # a history of exactly one row


def test_constant_velocity_extrapolates_a_linear_track():
    t = torch.arange(6, dtype=torch.float32)[:, None]
    track = (0.25 * t + (torch.arange(24, dtype=torch.float32) / 8 - 1.5)[None]).unsqueeze(0)  # [1,6,24]: multiples of 1/8, steps of 1/4 (every product and sum below is exact in fp32)
    cv = LatentAR.constant_velocity()
    assert cv.order == 2 and np.array_equal(cv.A[0], 2 * np.eye(24, dtype=np.float32)) and np.array_equal(cv.A[1], -np.eye(24, dtype=np.float32))
    assert torch.equal(cv.predict(track[:, :5]), track[:, 5])
    half = LatentAR.constant_velocity(0.5)  # h_1 + 0.5 (h_1 - h_2)
    assert torch.equal(half.predict(track[:, :5]), track[:, 4] + 0.125)
    assert torch.equal(LatentAR.constant_velocity(0.0).predict(track), track[:, -1])


def test_predict_is_the_stated_fp32_order_and_close_to_float64():
    g = np.random.default_rng(11)
    ar = LatentAR(g.standard_normal((4, 24, 24)) * 0.2, g.standard_normal(24))
    lb = _buffer(S=6, H=9, seed=4)
    got = ar.predict(lb)
    # the header's loop, one rounded product and one rounded sum at a time, in numpy float32
    h = lb.numpy()
    want = np.empty((6, 24), np.float32)
    for s in range(6):
        for i in range(24):
            acc = np.float32(ar.c[i])
            for k in range(4):
                for j in range(24):
                    acc = np.float32(acc + np.float32(ar.A[k, i, j] * h[s, 9 - 1 - k, j]))
            want[s, i] = acc
    assert np.array_equal(got.numpy(), want)
    # against float64: 97 terms of magnitude <= m, each rounded once and summed with one rounding each -- |error| <= 2 * 97 * eps32 * sum |terms|
    A64, h64 = ar.A.astype(np.float64), h.astype(np.float64)
    exact = ar.c.astype(np.float64) + sum(h64[:, 9 - 1 - k] @ A64[k].T for k in range(4))
    mass = np.abs(ar.c.astype(np.float64)) + sum(np.abs(h64[:, 9 - 1 - k]) @ np.abs(A64[k]).T for k in range(4))
    assert (np.abs(got.numpy().astype(np.float64) - exact) <= 2 * 97 * np.finfo(np.float32).eps * mass).all()
    assert np.abs(got.numpy() - exact).max() > 0.0  # (fp32 it is)


def test_fit_agrees_with_lstsq_on_the_same_design_matrix():
    """least_squares (a QR factorisation) against numpy.linalg.lstsq (an SVD) on the design matrix stacked here, in float64, on noise-free
    tracks of a known stable order-2 model (40 tracks of 14 frames: 480 windows, 49 unknowns per component, condition number 17).
    Measured: max |difference| = 1.29e-15 (and 8.9e-16 from the generating model).  The bar is 100 times the measured difference: 1.3e-13."""
    tracks, A, c, rho = _tracks()
    assert rho < 1.0
    X = np.concatenate([np.concatenate([z[1:-1], z[:-2], np.ones((len(z) - 2, 1))], axis=1) for z in tracks])  # [z[t-1], z[t-2], 1]
    Y = np.concatenate([z[2:] for z in tracks])
    W = np.linalg.lstsq(X, Y, rcond=None)[0]
    A64, c64 = LatentAR.least_squares(tracks, 2)
    diff = max(np.abs(A64[0] - W[:24].T).max(), np.abs(A64[1] - W[24:48].T).max(), np.abs(c64 - W[48]).max())
    print(f"least_squares against lstsq: {diff:.3e}; against the generating model: {max(np.abs(A64 - A).max(), np.abs(c64 - c).max()):.3e}")
    assert diff <= 1.3e-13
    Xd, Yd = LatentAR.design(tracks, 2)
    assert np.array_equal(Xd, X) and np.array_equal(Yd, Y)
    m = LatentAR.fit(tracks, 2)
    assert m.A.dtype == np.float32 and np.array_equal(m.A, A64.astype(np.float32)) and np.array_equal(m.c, c64.astype(np.float32))
    # the fitted model continues a track it has not seen
    held_out = _tracks(n=1, seed=3)[0][0]
    nxt = m.predict(torch.from_numpy(held_out[:-1].astype(np.float32)))
    assert np.abs(nxt.numpy() - held_out[-1]).max() < 1e-5
    # ridge shrinks the coefficients and leaves the bias row free
    r = LatentAR.fit(tracks, 2, ridge=10.0)
    assert np.linalg.norm(r.A) < np.linalg.norm(m.A) and np.abs(r.A - m.A).max() > 1e-3


def test_windows_do_not_cross_track_boundaries():
    tracks, _, _, _ = _tracks(n=30)
    g = np.random.default_rng(5)
    tracks = [z + 0.01 * g.standard_normal(z.shape) for z in tracks]  # (noise: a window across a boundary then changes the solution)
    X, _ = LatentAR.design(tracks, 2)
    assert X.shape == (30 * (14 - 2), 49)
    Xc, _ = LatentAR.design([np.concatenate(tracks)], 2)
    assert Xc.shape == (30 * 14 - 2, 49)                      # 2 more windows per boundary
    two, cat = LatentAR.fit(tracks, 2), LatentAR.fit([np.concatenate(tracks)], 2)
    assert np.abs(two.A - cat.A).max() > 1e-4
    # a track no longer than the order contributes nothing
    short = LatentAR.fit(tracks + [tracks[0][:2]], 2)
    assert np.array_equal(short.A, two.A) and np.array_equal(short.c, two.c)


def test_save_and_load(tmp_path):
    g = np.random.default_rng(2)
    ar = LatentAR(g.standard_normal((3, 24, 24)), g.standard_normal(24))
    path = str(tmp_path / "ar.npz")
    ar.save(path)
    back = LatentAR.load(path)
    assert back.order == 3 and np.array_equal(back.A, ar.A) and np.array_equal(back.c, ar.c)
    with np.load(path) as f:
        assert sorted(f.files) == ["A", "c"] and f["A"].dtype == np.float32


def test_shape_and_order_errors():
    eye = np.eye(24)
    assert LatentAR(eye).order == 1  # [24,24] is order 1
    for A, c, word in ((np.zeros((2, 24, 23)), None, "A must be"), (np.zeros((0, 24, 24)), None, "outside 1..4"), (np.zeros((5, 24, 24)), None, "outside 1..4"),
                       (eye, np.zeros(23), "c must be"), (eye * np.nan, None, "non-finite"), (eye, np.full(24, np.inf), "non-finite")):
        with pytest.raises(ValueError, match=word):
            LatentAR(A, c)
    cv = LatentAR.constant_velocity()
    with pytest.raises(ValueError, match="shorter than the order 2"):
        cv.predict(torch.zeros(3, 1, 24))
    with pytest.raises(ValueError, match="fp32"):
        cv.predict(torch.zeros(3, 4, 24, dtype=torch.float64))
    with pytest.raises(ValueError, match="fp32"):
        cv.predict(torch.zeros(3, 4, 23))
    tracks = _tracks(n=3)[0]
    for order in (0, 5):
        with pytest.raises(ValueError, match="outside 1..4"):
            LatentAR.fit(tracks, order)
    with pytest.raises(ValueError, match=r"must be \[T,24\]"):
        LatentAR.fit([np.zeros((10, 23))], 2)
    with pytest.raises(ValueError, match="no track is longer"):
        LatentAR.fit([np.zeros((2, 24))], 2)
    with pytest.raises(ValueError, match="windows for 49 unknowns"):
        LatentAR.fit(tracks, 2)                               # 36 windows
    with pytest.raises(ValueError, match="rank-deficient"):
        LatentAR.fit([np.ones((200, 24))], 2)
    with pytest.raises(ValueError, match="ridge must be"):
        LatentAR.fit(tracks, 2, ridge=-1.0)
    assert LatentAR.fit(tracks, 2, ridge=1e-3).order == 2     # ridge determines what the tracks alone do not

"""GPU (MI355X): dp_optimize_clip_lm_accel (include/dragposer_clip_accel.h) -- dp_optimize_clip_lm's clips with a second-difference term in
the loss -- against the fp64 oracle (tests/clip_accel_oracle.py): one step and three, by tests/test_hip_clip_lm.py's comparison (the latents
within max(4 x the fp32 oracle's own deviation from the fp64 one, 1e-6 of the latents' largest element), mu and the decisions, no sequence
left out), accel = 0.0 against dp_optimize_clip_lm bit for bit, the in-fill case, repeatability (two launches, graph replays, subsets of
outputs), a refused frame, a bf16-rounded context, and eval_drag --smooth-accel on a few frames.  The margins of these inputs are pinned on the
CPU in tests/test_clip_accel_oracle.py."""
import functools

import numpy as np
import pytest
import torch

import clip_accel_oracle as AO
import clip_lm_oracle as CO
import lm_oracle as LO
from oracle import ref_torch as R
from test_hip_clip_lm import LAM_TMP, _against_the_oracle, _rows

pytestmark = pytest.mark.gpu
# no second-difference window (T <= 2); one window, diagonal 1, 4, 1; 1, 5, 5, 1; the first full interior row; a ragged last workgroup of the
# rows kernel (35 frames, 4 per workgroup); 33 frames; a chain longer than a wave is wide
SHAPES = [(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (5, 7), (3, 33), (2, 65)]
SETTINGS = [(0.0, 0.5), (0.0, 50.0), (0.5, 5.0)]  # (lambda_smooth, lambda_accel)


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
def _inputs(S, T, trackers):
    return CO.clip_inputs(_models()[0], S, T, trackers=trackers)


@functools.lru_cache(maxsize=None)
def _oracles(S, T, trackers, steps, ls, la, mu):
    """(fp64, fp32) oracle runs of one case, computed once and shared"""
    b = _inputs(S, T, trackers)
    kw = {} if mu is None else dict(mu=np.full(S, mu))
    return tuple(AO.clip_lm(m, b, S, steps, ls, la, lam_tmp=LAM_TMP, **kw) for m in _models())


def _clip(steps, smooth, accel, **kw):
    from dragposer_amd import ClipLM

    return ClipLM(steps=steps, smooth=smooth, accel=accel, **kw)


def _run(opt, b, S, dev, clip, mu=None, lambda_tmp=LAM_TMP, **kw):
    from dragposer_amd.optimizer import to_device_batch

    d = to_device_batch(b, dev)
    out = opt.optimize_clip_lm(**d, n_sequences=S, clip=clip, lambda_tmp=lambda_tmp,
                               mu=torch.from_numpy(np.asarray(mu, np.float32).copy()).to(dev) if mu is not None else None, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _accel_loss_is_the_latents(got, S, T, la, label):
    """accel_loss is a double sum over the returned fp32 latents, so the oracle's sum over those same latents is what it is held to: within 1e-9
    of it, relative to itself or to the sequence's total (the orders of the additions differ, nothing else)"""
    want = AO.accel_coupling(torch.as_tensor(got["z"]).reshape(T, S, 24), la / 24.0).numpy()
    err = np.abs(got["accel_loss"] - want)
    print(f"  {label}: accel_loss {got['accel_loss'].tolist()}, largest difference from the oracle's sum over the returned latents {err.max():.2e}")
    assert (err <= 1e-9 * np.maximum(want, got["clip_loss"][:, 0])).all(), (got["accel_loss"], want)
    assert (got["accel_loss"] <= got["clip_loss"][:, 1] * (1 + 1e-12)).all()  # (a part of the coupling part)


@pytest.mark.parametrize("S,T", SHAPES)
def test_one_step_against_the_fp64_oracle(opts, dev, S, T):
    b = _inputs(S, T, 3)
    for ls, la in SETTINGS:
        for mu in (1e-2, 1e-6):
            ref, r32 = _oracles(S, T, 3, 1, ls, la, mu)
            got = _run(opts["fp32"], b, S, dev, _clip(1, ls, la), mu=np.full(S, mu))
            label = f"({S}, {T}) lambda_smooth {ls} lambda_accel {la} mu {mu:g}"
            _against_the_oracle(got, ref, r32, S, T, label, allow_out=0)  # (every one-step margin is 5e-2 or more: tests/test_clip_accel_oracle.py)
            assert (got["status"] == 0).all() and (got["iters"] == 1).all() and (got["info"] == 0).all()
            np.testing.assert_array_equal(got["z"], got["z_pre"])
            h = got["loss_hist"]
            assert h.shape == (S, 2) and (h[:, 1] <= h[:, 0]).all() and ((h[:, 1] < h[:, 0]) == (got["n_accepted"] == 1)).all()
            np.testing.assert_array_equal(h[:, 1], got["clip_loss"][:, 0])
            _accel_loss_is_the_latents(got, S, T, la, label)
            if T <= 2:
                assert (got["accel_loss"] == 0).all()
            # the forward results belong to the returned latents
            fwd = LO.forward_np(_models()[0], got["z"].astype(np.float64), b, 1.0, LAM_TMP)
            assert np.linalg.norm(got["pos"] - fwd["pos"], axis=-1).max() * 1000.0 < 0.05
            np.testing.assert_allclose(got["loss"], fwd["loss"], rtol=2e-3, atol=1e-8)


# Two cases are kept out, for the oracle's margins alone (tests/test_clip_accel_oracle.py pins them): (1, 3) with 3 trackers at (0, 0.5), whose only
# sequence has a step with margin 9.0e-4, below MARGIN, so nothing would be compared; and (2, 65) with 3 trackers at (0, 50), margin 1.05e-3, so
# close to MARGIN that an fp32 decision either way is no finding.  (2, 65) runs with 6 trackers instead.  Every case below leaves no sequence out.
SEVERAL = [(S, T, k, ls, la) for (S, T, k) in ((1, 4, 3), (1, 5, 3), (5, 7, 3), (3, 33, 3), (3, 33, 6), (5, 7, 6), (2, 65, 6)) for ls, la in SETTINGS]


@pytest.mark.parametrize("S,T,trackers,ls,la", SEVERAL)
def test_three_steps_against_the_fp64_oracle(opts, dev, S, T, trackers, ls, la):
    b = _inputs(S, T, trackers)
    ref, r32 = _oracles(S, T, trackers, 3, ls, la, None)
    got = _run(opts["fp32"], b, S, dev, _clip(3, ls, la))  # (mu=None: every sequence starts at mu0)
    label = f"({S}, {T}) {trackers} trackers lambda_smooth {ls} lambda_accel {la}"
    _against_the_oracle(got, ref, r32, S, T, label, allow_out=0)
    assert (got["status"] == 0).all() and (got["iters"] == 3).all()
    assert (np.diff(got["loss_hist"], axis=1) <= 0).all()  # the loss never increases
    assert ((np.diff(got["loss_hist"], axis=1) < 0).sum(1) == got["n_accepted"]).all()
    _accel_loss_is_the_latents(got, S, T, la, label)


@pytest.mark.parametrize("S,T", [(5, 7), (2, 65)])
def test_accel_zero_is_dp_optimize_clip_lm_bit_for_bit(opts, dev, S, T):
    b = _inputs(S, T, 3)
    old = _run(opts["fp32"], b, S, dev, _clip(3, 0.5, None))
    new = _run(opts["fp32"], b, S, dev, _clip(3, 0.5, 0.0))
    assert set(new) == set(old) | {"accel_loss"}
    for k in old:
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
    assert (new["accel_loss"] == 0).all() and (old["n_accepted"] > 0).any()  # (steps were taken: the equality is not that of two idle launches)


def test_infill_is_a_curve_not_a_polyline(opts, dev):
    """frames 0, 1 and T-1 carry data, the others none: with the acceleration term alone the gap is filled from the velocity at its start, which
    the first-difference solve cannot see"""
    m64, m32 = _models()
    S, T = 2, 9
    b = CO.infill_inputs(m64, S, T, keep=(0, 1, T - 1))
    ref, r32 = (AO.clip_lm(m, b, S, 3, 0.0, 5.0, lam_tmp=0.0) for m in (m64, m32))
    got = _run(opts["fp32"], b, S, dev, _clip(3, 0.0, 5.0), lambda_tmp=0.0)
    _against_the_oracle(got, ref, r32, S, T, "in-fill (2, 9) lambda_accel 5", allow_out=0)
    assert (got["status"] == 0).all() and (got["n_accepted"] >= 1).all()
    first = _run(opts["fp32"], b, S, dev, _clip(3, 5.0, None), lambda_tmp=0.0)
    bar = max(4.0 * np.abs(r32["z"] - ref["z"]).max(), 1e-6 * np.abs(ref["z"]).max())
    inner = np.abs(got["z"] - first["z"]).reshape(T, S, 24)[2:T - 1].max(axis=(1, 2))
    print(f"in-fill: interior frames differ from the first-difference solve by {inner.tolist()}, bar {bar:.3e}")
    assert (inner > bar).all()


def test_repeatable_subsets_and_graph_capture(opts, dev):
    from dragposer_amd.optimizer import to_device_batch

    opt, (S, T) = opts["fp32"], (3, 33)
    b = _inputs(S, T, 3)
    clip = _clip(3, 0.5, 5.0)
    a = _run(opt, b, S, dev, clip)
    c = _run(opt, b, S, dev, clip)
    filled = _run(opt, b, S, dev, clip, mu=np.full(S, 1e-2))
    for k in a:
        np.testing.assert_array_equal(a[k], c[k], err_msg=k)
        np.testing.assert_array_equal(a[k], filled[k], err_msg=k)
    for names in (("z",), ("pos", "clip_loss"), ("accel_loss",), ("loss", "iters", "n_accepted", "accel_loss"), ("status", "loss_hist", "info")):
        part = _run(opt, b, S, dev, clip, outputs=names)
        assert set(part) == set(names) | {"mu"}
        for k in part:
            np.testing.assert_array_equal(part[k], a[k], err_msg=k)
    d = to_device_batch(b, dev)
    out = opt.allocate_outputs(S * T)
    out.update(n_accepted=torch.empty(S, dtype=torch.int32, device=dev), info=torch.empty(S, dtype=torch.int32, device=dev),
               clip_loss=torch.empty(S, 2, dtype=torch.float64, device=dev), loss_hist=torch.empty(S, 4, dtype=torch.float64, device=dev),
               accel_loss=torch.empty(S, dtype=torch.float64, device=dev))
    mu = torch.full((S,), 1e-2, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        opt.optimize_clip_lm(**d, n_sequences=S, clip=clip, lambda_tmp=LAM_TMP, mu=mu, out=out, outputs=tuple(out))
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.optimize_clip_lm(**d, n_sequences=S, clip=clip, lambda_tmp=LAM_TMP, mu=mu, out=out, outputs=tuple(out))
    for _ in range(2):
        for v in out.values():
            v.fill_(-1)
        mu.fill_(1e-2)
        graph.replay()
        torch.cuda.synchronize()
        for k in out:
            np.testing.assert_array_equal(out[k].cpu().numpy(), a[k], err_msg=k)
        np.testing.assert_array_equal(mu.cpu().numpy(), a["mu"])


def test_a_refused_frame_stops_its_sequence_and_no_other(opts, dev):
    from dragposer_amd import _lib

    opt, (S, T) = opts["fp32"], (3, 5)
    b = {k: np.array(v) for k, v in _inputs(S, T, 6).items()}
    clip = _clip(3, 0.5, 5.0)
    row = 2 * S + 1  # frame 2 of sequence 1
    others = _rows(S, T, [True, False, True])
    seq1 = np.arange(S * T) % S == 1
    bad = {k: v.copy() for k, v in b.items()}
    bad["tgt_pos"][row, 13, 1] = np.nan  # (joint 13 is tracked in the 6-tracker recipe)
    assert bad["tracked"][row, 13]
    mu_in = np.asarray([0.5, 0.25, 0.125], np.float32)
    got = _run(opt, bad, S, dev, clip, mu=mu_in)
    want = _run(opt, b, S, dev, clip, mu=mu_in)
    assert got["info"].tolist() == [0, _lib.DP_CLIP_REFUSED_FRAME, 0] and (want["info"] == 0).all()
    assert got["n_accepted"][1] == 0 and got["mu"][1] == mu_in[1] and np.isnan(got["clip_loss"][1]).all() and np.isnan(got["loss_hist"][1]).all()
    assert np.isnan(got["accel_loss"][1])
    assert (got["iters"][seq1] == 0).all() and (got["iters"][others] == 3).all()
    assert got["status"][row] == _lib.DP_STATUS_NONFINITE_RESULT | _lib.DP_STATUS_BAD_TARGETS and np.isnan(got["z"][row]).all()
    rest = seq1 & (np.arange(S * T) != row)  # the sequence's other frames: their z0
    assert got["z"][rest].tobytes() == bad["z0"][rest].astype(np.float32).tobytes() and (got["status"][rest] == 0).all()
    # the other sequences: the bits of the launch without the fault
    for k in ("z", "z_pre", "pose", "pos", "rot", "world_rot", "disp", "world_disp", "loss", "iters", "status"):
        np.testing.assert_array_equal(got[k][others], want[k][others], err_msg=k)
    for k in ("mu", "n_accepted", "clip_loss", "loss_hist", "info", "accel_loss"):
        np.testing.assert_array_equal(got[k][[0, 2]], want[k][[0, 2]], err_msg=k)


def test_a_bf16_rounded_context_meets_its_own_oracle(opts, dev):
    S, T = 3, 33
    b = _inputs(S, T, 3)
    mb64, mb32 = (R.OracleModel(dtype=dt, weight_rounding="bf16") for dt in (torch.float64, torch.float32))
    ref, r32 = (AO.clip_lm(m, b, S, 3, 0.5, 5.0, lam_tmp=LAM_TMP) for m in (mb64, mb32))
    got = _run(opts["bf16"], b, S, dev, _clip(3, 0.5, 5.0))
    _against_the_oracle(got, ref, r32, S, T, "bf16 context (3, 33) lambda_smooth 0.5 lambda_accel 5", allow_out=0)
    assert (got["status"] == 0).all()


def test_eval_drag_smooth_accel(dev, tmp_path, capsys):
    """12 frames of tests/data/example_clip.bvh through eval_drag --smooth 0:2 --smooth-accel 5, the acceleration-only second pass: it runs,
    prints its line, and lowers the jitter; --smooth-accel alone and a bad value are refused"""
    import os

    from dragposer_amd import eval_drag

    clip = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "example_clip.bvh")
    base = [clip, "--max-frames", "12", "--out-dir", str(tmp_path)]
    r = eval_drag.main(base + ["--smooth", "0:2", "--smooth-accel", "5"])[0]
    text = capsys.readouterr().out
    assert "lambda_accel 5" in text, text
    h = r["smooth_loss_hist"]
    assert r["smooth_accel"] == 5.0 and h.shape == (3,) and (np.diff(h) <= 0).all() and h[-1] < h[0] and 1 <= r["smooth_accepted"] <= 2
    assert np.isfinite([r["mpjpe"], r["mpjpe_smooth"], r["jitter"], r["jitter_smooth"]]).all()
    print(f"eval_drag --smooth 0:2 --smooth-accel 5: jitter {r['jitter']:.4f} -> {r['jitter_smooth']:.4f}, MPJPE {r['mpjpe']:.4f} -> {r['mpjpe_smooth']:.4f}")
    assert r["jitter_smooth"] < r["jitter"]
    with pytest.raises(SystemExit, match="--smooth-accel requires --smooth"):
        eval_drag.main(base + ["--smooth-accel", "5"])
    for bad in ("-1", "nan", "x"):
        with pytest.raises(SystemExit, match="--smooth-accel: expected"):
            eval_drag.main(base + ["--smooth", "0:2", "--smooth-accel", bad])

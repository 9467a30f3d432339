"""GPU (MI355X): dp_optimize_clip_lm (include/dragposer_clip_lm.h) -- S sequences of T frames solved jointly, the latents tied frame to
frame -- against the fp64 oracle (tests/clip_lm_oracle.py): one step and several (the latents within max(4 x the fp32 oracle's own deviation
from the fp64 one, 1e-6 of the latents' largest element), mu and the decisions, on sequences whose oracle margin is at least MARGIN), T = 1
against dp_optimize_lm, the in-fill case and its certain rejection, repeatability (two launches, graph replays, subsets of outputs), a refused
frame, a bf16-rounded context, and eval_drag --smooth on a few frames.  The margins of these inputs are pinned on the CPU in tests/test_clip_lm_oracle.py."""
import functools

import numpy as np
import pytest
import torch

import clip_lm_oracle as CO
import lm_oracle as LO
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu
MARGIN = 1e-3  # tests/test_hip_lm.py's: a step whose oracle margin |L' - L| / L is below this may be decided either way
SHAPES = [(1, 1), (1, 2), (1, 3), (5, 7), (3, 33), (2, 65)]  # one block; both end blocks adjacent; one interior block; a ragged last workgroup
                                                              # (35 frames, 4 per workgroup); a chain longer than a wave is wide
LAM_TMP = 0.02


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
def _oracles(S, T, trackers, steps, ls, mu):
    """(fp64, fp32) oracle runs of one case, computed once and shared"""
    b = _inputs(S, T, trackers)
    kw = {} if mu is None else dict(mu=np.full(S, mu))
    return tuple(CO.clip_lm(m, b, S, steps, ls, lam_tmp=LAM_TMP, **kw) for m in _models())


def _clip(steps, smooth, **kw):
    from dragposer_amd import ClipLM

    return ClipLM(steps=steps, smooth=smooth, **kw)


def _run(opt, b, S, dev, clip, mu=None, lambda_tmp=LAM_TMP, **kw):
    from dragposer_amd.optimizer import to_device_batch

    d = to_device_batch(b, dev)
    out = opt.optimize_clip_lm(**d, n_sequences=S, clip=clip, lambda_tmp=lambda_tmp,
                               mu=torch.from_numpy(np.asarray(mu, np.float32).copy()).to(dev) if mu is not None else None, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _rows(S, T, seqs):
    """the rows t * S + s of the sequences in the boolean mask `seqs`"""
    return np.tile(np.asarray(seqs, bool), T)


def _against_the_oracle(got, ref, r32, S, T, label, allow_out):
    """z, mu and the decisions on the sequences none of whose steps has an oracle margin below MARGIN; -> the number left out"""
    sure = (ref["margin"] >= MARGIN).all(1)
    left_out = int((~sure).sum())
    dev32 = np.abs(r32["z"] - ref["z"])[_rows(S, T, sure)].max() if sure.any() else 0.0
    bar = max(4.0 * dev32, 1e-6 * np.abs(ref["z"]).max())
    dz = np.abs(got["z"] - ref["z"])[_rows(S, T, sure)].max() if sure.any() else 0.0
    print(f"{label}: kernel max |dz| {dz:.3e}, fp32 oracle {dev32:.3e}, bar {bar:.3e}, smallest oracle margin {ref['margin'].min():.3e}, "
          f"accepted {ref['n_accepted'].tolist()} (kernel {got['n_accepted'].tolist()}), sequences left out {left_out}/{S}")
    assert left_out <= allow_out, (left_out, S)
    np.testing.assert_array_equal(got["n_accepted"][sure], ref["n_accepted"][sure])
    np.testing.assert_allclose(got["mu"][sure], ref["mu"][sure], rtol=1e-6)
    assert dz <= bar, (dz, bar)
    rel = np.abs(got["clip_loss"][sure] - ref["clip_loss"][sure]).max(initial=0.0) / np.abs(ref["clip_loss"][sure, 0]).max(initial=1.0)
    print(f"  clip_loss: max difference relative to the largest total {rel:.2e}")
    return left_out


@pytest.mark.parametrize("S,T", SHAPES)
def test_one_step_against_the_fp64_oracle(opts, dev, S, T):
    b = _inputs(S, T, 3)
    for ls in (0.0, 0.5, 50.0):
        for mu in (1e-2, 1e-6):
            ref, r32 = _oracles(S, T, 3, 1, ls, mu)
            got = _run(opts["fp32"], b, S, dev, _clip(1, ls), mu=np.full(S, mu))
            _against_the_oracle(got, ref, r32, S, T, f"({S}, {T}) lambda_smooth {ls} mu {mu:g}", allow_out=0)  # (every one-step margin is 0.1 or more)
            assert (got["status"] == 0).all() and (got["iters"] == 1).all() and (got["info"] == 0).all()
            np.testing.assert_array_equal(got["z"], got["z_pre"])
            h = got["loss_hist"]
            assert h.shape == (S, 2) and (h[:, 1] <= h[:, 0]).all() and ((h[:, 1] < h[:, 0]) == (got["n_accepted"] == 1)).all()
            np.testing.assert_array_equal(h[:, 1], got["clip_loss"][:, 0])
            # the forward results belong to the returned latents
            fwd = LO.forward_np(_models()[0], got["z"].astype(np.float64), b, 1.0, LAM_TMP)
            assert np.linalg.norm(got["pos"] - fwd["pos"], axis=-1).max() * 1000.0 < 0.05
            np.testing.assert_allclose(got["loss"], fwd["loss"], rtol=2e-3, atol=1e-8)


# the 3-tracker cases and (3, 33) leave no sequence out in the oracle (tests/test_clip_lm_oracle.py pins their margins): they carry the claim.
# (5, 7) with 6 trackers leaves one of five out at lambda_smooth 0.5 and 5 and three at 0, which is why 0 is not among its cases; (2, 65) runs
# with 6 trackers, where the oracle leaves none out (with 3 it leaves one of two out at lambda_smooth 5).
SEVERAL = [(5, 7, 3, 0.0), (5, 7, 3, 0.5), (5, 7, 3, 5.0), (3, 33, 3, 0.0), (3, 33, 3, 0.5), (3, 33, 3, 5.0), (3, 33, 6, 0.0), (3, 33, 6, 0.5),
           (3, 33, 6, 5.0), (5, 7, 6, 0.5), (5, 7, 6, 5.0), (2, 65, 6, 0.0), (2, 65, 6, 0.5), (2, 65, 6, 5.0)]


@pytest.mark.parametrize("S,T,trackers,ls", SEVERAL)
def test_three_steps_against_the_fp64_oracle(opts, dev, S, T, trackers, ls):
    b = _inputs(S, T, trackers)
    ref, r32 = _oracles(S, T, trackers, 3, ls, None)
    got = _run(opts["fp32"], b, S, dev, _clip(3, ls))  # (mu=None: every sequence starts at mu0)
    carries = trackers == 3 or (S, T) == (3, 33)
    _against_the_oracle(got, ref, r32, S, T, f"({S}, {T}) {trackers} trackers lambda_smooth {ls}", allow_out=0 if carries else S // 5)
    assert (got["status"] == 0).all() and (got["iters"] == 3).all()
    assert (np.diff(got["loss_hist"], axis=1) <= 0).all()  # the loss never increases
    assert ((np.diff(got["loss_hist"], axis=1) < 0).sum(1) == got["n_accepted"]).all()


def test_one_frame_per_sequence_is_dp_optimize_lm(opts, dev):
    from dragposer_amd import LM
    from dragposer_amd.optimizer import to_device_batch

    S = 9
    b = _inputs(S, 1, 3)
    ref, r32 = _oracles(S, 1, 3, 3, 0.7, None)
    got = _run(opts["fp32"], b, S, dev, _clip(3, 0.7))
    per = opts["fp32"].optimize_lm(**to_device_batch(b, dev), lm=LM(3, early_stop=False), lambda_tmp=LAM_TMP)
    torch.cuda.synchronize()
    per = {k: v.cpu().numpy() for k, v in per.items()}
    sure = (ref["margin"] >= MARGIN).all(1)
    bar = max(4.0 * np.abs(r32["z"] - ref["z"])[sure].max(), 1e-6 * np.abs(ref["z"]).max())
    dz = np.abs(got["z"] - per["z"])[sure].max()
    print(f"T = 1: clip against dp_optimize_lm max |dz| {dz:.3e}, bar {bar:.3e}, compared on {int(sure.sum())}/{S}")
    assert sure.sum() >= S - S // 5 and dz <= bar
    np.testing.assert_array_equal(got["n_accepted"][sure], per["n_accepted"][sure])
    np.testing.assert_allclose(got["mu"][sure], per["mu"][sure], rtol=1e-6)
    assert (got["clip_loss"][:, 1] == 0).all()  # (no coupling part)


def test_infill_and_its_certain_rejection(opts, dev):
    m64, m32 = _models()
    S, T = 2, 9
    b = CO.infill_inputs(m64, S, T, keep=(0, 4, 8))
    ref, r32 = (CO.clip_lm(m, b, S, 3, 5.0, lam_tmp=0.0) for m in (m64, m32))
    got = _run(opts["fp32"], b, S, dev, _clip(3, 5.0), lambda_tmp=0.0)
    _against_the_oracle(got, ref, r32, S, T, "in-fill (2, 9) lambda_smooth 5", allow_out=0)
    assert (got["status"] == 0).all()
    # without coupling a frame without data makes every trial a certain rejection: A_t = 0 exactly, the first pivot is 0
    none = _run(opts["fp32"], b, S, dev, _clip(3, 0.0), lambda_tmp=0.0)
    assert (none["n_accepted"] == 0).all() and (none["iters"] == 3).all() and (none["status"] == 0).all()
    np.testing.assert_allclose(none["mu"], np.float32(1e-2) * 64.0, rtol=1e-6)
    assert none["z"].tobytes() == np.asarray(b["z0"], np.float32).tobytes()
    assert (none["loss_hist"] == none["loss_hist"][:, :1]).all()


def test_repeatable_mu_null_subsets_and_graph_capture(opts, dev):
    from dragposer_amd.optimizer import to_device_batch

    opt, (S, T) = opts["fp32"], (3, 33)
    b = _inputs(S, T, 3)
    clip = _clip(3, 0.5)
    a = _run(opt, b, S, dev, clip)
    c = _run(opt, b, S, dev, clip)
    filled = _run(opt, b, S, dev, clip, mu=np.full(S, 1e-2))
    for k in a:
        np.testing.assert_array_equal(a[k], c[k], err_msg=k)
        np.testing.assert_array_equal(a[k], filled[k], err_msg=k)
    for names in (("z",), ("pos", "clip_loss"), ("loss", "iters", "n_accepted"), ("status", "loss_hist", "info"), ("pose", "rot", "world_rot", "disp", "world_disp")):
        part = _run(opt, b, S, dev, clip, outputs=names)
        assert set(part) == set(names) | {"mu"}
        for k in part:
            np.testing.assert_array_equal(part[k], a[k], err_msg=k)
    d = to_device_batch(b, dev)
    out = opt.allocate_outputs(S * T)
    out.update(n_accepted=torch.empty(S, dtype=torch.int32, device=dev), info=torch.empty(S, dtype=torch.int32, device=dev),
               clip_loss=torch.empty(S, 2, dtype=torch.float64, device=dev), loss_hist=torch.empty(S, 4, dtype=torch.float64, device=dev))
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
    from dragposer_amd import LM, _lib
    from dragposer_amd.optimizer import to_device_batch

    opt, (S, T) = opts["fp32"], (3, 5)
    b = {k: np.array(v) for k, v in _inputs(S, T, 6).items()}
    clip = _clip(3, 0.5)
    clean = _run(opt, b, S, dev, clip)
    row = 2 * S + 1  # frame 2 of sequence 1
    others = _rows(S, T, [True, False, True])
    seq1 = np.arange(S * T) % S == 1
    for kind in ("state", "targets"):
        bad = {k: v.copy() for k, v in b.items()}
        if kind == "state":
            bad["z0"][row, 5] = np.nan
        else:
            bad["tgt_pos"][row, 13, 1] = np.nan  # (joint 13 is tracked in the 6-tracker recipe)
            assert bad["tracked"][row, 13]
        mu_in = np.asarray([0.5, 0.25, 0.125], np.float32)
        got = _run(opt, bad, S, dev, clip, mu=mu_in)
        want = _run(opt, b, S, dev, clip, mu=mu_in)
        assert got["info"].tolist() == [0, _lib.DP_CLIP_REFUSED_FRAME, 0]
        assert got["n_accepted"][1] == 0 and got["mu"][1] == mu_in[1] and np.isnan(got["clip_loss"][1]).all() and np.isnan(got["loss_hist"][1]).all()
        assert (got["iters"][seq1] == 0).all() and (got["iters"][others] == 3).all()
        # that frame: what dp_optimize_lm returns for it
        per = opt.optimize_lm(**to_device_batch(bad, dev), lm=LM(3, early_stop=False), lambda_tmp=LAM_TMP)
        torch.cuda.synchronize()
        assert got["status"][row] == int(per["status"][row]) == _lib.DP_STATUS_NONFINITE_RESULT | (_lib.DP_STATUS_BAD_STATE if kind == "state" else _lib.DP_STATUS_BAD_TARGETS)
        for k in ("z", "z_pre", "pose", "pos", "rot", "world_rot", "disp", "world_disp", "loss"):
            np.testing.assert_array_equal(got[k][row], per[k][row].cpu().numpy(), err_msg=k)
        assert np.isnan(got["z"][row]).all() and np.isnan(got["pos"][row]).all() == (kind == "state")
        # the sequence's other frames: the results of their z0
        rest = seq1 & (np.arange(S * T) != row)
        assert got["z"][rest].tobytes() == bad["z0"][rest].astype(np.float32).tobytes() and (got["status"][rest] == 0).all()
        fwd = LO.forward_np(_models()[0], bad["z0"][rest].astype(np.float64), {k: v[rest] for k, v in bad.items()}, 1.0, LAM_TMP)
        assert np.linalg.norm(got["pos"][rest] - fwd["pos"], axis=-1).max() * 1000.0 < 0.05
        np.testing.assert_allclose(got["loss"][rest], fwd["loss"], rtol=2e-3, atol=1e-8)
        # the other sequences: the bits of the launch without the fault
        for k in ("z", "z_pre", "pose", "pos", "rot", "world_rot", "disp", "world_disp", "loss", "iters", "status"):
            np.testing.assert_array_equal(got[k][others], want[k][others], err_msg=k)
        for k in ("mu", "n_accepted", "clip_loss", "loss_hist", "info"):
            np.testing.assert_array_equal(got[k][[0, 2]], want[k][[0, 2]], err_msg=k)
    assert (clean["info"] == 0).all()


def test_a_bf16_rounded_context_meets_its_own_oracle(opts, dev):
    S, T = 3, 33
    b = _inputs(S, T, 3)
    mb64, mb32 = (R.OracleModel(dtype=dt, weight_rounding="bf16") for dt in (torch.float64, torch.float32))
    ref, r32 = (CO.clip_lm(m, b, S, 3, 0.5, lam_tmp=LAM_TMP) for m in (mb64, mb32))
    got = _run(opts["bf16"], b, S, dev, _clip(3, 0.5))
    _against_the_oracle(got, ref, r32, S, T, "bf16 context (3, 33) lambda_smooth 0.5", allow_out=0)
    assert (got["status"] == 0).all()


def test_eval_drag_smooth(dev, tmp_path):
    """12 frames of tests/data/example_clip.bvh through eval_drag --smooth: the second pass starts from the first pass's latents (DragPose's
    keep_latents), lowers the sequence's loss and reports both passes; the flags it does not go with are refused"""
    import os

    from dragposer_amd import eval_drag

    clip = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "example_clip.bvh")
    base = [clip, "--max-frames", "12", "--out-dir", str(tmp_path)]
    for first in ([], ["--solver", "lm:2"]):
        r = eval_drag.main(base + ["--smooth", "5:2:0.1"] + first)[0]
        h = r["smooth_loss_hist"]
        assert h.shape == (3,) and (np.diff(h) <= 0).all() and h[-1] < h[0] and 1 <= r["smooth_accepted"] <= 2
        assert os.path.exists(r["out_smooth"]) and os.path.exists(r["out"]) and r["out_smooth"] != r["out"]
        assert np.isfinite([r["mpjpe"], r["mpjpe_smooth"], r["jitter"], r["jitter_smooth"], r["jitter_gt"]]).all()
        assert abs(r["mpjpe_smooth"] - r["mpjpe"]) < 0.05  # (the second pass starts from the first pass's latents: a wrong hand-over would not stay near)
    for flag in (["--tether", "2:0:1"], ["--gaps", "3:0.5"], ["--foot-lock"], ["--constraints", "reference"], ["--drop", "0:2:3"], ["--calibrate", "uniform"],
                 ["--balance", "0.1:1"], ["--model-skeleton"]):
        with pytest.raises(SystemExit, match="--smooth and " + flag[0]):
            eval_drag.main(base + ["--smooth", "5"] + flag)
    for bad in ("-1", "5:0", "5:2:-0.1", "5:2:0.1:7", "x"):
        with pytest.raises(SystemExit, match="--smooth: expected LAMBDA"):
            eval_drag.main(base + ["--smooth", bad])

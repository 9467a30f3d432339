"""GPU (MI355X): per-sequence skeletons in the joint clip solve and the LM solver (include/dragposer_clip_skeleton.h).  The context's own
skeleton passed on the call gives the plain calls' bits; a launch that mixes skeletons gives every sequence (every frame, in
dp_optimize_lm_skeleton) the bits of the plain call on a context CREATED with that skeleton; against the fp64 oracle
(tests/clip_skel_oracle.py) one step and three, by tests/test_hip_clip_lm.py's comparison and bar, no sequence left out; T = 1 against
dp_optimize_lm_skeleton; a bf16-rounded context; a refused skeleton row; repeatability and a graph replayed after the offsets changed in
place; fit_bones' offsets into the clip solve; eval_drag --smooth on a clip of other bone lengths.  The margins of these inputs, and that
each of them feels its skeleton by at least 10 x the bar, are pinned on the CPU in tests/test_clip_skel_oracle.py."""
import os

import numpy as np
import pytest
import torch

import clip_lm_oracle as CO
import clip_skel_oracle as KO
import lm_oracle as LO
from skeleton_cases import scaled_bvh_text
from test_hip_clip_lm import LAM_TMP, _against_the_oracle, _rows, _run
from test_hip_skeleton import _raw

pytestmark = pytest.mark.gpu
FRAME_OUTS = ("z", "z_pre", "pose", "pos", "rot", "world_rot", "disp", "world_disp", "loss", "iters", "status")
SEQ_OUTS = ("mu", "n_accepted", "clip_loss", "loss_hist", "info")
assert LAM_TMP == KO.LAM_TMP


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def skels():
    return KO.skeletons(KO.base_offsets())


@pytest.fixture(scope="module")
def opts(dev, skels):
    """the shipped model's context (fp32 and bf16-rounded), and one context CREATED with each foreign skeleton (the references)"""
    from dragposer_amd.optimizer import LatentOptimizer

    refs = [None] + [LatentOptimizer(device=dev, arrays=_raw(offsets=s)) for s in skels[1:]]
    refs[0] = LatentOptimizer(device=dev)
    return {"fp32": refs[0], "bf16": LatentOptimizer(device=dev, weight_dtype="bf16"), "refs": refs}


def _clip(steps, smooth, accel=None):
    from dragposer_amd import ClipLM

    return ClipLM(steps=steps, smooth=smooth, accel=accel)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _seq_outs(got):
    return SEQ_OUTS + (("accel_loss",) if "accel_loss" in got else ())


def _lm(opt, b, dev, offsets=None, steps=3):
    from dragposer_amd import LM
    from dragposer_amd.optimizer import to_device_batch

    out = opt.optimize_lm(**to_device_batch(b, dev), lm=LM(steps, early_stop=False), lambda_tmp=LAM_TMP, offsets=offsets)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("S,T", [(5, 7), (2, 65)])
@pytest.mark.parametrize("accel", [None, 5.0])
def test_the_contexts_own_skeleton_gives_the_plain_bits(opts, dev, skels, S, T, accel):
    opt = opts["fp32"]
    b = CO.clip_inputs(KO.models()[0], S, T, trackers=3)
    clip = _clip(3, 0.5, accel)
    plain = _run(opt, b, S, dev, clip)
    assert (plain["n_accepted"] > 0).any()  # (steps were taken: the equality is not that of two idle launches)
    for off in (_dev(skels[0], dev), _dev(np.stack([skels[0]] * S), dev)):  # stride 0, stride 66
        got = _run(opt, b, S, dev, clip, offsets=off)
        assert set(got) == set(plain)
        for k in plain:
            np.testing.assert_array_equal(got[k], plain[k], err_msg=f"{k}, offsets {tuple(off.shape)}")


def test_the_contexts_own_skeleton_gives_dp_optimize_lms_bits_on_every_joint(opts, dev, skels):
    opt = opts["fp32"]
    b = LO.every_joint_inputs(KO.models()[0], warm=True)
    plain = _lm(opt, b, dev)
    assert (plain["n_accepted"] > 0).all() and (plain["status"] == 0).all()
    for off in (_dev(skels[0], dev), _dev(np.stack([skels[0]] * 28), dev)):
        got = _lm(opt, b, dev, offsets=off)
        assert set(got) == set(plain)
        for k in plain:
            np.testing.assert_array_equal(got[k], plain[k], err_msg=f"{k}, offsets {tuple(off.shape)}")


@pytest.mark.parametrize("S,T", [(5, 7), (3, 33)])
@pytest.mark.parametrize("accel", [None, 5.0])
def test_mixed_skeletons_equal_one_context_per_skeleton(opts, dev, skels, S, T, accel):
    """five (three) skeletons across the waves of one workgroup: frame f belongs to sequence f % S"""
    ks = KO.k_of(S)
    b = KO.mixed_inputs(S, T, 3, 11)
    clip = _clip(3, 0.5, accel)
    got = _run(opts["fp32"], b, S, dev, clip, offsets=_dev(np.stack([skels[k] for k in ks]), dev))
    assert (got["status"] == 0).all() and (got["info"] == 0).all() and (got["n_accepted"] > 0).any()
    for k in sorted(set(ks)):
        want = _run(opts["refs"][k], b, S, dev, clip)  # the same batch, every sequence on skeleton k: sequence s with k(s) = k is the one compared
        seqs = np.asarray(ks) == k
        rows = _rows(S, T, seqs)
        for name in FRAME_OUTS:
            np.testing.assert_array_equal(got[name][rows], want[name][rows], err_msg=f"{name}, skeleton {k}")
        for name in _seq_outs(got):
            np.testing.assert_array_equal(got[name][seqs], want[name][seqs], err_msg=f"{name}, skeleton {k}")


def test_mixed_skeletons_per_frame_equal_one_context_per_skeleton_on_every_joint(opts, dev, skels):
    """the 28 frames form every joint's rows of J between them: a wrong bone in any tangent shows"""
    b, ks = KO.every_joint_mixed()
    got = _lm(opts["fp32"], b, dev, offsets=_dev(np.stack([skels[k] for k in ks]), dev))
    assert (got["status"] == 0).all() and (got["n_accepted"] > 0).all()
    for k in range(4):
        want = _lm(opts["refs"][k], b, dev)
        rows = np.asarray(ks) == k
        for name in got:
            np.testing.assert_array_equal(got[name][rows], want[name][rows], err_msg=f"{name}, skeleton {k}")


@pytest.mark.parametrize("S,T", KO.SHAPES)
def test_one_step_against_the_fp64_oracle(opts, dev, S, T):
    for ls, la in KO.SETTINGS:
        b, of_seq, ref, r32 = KO.case(S, T, 3, 1, ls, la, 1e-2, KO.ONE_STEP_SEED.get((S, T), 11))
        got = _run(opts["fp32"], b, S, dev, _clip(1, ls, la), mu=np.full(S, 1e-2), offsets=_dev(np.stack(of_seq), dev))
        _against_the_oracle(got, ref, r32, S, T, f"({S}, {T}) lambda_smooth {ls} lambda_accel {la} mu 0.01", allow_out=0)
        assert (got["status"] == 0).all() and (got["iters"] == 1).all() and (got["info"] == 0).all()
        np.testing.assert_array_equal(got["z"], got["z_pre"])
        h = got["loss_hist"]
        assert h.shape == (S, 2) and (h[:, 1] <= h[:, 0]).all() and ((h[:, 1] < h[:, 0]) == (got["n_accepted"] == 1)).all()
        np.testing.assert_array_equal(h[:, 1], got["clip_loss"][:, 0])
        # the forward results belong to the returned latents, on each sequence's own bones
        for s in range(S):
            rows = np.arange(s, S * T, S)
            fwd = LO.forward_np(KO.with_offsets(KO.models()[0], of_seq[s]), got["z"][rows].astype(np.float64), {k: np.asarray(v)[rows] for k, v in b.items()}, 1.0, LAM_TMP)
            assert np.linalg.norm(got["pos"][rows] - fwd["pos"], axis=-1).max() * 1000.0 < 0.05
            np.testing.assert_allclose(got["loss"][rows], fwd["loss"], rtol=2e-3, atol=1e-8)


@pytest.mark.parametrize("S,T,trackers,ls,la,seed", KO.SEVERAL)
def test_three_steps_against_the_fp64_oracle(opts, dev, S, T, trackers, ls, la, seed):
    b, of_seq, ref, r32 = KO.case(S, T, trackers, 3, ls, la, None, seed)
    got = _run(opts["fp32"], b, S, dev, _clip(3, ls, la), offsets=_dev(np.stack(of_seq), dev))  # (mu=None: every sequence starts at mu0)
    _against_the_oracle(got, ref, r32, S, T, f"({S}, {T}) {trackers} trackers lambda_smooth {ls} lambda_accel {la}", allow_out=0)
    assert (got["status"] == 0).all() and (got["iters"] == 3).all()
    assert (np.diff(got["loss_hist"], axis=1) <= 0).all()  # the loss never increases
    assert ((np.diff(got["loss_hist"], axis=1) < 0).sum(1) == got["n_accepted"]).all()


def test_one_frame_per_sequence_is_dp_optimize_lm_skeleton(opts, dev):
    S, trackers, ls, seed = KO.T1
    b, of_seq, ref, r32 = KO.case(S, 1, trackers, 3, ls, None, None, seed)
    off = _dev(np.stack(of_seq), dev)
    got = _run(opts["fp32"], b, S, dev, _clip(3, ls), offsets=off)
    per = _lm(opts["fp32"], b, dev, offsets=off)
    _against_the_oracle(got, ref, r32, S, 1, "T = 1 clip", allow_out=0)
    bar = KO.bar_of(ref, r32)
    dz = np.abs(got["z"] - per["z"]).max()
    print(f"T = 1: clip against dp_optimize_lm_skeleton max |dz| {dz:.3e}, bar {bar:.3e}")
    assert dz <= bar
    np.testing.assert_array_equal(got["n_accepted"], per["n_accepted"])
    np.testing.assert_allclose(got["mu"], per["mu"], rtol=1e-6)
    assert (got["clip_loss"][:, 1] == 0).all()  # (no coupling part)
    # dp_optimize_lm_skeleton against its own oracle ...
    ref_lm = KO.lm(KO.models()[0], b, of_seq, 3)
    assert np.abs(per["z"] - ref_lm["z"]).max() <= bar
    np.testing.assert_array_equal(per["n_accepted"], ref_lm["n_accepted"])
    # ... and its reported losses, the pass in double, belong to the latents they are reported for ON THE FRAME'S BONES (on the context's they
    # would be off by the centimetres of a 0.85 x or 1.12 x skeleton): the oracle's forward pass at those latents, tests/test_hip_clip_lm.py's tolerance
    for f in range(S):
        one = {k: np.asarray(v)[f:f + 1] for k, v in b.items()}
        m = KO.with_offsets(KO.models()[0], of_seq[f])
        np.testing.assert_allclose(per["loss"][f:f + 1], LO.forward_np(m, per["z"][f:f + 1].astype(np.float64), one, 1.0, LAM_TMP)["loss"], rtol=2e-3, atol=1e-8)
        np.testing.assert_allclose(per["loss0"][f:f + 1], LO.forward_np(m, one["z0"].astype(np.float64), one, 1.0, LAM_TMP)["loss"], rtol=2e-3, atol=1e-8)


def test_a_bf16_rounded_context_meets_its_own_oracle(opts, dev):
    S, T, trackers, ls, la, seed = KO.BF16
    b, of_seq, ref, r32 = KO.case(S, T, trackers, 3, ls, la, None, seed, rounding="bf16")
    got = _run(opts["bf16"], b, S, dev, _clip(3, ls, la), offsets=_dev(np.stack(of_seq), dev))
    _against_the_oracle(got, ref, r32, S, T, f"bf16 context ({S}, {T}) lambda_smooth {ls} lambda_accel {la}", allow_out=0)
    assert (got["status"] == 0).all()


@pytest.mark.parametrize("accel", [None, 5.0])
def test_a_refused_skeleton_stops_its_sequence_and_no_other(opts, dev, skels, accel):
    from dragposer_amd import _lib

    opt, (S, T) = opts["fp32"], (5, 7)
    ks = KO.k_of(S)
    b = KO.mixed_inputs(S, T, 3, 11)
    off = np.stack([skels[k] for k in ks])
    clip = _clip(3, 0.5, accel)
    mu_in = np.asarray([0.5, 0.25, 0.125, 0.5, 0.25], np.float32)
    clean = _run(opt, b, S, dev, clip, mu=mu_in, offsets=_dev(off, dev))
    assert (clean["info"] == 0).all() and (clean["status"] == 0).all()
    others, seq1 = _rows(S, T, [True, False, True, True, True]), np.arange(S * T) % S == 1
    for value in (np.nan, 2.0 * _lib.DP_INPUT_LIMIT, -np.inf):
        bad = off.copy()
        bad[1, 17, 2] = value
        got = _run(opt, b, S, dev, clip, mu=mu_in, offsets=_dev(bad, dev))
        assert got["info"].tolist() == [0, _lib.DP_CLIP_REFUSED_FRAME, 0, 0, 0]
        assert got["n_accepted"][1] == 0 and got["mu"][1] == mu_in[1] and np.isnan(got["clip_loss"][1]).all() and np.isnan(got["loss_hist"][1]).all()
        if accel is not None:
            assert np.isnan(got["accel_loss"][1])
        assert (got["status"][seq1] == _lib.DP_STATUS_NONFINITE_RESULT | _lib.DP_STATUS_BAD_STATE).all() and (got["iters"][seq1] == 0).all()
        for name in ("z", "z_pre", "pose", "pos", "rot", "world_rot", "disp", "world_disp", "loss"):
            assert np.isnan(got[name][seq1]).all(), name
        # the other four sequences: the bits of the clean launch
        for name in FRAME_OUTS:
            np.testing.assert_array_equal(got[name][others], clean[name][others], err_msg=name)
        for name in _seq_outs(got):
            np.testing.assert_array_equal(got[name][[0, 2, 3, 4]], clean[name][[0, 2, 3, 4]], err_msg=name)
    # row 0 of a skeleton is never read
    root = off.copy()
    root[:, 0] = np.nan
    got = _run(opt, b, S, dev, clip, mu=mu_in, offsets=_dev(root, dev))
    for name in got:
        np.testing.assert_array_equal(got[name], clean[name], err_msg=name)
    # ... and per frame in dp_optimize_lm_skeleton
    b28, ks28 = KO.every_joint_mixed()
    off28 = np.stack([skels[k] for k in ks28])
    clean28 = _lm(opt, b28, dev, offsets=_dev(off28, dev))
    bad28 = off28.copy()
    bad28[5, 21, 0] = np.nan
    bad28[:, 0] = np.inf
    got28 = _lm(opt, b28, dev, offsets=_dev(bad28, dev))
    rest = np.arange(28) != 5
    assert got28["status"][5] == _lib.DP_STATUS_NONFINITE_RESULT | _lib.DP_STATUS_BAD_STATE and np.isnan(got28["z"][5]).all() and np.isnan(got28["pos"][5]).all()
    for name in got28:
        if name != "mu":  # (mu of a refused frame is unchanged: the same as the clean launch's input, not its output)
            np.testing.assert_array_equal(got28[name][rest], clean28[name][rest], err_msg=name)


def test_repeatable_and_a_graph_sees_offsets_changed_in_place(opts, dev, skels):
    from dragposer_amd.optimizer import to_device_batch

    opt, (S, T) = opts["fp32"], (3, 33)
    ks = KO.k_of(S)
    b = KO.mixed_inputs(S, T, 3, 11)
    clip = _clip(3, 0.5, 5.0)
    first = np.stack([skels[k] for k in ks])
    second = np.stack([skels[k] for k in ks[::-1]])
    a = _run(opt, b, S, dev, clip, offsets=_dev(first, dev))
    c = _run(opt, b, S, dev, clip, offsets=_dev(first, dev))
    other = _run(opt, b, S, dev, clip, offsets=_dev(second, dev))
    for k in a:
        np.testing.assert_array_equal(a[k], c[k], err_msg=k)
    assert not np.array_equal(a["z"], other["z"])
    d = to_device_batch(b, dev)
    out = opt.allocate_outputs(S * T)
    out.update(n_accepted=torch.empty(S, dtype=torch.int32, device=dev), info=torch.empty(S, dtype=torch.int32, device=dev),
               clip_loss=torch.empty(S, 2, dtype=torch.float64, device=dev), loss_hist=torch.empty(S, 4, dtype=torch.float64, device=dev),
               accel_loss=torch.empty(S, dtype=torch.float64, device=dev))
    mu = torch.full((S,), 1e-2, device=dev)
    off = _dev(first, dev)
    kw = dict(n_sequences=S, clip=clip, lambda_tmp=LAM_TMP, mu=mu, out=out, outputs=tuple(out), offsets=off)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        opt.optimize_clip_lm(**d, **kw)
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.optimize_clip_lm(**d, **kw)
    for values, want in ((first, a), (second, other), (first, a)):
        for v in out.values():
            v.fill_(-1)
        mu.fill_(1e-2)
        off.copy_(_dev(values, dev))  # in place: the graph holds the tensor's address
        graph.replay()
        torch.cuda.synchronize()
        for k in out:
            np.testing.assert_array_equal(out[k].cpu().numpy(), want[k], err_msg=k)
        np.testing.assert_array_equal(mu.cpu().numpy(), want["mu"])


def test_fitted_bones_into_the_clip_solve(opts, dev):
    """targets of the 1.12 x performer: fit_bones (one uniform group) at the context-skeleton solution, its offsets into the clip solve"""
    from dragposer_amd.calibration import BoneGroups
    from dragposer_amd.optimizer import to_device_batch

    opt = opts["fp32"]
    S, T, _, ls, _ = KO.E2E
    b, true = KO.e2e_inputs()
    clip = _clip(3, ls)
    plain = _run(opt, b, S, dev, clip)
    d = to_device_batch(b, dev)
    fit = opt.fit_bones(_dev(plain["z"], dev), d["cur_rot"], d["tgt_pos"], d["w"], d["tracked"], BoneGroups.uniform())
    torch.cuda.synchronize()
    fitted = fit["offsets"].contiguous()
    scale = float(fit["scales"][0])
    got = _run(opt, b, S, dev, clip, offsets=fitted)
    print(f"end to end (2, 9): fitted scale {scale:.4f} (the performer's 1.12), clip loss {got['clip_loss'][:, 0].tolist()} with the fitted bones, "
          f"{plain['clip_loss'][:, 0].tolist()} with the context's")
    assert (got["clip_loss"][:, 0] < plain["clip_loss"][:, 0]).all() and (got["status"] == 0).all() and (plain["status"] == 0).all()
    m64, m32 = KO.models()
    fitted_np = fitted.cpu().numpy()
    for res, of_seq, label in ((got, [fitted_np] * S, "fitted bones"), (plain, [KO.base_offsets()] * S, "the context's bones")):
        ref, r32 = (KO.clip_lm(m, b, S, of_seq, 3, ls) for m in (m64, m32))
        _against_the_oracle(res, ref, r32, S, T, f"end to end (2, 9), {label}", allow_out=0)


def test_eval_drag_smooth_on_a_clip_of_other_bone_lengths(dev, tmp_path):
    """tests/data/example_clip.bvh and a copy with every OFFSET x 1.12 through eval_drag --smooth, in both orders: each skeleton is once the
    first file's and once the second's, and both files return"""
    from dragposer_amd import eval_drag

    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "example_clip.bvh")
    for order in (("a_plain.bvh", "b_scaled.bvh"), ("a_scaled.bvh", "b_plain.bvh")):
        folder = tmp_path / order[0][2:-4]
        folder.mkdir()
        for name in order:
            text = open(src).read()
            (folder / name).write_text(scaled_bvh_text(text, 1.12) if "scaled" in name else text)
        res = eval_drag.main([str(folder), "--max-frames", "12", "--smooth", "5:2:0.1", "--out-dir", str(tmp_path / ("out_" + order[0][2:-4]))])
        assert len(res) == 2
        for r in res:
            h = r["smooth_loss_hist"]
            print(f"eval_drag --smooth {os.path.basename(r['out'])}: loss {h.tolist()}, MPJPE {r['mpjpe']:.4f} -> {r['mpjpe_smooth']:.4f}")
            assert h.shape == (3,) and (np.diff(h) <= 0).all() and h[-1] < h[0]
            assert abs(r["mpjpe_smooth"] - r["mpjpe"]) < 0.05

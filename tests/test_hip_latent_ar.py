"""GPU: dp_optimize_sequence_ar (include/dragposer_latent_ar.h) -- dp_optimize_sequence_holds with every step's z_tgt row formed inside the
launch by a linear autoregressive predictor over the sequence's last history rows -- against the per-frame composition the header names:
optimize_terms with z_tgt = LatentAR.predict(latent_buf), then sequence_advance, then the latent copy, then the hold update.  The same
arithmetic in the same order: every comparison is bit for bit (NaN where NaN); no tolerance is involved."""
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from test_hip_holds import _update
from test_hip_sequence_constraints import H, HJ, OUT_KEYS, ST, STATE_KEYS, _assert_same, _clip, _opt, _row, _same, _state

pytestmark = pytest.mark.gpu

LOOP = dict(n_iter=10, stop_eps_pos=0.01 * 0.01, stop_eps_rot=0.01, min_loss_incr=0.00001)  # max_iter 10, the reference's early stop on
ADJ = (0, 13, 0.5)
LAM = 0.02
ALL_KEYS = OUT_KEYS + ("z_tgt", "scratch")
HOLD_KEYS = ALL_KEYS + ("trace",)


@functools.lru_cache(maxsize=None)
def _model(K, seed=7):
    """dense random A_1..A_K and c: every entry in play, the whole operator's gain below 1 so that the targets stay near the latents"""
    from dragposer_amd import LatentAR

    g = np.random.default_rng(seed + K)
    A = g.standard_normal((K, 24, 24)) * (0.6 / (K * np.sqrt(24.0)))
    A[0] += 0.3 * np.eye(24)
    return LatentAR(A, 0.05 * g.standard_normal(24))


def _state_ar(c, rows=H):
    """the clip's initial state with a history of `rows` rows whose last four differ (so h_1..h_4 are told apart from step 0 on)"""
    st = _state(c)
    g = torch.Generator(device="cpu").manual_seed(91)
    st.lbuf[:, -4:] += (0.05 * torch.randn(c.S, 4, 24, generator=g)).to(st.lbuf.device)
    if rows != H:
        st.lbuf, st.dbuf, st.hbuf = (b[:, -rows:].contiguous() for b in (st.lbuf, st.dbuf, st.hbuf))
    return st


def _table(c, held=False):
    """a table with a [T,S,4] per-frame term; `held`: two point-DISTANCE terms for holds besides"""
    from dragposer_amd.terms import Term, Terms

    ts = [Term.plane(4, (0.0, 1.0, 0.0), point=(0.0, -0.9, 0.0), weight=0.5, one_sided=True),
          Term.distance(8, point=(0.1, 0.0, 0.2), lo=0.0, hi=0.5, weight=0.5, per_frame=c.rows)]
    if held:
        ts += [Term.distance(4, point=(0.0, 0.0, 0.0), lo=0.0, hi=0.0, weight=0.8, drop_up=True),
               Term.distance(8, point=(0.0, 0.0, 0.0), lo=0.0, hi=0.02, weight=0.6)]
    return Terms(ts)


def _holds():
    from dragposer_amd import Hold, Holds

    return Holds([Hold(2, 0.0, 0.1, level=10.0), Hold(3, 0.0, 0.1, level=10.0)])  # (level +10: both latch at step 0 and feed their terms from step 1)


def _per_frame(c, ar, terms, st, holds=None, hstate=None, offsets=None, tgt_pos=None, t0=0, T=None, loop=LOOP):
    """the composition, frame by frame on the host -> (outputs with the z_tgt rows and the history rows, the state, the hold state)"""
    from dragposer_amd.terms import Terms

    opt, S, T = _opt(), c.S, T or c.T
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    hstate = hstate.clone() if holds is not None else None
    fr = opt.allocate_outputs(S, ("z", "z_pre", "pose", "disp", "world_disp", "world_rot", "pos", "loss", "iters", "status"))
    fr["loss_terms"] = torch.empty(S, len(terms), device=opt.device)
    o = {k: [] for k in HOLD_KEYS}
    nan = torch.full((S, 24), float("nan"), device=opt.device)
    for t in range(t0, t0 + T):
        zt = ar.predict(st.lbuf)
        tp = (tgt_pos[t] + (c.root[t] - st.gpos).unsqueeze(1)).contiguous()
        rows = [_row(x) for x in terms.frames(t, t + 1).terms]
        for i, h in enumerate(holds.holds if holds is not None else ()):
            rows[h.term] = replace(rows[h.term], per_frame=hstate[:, i].contiguous())
        opt.optimize_terms(st.latent, zt, st.grot, tp, c.tgt_rot[t], c.w, c.tracked, Terms(rows, terms.up_axis), global_pos=st.gpos, lr=1e-2,
                           lambda_rot=1.0, lambda_tmp=LAM, out=fr, outputs=tuple(fr), offsets=offsets, **loop)
        pose, pos = torch.empty(S, 88, device=opt.device), torch.empty(S, 3, device=opt.device)
        opt.sequence_advance(fr, st.gpos, st.grot, st.lbuf, st.dbuf, st.hbuf, HJ, pose_ret=pose, pos_ret=pos, adjust=ADJ, tgt_pos=tp)
        st.latent.copy_(fr["z"])
        if holds is not None:
            _update(terms, holds, hstate, fr["pos"], st.gpos)
        bad_state = (fr["status"] & ST.BAD_STATE) != 0  # (such a step used no target: the header's NaN row)
        for k, v in (("pose_ret", pose), ("pos_ret", pos), ("iters", fr["iters"]), ("status", fr["status"]), ("loss", fr["loss"]),
                     ("terms", fr["loss_terms"]), ("joint_pos", fr["pos"]), ("z_tgt", torch.where(bad_state[:, None], nan, zt)),
                     ("scratch", torch.cat((st.lbuf[:, -1], st.dbuf[:, -1], st.hbuf[:, -1]), dim=1)),
                     ("trace", hstate if holds is not None else torch.zeros(0))):
            o[k].append(v.clone())
    return {k: torch.stack(v) for k, v in o.items()}, st, hstate


def _launch(c, ar, terms, st, holds=None, hstate=None, offsets=None, tgt_pos=None, t0=0, T=None, loop=LOOP):
    """one launch over frames t0 .. t0 + T -> (outputs, the state, the hold state)"""
    opt, T = _opt(), T or c.T
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    sl = slice(t0, t0 + T)
    kw = {}
    if holds is not None:
        hstate = hstate.clone()
        kw = dict(holds=holds, hold_state=hstate, hold_trace=True)
    if terms is not None:
        kw["terms"] = terms.frames(t0, t0 + T)
    scratch = torch.empty(T, c.S, 24 + 3 + len(HJ), device=opt.device)
    o = opt.optimize_sequence(st.latent, tgt_pos[sl], c.tgt_rot[sl], c.root[sl], c.w, c.tracked, None, (0, 0), st.gpos, st.grot, st.lbuf, st.dbuf,
                              st.hbuf, HJ, lr=1e-2, lambda_rot=1.0, lambda_tmp=LAM, adjust=ADJ, offsets=offsets, scratch=scratch, ar=ar,
                              z_tgt_trace=True, **kw, **loop)
    o["terms"], o["z_tgt"], o["scratch"] = o.pop("loss_terms"), o.pop("z_tgt_trace"), scratch
    if holds is not None:
        o["trace"] = o.pop("hold_trace")
    return o, st, hstate


@pytest.mark.parametrize("K", [1, 2, 4])
def test_one_launch_equals_the_composition_at_the_ragged_shape(K):
    """S = 11 (a workgroup of 8 waves and one of 3), T = 20, dense A_1..A_K: every output of the call, the whole state, the z_tgt row every
    step used and the history rows handed to hist_scratch"""
    c, ar = _clip(11, 20), _model(K)
    exp, est, _ = _per_frame(c, ar, _table(c), _state_ar(c))
    got, gst, _ = _launch(c, ar, _table(c), _state_ar(c))
    torch.cuda.synchronize()
    _assert_same(got, exp, ALL_KEYS, K)
    _assert_same(gst, est, STATE_KEYS, K)
    assert int(exp["status"].max()) == 0 and bool(torch.isfinite(exp["pose_ret"]).all())
    assert bool((exp["loss"][..., 2] > 0).all())                        # the pull term is in every step's loss
    assert int(exp["iters"].min()) < int(exp["iters"].max())            # the early stop ends steps at different counts
    assert not torch.equal(exp["z_tgt"][1], exp["z_tgt"][0])            # the targets move with the sequence
    assert torch.equal(got["scratch"][:, :, :24], gst.lbuf[:, -20:].transpose(0, 1))  # the second launch appended what the steps handed over


def test_every_order_reads_its_own_rows():
    """hold() returns h_1 and constant_velocity() 2 h_1 - h_2, bit for bit, from the launch's own history rows"""
    from dragposer_amd import LatentAR

    c = _clip(11, 20)
    for ar, want in ((LatentAR.hold(), lambda h: 0.0 + 1.0 * h[1]), (LatentAR.constant_velocity(), lambda h: (0.0 + 2.0 * h[1]) + -1.0 * h[2])):
        st = _state_ar(c)
        before = st.lbuf[:, -2:].clone()
        got, gst, _ = _launch(c, ar, None, st, T=6)
        torch.cuda.synchronize()
        rows = torch.cat((before.transpose(0, 1), got["scratch"][:, :, :24]))  # [2 + T, S, 24]: rows[t + 1] is h_1 of step t
        for t in range(6):
            assert torch.equal(got["z_tgt"][t], want({1: rows[t + 1], 2: rows[t]})), (ar, t)


@pytest.mark.parametrize("S,T,K,rows", [(1, 1, 2, H), (9, 6, 4, 4), (3, 5, 1, 1)])
def test_small_shapes_and_a_history_as_short_as_the_order(S, T, K, rows):
    """one sequence of one step; history == K = 4 (more steps than rows: the second launch's append wraps) and history == K = 1"""
    c, ar = _clip(S, T, seed=33), _model(K)
    exp, est, _ = _per_frame(c, ar, _table(c), _state_ar(c, rows))
    got, gst, _ = _launch(c, ar, _table(c), _state_ar(c, rows))
    torch.cuda.synchronize()
    _assert_same(got, exp, ALL_KEYS, (S, T, K))
    _assert_same(gst, est, STATE_KEYS, (S, T, K))
    assert tuple(gst.lbuf.shape) == (S, rows, 24) and int(exp["status"].max()) == 0


def test_two_chained_launches_equal_one():
    """T = 20 as one launch = two launches of 10: the second loads from latent_buf what the first one's steps left"""
    c, ar = _clip(11, 20), _model(4)
    one, ost, _ = _launch(c, ar, _table(c), _state_ar(c))
    a, st, _ = _launch(c, ar, _table(c), _state_ar(c), T=10)
    b, st, _ = _launch(c, ar, _table(c), st, t0=10, T=10)
    torch.cuda.synchronize()
    _assert_same({k: torch.cat((a[k], b[k])) for k in ALL_KEYS}, one, ALL_KEYS, "chain")
    _assert_same(st, ost, STATE_KEYS, "chain")


def test_with_holds_mixed_skeletons_and_a_per_frame_term():
    """two holds, offsets [S,22,3] (stride 66, four skeletons over 11 sequences) and a [T,S,4] per-frame term in one launch"""
    c, ar, opt = _clip(11, 20), _model(2), _opt()
    own = torch.from_numpy(opt.host_model.arrays["offsets"]).to(opt.device).reshape(22, 3).contiguous()
    scale = torch.tensor([1.0, 0.9, 1.1, 1.05], device=opt.device)[torch.arange(c.S) % 4]
    mixed = (own[None] * scale[:, None, None]).contiguous()
    terms, holds, T = _table(c, held=True), _holds(), 10
    h0 = torch.zeros(c.S, 2, 4, device=opt.device)
    exp, est, eh = _per_frame(c, ar, terms, _state_ar(c), holds, h0, offsets=mixed, T=T)
    got, gst, gh = _launch(c, ar, terms, _state_ar(c), holds, h0, offsets=mixed, T=T)
    plain, _, _ = _launch(c, ar, terms, _state_ar(c), holds, h0, T=T)
    torch.cuda.synchronize()
    _assert_same(got, exp, HOLD_KEYS, "holds")
    _assert_same(gst, est, STATE_KEYS, "holds")
    assert _same(gh, eh) and bool((gh[..., 3] == 1).all())
    assert bool((exp["terms"][1:, :, 2:] != 0).any())                                  # the held terms are in the loss
    assert not torch.equal(got["pose_ret"][:, 1::4], plain["pose_ret"][:, 1::4])       # the skeletons are read


def test_no_terms_and_no_holds():
    """n_terms = 0 with a NULL dp_holds (terms=None) and with an empty dp_holds: the plain tracker loss with the predictor's pull"""
    from dragposer_amd import Holds
    from dragposer_amd.terms import Terms

    c, ar, T = _clip(11, 20), _model(2), 8
    exp, est, _ = _per_frame(c, ar, Terms(), _state_ar(c), T=T)
    got, gst, _ = _launch(c, ar, None, _state_ar(c), T=T)
    emp, pst, _ = _launch(c, ar, Terms(), _state_ar(c), Holds([]), torch.zeros(c.S, 0, 4, device=c.z0.device), T=T)
    torch.cuda.synchronize()
    for o, s in ((got, gst), (emp, pst)):
        _assert_same(o, exp, ALL_KEYS, "empty")
        _assert_same(s, est, STATE_KEYS, "empty")


def test_a_bad_tracker_sample_is_screened_and_stays_with_its_sequence():
    """a NaN position target at step 3 of sequence 5: that step returns the warm start's pose with BAD_TARGETS, the sequence is BAD_STATE
    from step 4 on (its z_tgt rows NaN: no target was used), the ten others are bit-identical to the clean launch"""
    c, ar = _clip(11, 20), _model(2)
    bad, step, T = 5, 3, 8
    tgt = c.tgt_pos.clone()
    tgt[step, bad, 13, 1] = float("nan")
    clean, cst, _ = _launch(c, ar, _table(c), _state_ar(c), T=T)
    got, gst, _ = _launch(c, ar, _table(c), _state_ar(c), tgt_pos=tgt, T=T)
    exp, est, _ = _per_frame(c, ar, _table(c), _state_ar(c), tgt_pos=tgt, T=T)
    torch.cuda.synchronize()
    _assert_same(got, exp, ALL_KEYS, "bad sample")
    _assert_same(gst, est, STATE_KEYS, "bad sample")
    assert int(got["status"][step, bad]) == ST.NONFINITE | ST.BAD_TARGETS and int(got["iters"][step, bad]) == 1
    assert bool(torch.isfinite(got["pose_ret"][step, bad]).all()) and bool(torch.isfinite(got["z_tgt"][step, bad]).all())
    assert bool((got["status"][step + 1:, bad] == (ST.NONFINITE | ST.BAD_STATE)).all())
    for k in ("pose_ret", "pos_ret", "loss", "z_tgt"):
        assert bool(got[k][step + 1:, bad].isnan().all()), k
    others = [s for s in range(c.S) if s != bad]
    for k in ALL_KEYS:
        assert torch.equal(got[k][:, others], clean[k][:, others]), k
        assert torch.equal(got[k][:step, bad], clean[k][:step, bad]), k
    for k in STATE_KEYS:
        assert torch.equal(getattr(gst, k)[others], getattr(cst, k)[others]), k


def test_a_target_beyond_the_input_limit_is_refused_not_computed_with():
    """coeffs = 1e6 I: the computed row exceeds DP_INPUT_LIMIT, the step reports BAD_TARGETS, the sequence is BAD_STATE from then on"""
    from dragposer_amd import LatentAR

    c, T = _clip(11, 20), 4
    ar = LatentAR(1.0e6 * np.eye(24, dtype=np.float32))
    got, gst, _ = _launch(c, ar, _table(c), _state_ar(c), T=T)
    exp, est, _ = _per_frame(c, ar, _table(c), _state_ar(c), T=T)
    torch.cuda.synchronize()
    _assert_same(got, exp, ALL_KEYS, "1e6")
    _assert_same(gst, est, STATE_KEYS, "1e6")
    assert bool((got["z_tgt"][0].abs().amax(dim=1) > 1.0e4).all()) and bool(torch.isfinite(got["z_tgt"][0]).all())
    assert bool((got["status"][0] == (ST.NONFINITE | ST.BAD_TARGETS)).all()) and bool((got["iters"][0] == 1).all())
    assert bool(torch.isfinite(got["pose_ret"][0]).all())  # the warm start's pose
    assert bool((got["status"][1:] == (ST.NONFINITE | ST.BAD_STATE)).all())


def test_run_frames_equals_the_loop_of_run():
    """DragPose.run_frames(ar=) is one launch for all T frames and equals T calls of run(ar=), with constraints (through
    Terms.from_constraints), per-sequence offsets and joint adjustment; lambda_temporal weighs the pull"""
    from dragposer_amd import Constraints
    from dragposer_amd.drag_pose import DragPose

    c, ar, opt = _clip(11, 20), _model(2), _opt()
    own = torch.from_numpy(opt.host_model.arrays["offsets"]).to(opt.device).reshape(22, 3).contiguous()
    mixed = (own[None] * torch.tensor([1.0, 0.95, 1.05], device=opt.device)[torch.arange(c.S) % 3][:, None, None]).contiguous()
    idx = np.array(R.TRACK6)
    wts = np.array([R.W6[j] for j in R.TRACK6], np.float32)
    kw = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2, max_iter=10, min_loss_incr=1e-5, learning_rate=1e-2, lambda_rot=1, lambda_temporal=0.15,
              height_indices=HJ, joint_adjustment_indices=(0, 3), joint_adjustment_weight=0.5, offsets=mixed,
              constraints=Constraints.reference(floor_level=-0.9), ar=ar)
    a, b, off = (DragPose(opt, None, np.zeros(24), np.ones(24), n_sequences=c.S) for _ in range(3))
    for dp in (a, b, off):
        dp.set_initial_state(c.z0, np.zeros((c.S, 3), np.float32), c.rot0, c.heights0)
    tp, tR = c.tgt_pos[:, :, idx], c.tgt_rot[:, :, idx].reshape(c.T, c.S, -1, 3, 3)
    pa, ga, ia, za = [], [], [], []
    for t in range(c.T):
        pose, gpos = a.run(tp[t], tR[t], idx, wts, **kw)
        pa.append(pose.clone()); ga.append(gpos.clone()); ia.append(a.last["iters"].clone()); za.append(a.last["z_tgt"].clone())
    calls = []
    seq = b.opt.optimize_sequence
    b.opt.optimize_sequence = lambda *x, **k: (calls.append(int(x[1].shape[0])), seq(*x, **k))[1]
    try:
        pb, gb, ib = b.run_frames(tp, tR, idx, wts, **kw)
    finally:
        del b.opt.optimize_sequence
    po, _, _ = off.run_frames(tp, tR, idx, wts, **{**kw, "lambda_temporal": 0.0})
    torch.cuda.synchronize()
    assert calls == [20]
    assert torch.equal(torch.stack(pa), pb) and torch.equal(torch.stack(ga), gb) and torch.equal(torch.stack(ia), ib)
    assert tuple(b.last_z_tgt.shape) == (c.T, c.S, 24) and torch.equal(torch.stack(za), b.last_z_tgt)
    assert torch.equal(b.last_z_tgt[0], ar.predict(c.z0.unsqueeze(1).repeat(1, 2, 1)))
    for attr in ("latent", "current_global_pos", "current_global_rot", "latent_buffer", "displacement_buffer", "heights_buffer"):
        assert torch.equal(getattr(a, attr), getattr(b, attr)), attr
    assert int(b.last_status.max()) == 0 and not torch.equal(po, pb)  # the weight is not a no-op
    assert torch.equal(a.last["loss"], b.last_loss[-1]) and bool((b.last_loss[..., 2] > 0).all()) and not off.last_loss[..., 2].any()


def test_the_command_lines_fit_a_model_and_evaluate_with_it(tmp_path, capsys):
    """python -m dragposer_amd.ar fit on the shipped clip, then eval_drag --latent-ar FILE on the 4-tracker configuration: the pull term runs
    with the configuration's lambda_temporal, the predictor is named in the output, and the frame loop on the device and --per-frame write
    the same bytes; cv:0.5 parses, and the switch is not a no-op"""
    import os

    from dragposer_amd import LatentAR, ar as ar_cli, eval_drag

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    clip = os.path.join(root, "tests", "data", "example_clip.bvh")
    path = str(tmp_path / "ar2.npz")
    fitted = ar_cli.main(["fit", clip, "--order", "2", "--ridge", "1e-4", "-o", path])
    assert "order 2, 238 windows of 1 clips" in capsys.readouterr().out
    back = LatentAR.load(path)
    assert back.order == 2 and np.array_equal(back.A, fitted.A) and np.array_equal(back.c, fitted.c)
    argv = [clip, "--config", os.path.join(root, "dragposer_amd", "config", "4_trackers_config.json"), "--max-frames", "48", "--keep-frames"]
    for d in ("device", "host", "cv", "plain"):
        os.makedirs(tmp_path / d)
    a = eval_drag.main(argv + ["--latent-ar", path, "--out-dir", str(tmp_path / "device")])[0]
    text = capsys.readouterr().out
    assert text.count("Latent predictor: order-2 model from") == 1 and "lambda_temporal 0.125)" in text and "pull term off" not in text
    b = eval_drag.main(argv + ["--latent-ar", path, "--out-dir", str(tmp_path / "host"), "--per-frame"])[0]
    assert a["frames"] == b["frames"] == 48 and os.path.getsize(a["out"]) > 0
    assert open(a["out"], "rb").read() == open(b["out"], "rb").read()
    cv = eval_drag.main(argv + ["--latent-ar", "cv:0.5", "--out-dir", str(tmp_path / "cv")])[0]
    assert "constant velocity, damping 0.5" in capsys.readouterr().out
    plain = eval_drag.main(argv + ["--out-dir", str(tmp_path / "plain")])[0]
    assert "pull term off" in capsys.readouterr().out
    assert not np.array_equal(a["poses"], plain["poses"]) and not np.array_equal(cv["poses"], plain["poses"])
    assert not np.array_equal(a["poses"], cv["poses"])

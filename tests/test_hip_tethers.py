"""GPU: dp_optimize_sequence_tethers (include/dragposer_tethers.h) -- dp_optimize_sequence_gaps with point-DISTANCE terms whose point
follows the joint's own reconstructed path -- against the per-frame composition the header names: optimize_terms with the tethered terms'
per_frame = the state's [S,4] rows (holds and gaps composed as their headers state), then sequence_advance, then the latent copy, then
Tethers.update.  The same arithmetic in the same order: every comparison is bit for bit (NaN where NaN); no tolerance is involved.  The
main shape is S = 11 (a workgroup of 8 waves and one of 3), T = 20, tgt_root on, joint adjustment (0, 13, 0.5), a table with a [T,S,4]
term, two tethers on joints no tracker observes: alpha 0 on a band (hi = 0.02), alpha 1 on a pin (lo = hi = 0)."""
import copy
from dataclasses import replace

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from test_hip_holds import _update
from test_hip_latent_ar import ADJ, LAM, LOOP, _holds, _model, _state_ar, _table
from test_hip_sequence_constraints import HJ, OUT_KEYS, ST, STATE_KEYS, _assert_same, _clip, _opt, _row, _same

pytestmark = pytest.mark.gpu

FIXED5 = dict(n_iter=5, stop_eps_pos=0.0, stop_eps_rot=0.0, min_loss_incr=-1e30)  # a fixed count: thresholds that never end the loop
KEYS = OUT_KEYS + ("scratch", "gap_trace", "tether_trace")
S, T = 11, 20
KNEE, ELBOW = 6, 19  # two joints outside the six trackers


def _tethered(c, held=False, weights=(0.6, 0.8)):
    """test_hip_latent_ar's table (with its two hold terms when `held`) and two tethered terms behind it -> (table, tethers)"""
    from dragposer_amd import Tether, Tethers
    from dragposer_amd.terms import Term, Terms

    base = _table(c, held=held)
    n = len(base)
    ts = base.terms + [Term.distance(KNEE, point=(0.0, 0.0, 0.0), lo=0.0, hi=0.02, weight=weights[0]),
                       Term.distance(ELBOW, point=(0.0, 0.0, 0.0), lo=0.0, hi=0.0, weight=weights[1])]
    return Terms(ts, base.up_axis), Tethers([Tether(n, 0.0), Tether(n + 1, 1.0)])


def _gaps(max_hold=0, decay=1.0):
    from dragposer_amd import Gaps

    return Gaps(max_hold, decay)


def _zeros(c, tethers):
    return torch.zeros(c.S, len(tethers), 8, device=c.z0.device), torch.zeros(c.S, 22, 16, device=c.z0.device)


def _per_frame(c, terms, tethers, st, tstate, gstate, gaps=None, ar=None, holds=None, hstate=None, present=None, tgt_pos=None, t0=0, T=None,
               offsets=None, loop=LOOP):
    """the composition, frame by frame on the host -> (outputs, the state, the tether state, the gap state, the hold state)"""
    from dragposer_amd.terms import Terms

    opt, S, T = _opt(), c.S, T or c.T
    gaps = gaps or _gaps()
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    tstate, gstate = tstate.clone(), gstate.clone()
    hstate = hstate.clone() if holds is not None else None
    fr = opt.allocate_outputs(S, ("z", "z_pre", "pose", "disp", "world_disp", "world_rot", "pos", "loss", "iters", "status"))
    fr["loss_terms"] = torch.empty(S, len(terms), device=opt.device)
    o = {k: [] for k in KEYS + ("z_tgt", "hold_trace")}
    for t in range(t0, t0 + T):
        zt = ar.predict(st.lbuf) if ar is not None else c.z_tgt[t]
        tp = (tgt_pos[t] + (c.root[t] - st.gpos).unsqueeze(1)).contiguous()
        tp_e, tr_e, w_e, on, code = gaps.step(gstate, tp, c.tgt_rot[t], c.w, c.tracked, st.gpos, present[t] if present is not None else None)
        rows = [_row(x) for x in terms.frames(t, t + 1).terms]
        for i, h in enumerate(holds.holds if holds is not None else ()):
            rows[h.term] = replace(rows[h.term], per_frame=hstate[:, i].contiguous())
        table = tethers.frame_terms(Terms(rows, terms.up_axis), tstate)
        opt.optimize_terms(st.latent, zt, st.grot, tp_e, tr_e, w_e, on, table, global_pos=st.gpos, lr=1e-2, lambda_rot=1.0, lambda_tmp=LAM, out=fr,
                           outputs=tuple(fr), offsets=offsets, **loop)
        tp_adj = tp_e.clone()  # a lost (or untracked) adjustment target: the adjusted joint's own position, so that adj = +0
        tp_adj[:, ADJ[1]] = torch.where(on[:, ADJ[1], None] != 0, tp_e[:, ADJ[1]], fr["pos"][:, ADJ[0]])
        pose, pos = torch.empty(S, 88, device=opt.device), torch.empty(S, 3, device=opt.device)
        opt.sequence_advance(fr, st.gpos, st.grot, st.lbuf, st.dbuf, st.hbuf, HJ, pose_ret=pose, pos_ret=pos, adjust=ADJ, tgt_pos=tp_adj)
        st.latent.copy_(fr["z"])
        if holds is not None:
            _update(terms, holds, hstate, fr["pos"], st.gpos)
        tethers.update(terms, tstate, fr["pos"], st.gpos)
        bits = ((code == 2).any(dim=1) * 16 + (code == 3).any(dim=1) * 32).to(torch.int32)
        for k, v in (("pose_ret", pose), ("pos_ret", pos), ("iters", fr["iters"]), ("status", fr["status"] | bits), ("loss", fr["loss"]),
                     ("terms", fr["loss_terms"]), ("joint_pos", fr["pos"]), ("z_tgt", zt), ("gap_trace", code), ("tether_trace", tstate),
                     ("hold_trace", hstate if holds is not None else torch.zeros(0)),
                     ("scratch", torch.cat((st.lbuf[:, -1], st.dbuf[:, -1], st.hbuf[:, -1]), dim=1))):
            o[k].append(v.clone())
    return {k: torch.stack(v) for k, v in o.items()}, st, tstate, gstate, hstate


def _launch(c, terms, tethers, st, tstate, gstate, gaps=None, ar=None, holds=None, hstate=None, present=None, tgt_pos=None, t0=0, T=None,
            offsets=None, loop=LOOP, trace=True, adjust=ADJ, lr=1e-2):
    """one launch over frames t0 .. t0 + T -> (outputs, the state, the tether state, the gap state, the hold state); tethers None:
    dp_optimize_sequence_gaps"""
    opt, T = _opt(), T or c.T
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    sl = slice(t0, t0 + T)
    gstate = gstate.clone()
    kw = dict(gaps=gaps or _gaps(), gap_state=gstate, gap_trace=True, present=present[sl].contiguous() if present is not None else None)
    if tethers is not None:
        tstate = tstate.clone()
        kw.update(tethers=tethers, tether_state=tstate, tether_trace=trace)
    if ar is not None:
        kw.update(ar=ar, z_tgt_trace=True)
    if holds is not None:
        hstate = hstate.clone()
        kw.update(holds=holds, hold_state=hstate, hold_trace=True)
    scratch = torch.empty(T, c.S, 24 + 3 + len(HJ), device=opt.device)
    o = opt.optimize_sequence(st.latent, tgt_pos[sl], c.tgt_rot[sl], c.root[sl], c.w, c.tracked, None if ar is not None else c.z_tgt[sl],
                              (c.S * 24, 24), st.gpos, st.grot, st.lbuf, st.dbuf, st.hbuf, HJ, lr=lr, lambda_rot=1.0, lambda_tmp=LAM, adjust=adjust,
                              offsets=offsets, scratch=scratch, terms=terms.frames(t0, t0 + T), **kw, **loop)
    o["terms"], o["scratch"] = o.pop("loss_terms"), scratch
    if ar is not None:
        o["z_tgt"] = o.pop("z_tgt_trace")
    return o, st, tstate, gstate, hstate


def _world(o, joint):
    """[T,S,3] where a renderer puts `joint`: the advanced global position + (P_joint - P_0)"""
    return o["pos_ret"] + (o["joint_pos"][:, :, joint] - o["joint_pos"][:, :, 0])


@pytest.mark.parametrize("loop", (LOOP, FIXED5), ids=("early10", "fixed5"))
def test_one_launch_equals_the_composition_at_the_ragged_shape(loop):
    """every output, the state arrays, the tether state and every trace row; the trace is the joints' own path"""
    c = _clip(S, T)
    terms, tethers = _tethered(c)
    ts0, gs0 = _zeros(c, tethers)
    exp, est, et, eg, _ = _per_frame(c, terms, tethers, _state_ar(c), ts0, gs0, loop=loop)
    got, gst, gt, gg, _ = _launch(c, terms, tethers, _state_ar(c), ts0, gs0, loop=loop)
    torch.cuda.synchronize()
    _assert_same(got, exp, KEYS, "launch")
    _assert_same(gst, est, STATE_KEYS, "launch")
    assert _same(gt, et) and _same(gg, eg) and torch.equal(gt, got["tether_trace"][-1])
    assert int(exp["status"].max()) == 0 and bool(torch.isfinite(got["tether_trace"]).all())
    tr = got["tether_trace"]
    assert bool((tr[..., 3] == 1).all()) and bool((tr[..., 7] == 1).all())
    for k, j in enumerate((KNEE, ELBOW)):
        assert torch.equal(tr[:, :, k, 4:7], _world(got, j))  # Wprev after step t is W(t)
    assert torch.equal(tr[:, :, 0, :3], tr[:, :, 0, 4:7])      # alpha 0: the point is the last position
    assert torch.equal(tr[0, :, 1, :3], tr[0, :, 1, 4:7]) and not torch.equal(tr[1:, :, 1, :3], tr[1:, :, 1, 4:7])  # alpha 1: from the second step on
    assert bool((got["terms"][0, :, -2:] == 0).all()) and bool((got["terms"][1:, :, -1] > 0).any())  # no path at step 0; the pin acts after it
    if loop is LOOP:
        assert int(exp["iters"].min()) < int(exp["iters"].max())  # the early stop ends steps at different counts


def test_two_stretches_chained_through_the_state():
    c = _clip(S, T)
    terms, tethers = _tethered(c)
    ts0, gs0 = _zeros(c, tethers)
    one, ost, ot, og, _ = _launch(c, terms, tethers, _state_ar(c), ts0, gs0)
    a, st, t1, g1, _ = _launch(c, terms, tethers, _state_ar(c), ts0, gs0, T=9)
    b, st, t2, g2, _ = _launch(c, terms, tethers, st, t1, g1, t0=9, T=11)
    torch.cuda.synchronize()
    _assert_same({k: torch.cat((a[k], b[k])) for k in KEYS}, one, KEYS, "chain")
    _assert_same(st, ost, STATE_KEYS, "chain")
    assert _same(t2, ot) and _same(g2, og) and bool(t1.any())


def test_one_sequence_of_one_frame():
    c = _clip(1, 1)
    terms, tethers = _tethered(c)
    ts0, gs0 = _zeros(c, tethers)
    ts0[0, 1] = torch.tensor([0.1, 0.2, -0.1, 1.0, 0.1, 0.21, -0.1, 1.0])  # a path already: the pin acts and alpha extrapolates at once
    exp, est, et, eg, _ = _per_frame(c, terms, tethers, _state_ar(c), ts0, gs0)
    got, gst, gt, gg, _ = _launch(c, terms, tethers, _state_ar(c), ts0, gs0)
    torch.cuda.synchronize()
    _assert_same(got, exp, KEYS, "1x1")
    _assert_same(gst, est, STATE_KEYS, "1x1")
    assert _same(gt, et) and _same(gg, eg) and float(got["terms"][0, 0, -1]) > 0.0
    assert not torch.equal(gt[0, 1, :3], gt[0, 1, 4:7])


def test_mixed_skeletons():
    c, opt = _clip(9, 6), _opt()
    own = torch.from_numpy(opt.host_model.arrays["offsets"]).to(opt.device).reshape(22, 3).contiguous()
    mixed = (own[None] * torch.tensor([1.0, 0.95, 1.05], device=opt.device)[torch.arange(c.S) % 3][:, None, None]).contiguous()
    terms, tethers = _tethered(c)
    ts0, gs0 = _zeros(c, tethers)
    exp, est, et, eg, _ = _per_frame(c, terms, tethers, _state_ar(c), ts0, gs0, offsets=mixed)
    got, gst, gt, gg, _ = _launch(c, terms, tethers, _state_ar(c), ts0, gs0, offsets=mixed)
    same, _, _, _, _ = _launch(c, terms, tethers, _state_ar(c), ts0, gs0)
    torch.cuda.synchronize()
    _assert_same(got, exp, KEYS, "skeletons")
    _assert_same(gst, est, STATE_KEYS, "skeletons")
    assert _same(gt, et) and _same(gg, eg)
    assert torch.equal(got["pose_ret"][:, 0::3], same["pose_ret"][:, 0::3]) and not torch.equal(got["pose_ret"][:, 1::3], same["pose_ret"][:, 1::3])


def test_a_nan_state_row():
    """sequence 4's knee row holds a NaN: step 0 is BAD_TARGETS, the sequence BAD_STATE from step 1 on, its tether rows as the composition
    leaves them (the refused steps repeat them); the ten other sequences are bit-identical to the run without the NaN"""
    c = _clip(S, 6)
    terms, tethers = _tethered(c)
    ts0, gs0 = _zeros(c, tethers)
    bad = ts0.clone()
    bad[4, 0] = torch.tensor([0.0, float("nan"), 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    exp, _, et, _, _ = _per_frame(c, terms, tethers, _state_ar(c), bad, gs0)
    got, gst, gt, gg, _ = _launch(c, terms, tethers, _state_ar(c), bad, gs0)
    clean, cst, ct, cg, _ = _launch(c, terms, tethers, _state_ar(c), ts0, gs0)
    torch.cuda.synchronize()
    assert int(got["status"][0, 4]) == ST.NONFINITE | ST.BAD_TARGETS and int(got["iters"][0, 4]) == 1
    assert bool((got["status"][1:, 4] == (ST.NONFINITE | ST.BAD_STATE)).all()) and bool(got["pose_ret"][1:, 4].isnan().all())
    assert _same(got["tether_trace"], exp["tether_trace"]) and _same(gt, et)
    assert _same(got["tether_trace"][1:, 4], got["tether_trace"][:1, 4].expand(5, -1, -1))  # the refused steps repeat the state
    others = [s for s in range(S) if s != 4]
    for k in KEYS:
        assert torch.equal(got[k][:, others], clean[k][:, others]), k
    for k in STATE_KEYS:
        assert torch.equal(getattr(gst, k)[others], getattr(cst, k)[others]), k
    assert torch.equal(gt[others], ct[others]) and torch.equal(gg[others], cg[others])
    for k in ("pose_ret", "pos_ret", "iters", "loss", "terms", "joint_pos"):
        assert _same(got[k], exp[k]), k  # (the composition refuses the same steps; its gap rule, unlike the launch's, goes on through them)


def test_an_inert_tether_leaves_its_rows_alone():
    """weight 0 on the knee's term: its rows of `state` and `trace`, pre-filled with a sentinel, are neither read (the sentinel would refuse
    the step) nor written; the elbow's tether runs as ever"""
    c = _clip(S, 6)
    terms, tethers = _tethered(c, weights=(0.0, 0.8))
    ts0, gs0 = _zeros(c, tethers)
    ts0[:, 0] = -7.5e8
    trace = torch.full((6, S, 2, 8), -7.5e8, device=ts0.device)
    exp, est, et, _, _ = _per_frame(c, terms, tethers, _state_ar(c), ts0, gs0)
    got, gst, gt, _, _ = _launch(c, terms, tethers, _state_ar(c), ts0, gs0, trace=trace)
    torch.cuda.synchronize()
    assert bool((gt[:, 0] == -7.5e8).all()) and bool((trace[:, :, 0] == -7.5e8).all())
    assert bool((gt[:, 1, 3] == 1).all()) and _same(gt, et) and _same(trace[:, :, 1], exp["tether_trace"][:, :, 1])
    _assert_same(got, exp, OUT_KEYS + ("scratch", "gap_trace"), "inert")
    _assert_same(gst, est, STATE_KEYS, "inert")
    assert int(got["status"].max()) == 0


def test_everything_at_once():
    """two holds on other terms, an order-2 LatentAR, Gaps(3, 0.7) with sequence 2's joint 17 blanked for 4 frames (held 3, lost 1)"""
    c, ar, gaps, holds = _clip(S, T), _model(2), _gaps(3, 0.7), _holds()
    terms, tethers = _tethered(c, held=True)
    ts0, gs0 = _zeros(c, tethers)
    hs0 = torch.zeros(S, 2, 4, device=ts0.device)
    present = torch.ones(T, S, 22, dtype=torch.uint8, device=ts0.device)
    present[5:9, 2, 17] = 0
    kw = dict(gaps=gaps, ar=ar, holds=holds, hstate=hs0, present=present)
    exp, est, et, eg, eh = _per_frame(c, terms, tethers, _state_ar(c), ts0, gs0, **kw)
    got, gst, gt, gg, gh = _launch(c, terms, tethers, _state_ar(c), ts0, gs0, **kw)
    torch.cuda.synchronize()
    _assert_same(got, exp, KEYS + ("z_tgt", "hold_trace"), "all")
    _assert_same(gst, est, STATE_KEYS, "all")
    assert _same(gt, et) and _same(gg, eg) and _same(gh, eh)
    assert got["gap_trace"][5:10, 2, 17].tolist() == [2, 2, 2, 3, 1] and bool((gh[:, :, 3] == 1).all())
    assert not (got["status"] & (ST.BAD_STATE | ST.BAD_TARGETS)).any() and bool(torch.isfinite(got["pose_ret"]).all())


@pytest.mark.parametrize("with_ar", (True, False))
def test_no_tether_is_the_gaps_call(with_ar):
    """n_tethers = 0: dp_optimize_sequence_gaps' bits on every output and state array"""
    from dragposer_amd import Tethers

    c, ar, gaps = _clip(S, T), (_model(2) if with_ar else None), _gaps(3, 0.7)
    terms = _table(c)
    present = torch.ones(T, S, 22, dtype=torch.uint8, device=c.z0.device)
    present[5:9, 2, 17] = 0
    none = Tethers([])
    ts0, gs0 = _zeros(c, none)
    got, gst, gt, gg, _ = _launch(c, terms, none, _state_ar(c), ts0, gs0, gaps=gaps, ar=ar, present=present)
    exp, est, _, eg, _ = _launch(c, terms, None, _state_ar(c), None, gs0, gaps=gaps, ar=ar, present=present)
    torch.cuda.synchronize()
    keys = OUT_KEYS + ("scratch", "gap_trace") + (("z_tgt",) if with_ar else ())
    _assert_same(got, exp, keys, with_ar)
    _assert_same(gst, est, STATE_KEYS, with_ar)
    assert _same(gg, eg) and tuple(got["tether_trace"].shape) == (T, S, 0, 8)


def test_run_frames_equals_the_loop_of_run_across_a_prediction():
    """a seeded predictor, window 8, native temporal, T = 20: run_frames(terms=, tethers=) cuts 8 / 8 / 4 and equals per-frame
    run(terms=, tethers=) on poses, positions, counts, the tether state after every frame and the whole state"""
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.temporal import TemporalPredictor

    c = _clip(S, T)
    terms, tethers = _tethered(c)
    terms = type(terms)([t for t in terms.terms if t.per_frame is None], terms.up_axis)  # (run() takes [S,4] rows only)
    tethers = type(tethers)([replace(t, term=t.term - 1) for t in tethers.tethers])
    torch.manual_seed(5)
    predictor = TemporalPredictor(n_encoder_layers=1, n_decoder_layers=1, dim_feedforward=16)
    idx = np.array(R.TRACK6)
    wts = np.array([R.W6[j] for j in R.TRACK6], np.float32)
    kw = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2, max_iter=10, min_loss_incr=1e-5, learning_rate=1e-2, lambda_rot=1, lambda_temporal=0.02,
              temporal_future_window=8, height_indices=HJ, joint_adjustment_indices=(0, 3), joint_adjustment_weight=0.5, terms=terms, tethers=tethers)
    dps = []
    for _ in range(2):
        dp = DragPose(_opt(), predictor, np.zeros(24), np.ones(24), n_sequences=c.S, native_temporal=True)
        dp.set_initial_state(c.z0, np.zeros((c.S, 3), np.float32), c.rot0, c.heights0)
        assert dp.tether_state is None
        dps.append(dp)
    a, b = dps
    tp, tR = c.tgt_pos[:, :, idx], c.tgt_rot[:, :, idx].reshape(c.T, c.S, -1, 3, 3)
    pa, ga, ia, ta = [], [], [], []
    for t in range(c.T):
        pose, gpos = a.run(tp[t], tR[t], idx, wts, **kw)
        pa.append(pose.clone()); ga.append(gpos.clone()); ia.append(a.last["iters"].clone()); ta.append(a.tether_state.clone())
    calls = []
    seq = b.opt.optimize_sequence
    b.opt.optimize_sequence = lambda *x, **k: (calls.append((int(x[1].shape[0]), k.get("tethers") is not None)), seq(*x, **k))[1]
    try:
        pb, gb, ib = b.run_frames(tp, tR, idx, wts, **kw)
    finally:
        del b.opt.optimize_sequence
    torch.cuda.synchronize()
    assert calls == [(8, True), (8, True), (4, True)]
    assert torch.equal(torch.stack(pa), pb) and torch.equal(torch.stack(ga), gb) and torch.equal(torch.stack(ia), ib)
    assert torch.equal(a.tether_state, b.tether_state) and torch.equal(torch.stack(ta), b.last_tether_trace)
    assert bool((b.tether_state[:, :, 3] == 1).all()) and bool(torch.isfinite(pb).all())
    for attr in ("latent", "current_global_pos", "current_global_rot", "latent_buffer", "displacement_buffer", "heights_buffer", "target_latent_buffer",
                 "gap_state"):
        assert torch.equal(getattr(a, attr), getattr(b, attr)), attr
    with pytest.raises(ValueError, match="run_frames"):
        a.run(tp[0], tR[0], idx, wts, live=True, **kw)
    b.set_initial_state(c.z0, np.zeros((c.S, 3), np.float32), c.rot0, c.heights0)
    assert b.tether_state is None  # a new sequence begins without a path


def test_a_tethered_hand_follows_a_jump_more_slowly():
    """One sequence, no joint adjustment, up to 30 iterations a frame at lr 3e-3 (an Adam step moves a latent component by at most lr, so a
    frame at rest moves the hand by millimetres and a frame after the jump by centimetres).  Sixty warm-up frames at lr 1e-2 on targets that
    stand still bring the reconstruction to rest; then twelve frames whose hand target (joint 17, tracked) jumps by 0.5 m at frame 6, once with a
    tether on that hand (hi = 0.02, weight 10) and once with the term's weight 0.  Before the jump the hand moves less than 0.02 m a frame,
    the band is never left and both runs give equal bits on frames 0..5; at frame 6 the tethered hand's displacement is strictly smaller."""
    from dragposer_amd import Tether, Tethers
    from dragposer_amd.terms import Term, Terms

    HAND = 17
    c0, opt = _clip(1, 12), _opt()
    c = copy.copy(c0)
    c.T = 60
    c.tgt_pos, c.tgt_rot = c0.tgt_pos[:1].repeat(60, 1, 1, 1), c0.tgt_rot[:1].repeat(60, 1, 1, 1)  # targets that stand still, in the world
    c.root, c.z_tgt = torch.zeros(60, 1, 3, device=opt.device), c0.z_tgt[:1].repeat(60, 1, 1)
    tethers = Tethers([Tether(0, 0.0)])
    table = lambda w: Terms([Term.distance(HAND, point=(0.0, 0.0, 0.0), lo=0.0, hi=0.02, weight=w)])
    ts0, gs0 = _zeros(c, tethers)
    kw = dict(adjust=None, lr=3e-3, loop=dict(LOOP, n_iter=30), T=12)
    warm, st, ts1, gs1, _ = _launch(c, table(10.0), tethers, _state_ar(c), ts0, gs0, **dict(kw, lr=1e-2, T=60))
    print("warm-up iterations:", warm["iters"][:, 0].tolist())
    jump = c.tgt_pos.clone()
    jump[6:, 0, HAND, 0] += 0.5
    on, _, _, _, _ = _launch(c, table(10.0), tethers, copy.deepcopy(st), ts1, gs1, tgt_pos=jump, **kw)
    off, _, _, _, _ = _launch(c, table(0.0), tethers, copy.deepcopy(st), ts1, gs1, tgt_pos=jump, **kw)
    torch.cuda.synchronize()
    w_on, w_off = _world(on, HAND)[:, 0], _world(off, HAND)[:, 0]
    last = ts1[0, 0, 4:7]  # the hand where the warm-up left it
    steps = torch.linalg.norm(torch.diff(torch.cat((last[None], w_off[:6])), dim=0), dim=1)
    print("hand steps before the jump (m):", steps.tolist(), "iterations", on["iters"][:, 0].tolist(), off["iters"][:, 0].tolist())
    assert float(steps.max()) < 0.02 and bool((on["terms"][:6] == 0).all())  # the premise: the band is never left before the jump
    for k in ("pose_ret", "pos_ret", "iters", "joint_pos", "loss"):
        assert torch.equal(on[k][:6], off[k][:6]), k
    d_on, d_off = float(torch.linalg.norm(w_on[6] - w_on[5])), float(torch.linalg.norm(w_off[6] - w_off[5]))
    print("hand displacement at the jump (m): tethered", d_on, "free", d_off)
    assert d_on < d_off and float(on["terms"][6, 0, 0]) > 0.0

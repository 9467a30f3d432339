"""GPU: dp_optimize_sequence_gaps (include/dragposer_gaps.h) -- dp_optimize_sequence_ar / _holds with a tracker set decided per step --
against the per-frame composition the header names: Gaps.step for the step's effective targets, weights and tracker set, optimize_terms on
them, then sequence_advance, then the latent copy.  The same arithmetic in the same order: every comparison is bit for bit (NaN where NaN);
no tolerance is involved.  The shape is S = 11 (a workgroup of 8 waves and one of 3), T = 20, max_iter 10 with the reference's early stop,
tgt_root on, joint adjustment (0, 13, 0.5), a table with a [T,S,4] term."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from test_hip_latent_ar import ADJ, LAM, LOOP, _holds, _model, _state_ar, _table
from test_hip_sequence_constraints import HJ, OUT_KEYS, ST, STATE_KEYS, _assert_same, _clip, _opt, _row, _same

pytestmark = pytest.mark.gpu

HELD_BIT, LOST_BIT, NONE_BIT = 16, 32, 64
KEYS = OUT_KEYS + ("scratch", "gap_trace")
S, T = 11, 20


def _gaps(max_hold=3, decay=0.7):
    from dragposer_amd import Gaps

    return Gaps(max_hold, decay)


@functools.lru_cache(maxsize=None)
def _script():
    """the issue's gap script on the clip -> (tgt_pos with the NaN samples, present [T,S,22])"""
    c = _clip(S, T)
    tgt = c.tgt_pos.clone()
    present = torch.ones(T, S, 22, dtype=torch.uint8, device=tgt.device)
    present[3:6, 2, 17] = 0               # sequence 2, joint 17: absent at steps 3-5 (held throughout), given through `present`
    tgt[8:15, 2, 13, 1] = float("nan")    # sequence 2, joint 13, the adjustment's target: a NaN component at steps 8-14 (held 3, lost 4, back at 15)
    present[0:4, 9, 0] = 0                # sequence 9, joint 0: absent from step 0 (never seen: lost until it appears at step 4)
    return tgt, present


def _zeros(c):
    return torch.zeros(c.S, 22, 16, device=c.z0.device)


def _per_frame(c, gaps, terms, st, gstate, ar=None, tgt_pos=None, present=None, t0=0, T=None, offsets=None):
    """the composition, frame by frame on the host -> (outputs, the state, the gap state)"""
    from dragposer_amd.terms import Terms

    opt, S, T = _opt(), c.S, T or c.T
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    gstate = gstate.clone()
    fr = opt.allocate_outputs(S, ("z", "z_pre", "pose", "disp", "world_disp", "world_rot", "pos", "loss", "iters", "status"))
    fr["loss_terms"] = torch.empty(S, len(terms), device=opt.device)
    o = {k: [] for k in KEYS + ("z_tgt",)}
    for t in range(t0, t0 + T):
        zt = ar.predict(st.lbuf) if ar is not None else c.z_tgt[t]
        tp = (tgt_pos[t] + (c.root[t] - st.gpos).unsqueeze(1)).contiguous()
        tp_e, tr_e, w_e, on, code = gaps.step(gstate, tp, c.tgt_rot[t], c.w, c.tracked, st.gpos, present[t] if present is not None else None)
        assert int(on.sum(dim=1).min()) >= 1  # (the composition is stated for E >= 1)
        rows = [_row(x) for x in terms.frames(t, t + 1).terms]
        opt.optimize_terms(st.latent, zt, st.grot, tp_e, tr_e, w_e, on, Terms(rows, terms.up_axis), global_pos=st.gpos, lr=1e-2, lambda_rot=1.0,
                           lambda_tmp=LAM, out=fr, outputs=tuple(fr), offsets=offsets, **LOOP)
        # a lost (or untracked) adjustment target: the adjusted joint's own position, so that adj = +0
        tp_adj = tp_e.clone()
        tp_adj[:, ADJ[1]] = torch.where(on[:, ADJ[1], None] != 0, tp_e[:, ADJ[1]], fr["pos"][:, ADJ[0]])
        pose, pos = torch.empty(S, 88, device=opt.device), torch.empty(S, 3, device=opt.device)
        opt.sequence_advance(fr, st.gpos, st.grot, st.lbuf, st.dbuf, st.hbuf, HJ, pose_ret=pose, pos_ret=pos, adjust=ADJ, tgt_pos=tp_adj)
        st.latent.copy_(fr["z"])
        bits = ((code == 2).any(dim=1) * HELD_BIT + (code == 3).any(dim=1) * LOST_BIT).to(torch.int32)
        for k, v in (("pose_ret", pose), ("pos_ret", pos), ("iters", fr["iters"]), ("status", fr["status"] | bits), ("loss", fr["loss"]),
                     ("terms", fr["loss_terms"]), ("joint_pos", fr["pos"]), ("z_tgt", zt), ("gap_trace", code),
                     ("scratch", torch.cat((st.lbuf[:, -1], st.dbuf[:, -1], st.hbuf[:, -1]), dim=1))):
            o[k].append(v.clone())
    return {k: torch.stack(v) for k, v in o.items()}, st, gstate


def _launch(c, gaps, terms, st, gstate, ar=None, tgt_pos=None, present=None, t0=0, T=None, offsets=None):
    """one launch over frames t0 .. t0 + T -> (outputs, the state, the gap state); gaps None: dp_optimize_sequence_ar / _terms"""
    opt, T = _opt(), T or c.T
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    sl = slice(t0, t0 + T)
    kw = {}
    if gaps is not None:
        gstate = gstate.clone()
        kw = dict(gaps=gaps, gap_state=gstate, gap_trace=True, present=present[sl].contiguous() if present is not None else None)
    if ar is not None:
        kw.update(ar=ar, z_tgt_trace=True)
    elif gaps is None:  # dp_optimize_sequence_holds, with no hold
        from dragposer_amd import Holds

        kw.update(holds=Holds([]), hold_state=torch.zeros(c.S, 0, 4, device=opt.device))
    scratch = torch.empty(T, c.S, 24 + 3 + len(HJ), device=opt.device)
    o = opt.optimize_sequence(st.latent, tgt_pos[sl], c.tgt_rot[sl], c.root[sl], c.w, c.tracked, None if ar is not None else c.z_tgt[sl],
                              (c.S * 24, 24), st.gpos, st.grot, st.lbuf, st.dbuf, st.hbuf, HJ, lr=1e-2, lambda_rot=1.0, lambda_tmp=LAM, adjust=ADJ,
                              offsets=offsets, scratch=scratch, terms=terms.frames(t0, t0 + T), **kw, **LOOP)
    o["terms"], o["scratch"] = o.pop("loss_terms"), scratch
    if ar is not None:
        o["z_tgt"] = o.pop("z_tgt_trace")
    return o, st, gstate


@pytest.mark.parametrize("with_ar", (True, False))
def test_one_launch_equals_the_composition_through_the_gap_script(with_ar):
    """1. held, lost and returning joints, the adjustment's target among them, with and without the predictor; 2. the nine sequences without a
    gap are bit-identical to the same launch with no gap anywhere"""
    c, ar, gaps = _clip(S, T), (_model(2) if with_ar else None), _gaps()
    tgt, present = _script()
    keys = KEYS + (("z_tgt",) if with_ar else ())
    exp, est, eg = _per_frame(c, gaps, _table(c), _state_ar(c), _zeros(c), ar, tgt, present)
    got, gst, gg = _launch(c, gaps, _table(c), _state_ar(c), _zeros(c), ar, tgt, present)
    clean, cst, cg = _launch(c, gaps, _table(c), _state_ar(c), _zeros(c), ar)
    torch.cuda.synchronize()
    _assert_same(got, exp, keys, with_ar)
    _assert_same(gst, est, STATE_KEYS, with_ar)
    assert _same(gg, eg)
    tr = got["gap_trace"]
    assert tr[3:6, 2, 17].tolist() == [2, 2, 2] and tr[6, 2, 17] == 1
    assert tr[8:16, 2, 13].tolist() == [2, 2, 2, 3, 3, 3, 3, 1]
    assert tr[0:5, 9, 0].tolist() == [3, 3, 3, 3, 1]
    assert set(tr.unique().tolist()) == {0, 1, 2, 3} and bool((tr[:, :, 1] == 0).all())
    status = got["status"]
    assert status[3:6, 2].tolist() == [HELD_BIT] * 3 and status[8:15, 2].tolist() == [HELD_BIT] * 3 + [LOST_BIT] * 4 and int(status[15, 2]) == 0
    assert status[0:5, 9].tolist() == [LOST_BIT] * 4 + [0]
    assert bool(torch.isfinite(got["pose_ret"]).all()) and bool(torch.isfinite(gg).all())
    assert float(gg[2, 13, 14]) == 1.0 and float(eg[9, 0, 12]) == 1.0  # both came back: factor 1, valid
    others = [s for s in range(S) if s not in (2, 9)]
    for k in keys:
        assert torch.equal(got[k][:, others], clean[k][:, others]), k
    for k in STATE_KEYS:
        assert torch.equal(getattr(gst, k)[others], getattr(cst, k)[others]), k
    assert torch.equal(gg[others], cg[others])
    assert not torch.equal(got["pose_ret"][:, 2], clean["pose_ret"][:, 2]) and not torch.equal(got["pose_ret"][:, 9], clean["pose_ret"][:, 9])


@pytest.mark.parametrize("with_ar", (True, False))
def test_a_clip_with_every_sample_present_equals_the_call_without_gaps(with_ar):
    """3. dp_optimize_sequence_ar's bits (dp_optimize_sequence_holds' with `ar` NULL) on every
    output and state array; gap_trace is 1 exactly on the tracked joints"""
    c, ar = _clip(S, T), (_model(2) if with_ar else None)
    present = torch.ones(T, S, 22, dtype=torch.uint8, device=c.z0.device)
    got, gst, gg = _launch(c, _gaps(), _table(c), _state_ar(c), _zeros(c), ar, present=present)
    nop, nst, ng = _launch(c, _gaps(0, 1.0), _table(c), _state_ar(c), _zeros(c), ar)
    exp, est, _ = _launch(c, None, _table(c), _state_ar(c), None, ar)
    torch.cuda.synchronize()
    keys = OUT_KEYS + ("scratch",) + (("z_tgt",) if with_ar else ())
    for o, s in ((got, gst), (nop, nst)):
        _assert_same(o, exp, keys, with_ar)
        _assert_same(s, est, STATE_KEYS, with_ar)
        assert torch.equal(o["gap_trace"], c.tracked[None].expand(T, S, 22))
    assert torch.equal(gg, ng) and int(exp["status"].max()) == 0
    trk = c.tracked.bool()
    assert bool((gg[..., 12][trk] == 1).all()) and bool((gg[..., 13:15][trk] == torch.tensor([0.0, 1.0], device=gg.device)).all())
    assert not gg[~trk].any() and torch.equal(gg[..., 3:12][trk], c.tgt_rot[T - 1][trk])


def test_a_cut_through_a_gap():
    """4. two chained launches of 10 steps equal one of 20: sequence 2's second gap (steps 8-14) straddles the cut, gap_state carries it"""
    c, ar, gaps = _clip(S, T), _model(2), _gaps()
    tgt, present = _script()
    one, ost, og = _launch(c, gaps, _table(c), _state_ar(c), _zeros(c), ar, tgt, present)
    a, st, g = _launch(c, gaps, _table(c), _state_ar(c), _zeros(c), ar, tgt, present, T=10)
    assert float(g[2, 13, 12]) == 1.0 and float(g[2, 13, 13]) == 2.0  # the cut falls inside the hold: age 2 of 3
    b, st, g = _launch(c, gaps, _table(c), st, g, ar, tgt, present, t0=10, T=10)
    torch.cuda.synchronize()
    _assert_same({k: torch.cat((a[k], b[k])) for k in KEYS + ("z_tgt",)}, one, KEYS + ("z_tgt",), "chain")
    _assert_same(st, ost, STATE_KEYS, "chain")
    assert _same(g, og)


def test_a_step_without_any_tracker():
    """5. sequence 5 loses every tracker at steps 6-12 with max_hold = 2: held at 6 and 7, E == 0 from 8 to 12 (DP_STATUS_NO_TRACKER, one pass,
    both tracker losses exactly 0, everything finite).  Launch A covers steps 0-12; from its final state steps 13-19 equal the composition
    again; the sequence never becomes BAD_STATE; the ten others equal the run without the blackout."""
    c, ar, gaps = _clip(S, T), _model(2), _gaps(2, 0.7)
    present = torch.ones(T, S, 22, dtype=torch.uint8, device=c.z0.device)
    present[6:13, 5] = 0
    full, fst, fg = _launch(c, gaps, _table(c), _state_ar(c), _zeros(c), ar, present=present)
    clean, cst, cg = _launch(c, gaps, _table(c), _state_ar(c), _zeros(c), ar)
    a, ast, ag = _launch(c, gaps, _table(c), _state_ar(c), _zeros(c), ar, present=present, T=13)
    import copy

    exp, est, eg = _per_frame(c, gaps, _table(c), copy.deepcopy(ast), ag, ar, present=present, t0=13, T=7)
    b, bst, bg = _launch(c, gaps, _table(c), ast, ag, ar, present=present, t0=13, T=7)
    torch.cuda.synchronize()
    keys = KEYS + ("z_tgt",)
    _assert_same(b, exp, keys, "after the blackout")
    _assert_same(bst, est, STATE_KEYS, "after the blackout")
    assert _same(bg, eg)
    _assert_same({k: torch.cat((a[k], b[k])) for k in keys}, full, keys, "A + B")
    st5 = full["status"][:, 5].tolist()
    assert st5[:6] == [0] * 6 and st5[6:8] == [HELD_BIT] * 2 and st5[8:13] == [LOST_BIT | NONE_BIT] * 5 and st5[13:] == [0] * 7
    assert not any(x & (ST.BAD_STATE | ST.BAD_TARGETS | ST.NONFINITE) for x in st5)
    assert full["iters"][8:13, 5].tolist() == [1] * 5
    assert bool((full["loss"][8:13, 5, :2] == 0).all()) and bool((full["loss"][8:13, 5, 2] > 0).all())  # the pull term acts alone
    trk = c.tracked[5].bool()
    assert bool((full["gap_trace"][8:13, 5][:, trk] == 3).all()) and bool((full["gap_trace"][6:8, 5][:, trk] == 2).all())
    for k in keys:
        assert bool(torch.isfinite(full[k][:, 5].float()).all()), k
    assert bool(torch.isfinite(fg).all()) and all(bool(torch.isfinite(getattr(fst, k)).all()) for k in STATE_KEYS)
    others = [s for s in range(S) if s != 5]
    for k in keys:
        assert torch.equal(full[k][:, others], clean[k][:, others]), k
    for k in STATE_KEYS:
        assert torch.equal(getattr(fst, k)[others], getattr(cst, k)[others]), k
    assert torch.equal(fg[others], cg[others])


def test_the_old_behaviour_is_still_there():
    """6. the same NaN sample through dp_optimize_sequence_ar: BAD_TARGETS at the step, BAD_STATE from the next on"""
    c, ar = _clip(S, T), _model(2)
    tgt, _ = _script()
    got, _, _ = _launch(c, None, _table(c), _state_ar(c), None, ar, tgt, T=12)
    torch.cuda.synchronize()
    assert int(got["status"][8, 2]) == ST.NONFINITE | ST.BAD_TARGETS and int(got["iters"][8, 2]) == 1
    assert bool((got["status"][9:, 2] == (ST.NONFINITE | ST.BAD_STATE)).all()) and bool(got["pose_ret"][9:, 2].isnan().all())
    assert int(got["status"][:, [s for s in range(S) if s != 2]].max()) == 0


@pytest.mark.parametrize("with_ar", (True, False))
def test_run_frames_equals_the_loop_of_run(with_ar):
    """7. DragPose.run_frames(gaps=, present=) equals T calls of run(gaps=, present=), with two holds, per-sequence skeletons and joint
    adjustment beside it; the gaps arrive as NaN samples and through `present`, in tracker-list order"""
    from dragposer_amd.drag_pose import DragPose

    c, ar, opt, gaps = _clip(S, T), (_model(2) if with_ar else None), _opt(), _gaps()
    own = torch.from_numpy(opt.host_model.arrays["offsets"]).to(opt.device).reshape(22, 3).contiguous()
    mixed = (own[None] * torch.tensor([1.0, 0.95, 1.05], device=opt.device)[torch.arange(c.S) % 3][:, None, None]).contiguous()
    idx = np.array(R.TRACK6)
    wts = np.array([R.W6[j] for j in R.TRACK6], np.float32)
    e17, e13 = list(idx).index(17), list(idx).index(13)
    kw = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2, max_iter=10, min_loss_incr=1e-5, learning_rate=1e-2, lambda_rot=1, lambda_temporal=0.15,
              height_indices=HJ, joint_adjustment_indices=(0, e13), joint_adjustment_weight=0.5, offsets=mixed, terms=_table(c, held=True),
              holds=_holds(), gaps=gaps)
    if with_ar:
        kw["ar"] = ar
    a, b = (DragPose(opt, None, np.zeros(24), np.ones(24), n_sequences=c.S) for _ in range(2))
    for dp in (a, b):
        dp.set_initial_state(c.z0, np.zeros((c.S, 3), np.float32), c.rot0, c.heights0)
        assert tuple(dp.gap_state.shape) == (c.S, 22, 16) and not dp.gap_state.any()
    tp, tR = c.tgt_pos[:, :, idx].clone(), c.tgt_rot[:, :, idx].reshape(c.T, c.S, -1, 3, 3)
    tp[8:15, 2, e13, 1] = float("nan")
    present = torch.ones(c.T, c.S, len(idx), dtype=torch.uint8, device=opt.device)
    present[3:6, 2, e17] = 0
    pa, ga, ia, ta = [], [], [], []
    for t in range(c.T):
        k = dict(kw, terms=kw["terms"].frames(t, t + 1))
        pose, gpos = a.run(tp[t], tR[t], idx, wts, present=present[t], **k)
        pa.append(pose.clone()); ga.append(gpos.clone()); ia.append(a.last["iters"].clone()); ta.append(a.last["gap_trace"].clone())
    pb, gb, ib = b.run_frames(tp, tR, idx, wts, present=present, **kw)
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(pa), pb) and torch.equal(torch.stack(ga), gb) and torch.equal(torch.stack(ia), ib)
    assert tuple(b.last_gap_trace.shape) == (c.T, c.S, 22) and torch.equal(torch.stack(ta), b.last_gap_trace)
    assert b.last_gap_trace[8:16, 2, 13].tolist() == [2, 2, 2, 3, 3, 3, 3, 1] and b.last_gap_trace[3:6, 2, 17].tolist() == [2, 2, 2]
    for attr in ("latent", "current_global_pos", "current_global_rot", "latent_buffer", "displacement_buffer", "heights_buffer", "gap_state", "hold_state"):
        assert torch.equal(getattr(a, attr), getattr(b, attr)), attr
    assert bool(torch.isfinite(pb).all()) and not (b.last_status & (ST.BAD_STATE | ST.BAD_TARGETS)).any()
    assert torch.equal(a.last["loss"], b.last_loss[-1])
    b.set_initial_state(c.z0, np.zeros((c.S, 3), np.float32), c.rot0, c.heights0)
    assert not b.gap_state.any()  # a sequence that begins holds nothing


def test_the_command_lines_blank_a_tracker_and_carry_on(tmp_path, capsys):
    """8. eval_drag --drop blanks a hand tracker's samples on the short clip, --gaps carries the clip through them: both position errors over
    the blanked frames alone are printed, the frame loop on the device and --per-frame write the same bytes, with and without --latent-ar"""
    from dragposer_amd import eval_drag

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    clip = os.path.join(root, "tests", "data", "example_clip.bvh")
    argv = [clip, "--config", os.path.join(root, "dragposer_amd", "config", "6_trackers_config.json"), "--max-frames", "48", "--keep-frames",
            "--drop", "17:10:8,17:30:4", "--gaps", "5:0.8"]
    for d in ("device", "host", "ar", "whole"):
        os.makedirs(tmp_path / d)
    a = eval_drag.main(argv + ["--out-dir", str(tmp_path / "device")])[0]
    text = capsys.readouterr().out
    assert "Blanked frames (12 of 48, --drop 17:10:8,17:30:4)" in text and "Gaps: max_hold 5, decay 0.8" in text
    b = eval_drag.main(argv + ["--out-dir", str(tmp_path / "host"), "--per-frame"])[0]
    assert a["frames"] == b["frames"] == 48 and open(a["out"], "rb").read() == open(b["out"], "rb").read()
    r = eval_drag.main(argv + ["--latent-ar", "hold", "--out-dir", str(tmp_path / "ar")])[0]
    w = eval_drag.main(argv[:6] + ["--out-dir", str(tmp_path / "whole")])[0]
    capsys.readouterr()
    for o in (a, r):
        assert np.isfinite(o["poses"]).all() and all(np.isfinite(o[k]) for k in ("mpjpe", "mpeepe", "mpjpe_blanked", "mpeepe_blanked"))
    assert "mpjpe_blanked" not in w
    assert not np.array_equal(a["poses"][10:], w["poses"][10:])  # (the blanked tracker is missed)
    assert not np.array_equal(a["poses"], r["poses"])

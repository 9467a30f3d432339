"""GPU: dp_live_step (include/dragposer_live.h) -- one step of dp_optimize_sequence_gaps with the history append done by the kernel -- frame by
frame against dp_optimize_sequence_gaps with one step, from identical starts.  The same instructions but for the append, so every comparison
is of the bits (NaN patterns included) on every output and state array; no tolerance is involved.  max_iter 10 with the reference's early
stop, tgt_root on, joint adjustment (0, 13, 0.5), a table with a per-frame term and two held terms."""
import copy

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from test_hip_latent_ar import ADJ, LAM, LOOP, _model, _state_ar, _table
from test_hip_sequence_constraints import HJ, ST, STATE_KEYS, _clip, _opt

pytestmark = pytest.mark.gpu

HELD_BIT, LOST_BIT, NONE_BIT = 16, 32, 64
S, T = 9, 64  # one full workgroup and a ragged one; more frames than the 60-row ring: every row has been shifted out
OUT = ("pose_ret", "pos_ret", "iters", "status", "loss", "loss_terms", "joint_pos", "hold_trace", "gap_trace")


def _bits(a, b):
    """equal bit for bit (torch.equal would call two NaNs different)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_floating_point():
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def _predictor(kind):
    from dragposer_amd import LatentAR

    return {"none": None, "hold": LatentAR.hold(), "ar4": _model(4)}[kind]  # the closed-form order 1; a seeded stable order 4


def _holds():
    """hold 0 latches at once (level +10: every height is below it); hold 1 starts held and lets go at once (level -10)"""
    from dragposer_amd import Hold, Holds

    return Holds([Hold(2, 0.0, 0.1, level=10.0), Hold(3, 0.0, 0.1, level=-10.0)])


def _start(c, rows=60):
    st = _state_ar(c, rows)
    hstate = torch.zeros(c.S, 2, 4, device=st.latent.device)
    hstate[:, 1] = torch.tensor([0.1, 0.0, 0.2, 1.0], device=st.latent.device)
    return st, hstate, torch.zeros(c.S, 22, 16, device=st.latent.device)


def _step(c, t, st, hstate, gstate, ar, gaps, live, tgt_pos, present, offsets):
    """frame t as one call, on (and into) the given state -> the call's outputs and its hist_scratch row"""
    opt = _opt()
    sl = slice(t, t + 1)
    scratch = torch.empty(1, c.S, 24 + 3 + len(HJ), device=opt.device)
    kw = dict(ar=ar, z_tgt_trace=True) if ar is not None else {}
    o = opt.optimize_sequence(st.latent, tgt_pos[sl], c.tgt_rot[sl], c.root[sl], c.w, c.tracked, None if ar is not None else c.z_tgt[sl],
                              (c.S * 24, 24), st.gpos, st.grot, st.lbuf, st.dbuf, st.hbuf, HJ, lr=1e-2, lambda_rot=1.0, lambda_tmp=LAM, adjust=ADJ,
                              offsets=offsets, scratch=scratch, terms=_table(c, held=True).frames(t, t + 1), holds=_holds(), hold_state=hstate,
                              hold_trace=True, gaps=gaps, gap_state=gstate, gap_trace=True,
                              present=present[sl].contiguous() if present is not None else None, live=live, **kw, **LOOP)
    o["scratch"] = scratch
    return o


def _walk(c, kind, frames, rows=60, tgt_pos=None, present=None, offsets=None, nan_from=None):
    """both calls frame by frame; after every frame every output and the whole state are compared -> the live side's outputs, stacked"""
    from dragposer_amd import Gaps

    ar, gaps = _predictor(kind), Gaps(3, 0.7)
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    a = _start(c, rows)
    b = copy.deepcopy(a)
    keys = OUT + ("scratch",) + (("z_tgt_trace",) if ar is not None else ())
    got = {k: [] for k in keys}
    for t in range(frames):
        if nan_from is not None and t == nan_from[0]:
            for side in (a, b):
                side[0].latent[nan_from[1]] = float("nan")
        oa = _step(c, t, *a, ar, gaps, True, tgt_pos, present, offsets)
        ob = _step(c, t, *b, ar, gaps, False, tgt_pos, present, offsets)
        for k in keys:
            assert _bits(oa[k], ob[k]), (k, t)
            got[k].append(oa[k][0].clone())
        for k in STATE_KEYS:
            assert _bits(getattr(a[0], k), getattr(b[0], k)), (k, t)
        assert _bits(a[1], b[1]) and _bits(a[2], b[2]), t
    torch.cuda.synchronize()
    return {k: torch.stack(v) for k, v in got.items()}, a


@pytest.mark.parametrize("kind", ("none", "hold", "ar4"))
def test_every_frame_equals_the_two_launch_call_through_the_script(kind):
    c = _clip(S, T)
    tgt = c.tgt_pos.clone()
    present = torch.ones(T, S, 22, dtype=torch.uint8, device=tgt.device)
    present[3:6, 2, 17] = 0             # a joint held through `present`
    tgt[8:15, 2, 13, 1] = float("nan")  # the adjustment's target: held 3 frames, lost 4 and back, through a NaN component
    present[30, 5] = 0                  # a blackout frame
    opt = _opt()
    own = torch.from_numpy(opt.host_model.arrays["offsets"]).to(opt.device).reshape(22, 3).contiguous()
    mixed = (own[None] * torch.tensor([1.0, 0.95, 1.05], device=opt.device)[torch.arange(S) % 3][:, None, None]).contiguous()
    got, (st, hstate, gstate) = _walk(c, kind, T, tgt_pos=tgt, present=present, offsets=mixed, nan_from=(20, 7))
    # ... and the script did what it says (so the equality above covered it)
    tr, status = got["gap_trace"], got["status"]
    assert tr[3:6, 2, 17].tolist() == [2, 2, 2] and tr[6, 2, 17] == 1
    assert tr[8:16, 2, 13].tolist() == [2, 2, 2, 3, 3, 3, 3, 1]
    assert int(status[30, 5]) & HELD_BIT and not int(status[30, 5]) & (ST.BAD_STATE | ST.BAD_TARGETS)
    ht = got["hold_trace"]
    assert bool((ht[0, :, 0, 3] == 1).all()) and bool((ht[0, :, 1, 3] == 0).all())  # a touch-down and a release, at the first frame
    assert bool((status[20:, 7] & ST.BAD_STATE != 0).all()) and bool((tr[20:, 7] == 0xFF).all()) and bool(got["scratch"][20:, 7].isnan().all())
    assert bool(st.lbuf[7, 60 - (T - 20):].isnan().all()) and bool(torch.isfinite(st.lbuf[7, :60 - (T - 20)]).all())
    others = [s for s in range(S) if s != 7]
    assert bool(torch.isfinite(got["pose_ret"][:, others]).all()) and bool(torch.isfinite(st.lbuf[others]).all())
    # every row of the ring is one of this run's: the last 60 hist_scratch rows, in order
    sc = got["scratch"][T - 60:].transpose(0, 1)
    assert _bits(st.lbuf, sc[..., :24].contiguous()) and _bits(st.dbuf, sc[..., 24:27].contiguous()) and _bits(st.hbuf, sc[..., 27:].contiguous())


@pytest.mark.parametrize("n_seq,frames,rows", [(1, 8, 60), (3, 7, 5)])  # S = 1; a history depth that is no multiple of the append's chunk
def test_small_shapes_and_a_short_history(n_seq, frames, rows):
    c = _clip(n_seq, 8)
    for kind in ("none", "ar4"):
        got, (st, _, _) = _walk(c, kind, frames, rows=rows)
        assert tuple(st.lbuf.shape) == (n_seq, rows, 24)
        n = min(frames, rows)
        assert _bits(st.lbuf[:, rows - n:], got["scratch"][frames - n:, :, :24].transpose(0, 1).contiguous())


def test_dragpose_run_live_equals_run():
    """DragPose.run(live=True) against live=False over 10 frames: terms, two holds, a predictor, gaps through NaN and `present`"""
    from dragposer_amd import Gaps
    from dragposer_amd.drag_pose import DragPose

    c, opt = _clip(S, T), _opt()
    idx = np.array(R.TRACK6)
    wts = np.array([R.W6[j] for j in R.TRACK6], np.float32)
    e17, e13 = list(idx).index(17), list(idx).index(13)
    kw = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2, max_iter=10, min_loss_incr=1e-5, learning_rate=1e-2, lambda_rot=1, lambda_temporal=0.15,
              height_indices=HJ, joint_adjustment_indices=(0, e13), joint_adjustment_weight=0.5, holds=_holds(), ar=_model(2), gaps=Gaps(3, 0.7))
    a, b = (DragPose(opt, None, np.zeros(24), np.ones(24), n_sequences=S) for _ in range(2))
    for dp in (a, b):
        dp.set_initial_state(c.z0, np.zeros((S, 3), np.float32), c.rot0, c.heights0)
    tp, tR = c.tgt_pos[:10, :, idx].clone(), c.tgt_rot[:10, :, idx].reshape(10, S, -1, 3, 3)
    tp[4:9, 2, e13, 1] = float("nan")
    present = torch.ones(10, S, len(idx), dtype=torch.uint8, device=opt.device)
    present[2:4, 2, e17] = 0
    for t in range(10):
        k = dict(kw, terms=_table(c, held=True).frames(t, t + 1))
        pa, ga = a.run(tp[t], tR[t], idx, wts, present=present[t], live=True, **k)
        pb, gb = b.run(tp[t], tR[t], idx, wts, present=present[t], **k)
        assert _bits(pa, pb) and _bits(ga, gb), t
        for key in ("iters", "status", "loss", "gap_trace", "z_tgt", "z"):
            assert _bits(a.last[key], b.last[key]), (key, t)
        for attr in ("latent", "current_global_pos", "current_global_rot", "latent_buffer", "displacement_buffer", "heights_buffer", "gap_state", "hold_state"):
            assert _bits(getattr(a, attr), getattr(b, attr)), (attr, t)
    assert a.last_gap_trace is not None and bool(torch.isfinite(pa).all())
    assert not hasattr(opt, "live_step")
    # live= alone configures nothing to run
    with pytest.raises(ValueError, match="live= goes with"):
        a.run(tp[0], tR[0], idx, wts, live=True)
    # ... and with terms alone it is Gaps(0, 1.0)
    a.set_initial_state(c.z0, np.zeros((S, 3), np.float32), c.rot0, c.heights0)
    b.set_initial_state(c.z0, np.zeros((S, 3), np.float32), c.rot0, c.heights0)
    k = {x: v for x, v in kw.items() if x not in ("holds", "ar", "gaps")}
    pa, ga = a.run(tp[0], tR[0], idx, wts, live=True, terms=_table(c).frames(0, 1), **k)
    pb, gb = b.run(tp[0], tR[0], idx, wts, gaps=Gaps(0, 1.0), terms=_table(c).frames(0, 1), **k)
    assert _bits(pa, pb) and _bits(ga, gb) and _bits(a.latent_buffer, b.latent_buffer)

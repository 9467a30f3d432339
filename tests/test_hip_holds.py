"""GPU: dp_optimize_sequence_holds (include/dragposer_holds.h) -- dp_optimize_sequence_terms with joints held where they touched down --
against the per-frame composition the header names: optimize_terms with the held term's per_frame = the [S,4] state rows, then
sequence_advance, then the latent copy, then the header's update with torch fp32 ops on `pos` and the advanced global position.  The same
arithmetic in the same order: every comparison is bit for bit (NaN where NaN); no tolerance is involved."""
import functools
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from test_hip_sequence_constraints import HJ, LOOPS, OUT_KEYS, ST, STATE_KEYS, _assert_same, _clip, _opt, _row, _same, _state

pytestmark = pytest.mark.gpu

J_HELD = (4, 8)        # the held joints
HELD_TERMS = (1, 4)    # their terms' places in _table(): not first, beside a PLANE, a joint-to-joint DISTANCE and a [T,S,4] per-frame term
# contact_lo / contact_hi of the ragged case: quantiles of the heights the clip reaches with the two terms off.  (40 % / 70 %, the first choice,
# gives 13 touch-downs and no release in the fixed-count loop: most sequences of this clip move one way only.  45 % / 55 % releases on both holds
# in both loops.)
QUANTILES = (0.45, 0.55)
ADJ = (0, 13, 0.5)


def _table(c, weights=(0.8, 0.6)):
    from dragposer_amd.terms import Term, Terms

    return Terms([Term.plane(4, (0.0, 1.0, 0.0), point=(0.0, -0.9, 0.0), weight=0.5, one_sided=True),
                  Term.distance(J_HELD[0], point=(0.0, 0.0, 0.0), lo=0.0, hi=0.0, weight=weights[0], drop_up=True),
                  Term.distance(3, 7, lo=0.1, hi=0.3, weight=2.0, drop_up=True),
                  Term.distance(8, point=(0.1, 0.0, 0.2), lo=0.0, hi=0.5, weight=0.5, per_frame=c.rows),
                  Term.distance(J_HELD[1], point=(0.0, 0.0, 0.0), lo=0.0, hi=0.02, weight=weights[1])])


def _holds(lo=(0.0, 0.0), hi=(0.1, 0.1), level=(0.0, 0.0)):
    from dragposer_amd import Hold, Holds

    return Holds([Hold(HELD_TERMS[i], float(lo[i]), float(hi[i]), level=float(level[i])) for i in range(2)])


def _update(terms, holds, state, pos, gpos):
    """the header's update, in its operations and order, on [S, n, 4] `state` in place"""
    up = terms.up_axis
    for i, h in enumerate(holds.holds):
        t = terms.terms[h.term]
        if t.weight == 0.0:
            continue  # inert
        W = gpos + (pos[:, t.joint_a] - pos[:, 0])
        hgt = W[:, up] - torch.tensor(h.level, dtype=torch.float32, device=W.device)
        lo, hi = (torch.tensor(x, dtype=torch.float32, device=W.device) for x in (h.contact_lo, h.contact_hi))
        for s in range(state.shape[0]):  # (the comparison forms as written: a NaN height or a NaN `held` takes the branch the header's text takes)
            if float(state[s, i, 3]) == 0.0:
                if bool(hgt[s] <= lo):
                    state[s, i, :3] = W[s]
                    state[s, i, 3] = 1.0
            elif bool(hgt[s] > hi):
                state[s, i, 3] = 0.0


def _per_frame(c, terms, holds, loop, use_root, adjust, hstate, offsets=None, tgt_pos=None, st=None, t0=0, T=None):
    """the composition, frame by frame on the host -> (outputs with `trace`, the state, the hold state)"""
    from dragposer_amd.terms import Terms

    opt, S, T = _opt(), c.S, T or c.T
    st = st or _state(c)
    hstate = hstate.clone()
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    fr = opt.allocate_outputs(S, ("z", "z_pre", "pose", "disp", "world_disp", "world_rot", "pos", "loss", "iters", "status"))
    fr["loss_terms"] = torch.empty(S, len(terms), device=opt.device)
    o = {k: [] for k in OUT_KEYS + ("trace",)}
    for t in range(t0, t0 + T):
        tp = (tgt_pos[t] + (c.root[t] - st.gpos).unsqueeze(1)).contiguous() if use_root else tgt_pos[t]
        rows = [_row(x) for x in terms.frames(t, t + 1).terms]
        for i, h in enumerate(holds.holds):
            if rows[h.term].weight != 0.0:
                rows[h.term] = replace(rows[h.term], per_frame=hstate[:, i].contiguous())
        opt.optimize_terms(st.latent, c.z_tgt[t], st.grot, tp, c.tgt_rot[t], c.w, c.tracked, Terms(rows, terms.up_axis), global_pos=st.gpos, lr=1e-2,
                           lambda_rot=1.0, lambda_tmp=0.02, out=fr, outputs=tuple(fr), offsets=offsets, **loop)
        pose, pos = torch.empty(S, 88, device=opt.device), torch.empty(S, 3, device=opt.device)
        opt.sequence_advance(fr, st.gpos, st.grot, st.lbuf, st.dbuf, st.hbuf, HJ, pose_ret=pose, pos_ret=pos, adjust=adjust,
                             tgt_pos=tp if adjust is not None else None)
        st.latent.copy_(fr["z"])
        _update(terms, holds, hstate, fr["pos"], st.gpos)
        for k, v in (("pose_ret", pose), ("pos_ret", pos), ("iters", fr["iters"]), ("status", fr["status"]), ("loss", fr["loss"]),
                     ("terms", fr["loss_terms"]), ("joint_pos", fr["pos"]), ("trace", hstate)):
            o[k].append(v.clone())
    return {k: torch.stack(v) for k, v in o.items()}, st, hstate


def _launch(c, terms, holds, loop, use_root, adjust, hstate, offsets=None, tgt_pos=None, st=None, t0=0, T=None):
    """one launch over frames t0 .. t0 + T -> (outputs with `trace`, the state, the hold state); holds=None: dp_optimize_sequence_terms"""
    opt, T = _opt(), T or c.T
    st = st or _state(c)
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    sl = slice(t0, t0 + T)
    kw = {}
    if holds is not None:
        hstate = hstate.clone()
        kw = dict(holds=holds, hold_state=hstate, hold_trace=True)
    o = opt.optimize_sequence(st.latent, tgt_pos[sl], c.tgt_rot[sl], c.root[sl] if use_root else None, c.w, c.tracked, c.z_tgt[sl], (c.S * 24, 24),
                              st.gpos, st.grot, st.lbuf, st.dbuf, st.hbuf, HJ, lr=1e-2, lambda_rot=1.0, lambda_tmp=0.02, adjust=adjust,
                              offsets=offsets, terms=terms.frames(t0, t0 + T), **kw, **loop)
    o["terms"] = o.pop("loss_terms")
    if holds is not None:
        o["trace"] = o.pop("hold_trace")
    return o, st, hstate


def _zeros(c, n=2):
    return torch.zeros(c.S, n, 4, device=c.z0.device)


def _row4(c, *vals):
    return torch.tensor(vals, dtype=torch.float32, device=c.z0.device)


def _heights(o, j):
    """[T,S] world height of joint j after every step, from a launch's outputs (level 0)"""
    return (o["pos_ret"] + (o["joint_pos"][:, :, j] - o["joint_pos"][:, :, 0]))[..., 1]


@functools.lru_cache(maxsize=None)
def _thresholds():
    """contact_lo / contact_hi per hold: QUANTILES of the heights the two joints reach in the ragged clip with their terms at weight 0"""
    c = _clip(11, 20)
    off, _, _ = _launch(c, _table(c, (0.0, 0.0)), None, LOOPS["it15"], True, ADJ, None)
    torch.cuda.synchronize()
    q = [torch.quantile(_heights(off, j).flatten(), torch.tensor(QUANTILES, device=off["pos_ret"].device)).tolist() for j in J_HELD]
    return tuple(x[0] for x in q), tuple(x[1] for x in q)


ALL_KEYS = OUT_KEYS + ("trace",)


@pytest.mark.parametrize("loop", ["it15", "early"])
def test_one_launch_equals_the_composition_at_the_ragged_shape(loop):
    """S = 11 (a workgroup of 8 waves and one of 3), T = 20, target_root and joint adjustment: every output, the whole state, the hold
    state and every row of the trace; and on the oracle's own trace the clip touches down, releases, and a held term is in the loss"""
    c = _clip(11, 20)
    lo, hi = _thresholds()
    terms, holds = _table(c), _holds(lo, hi)
    exp, est, eh = _per_frame(c, terms, holds, LOOPS[loop], True, ADJ, _zeros(c))
    got, gst, gh = _launch(c, terms, holds, LOOPS[loop], True, ADJ, _zeros(c))
    torch.cuda.synchronize()
    _assert_same(got, exp, ALL_KEYS, loop)
    _assert_same(gst, est, STATE_KEYS, loop)
    assert _same(gh, eh) and _same(gh, exp["trace"][-1])
    assert int(exp["status"].max()) == 0 and bool(torch.isfinite(exp["pose_ret"]).all())
    held = torch.cat((torch.zeros_like(exp["trace"][:1, ..., 3]), exp["trace"][..., 3]))  # [T+1,S,2]: before step 0, after every step
    downs, ups = int(((held[1:] == 1) & (held[:-1] == 0)).sum()), int(((held[1:] == 0) & (held[:-1] == 1)).sum())
    print(f"{loop}: contact_lo {lo} contact_hi {hi}: {downs} touch-downs, {ups} releases, held after the clip {held[-1].sum(0).tolist()}")
    assert downs >= 1 and ups >= 1
    assert bool((exp["terms"][..., list(HELD_TERMS)] != 0).any())  # a held term is in the loss
    if loop == "early":
        assert int(exp["iters"].min()) < int(exp["iters"].max())


def test_forced_and_never():
    """level = +10: every sequence latches at step 0 and never releases, the point stays W of step 0; level = -10: never latches, and the
    launch is dp_optimize_sequence_terms with the two terms fed [S,4] rows of s = 0"""
    c = _clip(11, 20)
    terms, loop = _table(c), LOOPS["early"]
    got, gst, gh = _launch(c, terms, _holds(level=(10.0, 10.0)), loop, True, ADJ, _zeros(c))
    torch.cuda.synchronize()
    tr = got["trace"]
    assert bool((tr[..., 3] == 1).all())
    for i, j in enumerate(J_HELD):
        W0 = got["pos_ret"][0] + (got["joint_pos"][0, :, j] - got["joint_pos"][0, :, 0])
        assert torch.equal(tr[0, :, i, :3], W0)
        assert torch.equal(tr[:, :, i, :3], W0[None].expand(c.T, -1, -1))
    assert torch.equal(gh, tr[-1])
    assert bool((got["terms"][0][:, list(HELD_TERMS)] == 0).all()) and bool((got["terms"][1:][..., list(HELD_TERMS)] != 0).any())
    # never
    got, gst, gh = _launch(c, terms, _holds(level=(-10.0, -10.0)), loop, True, ADJ, _zeros(c))
    off = torch.zeros(c.S, 4, device=c.z0.device)
    rows = list(terms.terms)
    for k in HELD_TERMS:
        rows[k] = replace(rows[k], per_frame=off)
    ref, rst, _ = _launch(c, type(terms)(rows, terms.up_axis), None, loop, True, ADJ, None)
    torch.cuda.synchronize()
    _assert_same(got, ref, OUT_KEYS, "never")
    _assert_same(gst, rst, STATE_KEYS, "never")
    assert not gh.any() and not got["trace"].any()


def test_stretches_chain_through_the_state():
    """T = 20 as one launch = two launches of 10 with the hold state (and the sequence state) carried, on everything"""
    c = _clip(11, 20)
    lo, hi = _thresholds()
    terms, holds, loop = _table(c), _holds(lo, hi), LOOPS["early"]
    one, ost, oh = _launch(c, terms, holds, loop, True, ADJ, _zeros(c))
    a, st, h = _launch(c, terms, holds, loop, True, ADJ, _zeros(c), T=10)
    b, st, h = _launch(c, terms, holds, loop, True, ADJ, h, st=st, t0=10, T=10)
    torch.cuda.synchronize()
    _assert_same({k: torch.cat((a[k], b[k])) for k in ALL_KEYS}, one, ALL_KEYS, "chain")
    _assert_same(st, ost, STATE_KEYS, "chain")
    assert _same(h, oh)
    assert bool((a["trace"][-1, ..., 3] == 1).any())  # something was held across the cut


@pytest.mark.parametrize("S,T", [(1, 1), (9, 6)])
def test_small_shapes(S, T):
    """one sequence of one step, and a workgroup of 8 waves with one of 1: a state that enters held, so that the term is on from step 0"""
    c = _clip(S, T, seed=33)
    terms, holds = _table(c), _holds((0.0, -0.2), (0.1, 0.3))
    h0 = _zeros(c)
    h0[:, 0] = _row4(c, 0.05, -0.1, 0.02, 1.0)
    h0[::2, 1] = _row4(c, -0.03, 0.2, 0.04, 0.5)  # (any held >= 0 scales the weight)
    exp, est, eh = _per_frame(c, terms, holds, LOOPS["it15"], True, ADJ, h0)
    got, gst, gh = _launch(c, terms, holds, LOOPS["it15"], True, ADJ, h0)
    torch.cuda.synchronize()
    _assert_same(got, exp, ALL_KEYS, (S, T))
    _assert_same(gst, est, STATE_KEYS, (S, T))
    assert _same(gh, eh)
    assert bool((exp["terms"][0][:, HELD_TERMS[0]] != 0).all())


def test_mixed_skeletons():
    """offsets [S,22,3], four skeletons over 11 sequences, against the per-frame calls with offsets="""
    c, opt = _clip(11, 20), _opt()
    own = torch.from_numpy(opt.host_model.arrays["offsets"]).to(opt.device).reshape(22, 3).contiguous()
    scale = torch.tensor([1.0, 0.9, 1.1, 1.05], device=opt.device)[torch.arange(c.S) % 4]
    mixed = (own[None] * scale[:, None, None]).contiguous()
    lo, hi = _thresholds()
    terms, holds = _table(c), _holds(lo, hi)
    exp, est, eh = _per_frame(c, terms, holds, LOOPS["it15"], True, ADJ, _zeros(c), offsets=mixed, T=10)
    got, gst, gh = _launch(c, terms, holds, LOOPS["it15"], True, ADJ, _zeros(c), offsets=mixed, T=10)
    plain, _, _ = _launch(c, terms, holds, LOOPS["it15"], True, ADJ, _zeros(c), T=10)
    torch.cuda.synchronize()
    _assert_same(got, exp, ALL_KEYS, "mixed")
    _assert_same(gst, est, STATE_KEYS, "mixed")
    assert _same(gh, eh)
    assert not torch.equal(got["pose_ret"][:, 1::4], plain["pose_ret"][:, 1::4])


def test_a_bad_state_row_is_screened_and_stays_with_its_sequence():
    """a NaN in sequence 5's row of hold 0: BAD_TARGETS at step 0 there, the bad-state fill from step 1 on, its hold state as it was; the
    ten others as in the clean launch"""
    c = _clip(11, 20)
    bad, T = 5, 6
    terms, holds, loop = _table(c), _holds(level=(10.0, 10.0)), LOOPS["early"]  # (level +10: the comparison never releases a held row)
    h0 = _zeros(c)
    h0[bad, 0] = _row4(c, float("nan"), 0.1, 0.2, 1.0)
    clean, cst, ch = _launch(c, terms, holds, loop, True, ADJ, _zeros(c), T=T)
    got, gst, gh = _launch(c, terms, holds, loop, True, ADJ, h0, T=T)
    exp, est, eh = _per_frame(c, terms, holds, loop, True, ADJ, h0, T=T)
    torch.cuda.synchronize()
    _assert_same(got, exp, ALL_KEYS, "bad row")
    _assert_same(gst, est, STATE_KEYS, "bad row")
    assert _same(gh, eh)
    assert int(got["status"][0, bad]) == ST.NONFINITE | ST.BAD_TARGETS and int(got["iters"][0, bad]) == 1
    assert bool((got["status"][1:, bad] == (ST.NONFINITE | ST.BAD_STATE)).all())
    for k in ("pose_ret", "pos_ret", "loss", "terms", "joint_pos"):
        assert bool(got[k][1:, bad].isnan().all()), k
    assert _same(gh[bad, 0], h0[bad, 0]) and _same(got["trace"][:, bad, 0], h0[bad, 0][None].expand(T, -1))
    others = [s for s in range(c.S) if s != bad]
    for k in ALL_KEYS:
        assert torch.equal(got[k][:, others], clean[k][:, others]), k
    for k in STATE_KEYS:
        assert torch.equal(getattr(gst, k)[others], getattr(cst, k)[others]), k
    assert torch.equal(gh[others], ch[others])


def test_a_hold_on_a_weight_zero_term_is_inert():
    """the hold on a term of weight 0 neither reads nor writes its state: whatever is there stays, and the launch equals one without it"""
    from dragposer_amd import Holds

    c = _clip(11, 20)
    lo, hi = _thresholds()
    terms, both, loop, T = _table(c, (0.0, 0.6)), _holds(lo, hi), LOOPS["early"], 10
    h0 = _zeros(c)
    h0[:, 0] = _row4(c, float("nan"), -1.0e9, float("inf"), -3.0)
    got, gst, gh = _launch(c, terms, both, loop, True, ADJ, h0, T=T)
    ref, rst, rh = _launch(c, terms, Holds(both.holds[1:]), loop, True, ADJ, _zeros(c, 1), T=T)
    torch.cuda.synchronize()
    _assert_same(got, ref, OUT_KEYS, "inert")
    _assert_same(gst, rst, STATE_KEYS, "inert")
    assert _same(gh[:, 0], h0[:, 0]) and _same(gh[:, 1], rh[:, 0]) and _same(got["trace"][:, :, 1], ref["trace"][:, :, 0])
    assert int(got["status"].max()) == 0


def test_run_frames_equals_the_loop_of_run_across_a_prediction():
    """a seeded predictor, window 8, native temporal, T = 20: run_frames(terms=, holds=) cuts 8 / 8 / 4 and equals per-frame
    run(terms=, holds=) on poses, positions, counts and the hold state"""
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.temporal import TemporalPredictor

    c = _clip(11, 20)
    lo, hi = _thresholds()
    terms = _table(c)
    terms = type(terms)([t for t in terms.terms if t.per_frame is None], terms.up_axis)  # (run() takes [S,4] rows only)
    from dragposer_amd import Hold, Holds
    holds = Holds([Hold(1, lo[0], hi[0]), Hold(3, 0.0, 0.1, level=10.0)])
    torch.manual_seed(5)
    predictor = TemporalPredictor(n_encoder_layers=1, n_decoder_layers=1, dim_feedforward=16)
    idx = np.array(R.TRACK6)
    wts = np.array([R.W6[j] for j in R.TRACK6], np.float32)
    kw = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2, max_iter=30, min_loss_incr=1e-5, learning_rate=1e-2, lambda_rot=1, lambda_temporal=0.02,
              temporal_future_window=8, height_indices=HJ, joint_adjustment_indices=(0, 3), joint_adjustment_weight=0.5, terms=terms, holds=holds)
    dps = []
    for _ in range(2):
        dp = DragPose(_opt(), predictor, np.zeros(24), np.ones(24), n_sequences=c.S, native_temporal=True)
        dp.set_initial_state(c.z0, np.zeros((c.S, 3), np.float32), c.rot0, c.heights0)
        assert dp.hold_state is None
        dps.append(dp)
    a, b = dps
    tp, tR = c.tgt_pos[:, :, idx], c.tgt_rot[:, :, idx].reshape(c.T, c.S, -1, 3, 3)
    pa, ga, ia, ha = [], [], [], []
    for t in range(c.T):
        pose, gpos = a.run(tp[t], tR[t], idx, wts, **kw)
        pa.append(pose.clone()); ga.append(gpos.clone()); ia.append(a.last["iters"].clone()); ha.append(a.hold_state.clone())
    calls = []
    seq = b.opt.optimize_sequence
    b.opt.optimize_sequence = lambda *x, **k: (calls.append(int(x[1].shape[0])), seq(*x, **k))[1]
    try:
        pb, gb, ib = b.run_frames(tp, tR, idx, wts, **kw)
    finally:
        del b.opt.optimize_sequence
    torch.cuda.synchronize()
    assert calls == [8, 8, 4]
    assert torch.equal(torch.stack(pa), pb) and torch.equal(torch.stack(ga), gb) and torch.equal(torch.stack(ia), ib)
    assert torch.equal(a.hold_state, b.hold_state) and torch.equal(torch.stack(ha), b.last_hold_trace)
    assert bool((b.hold_state[:, 1, 3] == 1).all()) and bool(b.hold_state[:, 1, :3].any())
    for attr in ("latent", "current_global_pos", "current_global_rot", "latent_buffer", "displacement_buffer", "heights_buffer", "target_latent_buffer"):
        assert torch.equal(getattr(a, attr), getattr(b, attr)), attr
    b.set_initial_state(c.z0, np.zeros((c.S, 3), np.float32), c.rot0, c.heights0)
    assert b.hold_state is None  # a new sequence begins with nothing held


def test_eval_drag_cli_with_foot_lock(tmp_path, capsys):
    """eval_drag --foot-lock on the 4-tracker configuration: runs, writes the BVH, prints the skate line after the reference's four; the
    frame loop on the device and --per-frame write the same bytes"""
    from dragposer_amd import eval_drag

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    argv = [os.path.join(root, "tests", "data", "example_clip.bvh"), "--config", os.path.join(root, "dragposer_amd", "config", "4_trackers_config.json"),
            "--max-frames", "48", "--foot-lock", "--up-axis", "2", "--floor-level", "-1.0", "--contact-height", "0.3", "0.5", "--keep-frames"]
    for d in ("device", "host", "plain"):
        os.makedirs(tmp_path / d)
    a = eval_drag.main(argv + ["--out-dir", str(tmp_path / "device")])[0]
    text = capsys.readouterr().out
    lines = [ln.split(":")[0] for ln in text.splitlines() if ":" in ln]
    i = lines.index("Evaluate Loss")
    assert lines[i:i + 4] == ["Evaluate Loss", "Mean Per Joint Position Error", "Mean End Effector Position Error", "Time"]
    assert lines[i + 4:].count("Foot skate") == 1
    b = eval_drag.main(argv + ["--out-dir", str(tmp_path / "host"), "--per-frame"])[0]
    assert a["frames"] == b["frames"] == 48 and os.path.getsize(a["out"]) > 0
    assert open(a["out"], "rb").read() == open(b["out"], "rb").read()
    assert repr(a["foot_skate"]) == repr(b["foot_skate"]) and a["contact_frames"] == b["contact_frames"]
    plain = eval_drag.main([x for x in argv if x != "--foot-lock"] + ["--out-dir", str(tmp_path / "plain")])[0]
    assert "foot_skate" not in plain and not np.array_equal(a["poses"], plain["poses"])  # the switch is not a no-op

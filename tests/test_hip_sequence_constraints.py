"""GPU: dp_optimize_sequence_constrained / dp_optimize_sequence_terms (include/dragposer_sequence_constraints.h) -- a clip with the
reference's extra loss terms or a term table, the frame loop inside one launch -- against the per-frame path built from calls that are
themselves pinned to the reference (tests/test_hip_constraints.py, test_hip_terms.py, test_hip_constraints_skeleton.py,
test_hip_sequences.py): optimize_constrained / optimize_terms + sequence_advance + a copy of the latent, frame by frame, which is what
DragPose.run(constraints=...) does.  The same arithmetic in the same order: every comparison is bit for bit (NaN where NaN)."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from oracle import ref_torch as R

pytestmark = pytest.mark.gpu

HJ = (0, 4, 8, 13, 17, 21)
H = 60  # the reference's history depth
ST = types.SimpleNamespace(NONFINITE=1, BAD_STATE=2, BAD_TARGETS=4)
# the loop's settings: a fixed count (thresholds that never end the loop; the while-condition still runs, as a sequence launch implies),
# one pass, and the reference's early stop (eval_drag.py:204-222)
LOOPS = {"it15": dict(n_iter=15, stop_eps_pos=0.0, stop_eps_rot=0.0, min_loss_incr=-1e30),
         "it1": dict(n_iter=1, stop_eps_pos=0.0, stop_eps_rot=0.0, min_loss_incr=-1e30),
         "early": dict(n_iter=100, stop_eps_pos=0.01 * 0.01, stop_eps_rot=0.01, min_loss_incr=0.00001)}


@functools.lru_cache(maxsize=None)
def _clip(S, T, seed=31):
    """S sequences of T frames that can be tracked: the targets are decode + FK of a slowly drifting latent under the rotation the frames
    before left, the root trajectory is the sum of their world displacements plus a little noise.  Built once per shape, on the CPU."""
    m = R.OracleModel()
    g = torch.Generator(device="cpu").manual_seed(seed)
    base, drift = torch.randn(S, 24, generator=g) * 0.3, torch.randn(S, 24, generator=g) * 0.02
    cr = torch.randn(S, 4, generator=g)
    cr = cr / torch.linalg.norm(cr, dim=-1, keepdim=True)
    rot0, pos, rot, root = cr.clone(), [], [], []
    gp = torch.zeros(S, 3)
    with torch.no_grad():
        for t in range(T):
            motion, disp = R.decoder_forward(m, base + t * drift)
            wd, wr, p, r, _ = R.pose_fk(m, motion, disp, cr)
            pos.append(p.float()); rot.append(r.reshape(S, 22, 9).float()); root.append(gp.clone())
            gp, cr = gp + wd.float(), wr.float()
    tracked = torch.zeros(S, 22, dtype=torch.uint8)
    w = torch.zeros(S, 22, 2)
    for j, wj in R.W6.items():
        tracked[:, j] = 1
        w[:, j] = torch.tensor(wj)
    trk = tracked.bool()[None, :, :, None]
    dev = torch.device("cuda:0")
    c = types.SimpleNamespace(S=S, T=T)
    c.tgt_pos = (torch.stack(pos) * trk).contiguous().to(dev)  # [T,S,22,3], relative to the root before the frame
    c.tgt_rot = (torch.stack(rot) * trk).contiguous().to(dev)
    c.root = (torch.stack(root) + 0.002 * torch.randn(T, S, 3, generator=g)).contiguous().to(dev)
    c.w, c.tracked = w.to(dev), tracked.to(dev)
    c.z0 = (base + 0.05 * torch.randn(S, 24, generator=g)).to(dev)
    c.z_tgt = (base[None] + torch.arange(T)[:, None, None] * drift[None] + 0.02 * torch.randn(T, S, 24, generator=g)).contiguous().to(dev)
    c.rot0 = rot0.to(dev)
    c.heights0 = torch.rand(S, len(HJ), generator=g).to(dev)
    c.rows = torch.rand(T, S, 4, generator=g)  # per-step rows of a term: a point near the origin, s in [0.5, 1.5)
    c.rows[..., :3] = 0.3 * (c.rows[..., :3] - 0.5)
    c.rows[..., 3] += 0.5
    c.rows = c.rows.contiguous().to(dev)
    c.held = torch.tensor([0.0, 1.0, 0.0, 0.7]).repeat(S, 1).contiguous().to(dev)  # one row per sequence: the floor's normal, s = 0.7
    return c


@functools.lru_cache(maxsize=None)
def _opt():
    from dragposer_amd.optimizer import LatentOptimizer

    return LatentOptimizer(device="cuda:0")


def _extras(c, kind):
    """the four-term block, or a 5-term table with one held and one per-step per_frame (rows [T,S,4]: the per-frame side reads rows[t])"""
    from dragposer_amd import Constraints
    from dragposer_amd.terms import Term, Terms

    if kind == "cons":
        return Constraints.reference(floor_level=-0.9)
    if kind == "empty":  # the plain tracker loss
        return Terms()
    if kind == "nogp":  # no PLANE and no point-DISTANCE term: nothing reads the global position, and the library is not given it
        return Terms([Term.distance(3, 7, lo=0.1, hi=0.3, weight=2.0, drop_up=True),
                      Term.align(13, (0.0, 0.0, 1.0), 0, (0.0, 0.0, 1.0), threshold=0.5, margin=0.2, weight=1.0, drop_up=True)])
    return Terms([Term.plane(4, (0.0, 1.0, 0.0), point=(0.0, -0.9, 0.0), weight=0.5, one_sided=True),
                  Term.distance(3, 7, lo=0.1, hi=0.3, weight=2.0, drop_up=True),
                  Term.distance(8, point=(0.1, 0.0, 0.2), lo=0.0, hi=0.5, weight=0.5, per_frame=c.rows),
                  Term.align(13, (0.0, 0.0, 1.0), 0, (0.0, 0.0, 1.0), threshold=0.5, margin=0.2, weight=1.0, drop_up=True),
                  Term.plane(8, (0.0, 1.0, 0.0), point=(0.0, -0.9, 0.0), weight=0.5, per_frame=c.held)])


def _state(c, sl=slice(None)):
    z0 = c.z0[sl].clone()
    return types.SimpleNamespace(latent=z0, gpos=torch.zeros_like(c.root[0][sl]), grot=c.rot0[sl].clone(), lbuf=z0.unsqueeze(1).repeat(1, H, 1),
                                 dbuf=torch.zeros(z0.shape[0], H, 3, device=z0.device), hbuf=c.heights0[sl].unsqueeze(1).repeat(1, H, 1).contiguous())


OUT_KEYS = ("pose_ret", "pos_ret", "iters", "status", "loss", "terms", "joint_pos")
STATE_KEYS = ("latent", "gpos", "grot", "lbuf", "dbuf", "hbuf")


def _per_frame(c, kind, loop, use_root, adjust, offsets=None, tgt_pos=None, st=None, T=None):
    """the frame loop on the host, from calls that exist without the sequence form (DragPose._run_constrained's two launches and copy)"""
    from dragposer_amd.terms import Terms

    opt, S, T = _opt(), c.S, T or c.T
    ext, st = _extras(c, kind), st or _state(c)
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    key, width = ("loss_extra", 4) if kind == "cons" else ("loss_terms", len(ext))
    fr = opt.allocate_outputs(S, ("z", "z_pre", "pose", "disp", "world_disp", "world_rot", "pos", "loss", "iters", "status"))
    fr[key] = torch.empty(S, width, device=opt.device)
    o = {k: [] for k in OUT_KEYS}
    for t in range(T):
        tp = (tgt_pos[t] + (c.root[t] - st.gpos).unsqueeze(1)).contiguous() if use_root else tgt_pos[t]  # eval_drag.py:186-199
        e = ext if kind == "cons" else Terms([_row(x) for x in ext.frames(t, t + 1).terms], ext.up_axis)
        run = opt.optimize_constrained if kind == "cons" else opt.optimize_terms
        run(st.latent, c.z_tgt[t], st.grot, tp, c.tgt_rot[t], c.w, c.tracked, e, global_pos=st.gpos, lr=1e-2, lambda_rot=1.0, lambda_tmp=0.02,
            out=fr, outputs=tuple(fr), offsets=offsets, **loop)
        pose, pos = torch.empty(S, 88, device=opt.device), torch.empty(S, 3, device=opt.device)
        opt.sequence_advance(fr, st.gpos, st.grot, st.lbuf, st.dbuf, st.hbuf, HJ, pose_ret=pose, pos_ret=pos, adjust=adjust,
                             tgt_pos=tp if adjust is not None else None)
        st.latent.copy_(fr["z"])
        for k, v in (("pose_ret", pose), ("pos_ret", pos), ("iters", fr["iters"]), ("status", fr["status"]), ("loss", fr["loss"]), ("terms", fr[key]),
                     ("joint_pos", fr["pos"])):
            o[k].append(v.clone())
    return {k: torch.stack(v) for k, v in o.items()}, st


def _row(term):
    """a term of one frame's table: its [1,S,4] slice of per-step rows as the [S,4] the per-frame call takes"""
    from dataclasses import replace

    return replace(term, per_frame=term.per_frame[0]) if term.per_frame is not None and term.per_frame.dim() == 3 else term


def _launch(c, kind, loop, use_root, adjust, offsets=None, tgt_pos=None, st=None, T=None):
    opt, T = _opt(), T or c.T
    ext, st = _extras(c, kind), st or _state(c)
    if kind != "cons":
        ext = ext.frames(0, T)
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    o = opt.optimize_sequence(st.latent, tgt_pos[:T], c.tgt_rot[:T], c.root[:T] if use_root else None, c.w, c.tracked, c.z_tgt[:T], (c.S * 24, 24),
                              st.gpos, st.grot, st.lbuf, st.dbuf, st.hbuf, HJ, lr=1e-2, lambda_rot=1.0, lambda_tmp=0.02, adjust=adjust,
                              offsets=offsets, **{"constraints" if kind == "cons" else "terms": ext}, **loop)
    o["terms"] = o.pop("loss_extra" if kind == "cons" else "loss_terms")
    return o, st


def _same(a, b):
    """bit for bit; a NaN equals a NaN (the refused frames' results)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_floating_point():
        return bool(((a == b) | (a.isnan() & b.isnan())).all())
    return torch.equal(a, b)


def _assert_same(got, exp, keys, what=""):
    for k in keys:
        a, b = (got[k], exp[k]) if isinstance(got, dict) else (getattr(got, k), getattr(exp, k))
        assert _same(a, b), (what, k, (a != b).nonzero()[:4].tolist())


CASES = [("it15", True, (0, 13, 0.5)), ("it1", False, (0, 13, 0.5)), ("early", True, None)]  # loop, target_root given, joint adjustment


@pytest.mark.parametrize("kind", ["cons", "terms"])
@pytest.mark.parametrize("loop,use_root,adjust", CASES)
def test_one_launch_equals_the_per_frame_path_at_the_ragged_shape(kind, loop, use_root, adjust):
    """S = 11 (a workgroup of 8 waves and one of 3), T = 20: poses, global positions, iteration counts, status, losses, the terms and
    joint positions of every step, and the whole state afterwards"""
    c = _clip(11, 20)
    exp, est = _per_frame(c, kind, LOOPS[loop], use_root, adjust)
    got, gst = _launch(c, kind, LOOPS[loop], use_root, adjust)
    torch.cuda.synchronize()
    _assert_same(got, exp, OUT_KEYS, (kind, loop))
    _assert_same(gst, est, STATE_KEYS, (kind, loop))
    assert int(exp["status"].max()) == 0 and bool(torch.isfinite(exp["pose_ret"]).all())
    it = exp["iters"]
    if loop == "early":  # the while-condition decides: not one count for all frames
        assert int(it.min()) >= 1 and int(it.max()) <= 100 and int(it.min()) < int(it.max())
    else:
        assert bool((it == LOOPS[loop]["n_iter"]).all())
    assert bool((exp["terms"] != 0).any())  # the terms are in the loss


@pytest.mark.parametrize("kind", ["nogp", "empty"])
def test_a_table_that_reads_no_global_position(kind):
    """a joint-DISTANCE and an ALIGN term, and the empty table: no term needs the global position, so dp_terms carries none; the launch
    still carries the state's own from step to step (target_root and joint adjustment use it) and equals the per-frame path"""
    c = _clip(11, 20)
    assert not _extras(c, kind).needs_global_pos
    loop, adjust = LOOPS["early"], (0, 13, 0.5)
    exp, est = _per_frame(c, kind, loop, True, adjust)
    got, gst = _launch(c, kind, loop, True, adjust)
    torch.cuda.synchronize()
    _assert_same(got, exp, OUT_KEYS, kind)
    _assert_same(gst, est, STATE_KEYS, kind)
    assert int(exp["status"].max()) == 0 and bool(torch.isfinite(exp["pos_ret"]).all())
    assert tuple(got["terms"].shape) == (c.T, c.S, len(_extras(c, kind)))
    assert not torch.equal(gst.gpos, torch.zeros_like(gst.gpos))  # the position moved, and was carried


@pytest.mark.parametrize("kind", ["cons", "terms"])
def test_single_step_equals_dragpose_run(kind):
    """a T = 1 launch (DragPose.run_frames over one frame) is DragPose.run(constraints= / terms=) of that frame"""
    from dragposer_amd.drag_pose import DragPose

    c = _clip(11, 20)
    ext = _extras(c, kind)
    if kind != "cons":
        ext = type(ext)([_row(x) for x in ext.frames(0, 1).terms], ext.up_axis)  # ([S,4] rows: what run() takes)
    idx = np.array(R.TRACK6)
    wts = np.array([R.W6[j] for j in R.TRACK6], np.float32)
    kw = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2, max_iter=30, min_loss_incr=1e-5, learning_rate=1e-2, lambda_rot=1, lambda_temporal=0.0,
              temporal_future_window=0, height_indices=HJ, joint_adjustment_indices=(0, 3), joint_adjustment_weight=0.5,
              **{"constraints" if kind == "cons" else "terms": ext})
    dps = []
    for _ in range(2):
        dp = DragPose(_opt(), None, np.zeros(24), np.ones(24), n_sequences=c.S)
        dp.set_initial_state(c.z0, np.zeros((c.S, 3), np.float32), c.rot0, c.heights0)
        dps.append(dp)
    a, b = dps
    tp, tR = c.tgt_pos[0][:, idx], c.tgt_rot[0][:, idx].reshape(c.S, -1, 3, 3)
    pa, ga = a.run(tp, tR, idx, wts, **kw)
    pb, gb, ib = b.run_frames(tp.unsqueeze(0), tR.unsqueeze(0), idx, wts, **kw)
    torch.cuda.synchronize()
    assert torch.equal(pa, pb[0]) and torch.equal(ga, gb[0]) and torch.equal(a.last["iters"], ib[0]) and torch.equal(a.last["status"], b.last_status[0])
    assert torch.equal(a.last["loss_extra" if kind == "cons" else "loss_terms"], b.last_terms[0])
    for attr in ("latent", "current_global_pos", "current_global_rot", "latent_buffer", "displacement_buffer", "heights_buffer"):
        assert torch.equal(getattr(a, attr), getattr(b, attr)), attr


def test_single_sequence_longer_than_the_history():
    """S = 1, T = 70: more steps than the 60-deep history buffers hold"""
    c = _clip(1, 70, seed=32)
    for kind in ("cons", "terms"):
        exp, est = _per_frame(c, kind, LOOPS["early"], True, (0, 13, 0.5))
        got, gst = _launch(c, kind, LOOPS["early"], True, (0, 13, 0.5))
        torch.cuda.synchronize()
        _assert_same(got, exp, OUT_KEYS, kind)
        _assert_same(gst, est, STATE_KEYS, kind)
        assert not torch.equal(gst.lbuf[:, 0], c.z0)  # every initial row has left the buffer


@pytest.mark.parametrize("kind", ["cons", "terms"])
def test_mixed_skeletons(kind):
    """offsets [S,22,3], four skeletons over 11 sequences, against the per-frame calls with offsets=; and the context's own skeleton
    passed as offsets= against the launch without"""
    c, opt = _clip(11, 20), _opt()
    own = torch.from_numpy(opt.host_model.arrays["offsets"]).to(opt.device).reshape(22, 3).contiguous()
    scale = torch.tensor([1.0, 0.9, 1.1, 1.05], device=opt.device)[torch.arange(c.S) % 4]
    mixed = (own[None] * scale[:, None, None]).contiguous()
    loop, adjust = LOOPS["it15"], (0, 13, 0.5)
    exp, est = _per_frame(c, kind, loop, True, adjust, offsets=mixed)
    got, gst = _launch(c, kind, loop, True, adjust, offsets=mixed)
    plain, pst = _launch(c, kind, loop, True, adjust)
    same, sst = _launch(c, kind, loop, True, adjust, offsets=own)
    per_seq, qst = _launch(c, kind, loop, True, adjust, offsets=own[None].repeat(c.S, 1, 1).contiguous())
    torch.cuda.synchronize()
    _assert_same(got, exp, OUT_KEYS, kind)
    _assert_same(gst, est, STATE_KEYS, kind)
    for o, s in ((same, sst), (per_seq, qst)):
        _assert_same(o, plain, OUT_KEYS, kind)
        _assert_same(s, pst, STATE_KEYS, kind)
    assert torch.equal(got["pose_ret"][:, 0::4], plain["pose_ret"][:, 0::4])  # (scale 1.0: the context's bones)
    assert not torch.equal(got["pose_ret"][:, 1::4], plain["pose_ret"][:, 1::4])


def test_stretches_between_temporal_predictions():
    """a seeded predictor, window 8, native temporal, T = 20: run_frames cuts 8 / 8 / 4 and equals per-frame run(constraints=...)"""
    from dragposer_amd import Constraints
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.temporal import TemporalPredictor

    c = _clip(11, 20)
    torch.manual_seed(5)
    predictor = TemporalPredictor(n_encoder_layers=1, n_decoder_layers=1, dim_feedforward=16)
    idx = np.array(R.TRACK6)
    wts = np.array([R.W6[j] for j in R.TRACK6], np.float32)
    kw = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2, max_iter=30, min_loss_incr=1e-5, learning_rate=1e-2, lambda_rot=1, lambda_temporal=0.02,
              temporal_future_window=8, height_indices=HJ, joint_adjustment_indices=(0, 3), joint_adjustment_weight=0.5,
              constraints=Constraints.reference(floor_level=-0.9))
    dps = []
    for _ in range(2):
        dp = DragPose(_opt(), predictor, np.zeros(24), np.ones(24), n_sequences=c.S, native_temporal=True)
        dp.set_initial_state(c.z0, np.zeros((c.S, 3), np.float32), c.rot0, c.heights0)
        dps.append(dp)
    a, b = dps
    tp, tR = c.tgt_pos[:, :, idx], c.tgt_rot[:, :, idx].reshape(c.T, c.S, -1, 3, 3)
    pa, ga, ia = [], [], []
    for t in range(c.T):
        pose, gpos = a.run(tp[t], tR[t], idx, wts, **kw)
        pa.append(pose.clone()); ga.append(gpos.clone()); ia.append(a.last["iters"].clone())
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
    for attr in ("latent", "current_global_pos", "current_global_rot", "latent_buffer", "displacement_buffer", "heights_buffer", "target_latent_buffer"):
        assert torch.equal(getattr(a, attr), getattr(b, attr)), attr
    assert a.current_index == b.current_index == 4


@pytest.mark.parametrize("kind", ["cons", "terms"])
def test_a_bad_target_is_screened_and_stays_with_its_sequence(kind):
    """sequence 5 of 11 gets a NaN position target at step 3: the warm start's pose after one pass there, NaN and BAD_STATE from step 4
    on and in the next launch; the ten others as in the clean run; all of it what the per-frame path gives on the same inputs"""
    c, opt = _clip(11, 20), _opt()
    bad, tb = 5, 3
    tgt = c.tgt_pos.clone()
    tgt[tb, bad, 13, 1] = float("nan")
    loop, adjust = LOOPS["early"], (0, 3, 0.5)
    exp, est = _per_frame(c, kind, loop, True, adjust, tgt_pos=tgt)
    clean, cst = _launch(c, kind, loop, True, adjust)
    got, gst = _launch(c, kind, loop, True, adjust, tgt_pos=tgt)
    torch.cuda.synchronize()
    _assert_same(got, exp, OUT_KEYS, kind)
    _assert_same(gst, est, STATE_KEYS, kind)
    others = [s for s in range(c.S) if s != bad]
    for k in OUT_KEYS:
        assert torch.equal(got[k][:, others], clean[k][:, others]), k
        assert torch.equal(got[k][:tb, bad], clean[k][:tb, bad]), k
    for k in STATE_KEYS:
        assert torch.equal(getattr(gst, k)[others], getattr(cst, k)[others]), k
    assert int(got["status"][tb, bad]) == ST.NONFINITE | ST.BAD_TARGETS and int(got["iters"][tb, bad]) == 1
    assert bool(torch.isfinite(got["pose_ret"][tb, bad]).all()) and bool(got["loss"][tb, bad].isnan().all())
    # the warm start's pose: decode + FK of the latent the step began with (the clean run's latent after step 2, which no call returns:
    # three clean steps from the start give it).  Another kernel's fp32 decode of O(1) channels: 1e-4 is a hundred times its rounding
    st3 = _launch(c, kind, loop, True, adjust, T=tb)[1]
    fwd = opt.forward(st3.latent, st3.grot, outputs=("pose",))["pose"]
    torch.cuda.synchronize()
    assert float((fwd[bad, 4:] - got["pose_ret"][tb, bad, 4:]).abs().max()) < 1e-4
    assert bool((got["status"][tb + 1:, bad] == (ST.NONFINITE | ST.BAD_STATE)).all()) and bool((got["iters"][tb + 1:, bad] == 1).all())
    for k in ("pose_ret", "pos_ret", "loss", "terms", "joint_pos"):
        assert bool(got[k][tb + 1:, bad].isnan().all()), k
    assert bool(gst.latent[bad].isnan().all()) and bool(gst.gpos[bad].isnan().all()) and bool(gst.grot[bad].isnan().all())
    # the next launch on that state, clean targets
    nxt, nst = _launch(c, kind, loop, True, adjust, st=gst, T=4)
    ref, rst = _per_frame(c, kind, loop, True, adjust, st=est, T=4)
    torch.cuda.synchronize()
    _assert_same(nxt, ref, OUT_KEYS, kind)
    _assert_same(nst, rst, STATE_KEYS, kind)
    assert bool((nxt["status"][:, bad] == (ST.NONFINITE | ST.BAD_STATE)).all()) and bool(nxt["pose_ret"][:, bad].isnan().all())
    assert int(nxt["status"][:, others].max()) == 0


def test_eval_drag_cli_with_the_reference_constraints(tmp_path):
    """eval_drag --constraints reference: the frame loop on the device and --per-frame return the same frames"""
    from dragposer_amd import eval_drag

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    argv = [os.path.join(root, "tests", "data", "example_clip.bvh"), "--config", os.path.join(root, "dragposer_amd", "config", "6_trackers_config.json"),
            "--max-frames", "48", "--constraints", "reference", "--keep-frames"]
    for d in ("device", "host", "plain"):
        os.makedirs(tmp_path / d)
    a = eval_drag.main(argv + ["--out-dir", str(tmp_path / "device")])[0]
    b = eval_drag.main(argv + ["--out-dir", str(tmp_path / "host"), "--per-frame"])[0]
    assert a["frames"] == b["frames"] == 48
    for k in ("poses", "pos", "iters"):
        assert np.array_equal(a[k], b[k]), k
    plain = eval_drag.main(argv[:-3] + ["--keep-frames", "--out-dir", str(tmp_path / "plain")])[0]
    assert not np.array_equal(a["poses"], plain["poses"])  # the switch is not a no-op

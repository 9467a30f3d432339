"""GPU: per-frame skeletons (include/dragposer_skeleton.h).  A launch that mixes skeletons frame by frame -- four per wave -- must give every
frame the bits one launch on a context CREATED with that frame's skeleton gives it; the context's own skeleton passed per frame must give the
plain call's bits; a refused skeleton row poisons its own frame only.  Every instantiation of the two new units (tests/skeleton_cases.py) runs."""
import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from skeleton_cases import LAYOUT_OF_UNIT, SKEL_INSTANTIATIONS, UNIT_W4_BP_SKEL, UNIT_W4_SKEL, skel_inst_id

pytestmark = pytest.mark.gpu

OUTS = ("z", "z_pre", "pose", "disp", "world_disp", "world_rot", "pos", "rot", "loss", "iters", "status")
FWD_OUTS = ("pose", "disp", "world_disp", "world_rot", "pos", "rot", "status")
MODES = {"fixed": dict(n_iter=50), "early": dict(n_iter=100, stop_eps_pos=1e-4, stop_eps_rot=1e-2, min_loss_incr=1e-5),
         "long": dict(n_iter=300)}


def _skeletons(base):
    """the model's skeleton, x0.85, x1.2, per-bone length factors in [0.8, 1.25] (seeded)"""
    rng = np.random.default_rng(7)
    per_bone = rng.uniform(0.8, 1.25, (22, 1)).astype(np.float32)
    out = [base, base * np.float32(0.85), base * np.float32(1.2), base * per_bone]
    return [np.ascontiguousarray(o, dtype=np.float32) for o in out]


def _raw(parents=None, offsets=None):
    raw = dict(np.load(R.DEFAULT_MODEL))
    if parents is not None:
        raw["parents"] = np.asarray(parents, np.int32)
    if offsets is not None:
        raw["offsets"] = offsets
    return raw


def _set_layout(opts, bp):
    from instantiations import set_layout

    return [set_layout(o, bp) for o in opts]


@pytest.fixture(scope="module")
def xsens():
    """the shipped model: one context with its own skeleton (the mixed launches), one per skeleton (the references)"""
    from dragposer_amd.optimizer import LatentOptimizer

    base = np.asarray(_raw()["offsets"], np.float32)
    skels = _skeletons(base)
    main = LatentOptimizer(device="cuda:0")
    refs = [LatentOptimizer(device="cuda:0", arrays=_raw(offsets=s)) for s in skels]
    yield main, refs, skels
    _set_layout([main] + refs, 1)


def _batch(B, seed=1234):
    from dragposer_amd.optimizer import to_device_batch

    return to_device_batch(R.synth_inputs(R.OracleModel(), B, trackers=6, seed=seed), "cuda:0")


def _mixed(skels, B):
    """[B,22,3]: frame f takes skeleton f % 4 -- every wave holds all four"""
    idx = np.arange(B) % len(skels)
    return torch.from_numpy(np.stack([skels[k] for k in idx])).cuda(), idx


def _assert_frames_equal(got, want, rows, names):
    for n in names:
        assert torch.equal(got[n][rows], want[n]), (n, (got[n][rows].float() - want[n].float()).abs().max().item())


def _run(opt, batch, mode, offsets=None, rows=None):
    b = batch if rows is None else {k: v[rows].contiguous() for k, v in batch.items()}
    if mode == "forward":
        return opt.forward(b["z0"], b["cur_rot"], outputs=FWD_OUTS, offsets=offsets)
    return opt.optimize(**b, lambda_tmp=0.02, kernel="w4", offsets=offsets, **MODES[mode])


@pytest.mark.parametrize("bp", [0, 1])
@pytest.mark.parametrize("mode", ["fixed", "early", "long", "forward"])
def test_mixed_batch_equals_one_context_per_skeleton(xsens, mode, bp):
    from instantiations import last_launch

    main, refs, skels = xsens
    assert _set_layout([main] + refs, bp) == [bp] * 5
    B = 1024
    batch = _batch(B)
    off, idx = _mixed(skels, B)
    got = _run(main, batch, mode, offsets=off)
    assert last_launch(main).unit == (UNIT_W4_BP_SKEL if bp else UNIT_W4_SKEL)
    names = FWD_OUTS if mode == "forward" else OUTS
    for k, ref in enumerate(refs):
        rows = torch.from_numpy(np.nonzero(idx == k)[0]).cuda()
        want = _run(ref, batch, mode, rows=rows)
        torch.cuda.synchronize()
        _assert_frames_equal(got, want, rows, names)
    if mode != "forward":
        assert int(got["status"].abs().sum()) == 0
        if mode == "early":
            assert int(got["iters"].min()) < int(got["iters"].max())  # (the while-condition did stop frames at different iterations)


def test_mixed_batch_on_another_tree():
    """one of tests/test_hip_topology.py's trees: other bone slots, virtual child bones on two joints"""
    from dragposer_amd.optimizer import LatentOptimizer
    from test_hip_topology import TREES, _model_arrays

    raw = _model_arrays(TREES["arms_at_two_levels"], seed=3)
    skels = _skeletons(np.asarray(raw["offsets"], np.float32))
    main = LatentOptimizer(device="cuda:0", arrays=raw)
    B = 512
    batch = _batch(B, seed=99)
    off, idx = _mixed(skels, B)
    for mode in ("fixed", "early"):
        got = _run(main, batch, mode, offsets=off)
        for k, s in enumerate(skels):
            r = dict(raw)
            r["offsets"] = s
            ref = LatentOptimizer(device="cuda:0", arrays=r)
            rows = torch.from_numpy(np.nonzero(idx == k)[0]).cuda()
            want = _run(ref, batch, mode, rows=rows)
            torch.cuda.synchronize()
            _assert_frames_equal(got, want, rows, OUTS)
            ref.close()


@pytest.mark.parametrize("inst", SKEL_INSTANTIATIONS, ids=skel_inst_id)
def test_every_instantiation_gives_the_plain_bits_on_the_contexts_own_skeleton(xsens, inst):
    """each row of the table launched (dp_debug_last_launch), with the context's skeleton passed per frame / per sequence: the plain call's bits"""
    from instantiations import last_launch

    main = xsens[0]
    assert _set_layout([main], LAYOUT_OF_UNIT[inst.unit]) == [LAYOUT_OF_UNIT[inst.unit]]
    own = torch.from_numpy(np.asarray(_raw()["offsets"], np.float32)).cuda()
    if inst.seq:
        S, T = 64, 6
        n_iter = 300 if inst.long else 100
        a = _seq_inputs(S, T, seed=11)
        got = _seq_direct(main, a, n_iter, offsets=own.expand(S, 22, 3).contiguous())  # (DragPose would take the plain launch for these)
        pick = last_launch(main)
        want = _seq_direct(main, a, n_iter)
        torch.cuda.synchronize()
        for n in got:
            assert torch.equal(got[n], want[n]), n
    else:
        B = 256
        batch = _batch(B, seed=5)
        kw = dict(MODES["early" if inst.early else "fixed"])
        kw["n_iter"] = 300 if inst.long else kw["n_iter"]
        got = main.optimize(**batch, lambda_tmp=0.02, kernel="w4", offsets=own.expand(B, 22, 3).contiguous(), **kw)
        pick = last_launch(main)
        want = main.optimize(**batch, lambda_tmp=0.02, kernel="w4", **kw)
        torch.cuda.synchronize()
        _assert_frames_equal(got, want, slice(None), OUTS)
        one = main.optimize(**batch, lambda_tmp=0.02, kernel="w4", offsets=own, **kw)  # (stride 0: one skeleton for the launch)
        _assert_frames_equal(one, want, slice(None), OUTS)
    assert tuple(pick) == tuple(inst), (pick, inst)


def _quat_mats(q):
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1)


def _seq_inputs(S, T, seed):
    g = torch.Generator().manual_seed(seed)
    E = 6
    mask = [0, 4, 8, 13, 17, 21]
    return dict(S=S, T=T, mask=mask, weights=np.array([[10, 10], [5, 0.01], [5, 0.01], [5, 0.01], [5, 0.01], [5, 0.01]], np.float32),
                tp=(0.4 * torch.randn(T, S, E, 3, generator=g)).cuda(), tR=_quat_mats(torch.randn(T, S, E, 4, generator=g)).reshape(T, S, E, 3, 3).cuda(),
                z0=(0.3 * torch.randn(S, 24, generator=g)).cuda(), gp=torch.randn(S, 3, generator=g).cuda(),
                gr=torch.nn.functional.normalize(torch.randn(S, 4, generator=g), dim=-1).cuda(), h=torch.rand(S, 6, generator=g).cuda())


def _drag(opt, a, rows=None):
    from dragposer_amd.drag_pose import DragPose

    sel = (lambda t: t) if rows is None else (lambda t: t[rows].contiguous())
    S = a["S"] if rows is None else len(rows)
    d = DragPose(opt, None, np.zeros(24, np.float32), np.ones(24, np.float32), n_sequences=S)
    d.set_initial_state(sel(a["z0"]), sel(a["gp"]), sel(a["gr"]), sel(a["h"]))
    return d


def _seq_run(opt, a, n_iter, offsets=None, rows=None):
    d = _drag(opt, a, rows)
    tp, tR = a["tp"], a["tR"]
    if rows is not None:
        tp, tR = tp[:, rows].contiguous(), tR[:, rows].contiguous()
    poses, gpos, iters = d.run_frames(tp, tR, a["mask"], a["weights"], stop_eps_pos=1e-4, stop_eps_rot=1e-2, max_iter=n_iter, learning_rate=1e-2,
                                      lambda_temporal=0, temporal_future_window=0, joint_adjustment_indices=(0, 0), joint_adjustment_weight=1.0,
                                      offsets=offsets)
    return dict(poses=poses, gpos=gpos, iters=iters, status=d.last_status, latent=d.latent, gp=d.current_global_pos, gr=d.current_global_rot)


def _seq_direct(opt, a, n_iter, offsets=None):
    """LatentOptimizer.optimize_sequence on the state DragPose would hold (one launch of T steps, no temporal pull)"""
    S, T, E = a["S"], a["T"], a["mask"]
    tp, tR = torch.zeros(T, S, 22, 3, device="cuda"), torch.zeros(T, S, 22, 9, device="cuda")
    tp[:, :, E], tR[:, :, E] = a["tp"], a["tR"].reshape(T, S, len(E), 9)
    w, tracked = torch.zeros(S, 22, 2, device="cuda"), torch.zeros(S, 22, dtype=torch.uint8, device="cuda")
    w[:, E], tracked[:, E] = torch.from_numpy(a["weights"]).cuda(), 1
    st = dict(latent=a["z0"].clone(), gp=a["gp"].clone(), gr=a["gr"].clone(), lb=a["z0"].unsqueeze(1).repeat(1, 60, 1).contiguous(),
              db=torch.zeros(S, 60, 3, device="cuda"), hb=a["h"].unsqueeze(1).repeat(1, 60, 1).contiguous())
    out = opt.optimize_sequence(st["latent"], tp, tR, None, w, tracked, torch.zeros(S, 24, device="cuda"), (0, 24), st["gp"], st["gr"], st["lb"],
                                st["db"], st["hb"], (0, 4, 8, 13, 17, 21), n_iter=n_iter, lambda_tmp=0.0, adjust=(0, 0, 1.0), offsets=offsets)
    out.update(st)
    return out


def test_sequences_of_four_skeletons_equal_each_skeletons_own_launch(xsens):
    main, refs, skels = xsens
    assert _set_layout([main] + refs, 1) == [1] * 5
    S, T = 64, 40
    a = _seq_inputs(S, T, seed=3)
    off, idx = _mixed(skels, S)
    got = _seq_run(main, a, 100, offsets=off)
    for k, ref in enumerate(refs):
        rows = torch.from_numpy(np.nonzero(idx == k)[0]).cuda()
        want = _seq_run(ref, a, 100, rows=rows)
        torch.cuda.synchronize()
        for n in got:
            g = got[n][rows] if n in ("latent", "gp", "gr") else got[n][:, rows]  # (per sequence / per step and sequence)
            assert torch.equal(g, want[n]), (k, n)
    assert int(got["status"].abs().sum()) == 0
    # DragPose.run frame by frame, the same [S,22,3] object every frame: run_frames' bits
    d = _drag(main, a)
    poses = []
    for t in range(T):
        p, _ = d.run(a["tp"][t], a["tR"][t], a["mask"], a["weights"], offsets=off, stop_eps_pos=1e-4, stop_eps_rot=1e-2, max_iter=100,
                     learning_rate=1e-2, lambda_temporal=0, temporal_future_window=0, joint_adjustment_indices=(0, 0), joint_adjustment_weight=1.0)
        poses.append(p.clone())
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(poses), got["poses"])
    assert torch.equal(d.current_global_pos, got["gp"]) and torch.equal(d.latent, got["latent"])
    # a later, different skeleton is honoured (not the first one kept for good)
    d2 = _drag(main, a)
    d2.run(a["tp"][0], a["tR"][0], a["mask"], a["weights"], offsets=off, max_iter=10, lambda_temporal=0, temporal_future_window=0)
    p_a = d2.last["pose"].clone()
    d3 = _drag(main, a)
    d3.run(a["tp"][0], a["tR"][0], a["mask"], a["weights"], offsets=off, max_iter=10, lambda_temporal=0, temporal_future_window=0)
    d3.set_initial_state(a["z0"], a["gp"], a["gr"], a["h"])
    d3.run(a["tp"][0], a["tR"][0], a["mask"], a["weights"], offsets=off * 1.3, max_iter=10, lambda_temporal=0, temporal_future_window=0)
    assert not torch.equal(d3.last["pose"], p_a)


def test_constraints_with_another_skeleton_are_refused(xsens):
    from dragposer_amd import Constraints

    main, _, skels = xsens
    a = _seq_inputs(1, 1, seed=2)
    d = _drag(main, a)
    with pytest.raises(ValueError, match="constraints="):
        d.run(a["tp"][0], a["tR"][0], a["mask"], a["weights"], offsets=torch.from_numpy(skels[2]), constraints=Constraints(),
              lambda_temporal=0, temporal_future_window=0)


def test_a_refused_skeleton_row_poisons_its_own_frame_only(xsens):
    from dragposer_amd import _lib

    main, _, skels = xsens
    _set_layout([main], 1)
    B = 256
    batch = _batch(B, seed=21)
    off, _ = _mixed(skels, B)
    clean = _run(main, batch, "fixed", offsets=off)
    bad = off.clone()
    bad[41, 7, 1] = float("nan")  # frame 41: wave 10, lane 1
    bad[130, 1, 0] = 1e5          # frame 130: beyond DP_INPUT_LIMIT (a root child's bone)
    bad[200, 0, :] = float("nan")  # row 0 is never read: frame 200 stays clean
    got = _run(main, batch, "fixed", offsets=bad)
    fwd_clean = _run(main, batch, "forward", offsets=off)
    fwd = _run(main, batch, "forward", offsets=bad)
    torch.cuda.synchronize()
    st = got["status"].cpu().numpy()
    refused = _lib.DP_STATUS_BAD_STATE | _lib.DP_STATUS_NONFINITE_RESULT  # (what a refused z0 / cur_rot reports: tests/test_hip_status.py)
    assert st[41] == refused and st[130] == refused and st[200] == 0
    assert fwd["status"][41].item() == refused and fwd["status"][130].item() == refused
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[41] = keep[130] = False
    for n in OUTS:
        assert torch.equal(got[n][keep], clean[n][keep]), n  # wave neighbours 40, 42, 43 and 128, 129, 131 included
    for n in FWD_OUTS:
        assert torch.equal(fwd[n][keep], fwd_clean[n][keep]), n
    assert torch.isnan(got["pos"][41]).all() and torch.isnan(got["z"][130]).all()


def test_w16_is_refused_and_auto_runs_the_skeleton_unit_at_any_size(xsens):
    from instantiations import last_launch

    main, _, skels = xsens
    _set_layout([main], 1)
    B = 16384
    batch = _batch(B, seed=8)
    off, _ = _mixed(skels, B)
    with pytest.raises(ValueError, match="w16"):
        main.optimize(**batch, n_iter=5, kernel="w16", offsets=off)
    assert main.auto_kernel(B) == "w16"  # (what plain dp_optimize takes at this size)
    out = main.optimize(**batch, n_iter=5, lambda_tmp=0.02, kernel="auto", offsets=off, outputs=("pos", "status"))
    torch.cuda.synchronize()
    assert last_launch(main).unit == UNIT_W4_BP_SKEL
    assert int(out["status"].abs().sum()) == 0 and bool(torch.isfinite(out["pos"]).all())


def _scaled_clip(src, dst, factor):
    """the clip with every OFFSET line scaled (plain text rewriting: the motion rows are untouched)"""
    out = []
    for line in open(src).read().splitlines(keepends=True):
        s = line.strip()
        if s.startswith("OFFSET"):
            ind = line[:len(line) - len(line.lstrip())]
            vals = [float(v) * factor for v in s.split()[1:]]
            line = ind + "OFFSET " + " ".join(f"{v:.6f}" for v in vals) + "\n"
        out.append(line)
    open(dst, "w").write("".join(out))


def test_eval_drag_runs_a_clip_of_other_bone_lengths_and_lockstep_keeps_each_clips_bits(tmp_path):
    """a clip with the model's topology and other bone lengths runs with its own skeleton (it used to exit); in a lock-step run beside the
    unscaled clip -- one launch per stretch for two performers -- each clip gets the bits of its solo run"""
    import os

    from dragposer_amd import eval_drag as E

    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "example_clip.bvh")
    d = tmp_path / "clips"
    d.mkdir()
    a, b = str(d / "a_clip.bvh"), str(d / "b_clip_scaled.bvh")
    open(a, "w").write(open(src).read())
    _scaled_clip(src, b, 1.12)
    common = ["--max-frames", "240", "--keep-frames"]
    solo_a = E.main([R.DEFAULT_MODEL, a, "--out-dir", str(tmp_path / "oa")] + common)[0]
    solo_b = E.main([R.DEFAULT_MODEL, b, "--out-dir", str(tmp_path / "ob")] + common)[0]
    both = E.main([R.DEFAULT_MODEL, str(d), "--lockstep", "--out-dir", str(tmp_path / "oab")] + common)
    for solo, lock in ((solo_a, both[0]), (solo_b, both[1])):
        for k in ("poses", "pos", "iters"):
            assert np.array_equal(solo[k], lock[k]), k
    assert np.isfinite(solo_b["poses"]).all() and np.isfinite(solo_b["pos"]).all()
    # the scaled performer is tracked about as well as the one the model's skeleton fits (metres; the error scales with the body)
    assert solo_b["mpjpe"] < 1.5 * solo_a["mpjpe"] + 0.01 and solo_b["mpeepe"] < 1.5 * solo_a["mpeepe"] + 0.01, (solo_a, solo_b)

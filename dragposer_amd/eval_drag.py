"""`eval_drag` on MI355X: the reference's offline evaluation CLI (python/src/eval_drag.py:21-293) with the
per-frame optimisation running in the HIP kernel.

    python -m dragposer_amd.eval_drag models/model_dancedb data/example/eval/example.bvh --config config/6_trackers_config.json

The reference's contract: `model_path` is the model FOLDER (generator.pt, data.pt and -- when trained -- temporal.pt, as
train.py / train_temporal.py save them), `input_path` a .bvh file or a directory of them, --config / --verbose as there, the
result written to data/eval_<name> relative to the working directory, and the reference's four result lines printed
verbatim (eval_drag.py:249-252).  Also accepted as `model_path`: this package's flat .npz fixture (default: the shipped
model_dancedb).  Stated in the output: because the reference's temporal.pt is not distributed with it the temporal
predictor is optional -- without one (no temporal.pt in the folder, no --temporal-checkpoint) the pull term is switched off
(lambda_temporal = 0) instead of pulling towards the predictions of an untrained network, unless --latent-ar names a predictor that
needs no training (dragposer_amd.ar, include/dragposer_latent_ar.h): then the configuration's lambda_temporal pulls towards its targets.
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from . import quat_np as Q
from .bvh import BVH
from .constraints import Constraints
from .drag_pose import DragPose
from .encoder import PoseEncoder
from .holds import Hold, Holds
from .model import DEFAULT_MODEL, NJ, load_model_arrays
from .motion import local_quats_from_bvh, prepare_motion
from .optimizer import LatentOptimizer
from .temporal import load_reference_checkpoint
from .terms import Term, Terms

SPARSE_JOINTS = [0, 4, 8, 13, 17, 21]  # train.py:32-39 (evaluation only)
HEIGHT_INDICES = [0, 4, 8, 13, 17, 21]
FOOT_LOCK_JOINTS = (4, 8)  # --foot-lock: the two joints Constraints.reference() keeps on the floor

DEFAULT_CONFIG = dict(  # eval_drag.py:68-131
    mask=[1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1],
    weights=[[10, 10]] + [[1, 0.01]] * 2 + [[5, 0.01]] + [[1, 0.01]] * 3 + [[5, 0.01]] + [[1, 0.01]] * 5 + [[5, 0.01]]
    + [[1, 0.01]] * 3 + [[5, 0.01]] + [[1, 0.01]] * 3 + [[5, 0.01]],
    enable_joint_adjustment=True, joint_adjustment_indices=[0, 0], joint_adjustment_weight=1.0,
    lambda_temporal=0.02, temporal_future_window=0)


def eval_pos_error(gt_bvh, eval_bvh, frames=None):
    """eval_metrics.eval_pos_error (eval_metrics.py:6-32): FK of both files with the root at the origin.  `frames`: a boolean mask, the
    means are then over those frames alone (--drop's second line)."""
    gq, _, parents, offsets = local_quats_from_bvh(gt_bvh)
    eq, _, _, _ = local_quats_from_bvh(eval_bvh)
    n = min(len(gq), len(eq))
    gp, _ = Q.fk(gq[:n], np.zeros((n, 3)), offsets, parents)
    ep, _ = Q.fk(eq[:n], np.zeros((n, 3)), offsets, parents)
    err = np.linalg.norm(ep - gp, axis=-1)
    if frames is not None:
        err = err[np.asarray(frames, bool)[:n]]
    return float(err.mean()), float(err[:, SPARSE_JOINTS[1:]].mean())


def foot_skate(gt_bvh, eval_bvh, contact_lo, floor_level=0.0, up=1, joints=FOOT_LOCK_JOINTS):
    """--foot-lock's extra line: the mean horizontal displacement per frame of `joints` in the result, over the frames on which the
    ground-truth joint is at or below `contact_lo` above the floor.  World positions by eval_pos_error's FK, each file's own root
    trajectory.  -> (the mean, or nan when no frame qualifies; the number of (frame, joint) pairs)"""
    gq, gpos, parents, offsets = local_quats_from_bvh(gt_bvh)
    eq, epos, _, _ = local_quats_from_bvh(eval_bvh)
    n = min(len(gq), len(eq))
    root = lambda p: np.asarray(p)[:n].reshape(n, -1, 3)[:, 0]
    gp, _ = Q.fk(gq[:n], root(gpos), offsets, parents)
    ep, _ = Q.fk(eq[:n], root(epos), offsets, parents)
    j = list(joints)
    contact = (gp[1:, j, up] - floor_level) <= contact_lo
    step = ep[1:, j] - ep[:-1, j]
    step[..., up] = 0.0
    d = np.linalg.norm(step, axis=-1)[contact]
    return (float(d.mean()) if d.size else float("nan")), int(d.size)


def motion_jitter(world_pos):
    """the jitter of a motion: the mean over frames 1..F-2 and all joints of |W(t+1) - 2 W(t) + W(t-1)|, the second difference of the joints'
    world positions [F, J, 3], in the positions' units (per frame squared).  nan for fewer than three frames."""
    w = np.asarray(world_pos, np.float64)
    if w.shape[0] < 3:
        return float("nan")
    return float(np.linalg.norm(w[2:] - 2.0 * w[1:-1] + w[:-2], axis=-1).mean())


def jitter(gt_bvh, eval_bvh):
    """--tether's extra line: motion_jitter of the result and of the ground truth over the same frames.  World positions by
    eval_pos_error's FK, each file's own root trajectory.  -> (the reconstruction's, the ground truth's)"""
    gq, gpos, parents, offsets = local_quats_from_bvh(gt_bvh)
    eq, epos, _, _ = local_quats_from_bvh(eval_bvh)
    n = min(len(gq), len(eq))
    root = lambda p: np.asarray(p)[:n].reshape(n, -1, 3)[:, 0]
    gp, _ = Q.fk(gq[:n], root(gpos), offsets, parents)
    ep, _ = Q.fk(eq[:n], root(epos), offsets, parents)
    return motion_jitter(ep), motion_jitter(gp)


def parse_tethers(items):
    """--tether J:HI:WEIGHT[:ALPHA], up to four times -> [(joint, hi, weight, alpha)]"""
    out = []
    for item in items:
        parts = item.split(":")
        try:
            if len(parts) not in (3, 4):
                raise ValueError("three or four fields")
            j, hi, w, alpha = int(parts[0]), float(parts[1]), float(parts[2]), (float(parts[3]) if len(parts) == 4 else 0.0)
            if not (0 <= j < NJ and np.isfinite(hi) and hi >= 0.0 and np.isfinite(w) and w >= 0.0 and 0.0 <= alpha <= 1.0):
                raise ValueError("J is a joint, HI and WEIGHT are finite and not negative, ALPHA lies in [0, 1]")
        except ValueError as e:
            raise SystemExit(f"--tether: expected J:HI:WEIGHT[:ALPHA], got {item!r} ({e})")
        out.append((j, hi, w, alpha))
    if len(out) > 4:
        raise SystemExit(f"--tether: at most 4 tethers, got {len(out)}")
    return out


def parse_balance(item, masses_path=None):
    """--balance RADIUS:WEIGHT [--balance-masses FILE] -> (radius, weight, 22 masses or None: uniform)"""
    try:
        radius, weight = (float(x) for x in item.split(":"))
        if not (np.isfinite(radius) and radius >= 0.0 and np.isfinite(weight) and weight >= 0.0):
            raise ValueError("RADIUS and WEIGHT are finite and not negative")
    except ValueError as e:
        raise SystemExit(f"--balance: expected RADIUS:WEIGHT, got {item!r} ({e})")
    masses = None
    if masses_path is not None:
        masses = [float(x) for x in open(masses_path).read().replace(",", " ").split()]
        if len(masses) != NJ:
            raise SystemExit(f"--balance-masses: {masses_path} holds {len(masses)} numbers, expected {NJ}")
    return radius, weight, masses


def balance_terms(spec, base):
    """--balance: one DISTANCE term (DROP_UP, lo = 0, hi = RADIUS) between the centroid of all joints and the midpoint of joints 4 and 8,
    appended to the table `base` -> a Terms with the two points (include/dragposer_points.h)"""
    from .points import Point, Points

    radius, weight, masses = spec
    pts = Points([Point.centroid(masses), Point.midpoint(*FOOT_LOCK_JOINTS)])
    term = Term.distance(pts.joint(0), pts.joint(1), lo=0.0, hi=radius, weight=weight, drop_up=True)
    return Terms(base.terms + [term], base.up_axis, pts)


def tether_terms(specs, base):
    """--tether: a point-DISTANCE term (lo = 0, hi = HI) per tethered joint and a tether on it, appended to the table `base` -> (Terms, Tethers)"""
    from .tethers import Tether, Tethers

    ts = [Term.distance(j, point=(0.0, 0.0, 0.0), lo=0.0, hi=hi, weight=w) for j, hi, w, _ in specs]
    return Terms(base.terms + ts, base.up_axis), Tethers([Tether(len(base) + i, alpha) for i, (_, _, _, alpha) in enumerate(specs)])


def foot_lock_terms(args, cons):
    """--foot-lock: two horizontal soft pins on FOOT_LOCK_JOINTS and their holds, appended to the reference's terms as a table when
    --constraints reference is given -> (Terms, Holds)"""
    base = Terms.from_constraints(cons) if cons is not None else Terms(up_axis=args.up_axis)  # (a table has one up axis: the constraints' own)
    lo, hi = args.contact_height
    pins = [Term.distance(j, point=(0.0, 0.0, 0.0), lo=0.0, hi=0.0, weight=args.foot_lock_weight, drop_up=True) for j in FOOT_LOCK_JOINTS]
    holds = Holds([Hold(len(base) + i, lo, hi, level=args.floor_level) for i in range(len(pins))])
    return Terms(base.terms + pins, base.up_axis), holds


def parse_drop(text, mask_idx, n_frames):
    """--drop J:START:LEN[,...] -> (a boolean [n_frames, E] array in tracker-list order: the samples of joint J that are blanked; a boolean
    [n_frames]: the frames named).  A joint that is not among the configuration's trackers has no sample to blank: its frames are still
    named, so that a configuration without that tracker is scored on the same frames."""
    drop, rows = np.zeros((n_frames, len(mask_idx)), bool), np.zeros(n_frames, bool)
    for item in text.split(","):
        try:
            j, start, length = (int(x) for x in item.split(":"))
        except ValueError:
            raise SystemExit(f"--drop: expected J:START:LEN[,...], got {item!r}")
        if not 0 <= j < NJ or start < 0 or length <= 0:
            raise SystemExit(f"--drop: {item!r}: J must be a joint, START must not be negative and LEN must be positive")
        rows[start:start + length] = True
        if j in list(mask_idx):
            drop[start:start + length, list(mask_idx).index(j)] = True
    return drop, rows


def result_to_bvh(poses, global_pos, means, stds, bvh, out_path):
    """train.result_to_bvh with are_root_rot_incr=False (train.py:437-509): normalised root-space quaternions
    whose root channels already hold the world rotation -> local Euler angles -> BVH."""
    sd4 = stds["dqs"].reshape(NJ, 8)[:, :4].reshape(88)
    mu4 = means["dqs"].reshape(NJ, 8)[:, :4].reshape(88)
    qs = (poses.astype(np.float64) * sd4 + mu4).reshape(-1, NJ, 4)
    _, _, parents, _, order = bvh.get_data()
    local = Q.from_root_space(qs, parents)
    rot = np.stack([np.degrees(Q.to_euler(local[:, j], order[j])) for j in range(NJ)], axis=1)
    bvh.set_data(rot, global_pos.astype(np.float64))
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    bvh.save(out_path)


def synthesize_targets(m, n_frames, mask_idx):
    """The per-frame targets of eval_drag.py:164-202 that do not depend on the running state: ground-truth root-space quaternions
    with the root channel replaced by the global rotation -> parent-local (from_root_quat) -> FK with the root at the origin.
    -> positions of the tracked joints relative to the root [F, E, 3] (the reference adds target_global_pos - current_global_pos
    to them, frame by frame: run_sequences does that on the device) and their global rotation matrices [F, E, 9]."""
    rq = m["root_quats"].copy()
    rq[:, 0] = m["global_rot"]
    local = Q.from_root_space(rq, m["parents"])
    p_rel, g_rot = Q.fk(local[:n_frames], np.zeros((n_frames, 3)), m["offsets"].astype(np.float64), m["parents"])
    return p_rel[:, mask_idx], Q.to_matrix(g_rot[:, mask_idx]).reshape(n_frames, len(mask_idx), 9)


def prepare_file(args, input_path, opt, encoder, cfg, raw):
    """BVH -> everything one sequence needs on the device (eval_drag.py:133-202): normalised motion, per-frame
    targets relative to the root, the ground-truth root trajectory, the encoder's initial latent."""
    dev = opt.device
    means = {"dqs": raw["means.dqs"], "displacement": raw["means.displacement"]}
    stds = {"dqs": raw["stds.dqs"], "displacement": raw["stds.displacement"]}
    bvh = BVH().load(input_path)
    m = prepare_motion(bvh, means, stds, HEIGHT_INDICES)
    if list(m["parents"]) != list(opt.host_model.parents):
        raise SystemExit(f"{input_path}: skeleton topology differs from the one the model fixture was exported with")
    # (other bone lengths are the clip's own: they drive its targets below and, as the reference's run(offsets=...), the optimisation --
    #  DragPose.run_frames / run(offsets=...), include/dragposer_skeleton.h)
    n_frames = len(m["dqs"]) if args.max_frames is None else min(args.max_frames, len(m["dqs"]))
    mask_idx = np.nonzero(np.asarray(cfg["mask"]))[0]
    # targets (eval_drag.py:164-202): FK of the ground-truth pose with the root at the origin, per frame; the
    # root translation relative to the running estimate is added inside the loop, on the device
    p_rel, r_mats = synthesize_targets(m, n_frames, mask_idx)
    dropped, rows = None, None
    if getattr(args, "drop", None):  # the blanked samples arrive as NaN, as a tracker out of view sends them
        dropped, rows = parse_drop(args.drop, mask_idx, n_frames)
        p_rel, r_mats = p_rel.copy(), r_mats.copy()
        p_rel[dropped], r_mats[dropped] = np.nan, np.nan
    if getattr(args, "initial_latent", None):
        # (parity runs: the reference draws the encoder's noise from torch's GLOBAL generator after its model constructors have
        #  consumed an implementation-defined amount of it -- eval_drag.py:23,49-51,152 -- so its latent is handed over instead)
        z0 = torch.tensor(np.load(args.initial_latent).reshape(1, -1), dtype=torch.float32, device=dev)
    else:
        gen = torch.Generator(device="cpu").manual_seed(2222)  # train.param["seed"]
        z0 = encoder.sample(torch.tensor(m["dqs"][0:1], device=dev), generator=gen)  # drag_pose.py:50
    return dict(path=input_path, bvh=bvh, m=m, n_frames=n_frames, means=means, stds=stds, z0=z0, dropped_rows=rows,
                offsets=torch.tensor(np.asarray(m["offsets"], np.float32).reshape(NJ, 3), device=dev),
                tp_rel=torch.tensor(p_rel, dtype=torch.float32, device=dev), tR=torch.tensor(r_mats, dtype=torch.float32, device=dev),
                gpos=torch.tensor(m["global_pos"][:n_frames], dtype=torch.float32, device=dev))


def calibrate_file(args, q, opt, cfg, raw):
    """--calibrate: the clip's bone lengths from its own tracker targets (dragposer_amd.calibrate, include/dragposer_calibration.h), as for a
    performer without a BVH file: FRAMES frames drawn evenly from the clip as independent frames -- z0 = 0, lambda_temporal = 0, cur_rot = the
    root's rotation one frame earlier, the root's displacement since then in the position targets -- start from the model's skeleton
    (raw["offsets"]; the clip's OFFSET table is read for the targets and for the printed ratios only).  -> the fitted offsets [22,3] on the device"""
    from .calibration import BoneGroups, calibrate

    name, n_fit, rounds = args.calibrate_spec
    groups = getattr(BoneGroups, name)()
    dev, m, n = opt.device, q["m"], q["n_frames"]
    if n < 2:
        raise SystemExit("--calibrate: the clip needs at least two frames")
    idx = np.unique(np.linspace(1, n - 1, min(n_fit, n - 1)).round().astype(np.int64))
    B = len(idx)
    mask_idx = np.nonzero(np.asarray(cfg["mask"]))[0]
    it, mt = torch.as_tensor(idx, device=dev), torch.as_tensor(mask_idx, device=dev)
    tgt_pos = torch.zeros(B, NJ, 3, device=dev)
    tgt_pos[:, mt] = q["tp_rel"][it] + (q["gpos"][it] - q["gpos"][it - 1]).unsqueeze(1)
    tgt_rot = torch.zeros(B, NJ, 9, device=dev)
    tgt_rot[:, mt] = q["tR"][it]
    w = torch.zeros(B, NJ, 2, device=dev)
    w[:, mt] = torch.as_tensor(np.asarray(cfg["weights"], np.float32)[mask_idx], device=dev)
    tracked = torch.zeros(B, NJ, dtype=torch.uint8, device=dev)
    tracked[:, mt] = 1
    batch = dict(z0=torch.zeros(B, 24, device=dev), z_tgt=torch.zeros(B, 24, device=dev),
                 cur_rot=torch.as_tensor(np.asarray(m["global_rot"], np.float32)[idx - 1], device=dev).contiguous(),
                 tgt_pos=tgt_pos, tgt_rot=tgt_rot, w=w, tracked=tracked)
    cal = calibrate(opt, batch, groups, rounds=rounds, n_iter=50, ridge=1e-3, lambda_tmp=0.0)
    last = cal.trace[-1]
    base, true = np.asarray(raw["offsets"], np.float64).reshape(NJ, 3), np.asarray(m["offsets"], np.float64).reshape(NJ, 3)
    print(f"Calibration: {name}, {B} frames, {rounds} rounds of 50 iterations (dragposer_amd.calibrate, include/dragposer_calibration.h); "
          f"frames used {last['frames']}, flags {last['flags']}, residual {last['rms'][0]:.5f} -> {last['rms'][1]:.5f}")
    for k in range(len(groups)):
        bones = groups.members(k)
        ratio = float(np.mean(np.linalg.norm(true[bones], axis=-1) / np.linalg.norm(base[bones], axis=-1)))
        print(f"  group {k}: fitted scale {float(last['scales'][k]):.4f}, true ratio {ratio:.4f} (bones {bones})")
    return cal.offsets


def run_sequences(args, seqs, opt, temporal_pack, cfg):
    """The frame loop (eval_drag.py:181-227) for S prepared sequences advancing in lock-step: one `DragPose.run`
    (two kernel launches) per frame index whatever S.  Sequences shorter than the longest keep receiving their last
    frame's targets; their surplus frames are dropped."""
    dev, S = opt.device, len(seqs)
    T = max(q["n_frames"] for q in seqs)
    mask_idx = np.nonzero(np.asarray(cfg["mask"]))[0]
    weights = np.asarray(cfg["weights"], np.float32)[mask_idx]
    temporal, means_latent, stds_latent = temporal_pack
    ar = getattr(args, "latent_ar_model", None)  # (main: --latent-ar; not together with a temporal checkpoint)
    lam_tmp = cfg["lambda_temporal"] if temporal is not None or ar is not None else 0.0
    window = cfg["temporal_future_window"] if temporal is not None else 0
    pad = lambda t: torch.cat((t, t[-1:].expand(T - t.shape[0], *t.shape[1:])), dim=0) if t.shape[0] < T else t
    tp_rel = torch.stack([pad(q["tp_rel"]) for q in seqs], dim=1).contiguous()  # [T, S, E, 3]
    tR = torch.stack([pad(q["tR"]) for q in seqs], dim=1).contiguous()
    gpos = torch.stack([pad(q["gpos"]) for q in seqs], dim=1).contiguous()      # [T, S, 3]
    # [S, 22, 3]: each clip's own skeleton (eval_drag.py:48,135,209) -- or what --calibrate fitted, or with --model-skeleton the model's
    offsets = torch.stack([q.get("run_offsets", q["offsets"]) for q in seqs]).contiguous()

    drag = DragPose(opt, temporal, means_latent, stds_latent, n_sequences=S, native_temporal=not getattr(args, "torch_temporal", False))
    drag.set_initial_state(torch.cat([q["z0"] for q in seqs], dim=0), np.stack([q["m"]["global_pos"][0] for q in seqs]),
                           np.stack([q["m"]["global_rot"][0] for q in seqs]), np.stack([q["m"]["heights"][0] for q in seqs]))
    ja = tuple(cfg["joint_adjustment_indices"]) if cfg["enable_joint_adjustment"] else None
    smooth = getattr(args, "smooth_spec", None) is not None
    drag.keep_latents = smooth  # (--smooth's second pass starts from every frame's latent)
    latents = torch.zeros(T, S, 24, device=dev) if smooth else None
    cons = None
    if getattr(args, "constraints", None) == "reference":  # the reference's `# Additional Losses` block (drag_pose.py:129-183), un-commented
        cons = Constraints.reference()
    extra = dict(constraints=cons)
    if getattr(args, "foot_lock", False):
        terms, holds = foot_lock_terms(args, cons)
        extra = dict(terms=terms, holds=holds)
    if getattr(args, "tether_specs", None):
        base = extra.get("terms")
        if base is None:
            base = Terms.from_constraints(cons) if cons is not None else Terms(up_axis=args.up_axis)
        extra.pop("constraints", None)
        extra["terms"], extra["tethers"] = tether_terms(args.tether_specs, base)
    if getattr(args, "balance_spec", None) is not None:
        base = Terms.from_constraints(cons) if cons is not None else Terms(up_axis=args.up_axis)
        extra = dict(terms=balance_terms(args.balance_spec, base))
    if ar is not None:
        extra["ar"] = ar
    if getattr(args, "gaps_model", None) is not None:
        if extra.get("constraints") is None:
            extra.pop("constraints", None)
        extra["gaps"] = args.gaps_model
    if getattr(args, "solver_model", None) is not None:
        extra = dict(solver=args.solver_model)
        if cons is not None:  # (the reference's extra terms as the solver's table in the LM loss: include/dragposer_sequence_lm_terms.h)
            args.solver_model.terms = Terms.from_constraints(cons)
    poses = torch.zeros(T, S, 88, device=dev)
    out_pos = torch.zeros(T, S, 3, device=dev)
    iters = torch.zeros(T, S, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t0 = time.time()
    if not getattr(args, "per_frame", False):
        # the frame loop on the device: one launch per stretch of frames between two temporal predictions (DragPose.run_frames)
        print(f"Frames: {T} (frame loop on the device)", flush=True)
        poses, out_pos, iters = drag.run_frames(tp_rel, tR.reshape(T, S, -1, 3, 3), mask_idx, weights, target_root=gpos, stop_eps_pos=0.01 * 0.01,
                                                stop_eps_rot=0.01, max_iter=args.max_iter, min_loss_incr=0.00001, learning_rate=1e-2, lambda_rot=1,
                                                lambda_temporal=lam_tmp, temporal_future_window=window, height_indices=HEIGHT_INDICES,
                                                joint_adjustment_indices=ja, joint_adjustment_weight=cfg["joint_adjustment_weight"], offsets=offsets, **extra)
        if smooth:
            latents = drag.last_latents
    for i in range(T if getattr(args, "per_frame", False) else 0):
        if i % 1000 == 0:
            print(f"Frame: {i + 1} out of {T}", flush=True)
        tp = tp_rel[i] + (gpos[i] - drag.current_global_pos).unsqueeze(1)  # eval_drag.py:186-199
        drag.run(tp, tR[i], mask_idx, weights, offsets=offsets, stop_eps_pos=0.01 * 0.01, stop_eps_rot=0.01, max_iter=args.max_iter,
                 min_loss_incr=0.00001, learning_rate=1e-2, lambda_rot=1, lambda_temporal=lam_tmp,
                 temporal_future_window=window, height_indices=HEIGHT_INDICES, joint_adjustment_indices=ja,
                 joint_adjustment_weight=cfg["joint_adjustment_weight"], verbose=args.verbose, out_pose=poses[i], out_pos=out_pos[i], **extra)
        iters[i] = drag.last["iters"]
        if smooth:
            latents[i] = drag.latent
    torch.cuda.synchronize()
    elapsed = time.time() - t0
    poses, out_pos, iters = poses.cpu().numpy(), out_pos.cpu().numpy(), iters.cpu().numpy()
    res = [dict(poses=poses[:q["n_frames"], k], pos=out_pos[:q["n_frames"], k], iters=iters[:q["n_frames"], k]) for k, q in enumerate(seqs)]
    if smooth:
        for k, q in enumerate(seqs):
            res[k]["latents"] = latents[:q["n_frames"], k].contiguous()
    return res, elapsed, lam_tmp, temporal is not None or ar is not None


def smooth_file(args, q, res, opt, cfg):
    """--smooth: the clip's frames once more, as ONE sequence solved jointly (LatentOptimizer.optimize_clip_lm, include/dragposer_clip_lm.h).  Frame
    t runs under what the first pass left before it -- cur_rot = the world root rotation it returned for frame t-1 (read back from the pose's
    root channels; the clip's own before frame 0), position targets shifted by its global position before frame t -- with z0 = z_tgt = its
    latent and lambda_tmp = ANCHOR.  -> dict(poses [T,88] with the world root rotation in the root channels, pos [T,3] advanced from the first
    pass's positions as the frame loop advances them, and the call's per-sequence outputs)"""
    clip, anchor = args.smooth_spec
    dev, m, T = opt.device, q["m"], q["n_frames"]
    # the clip's own bones, as the first pass ran on them: passed to the joint pass when they differ from the context's
    # (dp_optimize_clip_lm_skeleton, include/dragposer_clip_skeleton.h); when they agree the plain call is made, the same bits as ever
    own = np.asarray(m["offsets"], np.float32).reshape(NJ, 3)
    same = np.allclose(own[1:].astype(np.float64), np.asarray(opt.host_model.arrays["offsets"], np.float64).reshape(NJ, 3)[1:], atol=1e-6)
    offsets = None if same else torch.as_tensor(np.ascontiguousarray(own), device=dev)
    mask_idx = np.nonzero(np.asarray(cfg["mask"]))[0]
    mt = torch.as_tensor(mask_idx, device=dev)
    sd4 = q["stds"]["dqs"].reshape(NJ, 8)[:, :4].reshape(88)[:4].astype(np.float32)
    mu4 = q["means"]["dqs"].reshape(NJ, 8)[:, :4].reshape(88)[:4].astype(np.float32)
    rot_before = np.concatenate((np.asarray(m["global_rot"][0:1], np.float32), res["poses"][:T - 1, :4] * sd4 + mu4)).astype(np.float32)
    pos_before = torch.as_tensor(np.concatenate((np.asarray(m["global_pos"][0:1], np.float32), res["pos"][:T - 1])).astype(np.float32), device=dev)
    tgt_pos = torch.zeros(T, NJ, 3, device=dev)
    tgt_pos[:, mt] = q["tp_rel"][:T] + (q["gpos"][:T] - pos_before).unsqueeze(1)
    tgt_rot = torch.zeros(T, NJ, 9, device=dev)
    tgt_rot[:, mt] = q["tR"][:T]
    w = torch.zeros(T, NJ, 2, device=dev)
    w[:, mt] = torch.as_tensor(np.asarray(cfg["weights"], np.float32)[mask_idx], device=dev)
    tracked = torch.zeros(T, NJ, dtype=torch.uint8, device=dev)
    tracked[:, mt] = 1
    z = res["latents"]
    torch.cuda.synchronize()
    t0 = time.time()
    out = opt.optimize_clip_lm(z, z.clone(), torch.as_tensor(rot_before, device=dev).contiguous(), tgt_pos, tgt_rot, w, tracked, n_sequences=1, clip=clip,
                               lambda_rot=1.0, lambda_tmp=anchor, offsets=offsets)
    torch.cuda.synchronize()
    elapsed = time.time() - t0
    pos = pos_before + out["world_disp"]  # drag_pose.py:370, then the joint adjustment (drag_pose.py:377-384)
    if cfg["enable_joint_adjustment"]:
        j, k = cfg["joint_adjustment_indices"]
        pos = pos + (tgt_pos[:, int(mask_idx[k])] - out["pos"][:, int(j)]) * float(cfg["joint_adjustment_weight"])
    poses = out["pose"].clone()
    poses[:, :4] = (out["world_rot"] - torch.as_tensor(mu4, device=dev)) / torch.as_tensor(sd4, device=dev)
    return dict(poses=poses.cpu().numpy(), pos=pos.cpu().numpy(), time=elapsed, n_accepted=int(out["n_accepted"][0]), info=int(out["info"][0]),
                loss_hist=out["loss_hist"][0].cpu().numpy(), clip_loss=out["clip_loss"][0].cpu().numpy(), bad=int((out["status"] != 0).sum()))


def finish_file(args, q, res, elapsed, lam_tmp, has_temporal, shared=1):
    """write the result BVH, report the reference's metrics (eval_drag.py:229-252)"""
    name = os.path.basename(q["path"])
    out_path = os.path.join(args.out_dir, "eval_" + name)
    result_to_bvh(res["poses"], res["pos"], q["means"], q["stds"], q["bvh"], out_path)
    mpjpe, mpeepe = eval_pos_error(BVH().load(q["path"]), BVH().load(out_path))
    n = q["n_frames"]
    print(f"Evaluate Loss: {mpjpe + mpeepe}")
    print(f"Mean Per Joint Position Error: {mpjpe}")
    print(f"Mean End Effector Position Error: {mpeepe}")
    blank = None
    if q.get("dropped_rows") is not None and q["dropped_rows"].any():
        rows = q["dropped_rows"]
        blank = eval_pos_error(BVH().load(q["path"]), BVH().load(out_path), frames=rows)
        print(f"Blanked frames ({int(rows.sum())} of {len(rows)}, --drop {args.drop}): Mean Per Joint Position Error: {blank[0]} // "
              f"Mean End Effector Position Error: {blank[1]}")
    if getattr(args, "gaps_model", None) is not None:
        g = args.gaps_model
        print(f"Gaps: max_hold {g.max_hold}, decay {g.decay} (DragPose.run_frames(gaps=), include/dragposer_gaps.h)")
    print(f"Time: {elapsed}" + (f"  (shared by {shared} sequences in lock-step)" if shared > 1 else ""))
    if getattr(args, "latent_ar_model", None) is not None:
        how = "solver=LM(predictor=)" if getattr(args, "solver_model", None) is not None else "ar="
        print(f"Latent predictor: {args.latent_ar_text} (DragPose.run_frames({how}), include/dragposer_latent_ar.h)")
    print(f"Frames: {n}  ({n / elapsed:.1f} frames/s, mean iterations/frame {res['iters'].mean():.1f}, "
          f"lambda_temporal {lam_tmp}{'' if has_temporal else ' -- no temporal checkpoint given: pull term off'})")
    out = dict(mpjpe=mpjpe, mpeepe=mpeepe, time=elapsed, frames=n, out=out_path, mean_iters=float(res["iters"].mean()))
    if blank is not None:
        out.update(mpjpe_blanked=blank[0], mpeepe_blanked=blank[1])
    if getattr(args, "tether_specs", None):
        print("Tethers: " + ", ".join(f"joint {j} hi {hi} weight {w} alpha {a}" for j, hi, w, a in args.tether_specs) +
              " (DragPose.run_frames(tethers=), include/dragposer_tethers.h)")
    if getattr(args, "balance_spec", None) is not None:
        r, w, masses = args.balance_spec
        print(f"Balance: radius {r} weight {w}, the centroid of all joints ({'uniform masses' if masses is None else 'masses ' + args.balance_masses}) "
              f"within the radius of the midpoint of joints {FOOT_LOCK_JOINTS[0]} and {FOOT_LOCK_JOINTS[1]}, horizontally "
              "(DragPose.run_frames(terms=<with points>), include/dragposer_points.h)")
    if getattr(args, "foot_lock", False) or getattr(args, "tether_specs", None) or getattr(args, "balance_spec", None) is not None:
        up = Constraints.reference().up_axis if getattr(args, "constraints", None) == "reference" else args.up_axis
        skate, pairs = foot_skate(BVH().load(q["path"]), BVH().load(out_path), args.contact_height[0], args.floor_level, up)
        print(f"Foot skate: {skate} (mean horizontal displacement per frame of joints {FOOT_LOCK_JOINTS[0]} and {FOOT_LOCK_JOINTS[1]} over "
              f"{pairs} ground-truth contact frames)")
        out.update(foot_skate=skate, contact_frames=pairs)
    if getattr(args, "tether_specs", None):
        jit, jit_gt = jitter(BVH().load(q["path"]), BVH().load(out_path))
        print(f"Jitter: {jit} (mean |W(t+1) - 2 W(t) + W(t-1)| over the inner frames and all {NJ} joints; the ground truth's own: {jit_gt})")
        out.update(jitter=jit, jitter_gt=jit_gt)
    if res.get("smooth") is not None:
        sm, (clip, anchor) = res["smooth"], args.smooth_spec
        sm_path = os.path.join(args.out_dir, "eval_smooth_" + name)
        result_to_bvh(sm["poses"], sm["pos"], q["means"], q["stds"], q["bvh"], sm_path)
        mpjpe2, mpeepe2 = eval_pos_error(BVH().load(q["path"]), BVH().load(sm_path))
        jit1, jit_gt = jitter(BVH().load(q["path"]), BVH().load(out_path))
        jit2, _ = jitter(BVH().load(q["path"]), BVH().load(sm_path))
        accel = "" if clip.accel is None else f" lambda_accel {clip.accel:g} (include/dragposer_clip_accel.h)"
        print(f"Smooth: lambda {clip.smooth} steps {clip.steps} anchor {anchor}{accel} (LatentOptimizer.optimize_clip_lm, include/dragposer_clip_lm.h): "
              f"Mean Per Joint Position Error {mpjpe} -> {mpjpe2}, Mean End Effector Position Error {mpeepe} -> {mpeepe2}, jitter {jit1} -> {jit2} "
              f"(the ground truth's own: {jit_gt}); accepted {sm['n_accepted']} of {clip.steps} steps, sequence loss {sm['loss_hist'][0]:.6g} -> "
              f"{sm['loss_hist'][-1]:.6g} (coupling part {sm['clip_loss'][1]:.6g}), info {sm['info']}, frames with a status {sm['bad']}, {sm['time']:.3f} s")
        out.update(mpjpe_smooth=mpjpe2, mpeepe_smooth=mpeepe2, jitter=jit1, jitter_smooth=jit2, jitter_gt=jit_gt, out_smooth=sm_path,
                   smooth_accepted=sm["n_accepted"], smooth_loss_hist=sm["loss_hist"], smooth_accel=clip.accel)
    if getattr(args, "keep_frames", False):
        out.update(poses=res["poses"], pos=res["pos"], iters=res["iters"])
    return out


def evaluate_files(args, paths, opt, encoder, temporal_pack, cfg, raw):
    """one or more files as sequences in lock-step"""
    seqs = [prepare_file(args, p, opt, encoder, cfg, raw) for p in paths]
    for q in seqs:
        if getattr(args, "calibrate_spec", None) is not None:
            q["run_offsets"] = calibrate_file(args, q, opt, cfg, raw)
        elif getattr(args, "model_skeleton", False):
            q["run_offsets"] = torch.tensor(np.asarray(raw["offsets"], np.float32).reshape(NJ, 3), device=opt.device)
    results, elapsed, lam_tmp, has_temporal = run_sequences(args, seqs, opt, temporal_pack, cfg)
    out = []
    for q, r in zip(seqs, results):
        if len(seqs) > 1:
            print(f"Result {q['path']} ------------------------")
        if getattr(args, "smooth_spec", None) is not None:
            r["smooth"] = smooth_file(args, q, r, opt, cfg)
        out.append(finish_file(args, q, r, elapsed, lam_tmp, has_temporal, shared=len(seqs)))
    return out


def evaluate_file(args, input_path, opt, encoder, temporal_pack, cfg, raw):
    return evaluate_files(args, [input_path], opt, encoder, temporal_pack, cfg, raw)[0]


def latent_tracks(clips, model_path=None, device="cuda:0", max_frames=None):
    """[T_i,24] latent tracks of .bvh clips for LatentAR.fit: the pose encoder's mu (dp_encode) of every frame, prepared as above"""
    from .encoder import NativePoseEncoder

    model_path = model_path if model_path is not None else DEFAULT_MODEL
    raw = load_model_arrays(model_path, skeleton_bvh=clips[0])
    means = {"dqs": raw["means.dqs"], "displacement": raw["means.displacement"]}
    stds = {"dqs": raw["stds.dqs"], "displacement": raw["stds.displacement"]}
    enc = NativePoseEncoder(arrays=raw, device=device)
    tracks = []
    for path in clips:
        m = prepare_motion(BVH().load(path), means, stds, HEIGHT_INDICES)
        dqs = torch.tensor(np.asarray(m["dqs"][:max_frames], np.float32), device=device)
        tracks.append(enc.encode(dqs, outputs=("mu",))["mu"].cpu().numpy())
    return tracks


def main(argv=None):
    ap = argparse.ArgumentParser(description="Evaluate DragPoser (HIP backend)")
    ap.add_argument("model_path", nargs="?", default=DEFAULT_MODEL,
                    help="path to pytorch model folder (generator.pt, data.pt[, temporal.pt]) as the reference takes it, or a model fixture (.npz); "
                         "default: the shipped model_dancedb")
    ap.add_argument("input_path", help=".bvh file or a directory of .bvh files")
    ap.add_argument("--config", default=None, help="tracker config JSON (same keys as the reference's config/*.json)")
    ap.add_argument("--temporal-checkpoint", default=None, help="temporal.pt as saved by the reference's train_temporal.py")
    ap.add_argument("--torch-temporal", action="store_true",
                    help="run the temporal target block with PyTorch ops around nn.Transformer instead of dp_temporal_predict (one HIP launch)")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--max-frames", type=int, default=None)
    ap.add_argument("--out-dir", default="data")
    ap.add_argument("--keep-frames", action="store_true", help="callers of main(): also return the per-frame poses / global positions / iteration counts")
    ap.add_argument("--initial-latent", default=None,
                    help=".npy with the 24 numbers of the initial latent (instead of encoder(mu, logvar) + a seeded normal draw): for parity runs against "
                         "a recorded reference run, whose own draw depends on how much of torch's global generator its constructors consumed")
    ap.add_argument("--per-frame", action="store_true",
                    help="drive the frame loop from the host, one DragPose.run (two launches) per frame, as the reference does (default: the "
                         "frame loop runs on the device, DragPose.run_frames; same results)")
    ap.add_argument("--constraints", choices=("reference",), default=None,
                    help="add the reference's extra loss terms (the `# Additional Losses` block of DragPose.loss, every weight 1) to every frame's "
                         "loss: DragPose.run_frames(constraints=Constraints.reference()) -- the frame loop still in one launch per stretch --, or "
                         "with --per-frame DragPose.run(constraints=...), two launches per frame; same results -- for a BVH with the model's own skeleton: "
                         "run() does not route other bones together with constraints and raises, run_frames() takes them")
    ap.add_argument("--foot-lock", action="store_true",
                    help="hold joints 4 and 8 where they touched down: two horizontal soft pins (point-DISTANCE terms, lo = hi = 0, the up "
                         "component dropped) whose points are latched from the reconstruction itself (DragPose.run_frames(terms=, holds=), "
                         "include/dragposer_holds.h; with --per-frame DragPose.run(terms=, holds=), same results); with --constraints reference "
                         "they are appended to Terms.from_constraints(Constraints.reference()).  Prints one extra line, the foot skate.  The "
                         "defaults of the four options below are placeholders nobody has tuned: the best of the few settings tried on the "
                         "shipped example clips (DESIGN.md section 13d), where they do not lower the skate without raising the position error")
    ap.add_argument("--foot-lock-weight", type=float, default=1.0, help="weight of each of the two pins (placeholder default, untuned)")
    ap.add_argument("--contact-height", type=float, nargs=2, default=(0.03, 0.06), metavar=("LO", "HI"),
                    help="touch-down at or below LO, release above HI, heights above --floor-level (placeholder defaults, untuned)")
    ap.add_argument("--floor-level", type=float, default=-1.0,
                    help="the floor along the up axis (placeholder default, untuned: the shipped example clips' toes rest near -1.0)")
    ap.add_argument("--up-axis", type=int, choices=(0, 1, 2), default=2,
                    help="the axis heights are measured along and the pins drop (default z, the shipped example clips' up; --constraints "
                         "reference keeps its own, y)")
    ap.add_argument("--tether", action="append", default=None, metavar="J:HI:WEIGHT[:ALPHA]",
                    help="tie joint J to its own recent path: a point-DISTANCE term on it (lo = 0, hi = HI metres per frame free, weight WEIGHT) whose "
                         "point follows the joint's own reconstructed position, extrapolated by ALPHA times the last frame's motion (default 0) "
                         "(DragPose.run_frames(terms=, tethers=), include/dragposer_tethers.h; with --per-frame DragPose.run(terms=, tethers=), same "
                         "results).  Up to four times; the terms are appended to --foot-lock's and --constraints reference's table.  Prints the foot "
                         "skate line and one more, the jitter of the result beside the ground truth's own.  No default: nobody has tuned one "
                         "(DESIGN.md section 13h)")
    ap.add_argument("--balance", default=None, metavar="RADIUS:WEIGHT",
                    help="keep the centre of mass over the feet: one DISTANCE term (the up component dropped, lo = 0, hi = RADIUS metres, weight "
                         "WEIGHT) between the centroid of all 22 joints and the midpoint of joints 4 and 8 -- two points of "
                         "include/dragposer_points.h (DragPose.run_frames(terms=Terms(..., points=)); with --per-frame DragPose.run, same results).  "
                         "Alone or appended to --constraints reference's table; not together with --foot-lock, --tether, --latent-ar or --gaps "
                         "(a table with points takes none of those layers).  Prints its settings and the foot skate line.  No default: "
                         "single runs on the shipped clips favour a wide radius at a small weight (0.2:0.1), which nobody has repeated "
                         "(DESIGN.md section 13i)")
    ap.add_argument("--balance-masses", default=None, metavar="FILE",
                    help="--balance: 22 numbers (white space or commas), the joints' masses for the centroid, normalised to sum 1 (default: uniform)")
    ap.add_argument("--latent-ar", default=None, metavar="hold | cv[:DAMPING] | FILE.npz",
                    help="without a temporal checkpoint: pull the latent towards a linear autoregressive prediction from the sequence's own "
                         "recent latents, with the configuration's lambda_temporal instead of 0 (DragPose.run_frames(ar=), "
                         "include/dragposer_latent_ar.h; with --per-frame DragPose.run(ar=), same results).  hold: the last latent; cv: constant "
                         "velocity, optionally damped; FILE.npz: a model fitted by `python -m dragposer_amd.ar fit`")
    ap.add_argument("--drop", default=None, metavar="J:START:LEN[,...]",
                    help="blank the samples of tracker joint J on frames START .. START + LEN of the synthesised targets (NaN, as a tracker out of "
                         "view sends them); the position errors are then also printed over the blanked frames alone.  Without --gaps the clip ends "
                         "at the first blanked frame: every later result is NaN (DP_STATUS_BAD_STATE)")
    ap.add_argument("--gaps", default=None, metavar="MAX_HOLD:DECAY",
                    help="keep going through missing samples: a tracker whose sample is NaN is held at its last good sample for up to MAX_HOLD "
                         "frames at a weight that decays by DECAY per frame, and leaves the loss after that until it returns "
                         "(DragPose.run_frames(gaps=), include/dragposer_gaps.h; with --per-frame DragPose.run(gaps=), same results).  No default: "
                         "nobody has tuned one")
    ap.add_argument("--solver", default=None, metavar="lm[:STEPS]",
                    help="solve every frame by Levenberg-Marquardt steps (default 3) instead of Adam: DragPose.run_frames(solver=LM(STEPS)), the frame "
                         "loop on the device (dp_optimize_sequence_lm, include/dragposer_sequence_lm.h); with --per-frame DragPose.run(solver=), "
                         "dp_optimize_lm followed by dp_sequence_advance per frame, same results.  With --latent-ar the predictor becomes the "
                         "solver's (LM.predictor) and the configuration's lambda_temporal pulls towards its targets.  With --constraints reference "
                         "the reference's extra terms join the LM loss as the solver's table, LM(terms=Terms.from_constraints(Constraints.reference())) "
                         "(dp_optimize_sequence_lm_terms, include/dragposer_sequence_lm_terms.h; --per-frame: dp_optimize_lm_terms).  Not with "
                         "--foot-lock, --tether, --balance or --gaps, and for a BVH with the model's own skeleton")
    ap.add_argument("--smooth", default=None, metavar="LAMBDA[:STEPS[:ANCHOR]]",
                    help="after the clip's normal pass, a second pass over all its frames as ONE sequence solved jointly, the latents tied frame to "
                         "frame by LAMBDA |z_t - z_(t-1)|^2 / 24 inside the loss (LatentOptimizer.optimize_clip_lm, include/dragposer_clip_lm.h): "
                         "STEPS joint Levenberg-Marquardt steps (default 4) from the first pass's latents, each frame under the root rotation and "
                         "position the first pass left before it, with a pull of weight ANCHOR (default 0) towards the first pass's latent.  "
                         "Prints MPJPE and jitter before and after beside the ground truth's jitter and writes eval_smooth_<name>.  No default "
                         "LAMBDA: none has been found that helps on every clip.  Allowed after --solver and --latent-ar; not with --constraints, "
                         "--foot-lock, --tether, --balance, --gaps, --drop, --calibrate or --model-skeleton.  A BVH with another skeleton than "
                         "the model's runs the joint pass on its own bones (dp_optimize_clip_lm_skeleton, include/dragposer_clip_skeleton.h)")
    ap.add_argument("--smooth-accel", default=None, metavar="ACCEL",
                    help="with --smooth: ACCEL |z_(t+1) - 2 z_t + z_(t-1)|^2 / 24 joins the second pass's loss, an acceleration penalty beside "
                         "--smooth's velocity penalty (dp_optimize_clip_lm_accel, include/dragposer_clip_accel.h); --smooth 0:4 --smooth-accel 5 is "
                         "the acceleration-only pass.  No default: none has been found that helps on every clip")
    ap.add_argument("--calibrate", default=None, metavar="GROUPS[:FRAMES[:ROUNDS]]",
                    help="a performer without a BVH file: ignore the clip's OFFSET table for the optimisation and fit the bone lengths from the "
                         "tracker targets first -- GROUPS uniform | limbs | symmetric | per_bone (dragposer_amd.BoneGroups), FRAMES frames drawn "
                         "evenly from the clip (default 256) as independent frames, ROUNDS rounds (default 6) of 50 iterations and one dp_fit_bones "
                         "each (dragposer_amd.calibrate, include/dragposer_calibration.h) -- then run the clip with the fitted offsets.  Prints "
                         "the fitted scales beside the clip's true bone-length ratios.  Not with --solver")
    ap.add_argument("--model-skeleton", action="store_true",
                    help="ignore the clip's OFFSET table for the optimisation and run on the model's own skeleton (what --calibrate starts from); "
                         "the targets remain those of the clip's skeleton.  Not with --calibrate or --solver")
    ap.add_argument("--lockstep", action="store_true",
                    help="directory input: advance all files together, one kernel launch per frame index for all of them "
                         "(same per-file results; the reference evaluates them one after the other)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eval_drag needs a ROCm GPU: dragposer_amd has no CPU fallback")
    cfg = dict(DEFAULT_CONFIG)
    if args.config is not None:
        with open(args.config) as f:
            cfg = json.load(f)
    files = [args.input_path]
    if os.path.isdir(args.input_path):
        files = sorted(os.path.join(args.input_path, f) for f in os.listdir(args.input_path) if f.endswith(".bvh"))
        if not files:
            raise SystemExit(f"{args.input_path}: no .bvh files")
    raw = load_model_arrays(args.model_path, skeleton_bvh=files[0])  # (a model folder carries no skeleton: the evaluated BVH's, train.py:329-341)
    opt = LatentOptimizer(device=args.device, arrays=raw)
    encoder = PoseEncoder(arrays=raw).to(opt.device)
    tck = args.temporal_checkpoint
    if tck is None and os.path.isdir(args.model_path) and os.path.exists(os.path.join(args.model_path, "temporal.pt")):
        tck = os.path.join(args.model_path, "temporal.pt")  # train_temporal.load_model (train_temporal.py:474-482)
    if tck is not None:
        temporal_pack = load_reference_checkpoint(tck, opt.device)
    else:
        temporal_pack = (None, np.zeros(24, np.float32), np.ones(24, np.float32))
    if args.latent_ar is not None:
        if tck is not None:
            raise SystemExit("--latent-ar and a temporal checkpoint are two sources of the pull term's target: give one")
        from .ar import parse

        args.latent_ar_model, args.latent_ar_text = parse(args.latent_ar)
    args.tether_specs = parse_tethers(args.tether) if args.tether else None
    args.balance_spec = None
    if args.balance_masses is not None and args.balance is None:
        raise SystemExit("--balance-masses belongs to --balance")
    if args.balance is not None:
        for flag, given in (("--foot-lock", args.foot_lock), ("--tether", args.tether), ("--latent-ar", args.latent_ar), ("--gaps", args.gaps)):
            if given:
                raise SystemExit(f"--balance and {flag}: a table with points takes no holds, tethers, latent predictor or gaps (include/dragposer_points.h)")
        args.balance_spec = parse_balance(args.balance, args.balance_masses)
    args.calibrate_spec = None
    if args.calibrate is not None or args.model_skeleton:
        if args.solver is not None:
            raise SystemExit("--calibrate / --model-skeleton and --solver: the LM solver runs on the context's skeleton only (include/dragposer_lm.h, Not covered)")
        if args.calibrate is not None and args.model_skeleton:
            raise SystemExit("--calibrate and --model-skeleton: give one")
    if args.calibrate is not None:
        parts = args.calibrate.split(":")
        try:
            if not 1 <= len(parts) <= 3 or parts[0] not in ("uniform", "limbs", "symmetric", "per_bone"):
                raise ValueError("GROUPS is uniform, limbs, symmetric or per_bone")
            args.calibrate_spec = (parts[0], int(parts[1]) if len(parts) > 1 else 256, int(parts[2]) if len(parts) > 2 else 6)
            if args.calibrate_spec[1] < 1 or args.calibrate_spec[2] < 1:
                raise ValueError("FRAMES and ROUNDS are positive")
        except ValueError as e:
            raise SystemExit(f"--calibrate: expected GROUPS[:FRAMES[:ROUNDS]], got {args.calibrate!r} ({e})")
    args.solver_model = None
    if args.solver is not None:
        from .lm import LM

        name, _, steps = args.solver.partition(":")
        try:
            if name != "lm":
                raise ValueError("unknown solver " + repr(name))
            args.solver_model = LM(steps=int(steps) if steps else 3).check()
        except ValueError as e:
            raise SystemExit(f"--solver: expected lm[:STEPS] with 1 <= STEPS <= 64 ({e})")
        for flag, given in (("--foot-lock", args.foot_lock), ("--tether", args.tether), ("--balance", args.balance), ("--gaps", args.gaps)):
            if given:
                raise SystemExit(f"--solver and {flag}: the LM loss has the trackers, the pull and --constraints reference's table only "
                                 "(include/dragposer_lm.h, Not covered)")
        if args.latent_ar is not None:
            args.solver_model.predictor = args.latent_ar_model
        print(f"Solver: Levenberg-Marquardt, {args.solver_model.steps} steps per frame (DragPose.{'run' if args.per_frame else 'run_frames'}(solver=), "
              f"include/dragposer_{'lm' if args.per_frame else 'sequence_lm'}{'_terms' if args.constraints else ''}.h)")
    args.smooth_spec = None
    if args.smooth is not None:
        from .clip import ClipLM

        for flag, given in (("--constraints", args.constraints), ("--foot-lock", args.foot_lock), ("--tether", args.tether), ("--balance", args.balance),
                            ("--gaps", args.gaps), ("--drop", args.drop), ("--calibrate", args.calibrate)):
            if given:
                raise SystemExit(f"--smooth and {flag}: the clip loss has the trackers, the anchor and the coupling only (include/dragposer_clip_lm.h, Not covered)")
        if args.model_skeleton:
            raise SystemExit("--smooth and --model-skeleton: the joint pass runs on the context's skeleton only (include/dragposer_clip_lm.h, Not covered)")
        parts = args.smooth.split(":")
        try:
            if not 1 <= len(parts) <= 3:
                raise ValueError("one to three fields")
            anchor = float(parts[2]) if len(parts) > 2 else 0.0
            if not (anchor >= 0.0 and anchor < float("inf")):
                raise ValueError("ANCHOR is negative or not finite")
            args.smooth_spec = (ClipLM(steps=int(parts[1]) if len(parts) > 1 and parts[1] else 4, smooth=float(parts[0])).check(), anchor)
        except ValueError as e:
            raise SystemExit(f"--smooth: expected LAMBDA[:STEPS[:ANCHOR]] with LAMBDA >= 0, 1 <= STEPS <= 64 and ANCHOR >= 0 ({e})")
    if args.smooth_accel is not None:
        if args.smooth_spec is None:
            raise SystemExit("--smooth-accel requires --smooth (--smooth 0:4 --smooth-accel 5 is the acceleration-only pass)")
        try:
            args.smooth_spec[0].accel = float(args.smooth_accel)
            args.smooth_spec[0].check()
        except ValueError as e:
            raise SystemExit(f"--smooth-accel: expected ACCEL >= 0 and finite ({e})")
    args.gaps_model = None
    if args.gaps is not None:
        from .gaps import Gaps

        try:
            hold, decay = args.gaps.split(":")
            args.gaps_model = Gaps(int(hold), float(decay))
            args.gaps_model.check()
        except ValueError as e:
            raise SystemExit(f"--gaps: expected MAX_HOLD:DECAY with 0 <= MAX_HOLD <= 65535 and 0 < DECAY <= 1 ({e})")
    if args.lockstep and len(files) > 1:
        print(f"Evaluate {len(files)} files in lock-step ------------------------")
        return evaluate_files(args, files, opt, encoder, temporal_pack, cfg, raw)
    results = []
    for f in files:
        print(f"Evaluate {f} ------------------------")
        results.append(evaluate_file(args, f, opt, encoder, temporal_pack, cfg, raw))
    return results


if __name__ == "__main__":
    main()

"""Kernel times of dp_optimize_clip_lm (include/dragposer_clip_lm.h), split rows / chain / decision, beside
dp_optimize_sequence_lm's on the same clip in the same run.  Per shape (S, T) one profiled child process, no counters in it --
    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python tools/time_clip_lm.py --worker S T
-- which prepares the clip as eval_drag does (6 trackers; S copies in lock-step), runs the first pass DragPose.run_frames(solver=LM(3)) and then
`--rounds` + 1 calls of LatentOptimizer.optimize_clip_lm (3 steps, lambda_smooth 5) from its latents.  The parent reads the kernel trace: a call
is a fixed train of launches (dp_clip.hip: dp_launch_clip), so each launch's part is known from its place in the train.  Per part: the
median over the calls (the first left out) of the part's summed kernel time, (max - min) / median, and the same per step.
    python tools/time_clip_lm.py [--out profiles/clip_lm_times.txt]
Shapes: (1, 240) and (64, 240) on tests/data/example_clip.bvh, (1, 5052) on the example (tests/data/_local/example.bvh).
    python tools/time_clip_lm.py --accel 5 [--out profiles/clip_accel_times.txt]
also runs, in the same processes and after those calls, as many of dp_optimize_clip_lm_accel (include/dragposer_clip_accel.h, DESIGN.md section
18a: lambda_smooth 0, lambda_accel ACCEL) and reports both trains and the ratio of the two chains.
    python tools/time_clip_lm.py --skeleton [--out profiles/clip_skel_times.txt]
also runs, in the same processes and after the plain calls, as many of dp_optimize_clip_lm_skeleton (include/dragposer_clip_skeleton.h, DESIGN.md
section 18b) on the same clip with the context's own offsets passed per sequence (stride 66: the same problem and the same bits, so the two trains
do the same work), and reports both trains and, per part, the skeleton call's time over the plain call's with both spreads."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, SMOOTH = 3, 5.0
SHAPES = ((1, 240), (64, 240), (1, 5052))


def train(steps):
    """the parts of one call's launches, in order (dp_launch_clip)"""
    t = ["rows: z0's pass, A | g", "decision"]
    for k in range(steps):
        t += (["rows: A | g"] if k else []) + ["chain", "rows: trial", "decision"]
    return t + ["rows: results"]


def worker(S, T, rounds, accel=None, skeleton=False):
    import torch

    sys.path.insert(0, ROOT)
    from dragposer_amd import LM, ClipLM, eval_drag
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.encoder import PoseEncoder
    from dragposer_amd.model import DEFAULT_MODEL, load_model_arrays
    from dragposer_amd.optimizer import LatentOptimizer

    dev = torch.device("cuda:0")
    clip = os.path.join(ROOT, "tests", "data", "example_clip.bvh") if T <= 240 else os.path.join(ROOT, "tests", "data", "_local", "example.bvh")
    raw = load_model_arrays(DEFAULT_MODEL, skeleton_bvh=clip)
    opt = LatentOptimizer(device=dev, arrays=raw)
    cfg = dict(eval_drag.DEFAULT_CONFIG)
    q = eval_drag.prepare_file(argparse.Namespace(max_frames=T, drop=None, initial_latent=None), clip, opt, PoseEncoder(arrays=raw).to(dev), cfg, raw)
    assert int(q["n_frames"]) == T
    mask_idx = np.nonzero(np.asarray(cfg["mask"]))[0]
    weights = np.asarray(cfg["weights"], np.float32)[mask_idx]
    ja = tuple(cfg["joint_adjustment_indices"]) if cfg["enable_joint_adjustment"] else None
    rep = lambda t: t.unsqueeze(1).expand(t.shape[0], S, *t.shape[1:]).contiguous()
    tp_rel, tR, gpos = rep(q["tp_rel"][:T]), rep(q["tR"][:T]), rep(q["gpos"][:T])
    drag = DragPose(opt, None, np.zeros(24, np.float32), np.ones(24, np.float32), n_sequences=S)
    drag.keep_latents = True
    poses = pos = None
    for _ in range(rounds + 1):  # the first pass, the per-frame LM solver with the frame loop on the device
        drag.set_initial_state(q["z0"].expand(S, 24).contiguous(), np.repeat(q["m"]["global_pos"][0][None], S, 0),
                               np.repeat(q["m"]["global_rot"][0][None], S, 0), np.repeat(q["m"]["heights"][0][None], S, 0))
        poses, pos, _ = drag.run_frames(tp_rel, tR.reshape(T, S, -1, 3, 3), mask_idx, weights, target_root=gpos, solver=LM(STEPS), lambda_temporal=0.0,
                                        stop_eps_pos=1e-4, stop_eps_rot=1e-2, lambda_rot=1, temporal_future_window=0, height_indices=eval_drag.HEIGHT_INDICES,
                                        joint_adjustment_indices=ja, joint_adjustment_weight=cfg["joint_adjustment_weight"])
    torch.cuda.synchronize()
    # the second pass's batch, as eval_drag.smooth_file builds it, for all S copies: row t * S + s
    z = drag.last_latents.reshape(T * S, 24).contiguous()
    sd4 = torch.as_tensor(q["stds"]["dqs"].reshape(22, 8)[:, :4].reshape(88)[:4].astype(np.float32), device=dev)
    mu4 = torch.as_tensor(q["means"]["dqs"].reshape(22, 8)[:, :4].reshape(88)[:4].astype(np.float32), device=dev)
    rot0 = torch.as_tensor(np.repeat(np.asarray(q["m"]["global_rot"][0:1], np.float32)[None], S, 1), device=dev)
    pos0 = torch.as_tensor(np.repeat(np.asarray(q["m"]["global_pos"][0:1], np.float32)[None], S, 1), device=dev)
    rot_before = torch.cat((rot0, poses[:T - 1, :, :4] * sd4 + mu4)).reshape(T * S, 4).contiguous()
    pos_before = torch.cat((pos0, pos[:T - 1]))
    mt = torch.as_tensor(mask_idx, device=dev)
    tgt_pos = torch.zeros(T, S, 22, 3, device=dev)
    tgt_pos[:, :, mt] = tp_rel + (gpos - pos_before).unsqueeze(2)
    tgt_rot = torch.zeros(T, S, 22, 9, device=dev)
    tgt_rot[:, :, mt] = tR
    w = torch.zeros(T * S, 22, 2, device=dev)
    w[:, mt] = torch.as_tensor(weights, device=dev)
    tracked = torch.zeros(T * S, 22, dtype=torch.uint8, device=dev)
    tracked[:, mt] = 1
    for _ in range(rounds + 1):
        out = opt.optimize_clip_lm(z, z.clone(), rot_before, tgt_pos.reshape(T * S, 22, 3), tgt_rot.reshape(T * S, 22, 9), w, tracked, n_sequences=S,
                                   clip=ClipLM(steps=STEPS, smooth=SMOOTH), lambda_rot=1.0, lambda_tmp=0.0)
    torch.cuda.synchronize()
    print(f"WORKER S {S} T {T}: accepted {out['n_accepted'].tolist()[:4]}, sequence loss {out['loss_hist'][0].tolist()}", flush=True)
    if skeleton:
        own = torch.as_tensor(np.asarray(raw["offsets"], np.float32).reshape(1, 22, 3), device=dev).expand(S, 22, 3).contiguous()
        for _ in range(rounds + 1):
            sk = opt.optimize_clip_lm(z, z.clone(), rot_before, tgt_pos.reshape(T * S, 22, 3), tgt_rot.reshape(T * S, 22, 9), w, tracked, n_sequences=S,
                                      clip=ClipLM(steps=STEPS, smooth=SMOOTH), lambda_rot=1.0, lambda_tmp=0.0, offsets=own)
        torch.cuda.synchronize()
        print(f"WORKER S {S} T {T} offsets [{S}, 22, 3] (the context's own): accepted {sk['n_accepted'].tolist()[:4]}, sequence loss {sk['loss_hist'][0].tolist()}, "
              f"the plain call's bits: {bool(torch.equal(sk['z'], out['z']) and torch.equal(sk['loss_hist'], out['loss_hist']))}", flush=True)
    if accel is not None:
        for _ in range(rounds + 1):
            out = opt.optimize_clip_lm(z, z.clone(), rot_before, tgt_pos.reshape(T * S, 22, 3), tgt_rot.reshape(T * S, 22, 9), w, tracked, n_sequences=S,
                                       clip=ClipLM(steps=STEPS, smooth=0.0, accel=accel), lambda_rot=1.0, lambda_tmp=0.0)
        torch.cuda.synchronize()
        print(f"WORKER S {S} T {T} lambda_accel {accel:g}: accepted {out['n_accepted'].tolist()[:4]}, sequence loss {out['loss_hist'][0].tolist()}, "
              f"its second-difference part {out['accel_loss'].tolist()[:4]}", flush=True)


def summarise(path, S, T, rounds, lines, accel=None, skeleton=False):
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            rows.append((int(row["Start_Timestamp"]), row["Kernel_Name"], (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3))
    rows.sort()
    clip = [(n, d) for _, n, d in rows if "dp_clip_" in n]
    seq = np.asarray([d for _, n, d in rows if "dp_lm_seq_kernel" in n])
    parts = train(STEPS)
    n_train = (rounds + 1) * len(parts)
    assert len(clip) == n_train * (1 if accel is None and not skeleton else 2), (len(clip), len(parts))
    plain = {}
    chain = summarise_train(clip[:n_train], f"lambda_smooth {SMOOTH}", S, T, rounds, lines, plain)
    if skeleton:  # the second half of the trace: the same train with dp_clip_skel.hip's rows kernel, the chain and the decision as they are
        assert all(("skel" in n) == ("rows" in n) for n, _ in clip[n_train:]) and not any("skel" in n for n, _ in clip[:n_train])
        skel = {}
        summarise_train(clip[n_train:], f"lambda_smooth {SMOOTH}, offsets [{S}, 22, 3] (dp_optimize_clip_lm_skeleton)", S, T, rounds, lines, skel)
        spread = lambda v: (v.max() - v.min()) / np.median(v)
        for name, keys in (("rows kernel, all four passes", [k for k in plain if k.startswith("rows")]), ("chain", ["chain"]), ("decision", ["decision"])):
            a, b = sum(skel[k] for k in keys), sum(plain[k] for k in keys)
            lines.append(f"  {name}, dp_optimize_clip_lm_skeleton / dp_optimize_clip_lm: {np.median(a) / np.median(b):.4f}  (medians {np.median(a):.2f} / {np.median(b):.2f} "
                         f"microseconds per call; (max - min) / median {spread(a):.4f} / {spread(b):.4f})")
    if accel is not None:  # the second half of the trace: the same train, dp_clip_accel.hip's chain and decision in their places
        assert all(("accel" in n) == (("chain" in n) or ("decide" in n)) for n, _ in clip[n_train:])
        chain_accel = summarise_train(clip[n_train:], f"lambda_smooth 0, lambda_accel {accel:g} (dp_optimize_clip_lm_accel)", S, T, rounds, lines)
        lines.append(f"  chain, dp_optimize_clip_lm_accel / dp_optimize_clip_lm: {chain_accel / chain:.3f}  ({chain_accel / STEPS / T:.2f} against {chain / STEPS / T:.2f} "
                     "microseconds per frame per step)")
    if len(seq) > 1:
        v = seq[1:]
        lines.append(f"  dp_lm_seq_kernel (dp_optimize_sequence_lm, LM({STEPS}), the same clip, this run) n {len(v)}  median {np.median(v):11.2f}  "
                     f"(max - min) / median {(v.max() - v.min()) / np.median(v):.4f}  per frame of a sequence {np.median(v) / T:8.3f}")


def summarise_train(clip, label, S, T, rounds, lines, keep=None):
    """one entry point's calls (the first left out) -> lines; returns the chain's median time per call (keep: a dict that takes every part's
    times per call)"""
    parts = train(STEPS)
    lines.append(f"(S, T) = ({S}, {T}): {rounds} calls of {STEPS} steps, {label}; kernel time per call, microseconds")
    total = np.zeros(rounds)
    chain = 0.0
    for part in ("rows: z0's pass, A | g", "rows: A | g", "rows: trial", "rows: results", "chain", "decision"):
        idx = [i for i, p in enumerate(parts) if p == part]
        want = "rows" if part.startswith("rows") else "chain" if part == "chain" else "decide"
        per_call = []
        for c in range(1, rounds + 1):
            chunk = clip[c * len(parts):(c + 1) * len(parts)]
            assert all(want in chunk[i][0] for i in idx), (part, [chunk[i][0] for i in idx])
            per_call.append(sum(chunk[i][1] for i in idx))
        v = np.asarray(per_call)
        total += v
        if keep is not None:
            keep[part] = v
        if part == "chain":
            chain = float(np.median(v))
        lines.append(f"  {part:24s} launches {len(idx)}  median {np.median(v):11.2f}  (max - min) / median {(v.max() - v.min()) / np.median(v):.4f}  "
                     f"per launch {np.median(v) / len(idx):10.2f}  per launch and frame {np.median(v) / len(idx) / T:8.3f}")
    lines.append(f"  {'the call':24s} launches {len(parts)}  median {np.median(total):11.2f}  (max - min) / median {(total.max() - total.min()) / np.median(total):.4f}  "
                 f"per step {np.median(total) / STEPS:10.2f}  per step and frame of a sequence {np.median(total) / STEPS / T:8.3f}")
    return chain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", type=int, nargs=2, default=None, metavar=("S", "T"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--accel", type=float, default=None, metavar="ACCEL", help="also time dp_optimize_clip_lm_accel at lambda_smooth 0, lambda_accel ACCEL (> 0)")
    ap.add_argument("--skeleton", action="store_true", help="also time dp_optimize_clip_lm_skeleton on the same clip, the context's own offsets passed per sequence")
    ap.add_argument("--out", default=None, help="default: profiles/clip_lm_times.txt, with --accel profiles/clip_accel_times.txt, with --skeleton profiles/clip_skel_times.txt")
    args = ap.parse_args()
    if args.accel is not None and not args.accel > 0:
        raise SystemExit("--accel: expected ACCEL > 0 (0 runs dp_optimize_clip_lm's own train)")
    if args.accel is not None and args.skeleton:
        raise SystemExit("--accel and --skeleton: one comparison per run")
    if args.worker:
        return worker(args.worker[0], args.worker[1], args.rounds, args.accel, args.skeleton)
    args.out = args.out or os.path.join(ROOT, "profiles", "clip_skel_times.txt" if args.skeleton else "clip_lm_times.txt" if args.accel is None else "clip_accel_times.txt")
    lines = [("dp_optimize_clip_lm and dp_optimize_clip_lm_skeleton, the same processes" if args.skeleton else
              "dp_optimize_clip_lm" if args.accel is None else "dp_optimize_clip_lm and dp_optimize_clip_lm_accel, the same processes")
             + ": kernel times from rocprofv3 --kernel-trace --stats, one profiled process per shape (tools/time_clip_lm.py)"]
    for S, T in SHAPES:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                   "--worker", str(S), str(T), "--rounds", str(args.rounds)] + (["--accel", str(args.accel)] if args.accel is not None else []) + (["--skeleton"] if args.skeleton else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
            if r.returncode != 0:
                raise SystemExit(f"({S}, {T}): the profiled process ended with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            found = glob.glob(os.path.join(d, "**", "t_kernel_trace.csv"), recursive=True)
            if len(found) != 1:
                raise SystemExit(f"({S}, {T}): expected one kernel trace under {d}, found {found}")
            summarise(found[0], S, T, args.rounds, lines, args.accel, args.skeleton)
            lines += ["  " + l for l in r.stdout.splitlines() if l.startswith("WORKER")]
        print("\n".join(lines[-24:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

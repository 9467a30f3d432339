"""Times DragPose.run_frames(solver=LM(3)) -- the frame loop on the device, dp_optimize_sequence_lm (include/dragposer_sequence_lm.h) -- on the
frames of tests/data/example_clip.bvh (eval_drag's own preparation, 6 trackers, S copies of the clip in lock-step) against
  loop   the host loop over DragPose.run(solver=): dp_optimize_lm + dp_sequence_advance per frame (what run_frames(solver=) was before)
  adam   DragPose.run_frames without a solver: dp_optimize_sequence, Adam with the reference's early stop
  seq    the new launch;  seq_hold: the same with LM(3, predictor=LatentAR.hold()) and the configuration's lambda_temporal
Each variant runs `--rounds` times per size from the same initial state, the variants alternating (A B C A B C ...); a round is timed on the
host between two synchronisations, so the figure is what a caller waits for, launches included: microseconds per frame, median and
(max - min) / median.  `--tree PATH` imports dragposer_amd from another built checkout (the parent commit's, for dp_lm_kernel's own time there:
`--variants loop`).
Kernel times come from a run of its own under the profiler, no counters in it --
    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python tools/time_lm_sequence.py --rounds 7
    python tools/time_lm_sequence.py --summarise DIR/.../t_kernel_trace.csv
per kernel and grid size (S = 1: one workgroup; S = 64: 16): the launches' count, median, (max - min) / median and total."""
import argparse
import csv
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = ("dp_lm_seq_kernel", "dp_lm_kernel", "dp_sequence_advance_kernel", "dp_sequence_history_kernel", "dp_w4")


def summarise(path):
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = next((k for k in KERNELS if k in row["Kernel_Name"]), None)
            if name is not None:
                grid = int(row.get("Grid_Size", row.get("Grid_Size_X", 0)) or 0)
                groups.setdefault((name, grid), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    for (name, grid), v in sorted(groups.items()):
        v = np.asarray(v)
        print(f"{name:28s} grid {grid:6d}  n {len(v):6d}  median {np.median(v):10.2f} us  min {v.min():10.2f}  max {v.max():10.2f}  "
              f"(max - min) / median {(v.max() - v.min()) / np.median(v):.4f}  total {v.sum() * 1e-3:10.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 64])
    ap.add_argument("--frames", type=int, default=256, help="at most this many frames of the clip (it has 240)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--variants", nargs="*", default=["seq", "loop", "adam", "seq_hold"])
    ap.add_argument("--tree", default=ROOT, help="the built checkout whose dragposer_amd is imported (default: this one)")
    ap.add_argument("--summarise", default=None, metavar="KERNEL_TRACE_CSV", help="summarise a rocprofv3 kernel trace of this tool and exit")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    sys.path.insert(0, os.path.abspath(args.tree))
    from dragposer_amd import LM, LatentAR, eval_drag
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.encoder import PoseEncoder
    from dragposer_amd.model import DEFAULT_MODEL, load_model_arrays
    from dragposer_amd.optimizer import LatentOptimizer

    dev = torch.device("cuda:0")
    clip = os.path.join(ROOT, "tests", "data", "example_clip.bvh")
    raw = load_model_arrays(DEFAULT_MODEL, skeleton_bvh=clip)
    opt = LatentOptimizer(device=dev, arrays=raw)
    cfg = dict(eval_drag.DEFAULT_CONFIG)
    q = eval_drag.prepare_file(argparse.Namespace(max_frames=args.frames, drop=None, initial_latent=None), clip, opt, PoseEncoder(arrays=raw).to(dev), cfg, raw)
    T = int(q["n_frames"])
    mask_idx = np.nonzero(np.asarray(cfg["mask"]))[0]
    weights = np.asarray(cfg["weights"], np.float32)[mask_idx]
    ja = tuple(cfg["joint_adjustment_indices"]) if cfg["enable_joint_adjustment"] else None
    kw = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2, lambda_rot=1, temporal_future_window=0, height_indices=eval_drag.HEIGHT_INDICES,
              joint_adjustment_indices=ja, joint_adjustment_weight=cfg["joint_adjustment_weight"])
    print(f"{os.path.basename(clip)}: {T} frames, {len(mask_idx)} trackers, dragposer_amd of {os.path.abspath(args.tree)}", flush=True)
    for S in args.sizes:
        rep = lambda t: t.unsqueeze(1).expand(t.shape[0], S, *t.shape[1:]).contiguous()
        tp_rel, tR, gpos = rep(q["tp_rel"][:T]), rep(q["tR"][:T]), rep(q["gpos"][:T])
        drag = DragPose(opt, None, np.zeros(24, np.float32), np.ones(24, np.float32), n_sequences=S)

        def begin():
            drag.set_initial_state(q["z0"].expand(S, 24).contiguous(), np.repeat(q["m"]["global_pos"][0][None], S, 0),
                                   np.repeat(q["m"]["global_rot"][0][None], S, 0), np.repeat(q["m"]["heights"][0][None], S, 0))

        def frames(**extra):
            return drag.run_frames(tp_rel, tR.reshape(T, S, -1, 3, 3), mask_idx, weights, target_root=gpos, max_iter=100, learning_rate=1e-2, **kw, **extra)

        def loop():
            for t in range(T):
                tp = tp_rel[t] + (gpos[t] - drag.current_global_pos).unsqueeze(1)
                drag.run(tp, tR[t], mask_idx, weights, solver=LM(3), lambda_temporal=0.0, **kw)

        runs = {"seq": lambda: frames(solver=LM(3), lambda_temporal=0.0), "loop": loop, "adam": lambda: frames(lambda_temporal=0.0),
                "seq_hold": lambda: frames(solver=LM(3, predictor=LatentAR.hold()), lambda_temporal=cfg["lambda_temporal"])}
        times = {v: [] for v in args.variants}
        for r in range(args.rounds + 1):  # (round 0: warm-up, not counted)
            for v in args.variants:
                begin()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                runs[v]()
                torch.cuda.synchronize()
                if r > 0:
                    times[v].append((time.perf_counter() - t0) * 1e6 / T)
        for v in args.variants:
            x = np.asarray(times[v])
            print(f"S {S:3d}  {v:9s} n {len(x)}  median {np.median(x):9.2f} us / frame  min {x.min():9.2f}  max {x.max():9.2f}  "
                  f"(max - min) / median {(x.max() - x.min()) / np.median(x):.4f}", flush=True)


if __name__ == "__main__":
    main()

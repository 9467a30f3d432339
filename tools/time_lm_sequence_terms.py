"""Times dp_optimize_sequence_lm_terms (include/dragposer_sequence_lm_terms.h) -- the LM frame loop on the device with a term table in its
loss -- on the frames of tests/data/example_clip.bvh (eval_drag's own preparation, 6 trackers, S copies of the clip in lock-step, target_root
honoured) against
  loop       the host loop it replaces: LatentOptimizer.optimize_lm(terms=, global_pos=the running position) + sequence_advance + the latent
             copy per frame, with the targets shifted on the host (two launches per frame; the parent commit has both calls: `--tree`)
  seq        dp_optimize_sequence_lm, the same clip without a table
  adam       dp_optimize_sequence_terms: Adam with the reference's early stop (up to 100 iterations) on the same table
  seq_terms  the new launch
for the tables `custom` (tests/test_hip_terms.py's CUSTOM(), 3 terms) and `mixed16` (tests/lm_terms_oracle.py's 16 terms, its per-frame rows
[S,4] held) and the solvers `lm6` = LM(6, early_stop=False) and `lm3` = LM(3).  Each variant runs `--rounds` times per size from the same
initial state, the variants alternating; a round is timed on the host between two synchronisations, so the figure is what a caller waits for,
launches included: microseconds per frame, median and (max - min) / median.  `--tree PATH` imports dragposer_amd from another built checkout
(the parent commit's: `--variants loop seq adam`).
Kernel times come from a run of its own under the profiler, no counters in it --
    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python tools/time_lm_sequence_terms.py --rounds 7
    python tools/time_lm_sequence_terms.py --summarise DIR/.../t_kernel_trace.csv
per kernel and grid size: the launches' count, median, (max - min) / median and total."""
import argparse
import csv
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = ("dp_lm_seq_terms_kernel", "dp_lm_seq_kernel", "dp_lm_terms_kernel", "dp_lm_kernel", "dp_terms_seq_kernel", "dp_sequence_advance_kernel",
           "dp_sequence_history_kernel")


def summarise(path):
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = next((k for k in KERNELS if k in row["Kernel_Name"]), None)
            if name is None and "dp_" in row["Kernel_Name"]:
                name = row["Kernel_Name"].split("(")[0][:40]
            if name is not None:
                grid = int(row.get("Grid_Size", row.get("Grid_Size_X", 0)) or 0)
                groups.setdefault((name, grid), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    for (name, grid), v in sorted(groups.items()):
        v = np.asarray(v)
        print(f"{name:40s} grid {grid:6d}  n {len(v):6d}  median {np.median(v):10.2f} us  min {v.min():10.2f}  max {v.max():10.2f}  "
              f"(max - min) / median {(v.max() - v.min()) / np.median(v):.4f}  total {v.sum() * 1e-3:10.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 64])
    ap.add_argument("--frames", type=int, default=256, help="at most this many frames of the clip (it has 240)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--variants", nargs="*", default=["seq_terms", "loop", "seq", "adam"])
    ap.add_argument("--tables", nargs="*", default=["custom", "mixed16"])
    ap.add_argument("--solvers", nargs="*", default=["lm6", "lm3"])
    ap.add_argument("--tree", default=ROOT, help="the built checkout whose dragposer_amd is imported (default: this one)")
    ap.add_argument("--summarise", default=None, metavar="KERNEL_TRACE_CSV", help="summarise a rocprofv3 kernel trace of this tool and exit")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    sys.path.insert(0, os.path.join(ROOT, "tests"))  # (the tables: this checkout's, whichever package runs them)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.abspath(args.tree))
    from dataclasses import replace

    import lm_terms_oracle as LT
    from dragposer_amd import LM, eval_drag
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
    heights = tuple(int(h) for h in eval_drag.HEIGHT_INDICES)
    kw = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2, lambda_rot=1, temporal_future_window=0, height_indices=eval_drag.HEIGHT_INDICES,
              joint_adjustment_indices=ja, joint_adjustment_weight=cfg["joint_adjustment_weight"])
    solvers = {"lm6": LM(6, early_stop=False), "lm3": LM(3)}
    print(f"{os.path.basename(clip)}: {T} frames, {len(mask_idx)} trackers, dragposer_amd of {os.path.abspath(args.tree)}", flush=True)
    for S in args.sizes:
        rep = lambda t: t.unsqueeze(1).expand(t.shape[0], S, *t.shape[1:]).contiguous()
        tp_rel, tR, gpos = rep(q["tp_rel"][:T]), rep(q["tR"][:T]), rep(q["gpos"][:T])
        drag = DragPose(opt, None, np.zeros(24, np.float32), np.ones(24, np.float32), n_sequences=S)
        trk = drag._trackers(mask_idx, weights)
        dense_p = torch.zeros(T, S, 22, 3, device=dev).index_copy_(2, trk["mj"], tp_rel.reshape(T, S, -1, 3))
        dense_r = torch.zeros(T, S, 22, 9, device=dev).index_copy_(2, trk["mj"], tR.reshape(T, S, -1, 9))
        adjust = (int(ja[0]), int(trk["mj_host"][ja[1]]), float(cfg["joint_adjustment_weight"])) if ja is not None else None
        zero_tgt = torch.zeros(S, 24, device=dev)
        frame = opt.allocate_outputs(S, ("z", "z_pre", "pose", "disp", "world_disp", "world_rot", "pos", "loss", "iters", "status"))
        pose, pos, mu = torch.empty(S, 88, device=dev), torch.empty(S, 3, device=dev), torch.empty(S, device=dev)
        all_tables = LT.tables(S, dev)

        def begin():
            drag.set_initial_state(q["z0"].expand(S, 24).contiguous(), np.repeat(q["m"]["global_pos"][0][None], S, 0),
                                   np.repeat(q["m"]["global_rot"][0][None], S, 0), np.repeat(q["m"]["heights"][0][None], S, 0))
            mu.fill_(1e-2)

        def frames(**extra):
            return drag.run_frames(tp_rel, tR.reshape(T, S, -1, 3, 3), mask_idx, weights, target_root=gpos, max_iter=100, learning_rate=1e-2,
                                   lambda_temporal=0.0, **kw, **extra)

        def loop(lm, terms):
            for t in range(T):
                tp = dense_p[t] + (gpos[t] - drag.current_global_pos).unsqueeze(1)
                fr = opt.optimize_lm(drag.latent, zero_tgt, drag.current_global_rot, tp, dense_r[t], trk["w"], trk["tracked"], lm=lm, lambda_rot=1.0,
                                     lambda_tmp=0.0, mu=mu, stop_eps_pos=1e-4, stop_eps_rot=1e-2, out=frame, outputs=tuple(frame) + ("mu",), terms=terms,
                                     global_pos=drag.current_global_pos)
                opt.sequence_advance(fr, drag.current_global_pos, drag.current_global_rot, drag.latent_buffer, drag.displacement_buffer,
                                     drag.heights_buffer, heights, pose_ret=pose, pos_ret=pos, adjust=adjust, tgt_pos=tp if adjust is not None else None)
                drag.latent.copy_(fr["z"])

        for table in args.tables:
            terms = all_tables[table]
            for name in args.solvers:
                lm = solvers[name]
                runs = {"seq_terms": lambda: frames(solver=replace(lm, terms=terms)), "loop": lambda: loop(lm, terms), "seq": lambda: frames(solver=lm),
                        "adam": lambda: frames(terms=terms)}
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
                    print(f"S {S:3d}  {table:8s} {name}  {v:9s} n {len(x)}  median {np.median(x):9.2f} us / frame  min {x.min():9.2f}  max {x.max():9.2f}  "
                          f"(max - min) / median {(x.max() - x.min()) / np.median(x):.4f}", flush=True)


if __name__ == "__main__":
    main()

"""Tethers (dp_cons_tether.hip): what a tether costs a clip with a term table.  S sequences x T = 64 frames, 6 trackers,
Terms.from_constraints(Constraints.reference()) plus two point-DISTANCE terms on the knees (joints 2 and 6; hi = 0.02 with alpha 0, and
lo = hi = 0 with alpha 1), two loop settings -- `early`: max_iter 10 with the reference's early stop, `fixed`: 50 iterations at a fixed
count -- and per (S, setting) three variants, alternating (A B C A B C ...), each from the same initial state:
  * tethers    dp_optimize_sequence_tethers: the two terms tied to the knees' own path, one launch and one for the history buffers;
  * rows       (a) dp_optimize_sequence_gaps on the same table with the two terms fed fixed [S,4] rows (x, y, z, s = 1): the same arithmetic
               per iteration, no update;
  * per-frame  (b) the composition: T x (a one-step dp_optimize_sequence_gaps with the state rows, the update in torch), driven from Python
               -- DragPose.run(terms=, tethers=).
Every launch runs with Gaps(0, 1.0) and no sample missing.  One process; before the timed rounds the device is preconditioned as bench.py
does (the measured launch back to back for 60 ms of GPU time).  Without a profiler it prints wall time per clip from a host clock around
work that ends in a device synchronise, every variant's median, extremes and (max - min) / median, and the ratios.  Kernel times: one run
per loop setting under the profiler, then the trace summarised by kernel and launch size --
    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python tools/time_tethers.py --loop early --rounds 3 --no-per-frame
    python tools/time_tethers.py --summarise DIR/.../t_kernel_trace.csv
prints, per kernel and S, the number of launches, the median, the extremes and the spread, and the tether kernel against (a)'s kernel, also
as microseconds per step.  --lib PATH times another build of the library (the unit compiled with -DDP_TETHER_WPREV_GLOBAL=1)."""
import argparse
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T = 64
SIZES = (1, 64, 1024)
LOOPS = {"early": dict(n_iter=10, stop_eps_pos=0.01 * 0.01, stop_eps_rot=0.01, min_loss_incr=0.00001),
         "fixed": dict(n_iter=50, stop_eps_pos=0.0, stop_eps_rot=0.0, min_loss_incr=-1e30)}
HJ = (0, 4, 8, 13, 17, 21)
KNEES = (2, 6)
KERNELS = {"tethers": "dp_terms_tether_seq_kernel", "rows": "dp_terms_gap_seq_kernel"}
PRECONDITION_MS = 60.0


def summarise(path, sizes):
    """rocprofv3's kernel trace -> per (kernel, S): durations in microseconds of the T-step launches (the first of each, its warm-up, dropped;
    the per-frame variant's one-step launches of (a)'s kernel are told apart by their duration: under a fifth of the median)"""
    grid = {(S + 7) // 8 * 512: S for S in sizes}  # (the trace's grid is in work-items: a workgroup of 512 per 8 sequences)
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"].split("(")[0]
            S = grid.get(int(row["Grid_Size_X"])) if name in KERNELS.values() else None
            if S is not None:
                groups.setdefault((name, S), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    med, spread = {}, {}
    for (name, S), v in sorted(groups.items()):
        v = np.asarray(v)
        v = v[v > 0.2 * v.max()][1:]
        med[name, S], spread[name, S] = np.median(v), (v.max() - v.min()) / np.median(v)
        print(f"{name:28s} S {S:5d}  n {len(v):5d}  median {np.median(v):9.2f} us  min {v.min():9.2f}  max {v.max():9.2f}  "
              f"(max - min) / median {spread[name, S]:.4f}")
    for S in sizes:
        h, r = (KERNELS["tethers"], S), (KERNELS["rows"], S)
        if h in med and r in med:
            print(f"S {S:5d}: per clip, kernel time  tethers {med[h] * 1e-3:9.3f} ms  rows (a) {med[r] * 1e-3:9.3f} ms  tethers / rows {med[h] / med[r]:6.4f}"
                  f"   ((a)'s own spread {spread[r]:.4f})   difference per step {(med[h] - med[r]) / T:7.3f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--loop", choices=tuple(LOOPS) + ("both",), default="both")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--no-per-frame", action="store_true", help="leave variant (b) out (a profiled run: its one-step launches are not wanted in the trace)")
    ap.add_argument("--lib", default=None, help="another build of libdragposer_hip.so to time")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="no GPU work: summarise a rocprofv3 kernel trace of a run with the same --sequences")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.sequences)
    from dataclasses import replace

    import torch

    from dragposer_amd import Constraints, Gaps, Term, Terms, Tether, Tethers
    from dragposer_amd.optimizer import LatentOptimizer, to_device_batch
    from oracle import ref_torch as R

    dev = torch.device("cuda:0")
    opt = LatentOptimizer(device=dev, _lib_path=os.path.abspath(args.lib) if args.lib else None)
    base = Terms.from_constraints(Constraints.reference())
    ties = [Term.distance(KNEES[0], point=(0.0, 0.0, 0.0), lo=0.0, hi=0.02, weight=1.0),
            Term.distance(KNEES[1], point=(0.0, 0.0, 0.0), lo=0.0, hi=0.0, weight=1.0)]
    table = Terms(base.terms + ties, base.up_axis)
    n0 = len(base)
    tethers, gaps = Tethers([Tether(n0, 0.0), Tether(n0 + 1, 1.0)]), Gaps(0, 1.0)
    loops = tuple(LOOPS) if args.loop == "both" else (args.loop,)
    print(f"T = {T} frames per clip; wall time per clip, host clock around a device synchronise, {args.rounds} rounds, the variants alternating; "
          f"preconditioned with {PRECONDITION_MS:.0f} ms of the tethers launch" + (f"; library {args.lib}" if args.lib else ""))
    for S in args.sequences:
        d = to_device_batch(R.synth_inputs(R.OracleModel(), T * S, trackers=6, seed=S), dev)
        tp, tR = d["tgt_pos"].reshape(T, S, 22, 3), d["tgt_rot"].reshape(T, S, 22, 9)
        z_tgt = d["z_tgt"].reshape(T, S, 24)
        w, tracked = d["w"][:S].contiguous(), d["tracked"][:S].contiguous()
        init = dict(latent=d["z0"][:S].clone(), gpos=torch.zeros(S, 3, device=dev), grot=d["cur_rot"][:S].clone(),
                    lbuf=d["z0"][:S].unsqueeze(1).repeat(1, 60, 1), dbuf=torch.zeros(S, 60, 3, device=dev), hbuf=torch.zeros(S, 60, len(HJ), device=dev),
                    tether=torch.zeros(S, 2, 8, device=dev), gap=torch.zeros(S, 22, 16, device=dev))
        init["gpos"][:, 1] = 0.9
        st = {k: v.clone() for k, v in init.items()}
        rows = torch.zeros(S, 4, device=dev)
        rows[:, 1], rows[:, 3] = 0.4, 1.0  # (a fixed point near a knee's height, s = 1: the term is on in every step)
        fed = Terms(base.terms + [replace(p, per_frame=rows) for p in ties], base.up_axis)
        pose, pos = torch.empty(T, S, 88, device=dev), torch.empty(T, S, 3, device=dev)
        iters, status = torch.empty(T, S, dtype=torch.int32, device=dev), torch.empty(T, S, dtype=torch.int32, device=dev)
        loss, scratch = torch.empty(T, S, 3, device=dev), torch.empty(T, S, 24 + 3 + len(HJ), device=dev)
        per_step, jpos = torch.empty(T, S, len(table), device=dev), torch.empty(T, S, 22, 3, device=dev)
        for lname in loops:
            loop = LOOPS[lname]

            def sequence(terms, t0=0, n=T, **kw):
                sl = slice(t0, t0 + n)
                opt.optimize_sequence(st["latent"], tp[sl], tR[sl], None, w, tracked, z_tgt[sl], (S * 24, 24), st["gpos"], st["grot"], st["lbuf"],
                                      st["dbuf"], st["hbuf"], HJ, lr=1e-2, lambda_rot=1.0, lambda_tmp=0.02, pose_ret=pose[sl], pos_ret=pos[sl],
                                      iters=iters[sl], loss=loss[sl], scratch=scratch[sl], status=status[sl], terms=terms, loss_terms=per_step[sl],
                                      joint_pos=jpos[sl], gaps=gaps, gap_state=st["gap"], **kw, **loop)

            def per_frame():
                for t in range(T):
                    sequence(tethers.frame_terms(table, st["tether"]), t, 1)
                    tethers.update(table, st["tether"], jpos[t], st["gpos"])

            variants = {"tethers": lambda: sequence(table, tethers=tethers, tether_state=st["tether"]), "rows": lambda: sequence(fed)}
            if not args.no_per_frame:
                variants["per-frame"] = per_frame

            def clip(fn):
                for k, v in init.items():
                    st[k].copy_(v)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            first = clip(variants["tethers"])  # (also the first launch of this shape: code object loaded)
            live = float(st["tether"][..., 3].mean())
            for n in list(variants)[1:]:
                clip(variants[n])
            for _ in range(min(20000, int(PRECONDITION_MS * 1e-3 / max(clip(variants["tethers"]), 1e-6)) + 1)):
                variants["tethers"]()
            torch.cuda.synchronize()
            acc = {n: [] for n in variants}
            for _ in range(args.rounds):
                for n, fn in variants.items():
                    acc[n].append(clip(fn))
            for n, v in acc.items():
                v = np.asarray(v) * 1e3
                print(f"S {S:5d} {lname:5s} {n:9s} median {np.median(v):9.3f} ms  min {v.min():9.3f}  max {v.max():9.3f}  "
                      f"(max - min) / median {(v.max() - v.min()) / np.median(v):.4f}")
            m = {n: np.median(v) for n, v in acc.items()}
            tail = f"   per-frame / tethers {m['per-frame'] / m['tethers']:7.2f}" if "per-frame" in m else ""
            print(f"S {S:5d} {lname:5s} tethers / rows {m['tethers'] / m['rows']:7.4f}{tail}   "
                  f"(live after the clip: {live:.2f} of the tethers, first tethers launch {first * 1e3:.3f} ms)", flush=True)


if __name__ == "__main__":
    main()

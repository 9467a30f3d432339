"""Gaps (dp_cons_gap.hip): what deciding the tracker set per step costs a clip.  S sequences x T = 64 frames, 6
trackers, Terms.from_constraints(Constraints.reference()) plus two held horizontal soft pins on joints 4 and 8, a dense order-2 latent
predictor, two loop settings -- `early`: max_iter 10 with the reference's early stop, `fixed`: 50 iterations at a fixed count -- and per
(S, setting) two variants, alternating (A B A B ...), each from the same initial state:
  * gaps       dp_optimize_sequence_gaps (dp_terms_gap_ar_seq_kernel), max_hold 16, decay 0.9.  --gap none: every sample present, the clip
               computes what the other variant computes; --gap held: joint 17 of every sequence absent (through `present`) at steps 20-29,
               held throughout;
  * ar         dp_optimize_sequence_ar (dp_terms_ar_seq_kernel, the kernel before this unit existed) on the same clip, every sample present.
One process; before the timed rounds the device is preconditioned as bench.py does (the measured launch back to back for 60 ms of GPU
time).  Without a profiler it prints wall time per clip from a host clock around work that ends in a device synchronise, both variants'
median, extremes and (max - min) / median, and the ratio.  Kernel times: one run per loop setting and --gap under the profiler, then the
trace summarised by kernel and launch size --
    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python tools/time_gaps.py --loop early --gap none --rounds 3
    python tools/time_gaps.py --summarise DIR/.../t_kernel_trace.csv
prints, per kernel and S, the number of launches, the median, the extremes and the spread, and the new kernel against the other."""
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
KERNELS = {"gaps": "dp_terms_gap_ar_seq_kernel", "ar": "dp_terms_ar_seq_kernel"}
PRECONDITION_MS = 60.0


def summarise(path, sizes):
    """rocprofv3's kernel trace -> per (kernel, S): durations in microseconds (the first launch of each, its warm-up, dropped)"""
    grid = {(S + 7) // 8 * 512: S for S in sizes}  # (the trace's grid is in work-items: a workgroup of 512 per 8 frames / sequences)
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"].split("(")[0]
            S = grid.get(int(row["Grid_Size_X"])) if name in KERNELS.values() else None
            if S is not None:
                groups.setdefault((name, S), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    med, spread = {}, {}
    for (name, S), v in sorted(groups.items()):
        v = np.asarray(v[1:])
        med[name, S], spread[name, S] = np.median(v), (v.max() - v.min()) / np.median(v)
        print(f"{name:28s} S {S:5d}  n {len(v):5d}  median {np.median(v):9.2f} us  min {v.min():9.2f}  max {v.max():9.2f}  "
              f"(max - min) / median {spread[name, S]:.4f}")
    for S in sizes:
        h, r = (KERNELS["gaps"], S), (KERNELS["ar"], S)
        if h in med and r in med:
            print(f"S {S:5d}: per clip, kernel time  gaps {med[h] * 1e-3:9.3f} ms  ar {med[r] * 1e-3:9.3f} ms  gaps / ar {med[h] / med[r]:6.4f}"
                  f"   (the ar kernel's own (max - min) / median {spread[r]:.4f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--loop", choices=tuple(LOOPS) + ("both",), default="both")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--gap", choices=("none", "held"), default="none", help="the gaps variant's clip: every sample present / a 10-step held gap in every sequence")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="no GPU work: summarise a rocprofv3 kernel trace of a run with the same --sequences")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.sequences)
    import torch

    from dragposer_amd import Constraints, Gaps, Hold, Holds, LatentAR, Term, Terms
    from dragposer_amd.optimizer import LatentOptimizer, to_device_batch
    from oracle import ref_torch as R

    dev = torch.device("cuda:0")
    opt = LatentOptimizer(device=dev)
    base = Terms.from_constraints(Constraints.reference())
    pins = [Term.distance(j, point=(0.0, 0.0, 0.0), lo=0.0, hi=0.0, weight=1.0, drop_up=True) for j in (4, 8)]
    table = Terms(base.terms + pins, base.up_axis)
    n0 = len(base)
    holds = Holds([Hold(n0, 0.95, 1.0), Hold(n0 + 1, 0.95, 1.0)])  # (heights around the clips' 0.9: some sequences latch, some release)
    g = np.random.default_rng(7)
    A = g.standard_normal((args.order, 24, 24)) * (0.6 / (args.order * np.sqrt(24.0)))
    A[0] += 0.3 * np.eye(24)
    ar = LatentAR(A, 0.05 * g.standard_normal(24))
    gaps = Gaps(16, 0.9)
    loops = tuple(LOOPS) if args.loop == "both" else (args.loop,)
    print(f"T = {T} frames per clip; wall time per clip, host clock around a device synchronise, {args.rounds} rounds, the variants alternating; "
          f"preconditioned with {PRECONDITION_MS:.0f} ms of the gaps launch; order {args.order}; --gap {args.gap}")
    for S in args.sequences:
        d = to_device_batch(R.synth_inputs(R.OracleModel(), T * S, trackers=6, seed=S), dev)
        tp, tR = d["tgt_pos"].reshape(T, S, 22, 3), d["tgt_rot"].reshape(T, S, 22, 9)
        w, tracked = d["w"][:S].contiguous(), d["tracked"][:S].contiguous()
        init = dict(latent=d["z0"][:S].clone(), gpos=torch.zeros(S, 3, device=dev), grot=d["cur_rot"][:S].clone(),
                    lbuf=d["z0"][:S].unsqueeze(1).repeat(1, 60, 1), dbuf=torch.zeros(S, 60, 3, device=dev), hbuf=torch.zeros(S, 60, len(HJ), device=dev),
                    hold=torch.zeros(S, 2, 4, device=dev), gap=torch.zeros(S, 22, 16, device=dev))
        present = torch.ones(T, S, 22, dtype=torch.uint8, device=dev)
        if args.gap == "held":
            present[20:30, :, 17] = 0
        trace = torch.zeros(T, S, 22, dtype=torch.uint8, device=dev)
        init["gpos"][:, 1] = 0.9
        st = {k: v.clone() for k, v in init.items()}
        pose, pos = torch.empty(T, S, 88, device=dev), torch.empty(T, S, 3, device=dev)
        iters, status = torch.empty(T, S, dtype=torch.int32, device=dev), torch.empty(T, S, dtype=torch.int32, device=dev)
        loss, scratch = torch.empty(T, S, 3, device=dev), torch.empty(T, S, 24 + 3 + len(HJ), device=dev)
        per_step, jpos = torch.empty(T, S, len(table), device=dev), torch.empty(T, S, 22, 3, device=dev)
        for lname in loops:
            loop = LOOPS[lname]

            def sequence(**kw):
                opt.optimize_sequence(st["latent"], tp, tR, None, w, tracked, None, (0, 0), st["gpos"], st["grot"], st["lbuf"], st["dbuf"],
                                      st["hbuf"], HJ, lr=1e-2, lambda_rot=1.0, lambda_tmp=0.02, pose_ret=pose, pos_ret=pos, iters=iters, loss=loss,
                                      scratch=scratch, status=status, terms=table, loss_terms=per_step, joint_pos=jpos, holds=holds,
                                      hold_state=st["hold"], ar=ar, **kw, **loop)

            variants = {"gaps": lambda: sequence(gaps=gaps, gap_state=st["gap"], present=present, gap_trace=trace), "ar": lambda: sequence()}

            def clip(fn):
                for k, v in init.items():
                    st[k].copy_(v)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            first = clip(variants["gaps"])  # (also the first launch of this shape: code object loaded)
            bad, its_gaps = int(((status & 7) != 0).sum()), float(iters.float().mean())
            codes = [int((trace == k).sum()) for k in (1, 2, 3)]
            clip(variants["ar"])
            its_ar = float(iters.float().mean())  # (with a held gap the two clips end their steps at their own counts)
            for _ in range(min(20000, int(PRECONDITION_MS * 1e-3 / max(clip(variants["gaps"]), 1e-6)) + 1)):
                variants["gaps"]()
            torch.cuda.synchronize()
            acc = {n: [] for n in variants}
            for _ in range(args.rounds):
                for n, fn in variants.items():
                    acc[n].append(clip(fn))
            for n, v in acc.items():
                v = np.asarray(v) * 1e3
                print(f"S {S:5d} {lname:5s} {n:5s} median {np.median(v):9.3f} ms  min {v.min():9.3f}  max {v.max():9.3f}  "
                      f"(max - min) / median {(v.max() - v.min()) / np.median(v):.4f}")
            m = {n: np.median(v) for n, v in acc.items()}
            print(f"S {S:5d} {lname:5s} gaps / ar {m['gaps'] / m['ar']:7.4f}   (mean iterations per step: gaps {its_gaps:.2f}, ar {its_ar:.2f}; joint-steps present / "
                  f"held / lost in the gaps clip: {codes[0]} / {codes[1]} / {codes[2]}; steps refused: {bad}; first gaps launch {first * 1e3:.3f} ms)", flush=True)


if __name__ == "__main__":
    main()

"""Cost of per-frame skeletons in the constrained and term-table loops (dp_cons_skel.hip): B frames x 50 iterations
at a fixed count, 6 trackers, Constraints.reference() and the same block as a table, the variants alternating (A B C A B C ...):
  * plain     dp_optimize_constrained / dp_optimize_terms on the context's skeleton (dp_cons_kernel / dp_terms_kernel);
  * skeleton  the _skeleton forms with [B,22,3] offsets, four skeletons in every workgroup (dp_cons_skel_kernel / dp_terms_skel_kernel);
  * four      what a user had before: four plain launches on four contexts, one per skeleton, B/4 frames each.
Without a profiler it prints wall time per call from HIP events, every round, so the spread of each variant's own repeats is visible.
Kernel times: one run per size under the profiler, then the trace summarised by kernel and grid --
    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python tools/time_constraints_skeleton.py --frames 4096
    python tools/time_constraints_skeleton.py --frames 4096 --summarise DIR/.../t_kernel_trace.csv
prints, per kernel and launch size, the number of launches, the median, the extremes, and the ratios against the plain kernel beside
the plain kernel's own (max - min) / median."""
import argparse
import csv
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = {"cons": ("dp_cons_kernel", "dp_cons_skel_kernel"), "terms": ("dp_terms_kernel", "dp_terms_skel_kernel")}


def summarise(path, B):
    """rocprofv3's kernel trace -> per (kernel, frames of the launch): durations in microseconds, warm-up launches (the first of each) dropped"""
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"].split("(")[0]
            if "dp_cons" not in name and "dp_terms" not in name:
                continue
            gx, wx = int(row["Grid_Size_X"]), int(row["Workgroup_Size_X"])
            frames = {B // 8 * wx: B, B // 8: B, B // 32 * wx: B // 4, B // 32: B // 4}.get(gx)  # (the grid in work-items or in workgroups)
            if frames is None:
                continue
            groups.setdefault((name, frames), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    med = {}
    for (name, frames), v in sorted(groups.items()):
        v = np.asarray(v[1:])
        med[name, frames] = np.median(v)
        print(f"{name:22s} {frames:6d} frames  n {len(v):4d}  median {np.median(v):9.2f} us  min {v.min():9.2f}  max {v.max():9.2f}  "
              f"(max - min) / median {(v.max() - v.min()) / np.median(v):.4f}")
    for which, (plain, skel) in KERNELS.items():
        if (plain, B) in med and (skel, B) in med:
            print(f"{which:6s} B={B}: skeleton / plain {med[skel, B] / med[plain, B]:.4f}" +
                  (f"   four launches of B/4 (kernel time, summed) / skeleton {4 * med[plain, B // 4] / med[skel, B]:.4f}" if (plain, B // 4) in med else ""))


def _time(fn, reps):
    import torch

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="no GPU work: summarise a rocprofv3 kernel trace of a run with the same --frames")
    args = ap.parse_args()
    B = args.frames
    if args.summarise:
        return summarise(args.summarise, B)
    import torch

    from dragposer_amd import Constraints, Terms
    from dragposer_amd.optimizer import LatentOptimizer, to_device_batch
    from oracle import ref_torch as R

    assert B % 32 == 0, "--frames: a multiple of 32 (four launches of whole workgroups)"
    dev = torch.device("cuda:0")
    main_opt = LatentOptimizer(device=dev)
    base = np.asarray(main_opt.host_model.arrays["offsets"], np.float32)
    raw = dict(np.load(R.DEFAULT_MODEL))
    factors = (1.0, 0.85, 1.2, 1.1)
    four = [LatentOptimizer(device=dev, arrays={**raw, "offsets": base * np.float32(f)}) for f in factors]
    off = torch.from_numpy(np.stack([base * np.float32(factors[k % 4]) for k in range(B)])).contiguous().to(dev)
    d = to_device_batch(R.synth_inputs(R.OracleModel(), B, trackers=6, seed=B), dev)
    g = torch.zeros(B, 3, device=dev)
    g[:, 1] = 0.9
    quarters = [({k: v[q::4].contiguous() for k, v in d.items()}, g[q::4].contiguous()) for q in range(4)]
    cons = Constraints.reference()
    table = Terms.from_constraints(cons)
    kw = dict(n_iter=50, lambda_tmp=0.02)
    outs = {"cons": main_opt.allocate_outputs(B), "terms": main_opt.allocate_outputs(B)}
    outs["cons"]["loss_extra"] = torch.empty(B, 4, device=dev)
    outs["terms"]["loss_terms"] = torch.empty(B, len(table), device=dev)

    def four_launches(which):
        def run():
            for o, (dq, gq) in zip(four, quarters):
                if which == "cons":
                    o.optimize_constrained(**dq, constraints=cons, global_pos=gq, **kw)
                else:
                    o.optimize_terms(**dq, terms=table, global_pos=gq, **kw)
        return run

    variants = [
        ("cons plain", lambda: main_opt.optimize_constrained(**d, constraints=cons, global_pos=g, out=outs["cons"], **kw)),
        ("cons skeleton", lambda: main_opt.optimize_constrained(**d, constraints=cons, global_pos=g, out=outs["cons"], offsets=off, **kw)),
        ("cons four", four_launches("cons")),
        ("terms plain", lambda: main_opt.optimize_terms(**d, terms=table, global_pos=g, out=outs["terms"], **kw)),
        ("terms skeleton", lambda: main_opt.optimize_terms(**d, terms=table, global_pos=g, out=outs["terms"], offsets=off, **kw)),
        ("terms four", four_launches("terms")),
    ]
    for _, fn in variants:  # warm-up
        fn()
    torch.cuda.synchronize()
    acc = {n: [] for n, _ in variants}
    for _ in range(args.rounds):
        for n, fn in variants:
            acc[n].append(_time(fn, args.reps))
    print(f"B = {B} frames x 50 iterations; wall time per call from HIP events, {args.rounds} rounds x {args.reps} calls, the variants alternating")
    for n, v in acc.items():
        v = np.asarray(v) * 1e3
        print(f"{n:15s} median {np.median(v):8.4f} ms  min {v.min():8.4f}  max {v.max():8.4f}  (max - min) / median {(v.max() - v.min()) / np.median(v):.4f}")
    for which in ("cons", "terms"):
        p, s, f = (np.median(acc[f"{which} {x}"]) for x in ("plain", "skeleton", "four"))
        print(f"{which:6s} skeleton / plain {s / p:.4f}   four launches / skeleton {f / s:.4f}")


if __name__ == "__main__":
    main()

"""Times dp_optimize_terms_points (include/dragposer_points.h) against dp_optimize_terms at 4096 and 16 384 frames, 50 iterations at a
fixed count, on two tables of seven terms each:
  points   the reference table (Terms.from_constraints(Constraints.reference())) plus the balance term -- the centroid of all joints
           within a radius of the midpoint of the feet, two points -- through dp_terms_points_kernel
  joints   the reference table plus one more DISTANCE band naming joints (the hips and a foot, the reference's own stand-in for
           balance) through dp_terms_kernel, whose code this feature leaves as it was: the yardstick
The variants alternate within each size (A B A B ...).  Wall time per call from HIP events after a warm-up; one line per size.
Kernel-only times: a run of its own under the profiler, then the trace summarised by kernel and launch size --
    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python tools/time_points.py --rounds 3
    python tools/time_points.py --summarise DIR/.../t_kernel_trace.csv
--joints-only times the yardstick alone and needs nothing of the feature: copied into a checkout of the parent commit it times that
commit's kernel."""
import csv
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dragposer_amd import Constraints, Term, Terms  # noqa: E402
from dragposer_amd.optimizer import LatentOptimizer, to_device_batch  # noqa: E402
from oracle import ref_torch as R  # noqa: E402

RADIUS, WEIGHT = 0.1, 1.0


def joints_table():
    base = Terms.from_constraints(Constraints.reference())
    return Terms(base.terms + [Term.distance(0, 4, lo=0.0, hi=RADIUS, weight=WEIGHT, drop_up=True)], base.up_axis)


def points_table():
    from dragposer_amd import Point, Points

    base = Terms.from_constraints(Constraints.reference())
    pts = Points([Point.centroid(), Point.midpoint(4, 8)])
    return Terms(base.terms + [Term.distance(pts.joint(0), pts.joint(1), lo=0.0, hi=RADIUS, weight=WEIGHT, drop_up=True)], base.up_axis, pts)


KERNELS = {"joints": "dp_terms_kernel", "points": "dp_terms_points_kernel"}


def summarise(path, sizes):
    """rocprofv3's kernel trace -> per (kernel, B): the launches' durations in microseconds (the first of each, its warm-up, dropped)"""
    import numpy as np

    grid = {(B + 7) // 8 * 512: B for B in sizes}  # (the trace's grid is in work-items: a workgroup of 512 per 8 frames)
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"].split("(")[0]
            B = grid.get(int(row["Grid_Size_X"])) if name in KERNELS.values() else None
            if B is not None:
                groups.setdefault((name, B), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    med = {}
    for (name, B), v in sorted(groups.items()):
        v = np.asarray(v)[1:]
        med[name, B] = np.median(v)
        print(f"{name:24s} B {B:6d}  n {len(v):4d}  median {np.median(v):9.2f} us  min {v.min():9.2f}  max {v.max():9.2f}  "
              f"(max - min) / median {(v.max() - v.min()) / np.median(v):.4f}")
    for B in sizes:
        if (KERNELS["points"], B) in med and (KERNELS["joints"], B) in med:
            print(f"B {B:6d}  points / joints {med[KERNELS['points'], B] / med[KERNELS['joints'], B]:.4f}")


def _time(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps * 1e-3


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 16384])
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the variants per size")
    ap.add_argument("--joints-only", action="store_true", help="the yardstick alone (runs in a checkout without the feature)")
    ap.add_argument("--summarise", default=None, metavar="KERNEL_TRACE_CSV", help="summarise a rocprofv3 kernel trace of this tool and exit")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.sizes)
    dev = torch.device("cuda:0")
    opt = LatentOptimizer(device=dev)
    model = R.OracleModel()
    tables = {"joints": joints_table()}
    if not args.joints_only:
        tables["points"] = points_table()
    assert len({len(t) for t in tables.values()}) == 1
    n, lam = 50, 0.02
    for B in args.sizes:
        d = to_device_batch(R.synth_inputs(model, B, seed=B), dev)
        g = torch.zeros(B, 3, device=dev)
        g[:, 1] = 0.9
        runs = {k: (lambda t=t: opt.optimize_terms(**d, terms=t, global_pos=g, n_iter=n, lambda_tmp=lam)) for k, t in tables.items()}
        outs = {k: fn() for k, fn in runs.items()}  # warm-up
        torch.cuda.synchronize()
        active = {k: float((o["loss_terms"][:, -1] > 0).float().mean()) for k, o in outs.items()}
        best, every = {k: float("inf") for k in runs}, {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                t = _time(fn, 5)
                best[k] = min(best[k], t)
                every[k].append(t)
        line = f"B={B:6d}  " + "  ".join(f"{k} {v * 1e3:8.3f} ms (max {max(every[k]) * 1e3:8.3f}, last term active in {active[k]:.0%})" for k, v in best.items())
        if "points" in best:
            line += f"  points/joints {best['points'] / best['joints']:.3f}"
        print(line, flush=True)


if __name__ == "__main__":
    main()

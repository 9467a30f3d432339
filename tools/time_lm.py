"""Times dp_optimize_lm (include/dragposer_lm.h) against the two Adam kernels on the warm 6-tracker recipe (tests/lm_oracle.py:
z0 = z_src + 0.05 N(0,1), z_tgt = z0; lambda_rot 1, lambda_tmp 0.02) at 1, 64 and 4096 frames:
  lm1 lm2 lm4 lm8    dp_lm_kernel at 1, 2, 4, 8 steps (no early stop)
  terms10 terms50    dp_terms_kernel with an empty table (the one-frame-per-wave Adam loop) at 10 and 50 iterations
  w4_10 w4_50        dp_optimize on dp_w4 at 10 and 50 iterations
The variants alternate within each size (A B C ... A B C ...), one process.  Kernel times come from a run of its own under the profiler,
no counters in it, and the trace is then summarised with the launch plan the run wrote beside it --
    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python tools/time_lm.py --rounds 7 --plan DIR/plan.json
    python tools/time_lm.py --summarise DIR/.../t_kernel_trace.csv --plan DIR/plan.json
per variant and size: the launches' median, the plain (max - min) / median and the median total loss; then microseconds per LM step (the
slope between 1 and 8 steps) and, per size, the smallest step count whose median loss is at or below Adam-50's beside both Adam kernels."""
import csv
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

VARIANTS = ("lm1", "lm2", "lm4", "lm8", "terms10", "terms50", "w4_10", "w4_50")
KERNEL_OF = {"lm": "dp_lm_kernel", "terms": "dp_terms_kernel", "w4": "dp_w4"}


def _kernel(variant):
    return KERNEL_OF["lm" if variant.startswith("lm") else "terms" if variant.startswith("terms") else "w4"]


def summarise(path, plan_path):
    plan = json.load(open(plan_path))
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            if any(k in name for k in KERNEL_OF.values()):
                rows.append((int(row["Start_Timestamp"]), name, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3))
    rows.sort()
    launches = plan["launches"]
    assert len(rows) == len(launches), (len(rows), len(launches))
    groups = {}
    for (_, name, us), (B, variant, warm) in zip(rows, launches):
        assert _kernel(variant) in name, (name, variant)
        if not warm:
            groups.setdefault((B, variant), []).append(us)
    med = {}
    for (B, variant), v in groups.items():
        v = np.asarray(v)
        med[B, variant] = float(np.median(v))
        print(f"B {B:5d}  {variant:8s} n {len(v):3d}  median {np.median(v):9.2f} us  min {v.min():9.2f}  max {v.max():9.2f}  "
              f"(max - min) / median {(v.max() - v.min()) / np.median(v):.4f}  median loss {plan['loss'][f'{B}:{variant}']:.3e}")
    for B in sorted({b for b, _ in med}):
        loss = {v: plan["loss"][f"{B}:{v}"] for v in VARIANTS}
        print(f"B {B:5d}  per LM step (lm8 - lm1) / 7 = {(med[B, 'lm8'] - med[B, 'lm1']) / 7.0:.2f} us;  per Adam iteration: dp_terms_kernel "
              f"{(med[B, 'terms50'] - med[B, 'terms10']) / 40.0:.2f} us, dp_w4 {(med[B, 'w4_50'] - med[B, 'w4_10']) / 40.0:.2f} us")
        enough = [v for v in ("lm1", "lm2", "lm4", "lm8") if loss[v] <= loss["w4_50"]]
        if enough:
            v = enough[0]
            print(f"B {B:5d}  {v} reaches Adam-50's median loss ({loss[v]:.3e} <= {loss['w4_50']:.3e}): {med[B, v]:.2f} us against "
                  f"dp_terms_kernel {med[B, 'terms50']:.2f} us ({med[B, 'terms50'] / med[B, v]:.2f}x) and dp_w4 {med[B, 'w4_50']:.2f} us "
                  f"({med[B, 'w4_50'] / med[B, v]:.2f}x)")
        else:
            print(f"B {B:5d}  no step count up to 8 reaches Adam-50's median loss {loss['w4_50']:.3e}")


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 64, 4096])
    ap.add_argument("--rounds", type=int, default=7, help="alternations of the variants per size")
    ap.add_argument("--plan", default="lm_plan.json", help="where the run writes (and --summarise reads) the order of its launches and the losses")
    ap.add_argument("--summarise", default=None, metavar="KERNEL_TRACE_CSV", help="summarise a rocprofv3 kernel trace of this tool and exit")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.plan)
    import lm_oracle as LO
    from dragposer_amd import LM, Terms
    from dragposer_amd.optimizer import LatentOptimizer, to_device_batch
    from oracle import ref_torch as R

    dev = torch.device("cuda:0")
    opt = LatentOptimizer(device=dev)
    model = R.OracleModel()
    lam = 0.02
    launches, losses = [], {}
    for B in args.sizes:
        d = to_device_batch(LO.warm_inputs(model, B, trackers=6, seed=11), dev)
        out = opt.allocate_outputs(B)
        empty = Terms()
        runs = {}
        for s in (1, 2, 4, 8):
            runs[f"lm{s}"] = lambda s=s: opt.optimize_lm(**d, lm=LM(steps=s, early_stop=False), lambda_tmp=lam, out=out, outputs=("z", "loss", "iters"))
        for n in (10, 50):
            runs[f"terms{n}"] = lambda n=n: opt.optimize_terms(**d, terms=empty, n_iter=n, lambda_tmp=lam, out=out, outputs=("z", "loss", "iters"))
            runs[f"w4_{n}"] = lambda n=n: opt.optimize(**d, n_iter=n, lambda_tmp=lam, kernel="w4", out=out, outputs=("z", "loss", "iters"))
        for v in VARIANTS:  # warm-up, and the variant's loss
            o = runs[v]()
            torch.cuda.synchronize()
            launches.append((B, v, True))
            losses[f"{B}:{v}"] = float(o["loss"].sum(1).median())
        for _ in range(args.rounds):
            for v in VARIANTS:
                runs[v]()
                launches.append((B, v, False))
        torch.cuda.synchronize()
        print(f"B {B:5d}  median loss  " + "  ".join(f"{v} {losses[f'{B}:{v}']:.3e}" for v in VARIANTS), flush=True)
    with open(args.plan, "w") as f:
        json.dump(dict(launches=launches, loss=losses), f)


if __name__ == "__main__":
    main()

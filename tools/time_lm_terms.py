"""Times dp_optimize_lm_terms (include/dragposer_lm_terms.h) against dp_lm_kernel without terms and against dp_terms_kernel on the same table,
on the warm 6-tracker recipe (tests/lm_oracle.py; lambda_rot 1, lambda_tmp 0.02; global_pos and the tables of tests/lm_terms_oracle.py:
`custom` = tests/test_hip_terms.py's CUSTOM(), `mixed16` = its 16 terms of every type) at 1, 64 and 4096 frames:
  T:lmt1 .. T:lmt8   dp_lm_terms_kernel with table T at 1, 2, 3, 4, 6, 8 steps (no early stop)
  T:terms50          dp_terms_kernel with table T, 50 Adam iterations: the reference for the loss to reach
  lm1 lm8            dp_lm_kernel, no terms, at 1 and 8 steps
The variants alternate within each size, one process.  Kernel times come from a run of its own under the profiler, no counters in it, and
the trace is then summarised with the launch plan the run wrote beside it --
    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python tools/time_lm_terms.py --rounds 7 --plan DIR/plan.json
    python tools/time_lm_terms.py --summarise DIR/.../t_kernel_trace.csv --plan DIR/plan.json
per variant and size: the launches' median, (max - min) / median and the median TOTAL loss (the three numbers + the weighted terms); then
microseconds per step with and without terms, and the smallest step count whose median total loss is at or below dp_terms_kernel's after 50
iterations, beside that kernel's time."""
import csv
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

TABLES = ("custom", "mixed16")
STEPS = (1, 2, 3, 4, 6, 8)
VARIANTS = ("lm1", "lm8") + tuple(f"{t}:lmt{s}" for t in TABLES for s in STEPS) + tuple(f"{t}:terms50" for t in TABLES)
KERNELS = ("dp_lm_terms_kernel", "dp_lm_kernel", "dp_terms_kernel")


def _kernel(variant):
    return "dp_lm_kernel" if variant.startswith("lm") else "dp_lm_terms_kernel" if ":lmt" in variant else "dp_terms_kernel"


def summarise(path, plan_path):
    plan = json.load(open(plan_path))
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            if any(k in name for k in KERNELS):
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
        print(f"B {B:5d}  {variant:16s} n {len(v):3d}  median {np.median(v):9.2f} us  min {v.min():9.2f}  max {v.max():9.2f}  "
              f"(max - min) / median {(v.max() - v.min()) / np.median(v):.4f}  median total loss {plan['loss'][f'{B}:{variant}']:.3e}")
    for B in sorted({b for b, _ in med}):
        plain = (med[B, "lm8"] - med[B, "lm1"]) / 7.0
        print(f"B {B:5d}  per step without terms (lm8 - lm1) / 7 = {plain:.2f} us")
        for t in TABLES:
            step = (med[B, f"{t}:lmt8"] - med[B, f"{t}:lmt1"]) / 7.0
            want = plan["loss"][f"{B}:{t}:terms50"]
            print(f"B {B:5d}  {t}: per step (lmt8 - lmt1) / 7 = {step:.2f} us, {step / plain:.2f} x the step without terms; one step in all "
                  f"{med[B, f'{t}:lmt1']:.2f} us against {med[B, 'lm1']:.2f} us")
            enough = [s for s in STEPS if plan["loss"][f"{B}:{t}:lmt{s}"] <= want]
            if enough:
                s = enough[0]
                print(f"B {B:5d}  {t}: {s} steps reach dp_terms_kernel's median total loss after 50 iterations ({plan['loss'][f'{B}:{t}:lmt{s}']:.3e} <= "
                      f"{want:.3e}): {med[B, f'{t}:lmt{s}']:.2f} us against {med[B, f'{t}:terms50']:.2f} us "
                      f"({med[B, f'{t}:terms50'] / med[B, f'{t}:lmt{s}']:.2f}x)")
            else:
                print(f"B {B:5d}  {t}: no step count up to 8 reaches dp_terms_kernel's median total loss {want:.3e} (8 steps: "
                      f"{plan['loss'][f'{B}:{t}:lmt8']:.3e}, {med[B, f'{t}:lmt8']:.2f} us against {med[B, f'{t}:terms50']:.2f} us)")


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 64, 4096])
    ap.add_argument("--rounds", type=int, default=7, help="alternations of the variants per size")
    ap.add_argument("--plan", default="lm_terms_plan.json", help="where the run writes (and --summarise reads) the order of its launches and the losses")
    ap.add_argument("--summarise", default=None, metavar="KERNEL_TRACE_CSV", help="summarise a rocprofv3 kernel trace of this tool and exit")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.plan)
    import lm_oracle as LO
    import lm_terms_oracle as LT
    from dragposer_amd import LM
    from dragposer_amd.optimizer import LatentOptimizer, to_device_batch
    from oracle import ref_torch as R

    dev = torch.device("cuda:0")
    opt = LatentOptimizer(device=dev)
    model = R.OracleModel()
    lam = 0.02
    launches, losses = [], {}
    for B in args.sizes:
        d = to_device_batch(LO.warm_inputs(model, B, trackers=6, seed=11), dev)
        gp = torch.from_numpy(LT.global_pos(B)).to(dev)
        out = opt.allocate_outputs(B)
        tables = LT.tables(B, dev)
        runs = {}
        for s in (1, 8):
            runs[f"lm{s}"] = lambda s=s: opt.optimize_lm(**d, lm=LM(steps=s, early_stop=False), lambda_tmp=lam, out=out, outputs=("z", "loss", "iters"))
        for t in TABLES:
            lt = torch.empty(B, len(tables[t]), device=dev)
            o2 = dict(out, loss_terms=lt)
            for s in STEPS:
                runs[f"{t}:lmt{s}"] = lambda s=s, t=t, o2=o2: opt.optimize_lm(**d, lm=LM(steps=s, early_stop=False), lambda_tmp=lam, terms=tables[t], global_pos=gp,
                                                                             out=o2, outputs=("z", "loss", "iters", "loss_terms"))
            runs[f"{t}:terms50"] = lambda t=t, o2=o2: opt.optimize_terms(**d, terms=tables[t], global_pos=gp, n_iter=50, lambda_tmp=lam, out=o2,
                                                                         outputs=("z", "loss", "iters", "loss_terms"))
        for v in VARIANTS:  # warm-up, and the variant's loss
            o = runs[v]()
            torch.cuda.synchronize()
            launches.append((B, v, True))
            tot = o["loss"].sum(1) + (o["loss_terms"].sum(1) if "loss_terms" in o else 0.0)
            losses[f"{B}:{v}"] = float(tot.median())
        for _ in range(args.rounds):
            for v in VARIANTS:
                runs[v]()
                launches.append((B, v, False))
        torch.cuda.synchronize()
        print(f"B {B:5d}  median total loss  " + "  ".join(f"{v} {losses[f'{B}:{v}']:.3e}" for v in VARIANTS), flush=True)
    with open(args.plan, "w") as f:
        json.dump(dict(launches=launches, loss=losses), f)


if __name__ == "__main__":
    main()

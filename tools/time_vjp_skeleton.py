"""Cost of per-frame skeletons in the vector-Jacobian product (include/dragposer_grad.h): dp_forward_vjp (dp_vjp_kernel, the context's
bones) against dp_forward_vjp_skeleton (dp_vjp_skel_kernel, [B,22,3], four skeletons mixed per wave) without and with dL/d(offsets), on the
same inputs with all six upstream gradients, at 4096 / 65 536 / 262 144 frames.  The three variants alternate (A B C A B C ...).

Kernel times: run it under
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_vjp_skeleton.py
and then `python tools/time_vjp_skeleton.py --summarise DIR` (the same --rounds / --reps), which splits the rows of the one skeleton kernel
into its two variants by launch order and prints median / mean kernel time per variant and size, and the ratios to dp_vjp_kernel.
Without a profiler it prints wall time per call from HIP events (profiles/vjp_skeleton_times.txt)."""
import argparse
import csv
import glob
import os
import sys

import numpy as np

VARIANTS = ("plain", "skeleton", "skeleton+doffsets")
SHAPES = {"pose": (88,), "disp": (3,), "world_disp": (3,), "world_rot": (4,), "pos": (22, 3), "rot": (22, 9)}


def _time(fn, reps):
    import torch

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps * 1e-3


def run(args):
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from dragposer_amd.optimizer import LatentOptimizer

    dev = torch.device("cuda:0")
    opt = LatentOptimizer(device=dev)
    base = torch.from_numpy(np.asarray(opt.host_model.arrays["offsets"], np.float32))
    for B in args.frames:
        g = torch.Generator().manual_seed(B)
        z = (torch.randn(B, 24, generator=g) * 0.5).to(dev)
        cr = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=-1).to(dev)
        grads = {n: torch.randn((B,) + s, generator=g).to(dev) for n, s in SHAPES.items()}
        off = (base.unsqueeze(0) * torch.tensor([1.0, 0.85, 1.2, 1.1])[torch.arange(B) % 4].reshape(B, 1, 1)).contiguous().to(dev)
        out = {"dz": torch.empty(B, 24, device=dev), "dcur_rot": torch.empty(B, 4, device=dev), "status": torch.empty(B, dtype=torch.int32, device=dev)}
        out_d = dict(out, doffsets=torch.empty(B, 22, 3, device=dev))
        fns = {"plain": lambda: opt.forward_vjp(z, cr, grads, out=out),
               "skeleton": lambda: opt.forward_vjp(z, cr, grads, out=out, offsets=off),
               "skeleton+doffsets": lambda: opt.forward_vjp(z, cr, grads, out=out_d, offsets=off)}
        for v in VARIANTS:  # warm-up: one launch each
            fns[v]()
        torch.cuda.synchronize()
        acc = {v: [] for v in VARIANTS}
        for _ in range(args.rounds):
            for v in VARIANTS:
                acc[v].append(_time(fns[v], args.reps))
        med = {v: float(np.median(acc[v])) * 1e3 for v in VARIANTS}
        print(f"B={B:7d}  " + "  ".join(f"{v} {med[v]:.4f} ms" for v in VARIANTS)
              + f"  ratios {med['skeleton'] / med['plain']:.4f} / {med['skeleton+doffsets'] / med['plain']:.4f}  (wall per call, HIP events, "
              f"median of {args.rounds} rounds x {args.reps})", flush=True)


def summarise(args):
    paths = glob.glob(os.path.join(args.summarise, "**", "*kernel_trace.csv"), recursive=True)
    if len(paths) != 1:
        raise SystemExit(f"expected one *kernel_trace.csv under {args.summarise}, found {paths}")
    rows = [r for r in csv.DictReader(open(paths[0])) if "dp_vjp" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    times = {}  # (variant, grid) -> [ms]
    for B in args.frames:
        grid = str(-(-B // 64) * 64)
        at = [r for r in rows if (r.get("Grid_Size") or r.get("Grid_Size_X")) == grid]
        plain = [r for r in at if "dp_vjp_kernel" in r["Kernel_Name"]]
        skel = [r for r in at if "dp_vjp_skel_kernel" in r["Kernel_Name"]]
        want = 1 + args.rounds * args.reps
        if len(plain) != want or len(skel) != 2 * want:
            raise SystemExit(f"B={B}: {len(plain)} / {len(skel)} launches of the two kernels, expected {want} / {2 * want}")
        ms = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6  # noqa: E731  (ns)
        times[("plain", B)] = [ms(r) for r in plain]
        # the skeleton kernel's launches in order: one warm-up of each variant, then per round `reps` without and `reps` with doffsets
        lab = ["skeleton", "skeleton+doffsets"] + [("skeleton", "skeleton+doffsets")[((i // args.reps) % 2)] for i in range(2 * args.rounds * args.reps)]
        for v in VARIANTS[1:]:
            times[(v, B)] = [ms(r) for r, l in zip(skel, lab) if l == v]
    for B in args.frames:
        med = {v: float(np.median(times[(v, B)])) for v in VARIANTS}
        for v in VARIANTS:
            t = times[(v, B)]
            print(f"  {v:18s} frames {B:7d}  launches {len(t):4d}  median {med[v]:.4f} ms  mean {np.mean(t):.4f} ms  min {np.min(t):.4f} ms"
                  + ("" if v == "plain" else f"  ratio to plain (medians) {med[v] / med['plain']:.4f}"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=lambda s: [int(x) for x in s.split(",")], default=[4096, 65536, 262144])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--summarise", metavar="DIR", help="summarise the kernel trace rocprofv3 wrote under DIR (no GPU needed)")
    args = ap.parse_args()
    summarise(args) if args.summarise else run(args)


if __name__ == "__main__":
    main()

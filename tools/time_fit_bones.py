"""Times dp_fit_bones (include/dragposer_calibration.h) beside the dp_optimize_skeleton launch of the same batch, on recipe S with six
trackers and targets on a skeleton scaled per group (tests/fit_bones_oracle.py), at 64 and 4096 frames:
  fit1 fit3 fit21   dp_fit_rows_kernel + dp_fit_solve_kernel with BoneGroups.uniform / limbs / per_bone (K = 1, 3, 21), ridge 1e-3
  opt50             dp_optimize_skeleton, 50 Adam iterations, offsets = the model's skeleton: the other half of a calibration round
The variants alternate within each size, one process.  Kernel times come from a run of its own under the profiler, no counters in it, and
the trace is then summarised with the launch plan the run wrote beside it --
    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python tools/time_fit_bones.py --rounds 7 --plan DIR/plan.json
    python tools/time_fit_bones.py --summarise DIR/.../t_kernel_trace.csv --plan DIR/plan.json
per variant and size: the launches' median and (max - min) / median, the fit as the sum of its two kernels.
    python tools/time_fit_bones.py --toy
times, outside the profiler and by the host's clock around a synchronise, what a user had before: INTEGRATION.md section 2a's loop at 64
frames, 300 torch.optim.Adam iterations of decode_fk(offsets=s * base) forward + backward on one scalar scale (median of 7)."""
import csv
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

VARIANTS = ("fit1", "fit3", "fit21", "opt50")
GROUPS = {"fit1": "uniform", "fit3": "limbs", "fit21": "per_bone"}
FIT_KERNELS = ("dp_fit_rows_kernel", "dp_fit_solve_kernel")


def summarise(path, plan_path):
    plan = json.load(open(plan_path))
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            if "dp_fit_" in name or "dp_w4" in name:
                rows.append((int(row["Start_Timestamp"]), name, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3))
    rows.sort()
    groups, i = {}, 0
    for B, variant, warm in plan["launches"]:
        if variant == "opt50":
            (_, name, us), i = rows[i], i + 1
            assert "dp_w4" in name, (name, variant)
            parts = (us,)
        else:
            (_, n0, u0), (_, n1, u1), i = rows[i], rows[i + 1], i + 2
            assert FIT_KERNELS[0] in n0 and FIT_KERNELS[1] in n1, (n0, n1, variant)
            parts = (u0 + u1, u0, u1)
        if not warm:
            groups.setdefault((B, variant), []).append(parts)
    assert i == len(rows), (i, len(rows))
    med = {}
    for (B, variant), v in groups.items():
        v = np.asarray(v)
        t = v[:, 0]
        med[B, variant] = float(np.median(t))
        extra = "" if variant == "opt50" else f"  (rows {np.median(v[:, 1]):.2f} us + solve {np.median(v[:, 2]):.2f} us)"
        print(f"B {B:5d}  {variant:6s} n {len(t):3d}  median {np.median(t):9.2f} us  min {t.min():9.2f}  max {t.max():9.2f}  "
              f"(max - min) / median {(t.max() - t.min()) / np.median(t):.4f}{extra}")
    for B in sorted({b for b, _ in med}):
        print(f"B {B:5d}  the fit as a fraction of the optimise launch of 50 iterations: " +
              ", ".join(f"{v} {med[B, v] / med[B, 'opt50']:.3f}" for v in VARIANTS[:3]))


def toy(opt, dev, rounds=7):
    import fit_bones_oracle as FO
    from dragposer_amd import decode_fk
    from dragposer_amd.optimizer import to_device_batch
    from oracle import ref_torch as R

    model = R.OracleModel()
    b = R.synth_inputs(FO.scaled_model(model, FO.UNIFORM, [1.12]), 64, trackers=6, seed=3)
    d = to_device_batch(b, dev)
    z = torch.from_numpy(b["z_src"]).to(dev)
    base = torch.from_numpy(np.ascontiguousarray(opt.host_model.arrays["offsets"], dtype=np.float32)).to(dev)
    trk = d["tracked"].float()
    times, last = [], None
    for _ in range(rounds + 1):  # (the first is the warm-up)
        s = torch.ones((), device=dev, requires_grad=True)
        adam = torch.optim.Adam([s], lr=1e-2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(300):
            o = decode_fk(opt, z, d["cur_rot"], outputs=("pos",), offsets=s * base)
            loss = (((o["pos"] - d["tgt_pos"]) ** 2).sum(-1) * trk).sum() / trk.sum()
            adam.zero_grad()
            loss.backward()
            adam.step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        last = float(s.detach())
    t = np.asarray(times[1:])
    print(f"B    64  the loop of INTEGRATION.md section 2a (300 Adam iterations, one scalar scale, latents at their true values): n {len(t)}  median "
          f"{np.median(t):.1f} ms  min {t.min():.1f}  max {t.max():.1f}  (max - min) / median {(t.max() - t.min()) / np.median(t):.4f}  scale {last:.4f} (true 1.12)")


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 4096])
    ap.add_argument("--rounds", type=int, default=7, help="alternations of the variants per size")
    ap.add_argument("--plan", default="fit_bones_plan.json", help="where the run writes (and --summarise reads) the order of its launches")
    ap.add_argument("--summarise", default=None, metavar="KERNEL_TRACE_CSV", help="summarise a rocprofv3 kernel trace of this tool and exit")
    ap.add_argument("--toy", action="store_true", help="time section 2a's loop by the host's clock instead (not under the profiler)")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.plan)
    import fit_bones_oracle as FO
    from dragposer_amd import BoneGroups
    from dragposer_amd.optimizer import LatentOptimizer, to_device_batch
    from oracle import ref_torch as R

    dev = torch.device("cuda:0")
    opt = LatentOptimizer(device=dev)
    if args.toy:
        return toy(opt, dev, args.rounds)
    model = R.OracleModel()
    base = torch.from_numpy(np.ascontiguousarray(opt.host_model.arrays["offsets"], dtype=np.float32)).to(dev)
    launches = []
    for B in args.sizes:
        d = to_device_batch(R.synth_inputs(FO.scaled_model(model, FO.LIMBS, [1.15, 0.92, 1.08]), B, trackers=6, seed=3), dev)
        out = opt.allocate_outputs(B, names=("z",))
        runs = {"opt50": lambda: opt.optimize(**d, n_iter=50, lambda_tmp=0.0, offsets=base, out=out, outputs=("z",))}
        for v, name in GROUPS.items():
            g = getattr(BoneGroups, name)()
            fo = {k: t for k, t in opt.fit_bones(d["z0"], d["cur_rot"], d["tgt_pos"], d["w"], d["tracked"], g).items()}
            torch.cuda.synchronize()
            launches.append((B, v, True))  # (the call that made the output tensors: a warm-up)
            runs[v] = lambda g=g, fo=fo: opt.fit_bones(d["z0"], d["cur_rot"], d["tgt_pos"], d["w"], d["tracked"], g, out=fo)
        for v in VARIANTS:  # warm-up
            runs[v]()
            torch.cuda.synchronize()
            launches.append((B, v, True))
        for _ in range(args.rounds):
            for v in VARIANTS:
                runs[v]()
                launches.append((B, v, False))
        torch.cuda.synchronize()
        print(f"B {B:5d}  done", flush=True)
    with open(args.plan, "w") as f:
        json.dump(dict(launches=launches), f)


if __name__ == "__main__":
    main()

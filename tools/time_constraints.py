"""Times dp_optimize_constrained against the decode_fk + torch.optim.Adam loop of INTEGRATION.md section 2a on the same loss (tracker +
temporal + one-sided floor) and the same inputs, at 1, 64, 4096 and 16 384 frames, 50 iterations at a fixed count (plus the kernel's
early-stop case).  Wall time per call from HIP events after a warm-up; prints one line per size.  Kernel-only times: run this file
under `rocprofv3 --kernel-trace --stats -- python tools/time_constraints.py` in a separate run."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dragposer_amd import Constraints, decode_fk  # noqa: E402
from dragposer_amd.optimizer import LatentOptimizer, to_device_batch  # noqa: E402
from oracle import ref_torch as R  # noqa: E402

FLOP = 35520  # decoder forward + backward per frame-iteration (the kinematics and terms not counted)


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
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
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 64, 4096, 16384])
    ap.add_argument("--kernel-only", action="store_true", help="launch only dp_optimize_constrained (for a rocprofv3 --kernel-trace run)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    opt = LatentOptimizer(device=dev)
    model = R.OracleModel()
    cons = Constraints(w_feet_floor=1.0, floor_one_sided=True)
    n, lam = 50, 0.02
    for B in args.sizes:
        d = to_device_batch(R.synth_inputs(model, B, seed=B), dev)
        g = torch.zeros(B, 3, device=dev)
        g[:, 1] = 0.9
        k = _time(lambda: opt.optimize_constrained(**d, constraints=cons, global_pos=g, n_iter=n, lambda_tmp=lam), 5)
        ke = _time(lambda: opt.optimize_constrained(**d, constraints=cons, global_pos=g, n_iter=n, lambda_tmp=lam, stop_eps_pos=1e-4,
                                                    stop_eps_rot=1e-2, min_loss_incr=1e-5), 5)
        if args.kernel_only:
            print(f"B={B:6d}  kernel {k * 1e3:8.3f} ms  early-stop {ke * 1e3:8.3f} ms", flush=True)
            continue
        trk = d["tracked"].float()
        E = trk.sum(1)

        def torch_loop():
            z = d["z0"].clone().requires_grad_()
            adam = torch.optim.Adam([z], lr=1e-2)
            for _ in range(n):
                o = decode_fk(opt, z, d["cur_rot"], outputs=("pos", "rot"))
                lp = (((o["pos"] - d["tgt_pos"]) ** 2).sum(-1) * d["w"][..., 0] * trk).sum(1) / (3.0 * E)
                lr_ = (((o["rot"] - d["tgt_rot"]) ** 2).sum(-1) * d["w"][..., 1] * trk).sum(1) / (9.0 * E)
                lt = lam * ((z - d["z_tgt"]) ** 2).mean(1)
                fl = (torch.relu(-(g[:, 1:2] + o["pos"][:, [4, 8], 1])) ** 2).mean(1)
                adam.zero_grad()
                (lp + lr_ + lt + fl).sum().backward()
                adam.step()

        t = _time(torch_loop, 2)
        print(f"B={B:6d}  kernel {k * 1e3:8.3f} ms ({B / k:12.0f} frames/s, {B * n * FLOP / k / 157.3e12:.5f} of 157.3 TF)  "
              f"early-stop {ke * 1e3:8.3f} ms  torch loop {t * 1e3:8.3f} ms  speed-up {t / k:7.1f}x", flush=True)


if __name__ == "__main__":
    main()

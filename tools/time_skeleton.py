"""Cost of per-frame skeletons (include/dragposer_skeleton.h): the dp_w4sk units against the plain units on the same inputs, the variants
alternating (A B A B ...):
  * 4096 frames, 50 iterations at a fixed count, 6 trackers: dp_optimize (context's skeleton) vs dp_optimize_skeleton ([B,22,3], four
    skeletons mixed per wave);
  * whole-sequence launches, S = 1024 sequences over 10 steps: dp_optimize_sequence vs dp_optimize_sequence_skeleton ([S,22,3] rows of the
    context's OWN skeleton: the sequences run the while-condition, and only the same bones -- hence the same bits, tests/test_hip_skeleton.py
    -- make both variants do the same number of iterations; the mean is printed per variant).
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_skeleton.py` and read the stats rows of dp_w4[_bp]_kernel
against dp_w4sk[_bp]_kernel (both layouts: --layout).  Without a profiler it prints wall time per call from HIP events."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dragposer_amd.optimizer import LatentOptimizer, to_device_batch  # noqa: E402
from oracle import ref_torch as R  # noqa: E402


def _time(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps * 1e-3


def _skels(opt, n):
    base = torch.from_numpy(np.asarray(opt.host_model.arrays["offsets"], np.float32))
    f = torch.tensor([1.0, 0.85, 1.2, 1.1])[torch.arange(n) % 4].reshape(n, 1, 1)
    return (base.unsqueeze(0) * f).contiguous().cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--sequences", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layout", type=int, default=-1, help="dp_debug_set_w4_layout: 0 dense, 1 body-part, -1 the context's own choice")
    args = ap.parse_args()
    opt = LatentOptimizer(device="cuda:0")
    if args.layout >= 0:
        torch.cuda.synchronize()
        assert opt.lib.dp_debug_set_w4_layout(opt.ctx, args.layout) == args.layout
    B = args.frames
    batch = to_device_batch(R.synth_inputs(R.OracleModel(), B, trackers=6), opt.device)
    off = _skels(opt, B)
    out = opt.allocate_outputs(B)
    plain = opt.plan(**batch, n_iter=50, lambda_tmp=0.02, kernel="w4", out=out)
    skel = opt.plan(**batch, n_iter=50, lambda_tmp=0.02, kernel="w4", out=out, offsets=off)
    S, T = args.sequences, args.steps
    g = torch.Generator().manual_seed(3)
    E = [0, 4, 8, 13, 17, 21]
    tp = torch.zeros(T, S, 22, 3)
    tp[:, :, E] = 0.4 * torch.randn(T, S, 6, 3, generator=g)
    q = torch.nn.functional.normalize(torch.randn(T, S, 22, 4, generator=g), dim=-1)
    w_, x, y, z = q.unbind(-1)
    tR = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w_ * z), 2 * (x * z + w_ * y), 2 * (x * y + w_ * z), 1 - 2 * (x * x + z * z),
                      2 * (y * z - w_ * x), 2 * (x * z - w_ * y), 2 * (y * z + w_ * x), 1 - 2 * (x * x + y * y)], dim=-1)
    w = torch.zeros(S, 22, 2)
    w[:, E] = torch.tensor([[10.0, 10.0]] + [[5.0, 0.01]] * 5)
    tracked = torch.zeros(S, 22, dtype=torch.uint8)
    tracked[:, E] = 1
    tp, tR, w, tracked = tp.cuda(), tR.contiguous().cuda(), w.cuda(), tracked.cuda()
    soff = torch.from_numpy(np.asarray(opt.host_model.arrays["offsets"], np.float32)).cuda().expand(S, 22, 3).contiguous()
    lat0 = (0.3 * torch.randn(S, 24, generator=g)).cuda()
    zt = torch.zeros(S, 24, device="cuda")

    seq_iters = {}

    def seq(offsets):
        def run():
            st = dict(latent=lat0.clone(), gp=torch.zeros(S, 3, device="cuda"), gr=torch.tensor([1.0, 0, 0, 0], device="cuda").repeat(S, 1),
                      lb=lat0.unsqueeze(1).repeat(1, 4, 1), db=torch.zeros(S, 4, 3, device="cuda"), hb=torch.zeros(S, 4, 6, device="cuda"))
            r = opt.optimize_sequence(st["latent"], tp, tR, None, w, tracked, zt, (0, 24), st["gp"], st["gr"], st["lb"], st["db"], st["hb"],
                                      (0, 4, 8, 13, 17, 21), n_iter=100, lr=1e-2, lambda_tmp=0.0, offsets=offsets)
            seq_iters[offsets is None] = r["iters"]
        return run

    variants = [("frames plain", plain), ("frames skeleton", skel), ("sequences plain", seq(None)), ("sequences skeleton", seq(soff))]
    for _, fn in variants:  # warm-up
        fn()
    torch.cuda.synchronize()
    acc = {n: [] for n, _ in variants}
    for _ in range(args.rounds):
        for n, fn in variants:
            acc[n].append(_time(fn, args.reps))
    for n, v in acc.items():
        print(f"{n:22s} median {np.median(v) * 1e3:8.4f} ms per call (wall, HIP events; {args.rounds} rounds x {args.reps})")
    it_p, it_s = float(seq_iters[True].float().mean()), float(seq_iters[False].float().mean())
    print(f"sequences: mean iterations per step, plain {it_p:.4f}, skeleton {it_s:.4f} (equal: {bool(torch.equal(seq_iters[True], seq_iters[False]))})")
    print(f"ratio frames    {np.median(acc['frames skeleton']) / np.median(acc['frames plain']):.4f}")
    print(f"ratio sequences {np.median(acc['sequences skeleton']) / np.median(acc['sequences plain']):.4f}")


if __name__ == "__main__":
    main()

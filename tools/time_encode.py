"""Time the pose encoder per call -- dp_encode (dragposer_amd.NativePoseEncoder, one launch) and the PyTorch PoseEncoder (about
fourteen ops, what set_initial_pose runs by default) on the same GPU in the same run, the two alternating -- at the sizes
set_initial_pose sees (1, 64, 1024 poses) and the bulk sizes of encoding a data set (65 536, 1 048 576).

Per size and variant: device time per call (torch events around a batch of back-to-back calls) and wall time per call (host clock
around one call and a synchronise).  The device is preconditioned first (the measured launches back to back for PRECONDITION_MS, as
bench.py does, so the shader clock is the one a busy GPU holds).  Also printed: the share of the 157.3 TFLOP/s fp32 MFMA roofline on
the 67 072 useful FLOP per pose and on the FLOP the kernel issues (its padded 16 x 4 blocks, none skipped).
`python tools/time_encode.py [out.txt]`; the results of record are profiles/encode_times.txt."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dragposer_amd.encoder import NativePoseEncoder, PoseEncoder  # noqa: E402

SIZES = (1, 64, 1024, 65536, 1048576)
USEFUL_FLOP = 2 * (112 * 176 + 72 * 112 + 48 * 72 + 48 * 48)  # 67 072 per pose
ISSUED_FLOP = 2 * 16 * 4 * (7 * 44 + 5 * 28 + 3 * 20 + 3 * 12)  # 544 MFMAs of 16 x 16 x 4 per 16 poses = 69 632 per pose
PEAK = 157.3e12
PRECONDITION_MS = 60.0


def _device_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def _wall_us(fn, n):
    torch.cuda.synchronize()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    t.sort()
    return t[len(t) // 2] * 1e6  # median


def main():
    dev = torch.device("cuda:0")
    native, eager = NativePoseEncoder(device=dev), PoseEncoder().to(dev)
    lines = [f"{torch.cuda.get_device_name(0)}; per pose {USEFUL_FLOP} useful FLOP, {ISSUED_FLOP} issued (no block skipped), "
             f"{4 * (176 + 24 + 3 * 24 + 1)} B of HBM traffic; roofline {PEAK / 1e12:.1f} TFLOP/s fp32 MFMA"]
    for n in SIZES:
        g = torch.Generator().manual_seed(n)
        x, e = torch.randn(n, 176, generator=g).to(dev), torch.randn(n, 24, generator=g).to(dev)
        out = native.encode(x, eps=e)

        def hip():
            native.encode(x, eps=e, out=out)

        def torch_path():
            with torch.no_grad():
                mu, lv = eager(x)
                return mu + e * torch.exp(0.5 * lv), mu, lv

        reps = 200 if n <= 65536 else 20
        per = max(_device_us(hip, 5), 1.0)
        for _ in range(min(20000, int(PRECONDITION_MS * 1e3 / per) + 1)):
            hip()
        dev_us, wall_us = {"hip": [], "torch": []}, {"hip": [], "torch": []}
        for _ in range(3):  # the variants alternate
            for name, fn in (("hip", hip), ("torch", torch_path)):
                dev_us[name].append(_device_us(fn, reps))
                wall_us[name].append(_wall_us(fn, max(reps // 10, 5)))
        d = {k: min(v) for k, v in dev_us.items()}
        w = {k: min(v) for k, v in wall_us.items()}
        lines.append(f"n={n}: dp_encode {d['hip']:.1f} us device, {w['hip']:.1f} us wall per call; torch PoseEncoder {d['torch']:.1f} us device, "
                     f"{w['torch']:.1f} us wall ({d['torch'] / d['hip']:.2f}x device, {w['torch'] / w['hip']:.2f}x wall); dp_encode "
                     f"{n * USEFUL_FLOP / d['hip'] / 1e6:.2f} TFLOP/s useful = {100 * n * USEFUL_FLOP / (d['hip'] * 1e-6) / PEAK:.1f} % of the roofline, "
                     f"{100 * n * ISSUED_FLOP / (d['hip'] * 1e-6) / PEAK:.1f} % on the FLOP issued")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

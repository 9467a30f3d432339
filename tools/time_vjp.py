"""Time dp_forward_vjp (all six upstream gradients) at 4096 / 65536 / 262144 frames, and torch autograd through oracle.ref_torch (fp32,
same GPU) beside it.  Wall-clock per call from torch events after warm-up; the kernel's own time is what
`rocprofv3 --kernel-trace --stats -- python tools/time_vjp.py` reports for dp_vjp_kernel.  Prints one line per size and the
FLOP / byte model the roofline share is computed from (profiles/vjp_times.txt)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dragposer_amd.optimizer import LatentOptimizer  # noqa: E402
from oracle import ref_torch as R  # noqa: E402

SHAPES = {"pose": (88,), "disp": (3,), "world_disp": (3,), "world_rot": (4,), "pos": (22, 3), "rot": (22, 9)}
# per frame: the decoder forward (24x40 + 40x60 + 92x60 products, the 91 rows used) and its transpose, 2 FLOP per multiply-add
FLOP = 2 * (24 * 40 + 40 * 60 + 91 * 60) * 2
BYTES = 4 * (24 + 4 + sum(int(torch.tensor(s).prod()) for s in SHAPES.values()) + 24 + 4 + 1)


def _events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3  # us


def main():
    dev = torch.device("cuda:0")
    opt = LatentOptimizer(device=dev)
    m = R.OracleModel()
    for k in ("Wf", "bf", "mu4", "sd4", "mu_d", "sd_d", "offsets"):
        setattr(m, k, getattr(m, k).to(dev))
    m.U, m.W, m.b = [u.to(dev) for u in m.U], [w.to(dev) for w in m.W], [b.to(dev) for b in m.b]
    print(f"model: {FLOP} FLOP/frame, {BYTES} B/frame of HBM traffic")
    for B in (4096, 65536, 262144):
        g = torch.Generator(device="cpu").manual_seed(B)
        z = (torch.randn(B, 24, generator=g) * 0.5).to(dev)
        cr = torch.nn.functional.normalize(torch.randn(B, 4, generator=g), dim=-1).to(dev)
        grads = {n: torch.randn((B,) + s, generator=g).to(dev) for n, s in SHAPES.items()}
        out = {"dz": torch.empty(B, 24, device=dev), "dcur_rot": torch.empty(B, 4, device=dev),
               "status": torch.empty(B, dtype=torch.int32, device=dev)}
        call = lambda: opt.forward_vjp(z, cr, grads, out=out)  # noqa: E731
        _events(call, 20)
        us = _events(call, 200)

        def autograd():
            zt = z.clone().requires_grad_()
            ct = cr.clone().requires_grad_()
            motion, disp = R.decoder_forward(m, zt)
            wd, wr, pos, rot, d = R.pose_fk(m, motion, disp, ct)
            outs = dict(pose=motion, disp=d, world_disp=wd, world_rot=wr, pos=pos, rot=rot.reshape(-1, 22, 9))
            L = sum((outs[n] * grads[n]).sum() for n in SHAPES)
            torch.autograd.grad(L, (zt, ct))

        _events(autograd, 3)
        ta = _events(autograd, 10)
        print(f"B={B}: dp_forward_vjp {us:.1f} us/call (wall, events) = {B * FLOP / us / 1e6:.2f} TFLOP/s, {B * BYTES / us / 1e6:.3f} TB/s; "
              f"torch autograd through oracle.ref_torch fp32 {ta:.1f} us/call ({ta / us:.1f}x)")


if __name__ == "__main__":
    main()

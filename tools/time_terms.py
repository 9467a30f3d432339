"""Times dp_optimize_terms: the reference block as a table (Terms.from_constraints(Constraints.reference())) against
dp_optimize_constrained(Constraints.reference()), and a 3-term custom table (a hand above a table, the knees apart, the head facing +x)
against the decode_fk + torch.optim.Adam loop on the same loss, at 1, 4096 and 16 384 frames, 50 iterations at a fixed count.  The
variants alternate within each size (A B A B ...).  Wall time per call from HIP events after a warm-up; one line per size.  Kernel-only
times: run `rocprofv3 --kernel-trace --stats -- python tools/time_terms.py --kernel-only` in a separate run (dp_cons_kernel is the
four-term kernel, dp_terms_kernel the table)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dragposer_amd import Constraints, Term, Terms, decode_fk  # noqa: E402
from dragposer_amd.optimizer import LatentOptimizer, to_device_batch  # noqa: E402
from oracle import ref_torch as R  # noqa: E402


def custom():
    return Terms([Term.plane(17, (0, 1, 0), (0, -0.2, 0), weight=2.0, one_sided=True),
                  Term.distance(2, 6, lo=0.25, hi=10.0, weight=4.0, drop_up=True),
                  Term.align(13, (0, 0, 1), dir=(1, 0, 0), threshold=0.2, margin=0.0, weight=0.5, drop_up=True)])


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
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 4096, 16384])
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the variants per size")
    ap.add_argument("--kernel-only", action="store_true", help="no torch loop (for a rocprofv3 --kernel-trace run)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    opt = LatentOptimizer(device=dev)
    model = R.OracleModel()
    cons = Constraints.reference()
    table, cust = Terms.from_constraints(cons), custom()
    n, lam = 50, 0.02
    for B in args.sizes:
        d = to_device_batch(R.synth_inputs(model, B, seed=B), dev)
        g = torch.zeros(B, 3, device=dev)
        g[:, 1] = 0.9
        trk = d["tracked"].float()
        E = trk.sum(1)

        def torch_loop():
            z = d["z0"].clone().requires_grad_()
            adam = torch.optim.Adam([z], lr=1e-2)
            for _ in range(n):
                o = decode_fk(opt, z, d["cur_rot"], outputs=("pos", "rot"))
                pos, rot = o["pos"], o["rot"].reshape(B, 22, 3, 3)
                lp = (((pos - d["tgt_pos"]) ** 2).sum(-1) * d["w"][..., 0] * trk).sum(1) / (3.0 * E)
                lr_ = (((o["rot"] - d["tgt_rot"]) ** 2).sum(-1) * d["w"][..., 1] * trk).sum(1) / (9.0 * E)
                lt = lam * ((z - d["z_tgt"]) ** 2).mean(1)
                hand = 2.0 * torch.relu(-(g[:, 1] + pos[:, 17, 1] + 0.2)) ** 2
                u = (pos[:, 2] - pos[:, 6])[:, [0, 2]]
                knees = 4.0 * torch.relu(0.25 ** 2 - (u ** 2).sum(-1))
                a = (rot[:, 13, :, 2])[:, [0, 2]]
                na = a.norm(dim=-1)
                c = a[:, 0] / na
                head = torch.where(na > 0.2, 0.5 * (1.0 - torch.clamp(c, max=1.0)) ** 2, torch.zeros_like(c))
                adam.zero_grad()
                (lp + lr_ + lt + hand + knees + head).sum().backward()
                adam.step()

        runs = {
            "constrained": lambda: opt.optimize_constrained(**d, constraints=cons, global_pos=g, n_iter=n, lambda_tmp=lam),
            "table": lambda: opt.optimize_terms(**d, terms=table, global_pos=g, n_iter=n, lambda_tmp=lam),
            "custom": lambda: opt.optimize_terms(**d, terms=cust, global_pos=g, n_iter=n, lambda_tmp=lam),
        }
        if not args.kernel_only:
            runs["torch_loop"] = torch_loop
        for fn in runs.values():  # warm-up
            fn()
        torch.cuda.synchronize()
        best = {k: float("inf") for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                best[k] = min(best[k], _time(fn, 1 if k == "torch_loop" else 5))
        line = f"B={B:6d}  " + "  ".join(f"{k} {v * 1e3:8.3f} ms" for k, v in best.items())
        line += f"  table/constrained {best['table'] / best['constrained']:.3f}"
        if "torch_loop" in best:
            line += f"  torch_loop/custom {best['torch_loop'] / best['custom']:.1f}x"
        print(line, flush=True)


if __name__ == "__main__":
    main()

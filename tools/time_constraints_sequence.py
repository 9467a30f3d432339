"""A constrained clip: the frame loop in one launch (dp_cons_seq.hip) against the per-frame path it replaces.
S sequences x T = 64 frames, 6 trackers, Constraints.reference() and the same block as a term table, two loop settings -- `early`: max_iter
10 with the reference's early stop, `fixed`: 50 iterations at a fixed count -- and per (S, setting, kind) two variants, alternating
(A B A B ...), each from the same initial state:
  * per-frame  what DragPose.run(constraints=...) does: T x (dp_optimize_constrained / dp_optimize_terms, dp_sequence_advance, a device
               copy of the latent), driven from Python;
  * sequence   dp_optimize_sequence_constrained / dp_optimize_sequence_terms: one launch, and one for the history buffers.
One process; before the timed rounds the device is preconditioned as bench.py does (the measured launch back to back for 60 ms of GPU
time).  Without a profiler it prints wall time per clip from a host clock around work that ends in a device synchronise, every variant's
median, extremes and (max - min) / median, and the ratio.  Kernel times: one run per loop setting under the profiler, then the trace
summarised by kernel and launch size --
    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python tools/time_constraints_sequence.py --loop early --rounds 3
    python tools/time_constraints_sequence.py --loop early --summarise DIR/.../t_kernel_trace.csv
prints, per kernel and S, the number of launches, the median, the extremes and the spread, and per clip T x (optimise + advance) against
sequence + history (the per-frame path's latent copy is not a kernel of the library and is left out: the ratio flatters that path)."""
import argparse
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T = 64
SIZES = (1, 64, 1024)
LOOPS = {"early": dict(n_iter=10, stop_eps_pos=0.01 * 0.01, stop_eps_rot=0.01, min_loss_incr=0.00001),
         "fixed": dict(n_iter=50, stop_eps_pos=0.0, stop_eps_rot=0.0, min_loss_incr=-1e30)}
HJ = (0, 4, 8, 13, 17, 21)
PER_FRAME = {"cons": "dp_cons_kernel", "terms": "dp_terms_kernel"}
SEQUENCE = {"cons": "dp_cons_seq_kernel", "terms": "dp_terms_seq_kernel"}
PRECONDITION_MS = 60.0


def summarise(path, sizes):
    """rocprofv3's kernel trace -> per (kernel, S): durations in microseconds (the first launch of each, its warm-up, dropped)"""
    # (the trace's grid is in work-items) the optimise kernels: a workgroup of 512 per 8 frames / sequences; the epilogue kernels: one of 64 per sequence
    wave = {}
    for S in sizes:
        wave.update({("opt", (S + 7) // 8 * 512): S, ("epi", S * 64): S})
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"].split("(")[0]
            if name.startswith("dp_sequence_"):
                S = wave.get(("epi", int(row["Grid_Size_X"]))) if int(row["Workgroup_Size_X"]) == 64 else None
            elif name in tuple(PER_FRAME.values()) + tuple(SEQUENCE.values()):
                S = wave.get(("opt", int(row["Grid_Size_X"])))
            else:
                continue
            if S is not None:
                groups.setdefault((name, S), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    med, spread = {}, {}
    for (name, S), v in sorted(groups.items()):
        v = np.asarray(v[1:])
        med[name, S], spread[name, S] = np.median(v), (v.max() - v.min()) / np.median(v)
        print(f"{name:28s} S {S:5d}  n {len(v):5d}  median {np.median(v):9.2f} us  min {v.min():9.2f}  max {v.max():9.2f}  "
              f"(max - min) / median {spread[name, S]:.4f}")
    adv, hist = "dp_sequence_advance_kernel", "dp_sequence_history_kernel"
    for kind in ("cons", "terms"):
        for S in sizes:
            keys = ((PER_FRAME[kind], S), (adv, S), (SEQUENCE[kind], S), (hist, S))
            if all(k in med for k in keys):
                a, b = T * (med[keys[0]] + med[keys[1]]), med[keys[2]] + med[keys[3]]
                print(f"{kind:6s} S {S:5d}: per clip, kernel time  per-frame {a * 1e-3:9.3f} ms  sequence {b * 1e-3:9.3f} ms  per-frame / sequence {a / b:6.3f}"
                      f"   (the per-frame kernel's own spread {spread[keys[0]]:.4f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--loop", choices=tuple(LOOPS) + ("both",), default="both")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="no GPU work: summarise a rocprofv3 kernel trace of a run with the same --sequences")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.sequences)
    import torch

    from dragposer_amd import Constraints, Terms
    from dragposer_amd.optimizer import LatentOptimizer, to_device_batch
    from oracle import ref_torch as R

    dev = torch.device("cuda:0")
    opt = LatentOptimizer(device=dev)
    cons = Constraints.reference()
    ext = {"cons": cons, "terms": Terms.from_constraints(cons)}
    loops = tuple(LOOPS) if args.loop == "both" else (args.loop,)
    print(f"T = {T} frames per clip; wall time per clip, host clock around a device synchronise, {args.rounds} rounds, the variants alternating; "
          f"preconditioned with {PRECONDITION_MS:.0f} ms of the sequence launch")
    for S in args.sequences:
        d = to_device_batch(R.synth_inputs(R.OracleModel(), T * S, trackers=6, seed=S), dev)
        tp, tR = d["tgt_pos"].reshape(T, S, 22, 3), d["tgt_rot"].reshape(T, S, 22, 9)
        z_tgt = d["z_tgt"].reshape(T, S, 24)
        w, tracked = d["w"][:S].contiguous(), d["tracked"][:S].contiguous()
        init = dict(latent=d["z0"][:S].clone(), gpos=torch.zeros(S, 3, device=dev), grot=d["cur_rot"][:S].clone(),
                    lbuf=d["z0"][:S].unsqueeze(1).repeat(1, 60, 1), dbuf=torch.zeros(S, 60, 3, device=dev), hbuf=torch.zeros(S, 60, len(HJ), device=dev))
        init["gpos"][:, 1] = 0.9
        st = {k: v.clone() for k, v in init.items()}
        pose, pos = torch.empty(T, S, 88, device=dev), torch.empty(T, S, 3, device=dev)
        iters, status = torch.empty(T, S, dtype=torch.int32, device=dev), torch.empty(T, S, dtype=torch.int32, device=dev)
        loss, scratch = torch.empty(T, S, 3, device=dev), torch.empty(T, S, 24 + 3 + len(HJ), device=dev)
        for lname in loops:
            loop = LOOPS[lname]
            for kind in ("cons", "terms"):
                key, width = ("loss_extra", 4) if kind == "cons" else ("loss_terms", len(ext[kind]))
                fr = opt.allocate_outputs(S, ("z", "z_pre", "pose", "disp", "world_disp", "world_rot", "pos", "loss", "iters", "status"))
                fr[key] = torch.empty(S, width, device=dev)
                per_step = torch.empty(T, S, width, device=dev)
                jpos = torch.empty(T, S, 22, 3, device=dev)
                run = opt.optimize_constrained if kind == "cons" else opt.optimize_terms

                def per_frame():
                    for t in range(T):
                        run(st["latent"], z_tgt[t], st["grot"], tp[t], tR[t], w, tracked, ext[kind], global_pos=st["gpos"], lr=1e-2, lambda_rot=1.0,
                            lambda_tmp=0.02, out=fr, outputs=tuple(fr), **loop)
                        opt.sequence_advance(fr, st["gpos"], st["grot"], st["lbuf"], st["dbuf"], st["hbuf"], HJ, pose_ret=pose[t], pos_ret=pos[t])
                        st["latent"].copy_(fr["z"])

                def sequence():
                    opt.optimize_sequence(st["latent"], tp, tR, None, w, tracked, z_tgt, (S * 24, 24), st["gpos"], st["grot"], st["lbuf"], st["dbuf"],
                                          st["hbuf"], HJ, lr=1e-2, lambda_rot=1.0, lambda_tmp=0.02, pose_ret=pose, pos_ret=pos, iters=iters, loss=loss,
                                          scratch=scratch, status=status, **{"constraints" if kind == "cons" else "terms": ext[kind], key: per_step,
                                                                             "joint_pos": jpos}, **loop)

                def clip(fn):
                    for k, v in init.items():
                        st[k].copy_(v)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0

                per = clip(sequence)  # (also the first launch of this shape: code object loaded)
                clip(per_frame)
                for _ in range(min(20000, int(PRECONDITION_MS * 1e-3 / max(clip(sequence), 1e-6)) + 1)):
                    sequence()
                torch.cuda.synchronize()
                acc = {"per-frame": [], "sequence": []}
                for _ in range(args.rounds):
                    acc["per-frame"].append(clip(per_frame))
                    acc["sequence"].append(clip(sequence))
                mean_it = float(iters.float().mean())
                for n, v in acc.items():
                    v = np.asarray(v) * 1e3
                    print(f"S {S:5d} {lname:5s} {kind:5s} {n:9s} median {np.median(v):9.3f} ms  min {v.min():9.3f}  max {v.max():9.3f}  "
                          f"(max - min) / median {(v.max() - v.min()) / np.median(v):.4f}")
                print(f"S {S:5d} {lname:5s} {kind:5s} per-frame / sequence {np.median(acc['per-frame']) / np.median(acc['sequence']):7.2f}   "
                      f"(mean iterations per frame {mean_it:.1f}, first sequence launch {per * 1e3:.3f} ms)", flush=True)


if __name__ == "__main__":
    main()

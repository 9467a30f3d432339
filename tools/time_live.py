"""The live step (dp_cons_live.hip): what appending the frame's history row inside the kernel saves a live frame.
6 trackers, Terms.from_constraints(Constraints.reference()) plus two held horizontal soft pins on joints 4 and 8, a dense order-2 latent
predictor, Gaps(16, 0.9), max_iter 10 with the reference's early stop; S = 1 and S = 64 sequences.  Two variants, alternating in one process
in rounds of --frames frames (A B A B ...), every round from the same initial state and fed the same frames, so every round of both variants
is the same work and ends on the same bits:
  * (a) gaps   dp_optimize_sequence_gaps with one step: dp_terms_gap_ar_seq_kernel, then dp_sequence_history_kernel (two launches);
  * (b) live   dp_live_step: dp_live_ar_kernel (one launch).
Without arguments (profiler off) it prints
  * the wall time per one-step call of LatentOptimizer.optimize_sequence, host clock around a round that ends in a device synchronise;
  * the wall time per drag_pose_present call of libDragPoserDLL.so (one performer: S = 1), two handles configured alike, one of them sent
    through the two-launch call by the plug-in's private measuring hook;
per variant the median over the rounds, the extremes, (a)'s own (max - min) / median, and b / a.  Kernel times: a run of its own under the
profiler, then the trace summarised --
    rocprofv3 --kernel-trace --stats -d DIR -o t --output-format csv -- python tools/time_live.py --kernels-only
    python tools/time_live.py --summarise DIR/.../t_kernel_trace.csv
prints per kernel and S the launches' median and extremes, and per S the kernel time per frame of (a) (its two kernels, frame by frame) and
(b), by rounds as above."""
import argparse
import csv
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T = 64
SIZES = (1, 64)
LOOP = dict(n_iter=10, stop_eps_pos=0.01 * 0.01, stop_eps_rot=0.01, min_loss_incr=0.00001)
HJ = (0, 4, 8, 13, 17, 21)
GAP, HIST, LIVE = "dp_terms_gap_ar_seq_kernel", "dp_sequence_history_kernel", "dp_live_ar_kernel"


def _line(name, v, unit):
    v = np.asarray(v)
    print(f"  {name:46s} median {np.median(v):9.3f} {unit}  min {v.min():9.3f}  max {v.max():9.3f}  (max - min) / median {(v.max() - v.min()) / np.median(v):.4f}")
    return float(np.median(v)), float((v.max() - v.min()) / np.median(v))


def summarise(path, sizes, frames, warmup):
    """rocprofv3's kernel trace of --kernels-only -> per S the kernel time per frame of both variants, by rounds of `frames` frames"""
    step_grid = {(S + 7) // 8 * 512: S for S in sizes}  # (work-items: a workgroup of 512 per 8 sequences)
    hist_grid = {S * 64: S for S in sizes}              # (a workgroup of 64 per sequence)
    d = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"].split("(")[0]
            if name in (GAP, HIST, LIVE):
                S = (hist_grid if name == HIST else step_grid).get(int(row["Grid_Size_X"]))
                if S is not None:
                    d.setdefault((name, S), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    for S in sizes:
        if (LIVE, S) not in d:
            continue
        gap, hist, live = (np.asarray(d[k, S][warmup:]) for k in (GAP, HIST, LIVE))  # (each variant's warm-up frames come first)
        n = min(len(gap), len(hist), len(live)) // frames * frames
        print(f"S {S}: kernel time, {n} frames per variant after {warmup} warm-up frames, rounds of {frames}")
        _line(GAP + " per launch", gap[:n], "us")
        _line(HIST + " per launch", hist[:n], "us")
        _line(LIVE + " per launch", live[:n], "us")
        a = (gap[:n] + hist[:n]).reshape(-1, frames).mean(axis=1)
        b = live[:n].reshape(-1, frames).mean(axis=1)
        ma, sa = _line("(a) gaps + history, per frame, by round", a, "us")
        mb, _ = _line("(b) live, per frame, by round", b, "us")
        print(f"  b / a {mb / ma:.4f}   ((a)'s own (max - min) / median {sa:.4f}; a - b {ma - mb:.3f} us per frame)")


class F3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class F2(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class Qt(C.Structure):
    _fields_ = [("w", C.c_float), ("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


def _plugin(table, holds, ar, gaps, cr0, two_launch):
    from dragposer_amd import _lib as L
    from oracle import ref_torch as R

    L.load()
    lib = C.CDLL(os.path.join(ROOT, "dragposer_amd", "lib", "libDragPoserDLL.so"))
    lib.init_drag_poser.restype = C.c_void_p
    lib.drag_poser_last_error.restype = C.c_char_p
    for name, args in (("drag_poser_last_error", [C.c_void_p]), ("set_reference_skeleton", [C.c_void_p, C.c_char_p]), ("load_models", [C.c_void_p, C.c_char_p]),
                       ("set_mask_and_weights", [C.c_void_p, C.POINTER(C.c_float), C.POINTER(F2)]), ("init_drag_model", [C.c_void_p, F3, Qt]),
                       ("set_optim_params", [C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_float]), ("set_lambdas", [C.c_void_p, C.c_float, C.c_float, C.c_int]),
                       ("drag_poser_set_terms", [C.c_void_p, C.c_int, C.POINTER(L.DpTerm), C.c_int]), ("drag_poser_set_holds", [C.c_void_p, C.c_int, C.POINTER(L.DpHold)]),
                       ("drag_poser_set_gaps", [C.c_void_p, C.c_int, C.c_float]), ("drag_poser_debug_two_launch", [C.c_void_p, C.c_int]),
                       ("drag_poser_set_latent_ar", [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
                       ("drag_pose_present", [C.c_void_p, C.c_int, C.POINTER(F3), C.POINTER(Qt), C.POINTER(C.c_ubyte), C.POINTER(Qt), C.POINTER(F3)]),
                       ("drag_poser_get_latent", [C.c_void_p, C.POINTER(C.c_float)]), ("destroy_drag_poser", [C.c_void_p])):
        getattr(lib, name).argtypes = args
    h = lib.init_drag_poser()
    lib.set_reference_skeleton(h, os.path.join(ROOT, "tests", "data", "example_clip.bvh").encode())
    lib.load_models(h, os.path.join(ROOT, "dragposer_amd", "data").encode())
    mask, w = np.zeros(22, np.float32), np.ones((22, 2), np.float32)
    mask[R.TRACK6] = 1
    for j, wj in R.W6.items():
        w[j] = wj
    lib.set_mask_and_weights(h, mask.ctypes.data_as(C.POINTER(C.c_float)), w.ctypes.data_as(C.POINTER(F2)))
    lib.set_optim_params(h, 1e-4, 1e-2, 10, 1e-2)
    lib.init_drag_model(h, F3(0.0, 0.9, 0.0), Qt(*[float(v) for v in cr0]))
    arr = (L.DpTerm * len(table))(*[t.to_struct() for t in table.terms])
    lib.drag_poser_set_terms(h, len(table), arr, table.up_axis)
    harr = (L.DpHold * len(holds.holds))(*[L.DpHold(term=x.term, level=x.level, contact_lo=x.contact_lo, contact_hi=x.contact_hi) for x in holds.holds])
    lib.drag_poser_set_holds(h, len(holds.holds), harr)
    A, c = np.ascontiguousarray(ar.A, np.float32), np.ascontiguousarray(ar.c, np.float32)
    lib.drag_poser_set_latent_ar(h, ar.order, A.ctypes.data_as(C.POINTER(C.c_float)), c.ctypes.data_as(C.POINTER(C.c_float)))
    lib.drag_poser_set_gaps(h, gaps.max_hold, gaps.decay)
    lib.set_lambdas(h, 1.0, 0.02, 0)
    lib.drag_poser_debug_two_launch(h, 1 if two_launch else 0)
    assert lib.drag_poser_last_error(h) == b"", lib.drag_poser_last_error(h)
    return lib, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--frames", type=int, default=256, help="frames per round and variant (a multiple of the 64-frame clip: every round sees the same frames)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=256, help="frames per variant before the first round")
    ap.add_argument("--kernels-only", action="store_true", help="the library calls alone (the run under the profiler)")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="no GPU work: summarise a rocprofv3 kernel trace of a --kernels-only run with the same arguments")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.sequences, args.frames, args.warmup)
    import torch

    from dragposer_amd import Constraints, Gaps, Hold, Holds, LatentAR, Term, Terms
    from dragposer_amd.optimizer import LatentOptimizer, to_device_batch
    from oracle import ref_torch as R

    dev = torch.device("cuda:0")
    opt = LatentOptimizer(device=dev)
    base = Terms.from_constraints(Constraints.reference())
    pins = [Term.distance(j, point=(0.0, 0.0, 0.0), lo=0.0, hi=0.0, weight=1.0, drop_up=True) for j in (4, 8)]
    table = Terms(base.terms + pins, base.up_axis)
    holds = Holds([Hold(len(base), 0.95, 1.0), Hold(len(base) + 1, 0.95, 1.0)])
    g = np.random.default_rng(7)
    A = g.standard_normal((2, 24, 24)) * (0.6 / (2 * np.sqrt(24.0)))
    A[0] += 0.3 * np.eye(24)
    ar, gaps = LatentAR(A, 0.05 * g.standard_normal(24)), Gaps(16, 0.9)
    print(f"{args.rounds} rounds of {args.frames} frames per variant, the variants alternating, after {args.warmup} warm-up frames each; "
          f"max_iter 10 with the early stop; order 2; Gaps(16, 0.9); every sample present")
    for S in args.sequences:
        d = to_device_batch(R.synth_inputs(R.OracleModel(), T * S, trackers=6, seed=S), dev)
        tp, tR = d["tgt_pos"].reshape(T, S, 22, 3), d["tgt_rot"].reshape(T, S, 22, 9)
        w, tracked = d["w"][:S].contiguous(), d["tracked"][:S].contiguous()

        def fresh():
            st = dict(latent=d["z0"][:S].clone(), gpos=torch.zeros(S, 3, device=dev), grot=d["cur_rot"][:S].clone(),
                      lbuf=d["z0"][:S].unsqueeze(1).repeat(1, 60, 1), dbuf=torch.zeros(S, 60, 3, device=dev), hbuf=torch.zeros(S, 60, len(HJ), device=dev),
                      hold=torch.zeros(S, 2, 4, device=dev), gap=torch.zeros(S, 22, 16, device=dev), t=0)
            st["gpos"][:, 1] = 0.9
            st["out"] = dict(pose_ret=torch.empty(1, S, 88, device=dev), pos_ret=torch.empty(1, S, 3, device=dev), iters=torch.empty(1, S, dtype=torch.int32, device=dev),
                             status=torch.empty(1, S, dtype=torch.int32, device=dev), loss=torch.empty(1, S, 3, device=dev),
                             scratch=torch.empty(1, S, 24 + 3 + len(HJ), device=dev), loss_terms=torch.empty(1, S, len(table), device=dev),
                             joint_pos=torch.empty(1, S, 22, 3, device=dev), gap_trace=torch.zeros(1, S, 22, dtype=torch.uint8, device=dev))
            return st

        states = {"gaps": fresh(), "live": fresh()}
        init = {k: v.clone() for k, v in states["gaps"].items() if k not in ("t", "out")}

        def frame(name):
            st = states[name]
            t = st["t"] % T
            st["t"] += 1
            opt.optimize_sequence(st["latent"], tp[t:t + 1], tR[t:t + 1], None, w, tracked, None, (0, 0), st["gpos"], st["grot"], st["lbuf"], st["dbuf"],
                                  st["hbuf"], HJ, lr=1e-2, lambda_rot=1.0, lambda_tmp=0.02, terms=table, holds=holds, hold_state=st["hold"], ar=ar, gaps=gaps,
                                  gap_state=st["gap"], live=name == "live", **st["out"], **LOOP)

        def round_of(name, n):
            st = states[name]
            for k, v in init.items():  # every round is the same work: the same frames from the same state
                st[k].copy_(v)
            st["t"] = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                frame(name)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e6

        for name in states:
            round_of(name, args.warmup)
        acc = {name: [] for name in states}
        for _ in range(args.rounds):
            for name in states:
                acc[name].append(round_of(name, args.frames))
        same = all(torch.equal(states["gaps"][k].view(torch.int32), states["live"][k].view(torch.int32)) for k in ("latent", "lbuf", "dbuf", "hbuf", "gap", "hold"))
        its = float(states["live"]["out"]["iters"].float().mean())
        print(f"S {S}: wall time per one-step call of optimize_sequence (both variants ended on the same bits: {same}; iterations of the last frame {its:.1f})")
        ma, sa = _line("(a) gaps: two launches", acc["gaps"], "us")
        mb, _ = _line("(b) live: one launch", acc["live"], "us")
        print(f"  b / a {mb / ma:.4f}   ((a)'s own (max - min) / median {sa:.4f}; a - b {ma - mb:.3f} us per frame)", flush=True)
    if args.kernels_only:
        return
    # the plug-in: one performer per handle
    m = R.OracleModel()
    b = R.synth_inputs(m, T, trackers=6, seed=1)
    idx = np.array(R.TRACK6)
    quats = np.array([[1.0, 0, 0, 0], [0.5, 0.5, 0.5, 0.5], [0.5, -0.5, 0.5, 0.5], [0, 1.0, 0, 0]])
    tq = quats[np.random.default_rng(3).integers(0, 4, size=(T, 6))]
    tps = [(F3 * 6)(*[F3(*map(float, p)) for p in b["tgt_pos"][t, idx]]) for t in range(T)]
    tqs = [(Qt * 6)(*[Qt(*map(float, q)) for q in tq[t]]) for t in range(T)]
    prs = (C.c_ubyte * 6)(1, 1, 1, 1, 1, 1)
    handles = {"gaps": _plugin(table, holds, ar, gaps, b["cur_rot"][0], True), "live": _plugin(table, holds, ar, gaps, b["cur_rot"][0], False)}
    res_pose, res_pos, at = (Qt * 22)(), (F3 * 1)(), {"gaps": 0, "live": 0}

    def calls(name, n):
        lib, h = handles[name]
        t0 = time.perf_counter()
        for _ in range(n):
            t = at[name] % T
            at[name] += 1
            lib.drag_pose_present(h, 6, tps[t], tqs[t], prs, res_pose, res_pos)
        dt = (time.perf_counter() - t0) / n * 1e6
        assert lib.drag_poser_last_error(h) == b"", lib.drag_poser_last_error(h)
        return dt

    for name in handles:
        calls(name, args.warmup)
    acc = {name: [] for name in handles}
    for _ in range(args.rounds):
        for name in handles:
            acc[name].append(calls(name, args.frames))
    z = {}
    for name, (lib, h) in handles.items():
        z[name] = np.zeros(24, np.float32)
        lib.drag_poser_get_latent(h, z[name].ctypes.data_as(C.POINTER(C.c_float)))
        lib.destroy_drag_poser(h)
    print(f"plug-in, S 1: wall time per drag_pose_present call, upload, launch(es), download and synchronise (both handles ended on the same latent: "
          f"{bool(np.array_equal(z['gaps'], z['live']))})")
    ma, sa = _line("(a) the two-launch call", acc["gaps"], "us")
    mb, _ = _line("(b) dp_live_step", acc["live"], "us")
    print(f"  b / a {mb / ma:.4f}   ((a)'s own (max - min) / median {sa:.4f}; a - b {ma - mb:.3f} us per frame)", flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Every refusal of the optimise / forward entry points of the C ABI, one line per malformed call:

    entry point | case | return code | dp_last_error

Host-only: every call runs on a dp_debug_host_ctx context (no device, no device memory), so nothing is launched and no GPU is
needed.  Two builds of the library refuse alike when their tables are equal:

    python tools/abi_refusals.py --lib A/libdragposer_hip.so > a.txt;  python tools/abi_refusals.py --lib B/libdragposer_hip.so > b.txt;  diff a.txt b.txt

(the same for libdragposer_hip_ref8.so).  A case is the well-formed call with one or two defects; a defect is `benign` when the
library accepts it (an optional pointer left NULL, a struct_size that is exact or larger with a zeroed tail).  A call whose
defects are all benign passes every argument check and is refused for the missing device image (DP_ERR_DEVICE).
--skip-unrefused-plain leaves those rows of dp_optimize, dp_forward and dp_optimize_sequence out, and dp_optimize's unknown kernel
selector, the one refusal that comes after everything else: a library older than that test of theirs must not be given them.  dp_sequence_advance needs no device image; a call that passes its checks goes to the
HIP runtime, whose answer depends on the machine, so its rows of that kind are never issued.
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dragposer_amd import _lib  # noqa: E402

PTR = 0x10000  # stands for a device pointer: never dereferenced on a context without a device
PLAIN = ("dp_optimize", "dp_forward", "dp_optimize_sequence")
BATCH_PTRS = ("z0", "z_tgt", "cur_rot", "tgt_pos", "tgt_rot", "w", "tracked")
_last = {T: T._fields_[-1][0] for T in (_lib.DpParams, _lib.DpResult, _lib.DpSeqResults, _lib.DpSkeletonIn, _lib.DpGradIn,
                                        _lib.DpConstraints, _lib.DpTerms, _lib.DpHolds, _lib.DpLatentAR, _lib.DpGaps, _lib.DpTethers,
                                        _lib.DpSeqExtra)}


def min_size(T):
    """the first version of every sized struct ends with the last field this binding declares"""
    f = getattr(T, _last[T])
    return f.offset + f.size


def sized(T, **fields):
    """a T at the start of a zeroed 8 KiB buffer, so that any struct_size up to 4096 stays inside memory the caller owns"""
    buf = bytearray(8192)
    init = T(**fields)
    buf[:C.sizeof(T)] = bytes(init)
    s = T.from_buffer(buf)
    s._keep = (buf, init)
    return s


def batch():
    return _lib.DpBatch(4, *([PTR] * 7))


def params():
    return sized(_lib.DpParams, n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0, lambda_tmp=0.02, min_loss_incr=float("-inf"))


def result():
    s = sized(_lib.DpResult)
    for name, _ in _lib.DpResult._fields_[2:-1]:
        setattr(s, name, PTR)
    return s


def skeleton():
    return sized(_lib.DpSkeletonIn, offsets=PTR, stride=_lib.DP_SKELETON_STRIDE)


def terms():
    t = _lib.DpTerm(type=_lib.DP_TERM_PLANE, joint_a=3, weight=1.0)
    s = sized(_lib.DpTerms, n_terms=1, terms=C.addressof(t), global_pos=PTR, loss_terms=PTR)
    s._term = t
    return s


def seq_args():
    fr = _lib.DpSeqFrames(n_steps=3, tgt_pos=PTR, tgt_rot=PTR, tgt_root=PTR, w=PTR, tracked=PTR, z_tgt=PTR, z_tgt_step=24, z_tgt_seq=0)
    st = _lib.DpSeqState(PTR, PTR, PTR, PTR, PTR, 4, 2)
    st.height_joints[0], st.height_joints[1] = 4, 8
    res = sized(_lib.DpSeqResults)
    for name, _ in _lib.DpSeqResults._fields_[2:]:
        setattr(res, name, PTR)
    return fr, st, res


# entry point -> its arguments after ctx and before the stream, in order, well-formed
def _optimize(extra=None):
    a = {"in": batch(), "p": params()}
    if extra:
        a[extra[0]] = extra[1]()
    a["out"] = result()
    return a


def _forward(skel=False, vjp=False):
    a = {"n_frames": 4, "z": C.c_void_p(PTR), "cur_rot": C.c_void_p(PTR)}
    if skel:
        a["skel"] = skeleton()
    if not vjp:
        a["out"] = result()
        return a
    a.update(g=sized(_lib.DpGradIn, pos=PTR), dz=C.c_void_p(PTR), dcur_rot=C.c_void_p(PTR))
    if skel:
        a["doffsets"] = C.c_void_p(PTR)
    a["status"] = C.c_void_p(PTR)
    return a


def _sequence(skel=False):
    fr, st, res = seq_args()
    a = {"n_seq": 2, "latent": C.c_void_p(PTR), "fr": fr, "p": params()}
    if skel:
        a["skel"] = skeleton()
    a.update(st=st, adj=_lib.DpSeqStep(adjust_joint=-1), out=res)
    return a


def _tethers():
    """dp_optimize_sequence_tethers (include/dragposer_tethers.h): a table of a plane and two point-DISTANCE terms, a hold on the first of
    them and a tether on the second, the predictor and the gap rule beside them"""
    fr, st, res = seq_args()
    fr.z_tgt = None  # (the predictor is the targets' one source)
    rows = (_lib.DpTerm * 3)(_lib.DpTerm(type=_lib.DP_TERM_PLANE, joint_a=3, weight=1.0),
                             _lib.DpTerm(type=_lib.DP_TERM_DISTANCE, joint_a=8, joint_b=-1, weight=0.8),
                             _lib.DpTerm(type=_lib.DP_TERM_DISTANCE, joint_a=6, joint_b=-1, weight=0.6, p1=0.02))
    t = sized(_lib.DpTerms, n_terms=3, terms=C.addressof(rows))
    hold = _lib.DpHold(term=1, level=0.0, contact_lo=0.02, contact_hi=0.05)
    tether = _lib.DpTether(term=2, alpha=0.5)
    a = {"n_seq": 2, "latent": C.c_void_p(PTR), "fr": fr, "p": params(), "t": t,
         "holds": sized(_lib.DpHolds, n_holds=1, holds=C.addressof(hold), state=PTR),
         "ar": sized(_lib.DpLatentAR, order=2, coeffs=PTR, bias=PTR), "gaps": sized(_lib.DpGaps, max_hold=3, decay=0.7, state=PTR),
         "tethers": sized(_lib.DpTethers, n_tethers=1, tethers=C.addressof(tether), state=PTR, trace=PTR), "skel": skeleton(), "st": st,
         "adj": _lib.DpSeqStep(adjust_joint=-1), "out": res, "extra": sized(_lib.DpSeqExtra)}
    a["t"]._rows, a["holds"]._hold, a["tethers"]._tether = rows, hold, tether
    return a


def tether_cases():
    """dp_tethers' own refusals in the header's order, each with a later stage's fault beside it, and the stages before dp_tethers"""
    def entry(name, value):
        return (f"tethers[0].{name} = {value}", lambda a: setattr(a["tethers"]._tether, name, value), False)

    def term(i, name, value):
        return (f"terms[{i}].{name} = {value}", lambda a: setattr(a["t"]._rows[i], name, value), False)

    late = entry("alpha", 2.0)
    out = [[field("tethers", "n_tethers", v), late] for v in (-1, _lib.DP_MAX_TETHERS + 1)]
    out += [[field("tethers", "tethers", None), field("tethers", "state", None)], [field("tethers", "state", None), late],
            [field("tethers", "n_tethers", 0, benign=True), field("tethers", "tethers", None, benign=True), field("tethers", "state", None, benign=True)],
            [field("tethers", "trace", None, benign=True)]]
    out += [[entry("term", v), late] for v in (-1, 3)]
    out += [[entry("term", 0), late], [term(2, "joint_b", 4), late], [term(2, "per_frame", PTR), late], [entry("term", 1), late]]
    out += [[entry("alpha", v)] for v in (-0.25, 1.5, float("nan"), float("inf"))]
    out += [[field("gaps", "decay", 0.0), late], [field("ar", "order", 0), late], [field("holds", "n_holds", 9), late],
            [field("holds", "reserved0", 3), late], [null_arg("holds", benign=True)], [null_arg("ar"), late]]
    return out


def _advance():
    _, st, _ = seq_args()
    return {"n_seq": 2, "res": result(), "st": st, "step": _lib.DpSeqStep(adjust_joint=-1)}


ENTRY_POINTS = {
    "dp_optimize": _optimize,
    "dp_optimize_skeleton": lambda: _optimize(("skel", skeleton)),
    "dp_forward": _forward,
    "dp_forward_skeleton": lambda: _forward(skel=True),
    "dp_forward_vjp": lambda: _forward(vjp=True),
    "dp_forward_vjp_skeleton": lambda: _forward(skel=True, vjp=True),
    "dp_optimize_constrained": lambda: _optimize(("c", lambda: sized(_lib.DpConstraints, loss_extra=PTR))),
    "dp_optimize_terms": lambda: _optimize(("t", terms)),
    "dp_optimize_sequence": _sequence,
    "dp_optimize_sequence_skeleton": lambda: _sequence(skel=True),
    "dp_sequence_advance": _advance,
    "dp_optimize_sequence_tethers": _tethers,
}
OPTIONAL = {("dp_optimize", "out"), ("dp_optimize_skeleton", "out"), ("dp_forward_vjp", "dcur_rot"), ("dp_forward_vjp", "status"),
            ("dp_forward_vjp_skeleton", "dcur_rot"), ("dp_forward_vjp_skeleton", "doffsets"), ("dp_forward_vjp_skeleton", "status"),
            ("dp_optimize_sequence", "adj"), ("dp_optimize_sequence_skeleton", "adj")}
OPTIONAL |= {("dp_optimize_sequence_tethers", k) for k in ("holds", "skel", "adj", "extra")}


# a defect: (label, function that spoils the argument dict, benign)
def null_arg(name, benign=False):
    return (f"{name} NULL", lambda a: a.__setitem__(name, None), benign)


def field(arg, name, value, benign=False):
    return (f"{arg}.{name} = {value}", lambda a: setattr(a[arg], name, value), benign)


def size_defects(arg, T):
    exact, lo = C.sizeof(T), min_size(T)
    return [field(arg, "struct_size", v, benign=v in (exact, exact + 8)) for v in (0, 8, lo - 1, exact, exact + 8, 5000)]


def cases(ep, args):
    """[(label, [defects])] of one entry point, whose well-formed arguments are `args`"""
    out = [[null_arg("ctx")]]
    is_sized = {k: type(v) for k, v in args.items() if isinstance(v, _lib._Sized)}
    for k, v in args.items():
        if not isinstance(v, int):
            out.append([null_arg(k, (ep, k) in OPTIONAL)])
    for k, T in is_sized.items():
        out += [[d] for d in size_defects(k, T)]
        if T is not _lib.DpParams:
            out.append([field(k, "reserved0", 3)])
    count = "n_frames" if "n_frames" in args else "n_seq" if "n_seq" in args else None
    bad_count = [field("in", "n_frames", v) for v in (0, -1)] if count is None else \
        [(f"{count} = {v}", lambda a, v=v: a.__setitem__(count, v), False) for v in (0, -1)]
    out += [[d] for d in bad_count]
    if "in" in args:
        out += [[field("in", n, None)] for n in BATCH_PTRS]
    if "fr" in args:
        out += [[field("fr", n, None)] for n in ("tgt_pos", "tgt_rot", "w", "tracked", "z_tgt")] + [[field("fr", "n_steps", 0)]]
    if "st" in args:
        out += [[field("st", n, None)] for n in ("global_pos", "global_rot", "latent_buf", "disp_buf", "heights_buf")]
        out += [[field("st", "history", 0)], [field("st", "n_heights", 9)]]
    if "skel" in args:
        out += [[field("skel", "offsets", None)], [field("skel", "stride", 5)], [field("skel", "stride", 0, benign=True)]]
    if "p" in args:
        out += [[field("p", n, v)] for n, v in (("n_iter", 0), ("n_iter", _lib.DP_MAX_ITERS + 1), ("lr", 0.0), ("beta1", 1.0), ("beta2", -0.1),
                                               ("eps", 0.0))]
        # (benign for dp_optimize_sequence*, which read no selector but DP_KERNEL_W16 with a skeleton; dp_optimize tests it last, where
        #  a library without the device-image test has already read the image: skipped with the calls that pass, below)
        out.append([field("p", "kernel", 7, benign="sequence" in ep or ep == "dp_optimize")])
        if "skel" in args:
            out.append([field("p", "kernel", _lib.DP_KERNEL_W16)])
    # pairs of defects: the order of the checks
    if "p" in args and "out" in args:
        out.append([field("p", "struct_size", 8), field("out", "struct_size", 8)])
    for k in ("c", "t", "g", "skel"):
        if k in args:
            out.append([field(k, "struct_size", 8), bad_count[0]])
    if "p" in args:
        out.append([field("in", "z0", None) if "in" in args else field("fr", "tgt_pos", None), field("p", "lr", 0.0)])
    if "p" in args and "skel" in args:
        out.append([field("skel", "stride", 5), field("p", "kernel", 7)])
    if ep == "dp_optimize_sequence_tethers":
        out += tether_cases()
    out.append([])
    return [(" + ".join(d[0] for d in c) or "well-formed", c) for c in out]


def run(lib, ep, skip_unrefused_plain):
    for label, defects in cases(ep, ENTRY_POINTS[ep]()):
        if all(d[2] for d in defects) and (ep == "dp_sequence_advance" or (skip_unrefused_plain and ep in PLAIN)):
            continue
        ctx = C.c_void_p()
        assert lib.dp_debug_host_ctx(C.byref(ctx)) == _lib.DP_OK  # (a fresh context: its message starts empty)
        args = {"ctx": ctx, **ENTRY_POINTS[ep]()}
        for _, spoil, _ in defects:
            spoil(args)
        if args["ctx"] is None:
            lib.dp_fold_decoder(None, None)  # sets the context-less message, so that a refusal which leaves it alone shows
        rc = getattr(lib, ep)(*[v if v is None or isinstance(v, (int, C.c_void_p)) else C.byref(v) for v in args.values()], None)
        msg = lib.dp_last_error(args["ctx"])
        print(f"{ep} | {label} | {rc} | {msg.decode() if msg else ''}", flush=True)
        lib.dp_destroy(ctx)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=_lib.LIB_PATH, help="the library to drive (default: this tree's libdragposer_hip.so)")
    ap.add_argument("--skip-unrefused-plain", action="store_true",
                    help="leave out the calls of dp_optimize, dp_forward and dp_optimize_sequence that pass every argument check")
    ap.add_argument("entry_points", nargs="*", default=list(ENTRY_POINTS))
    o = ap.parse_args()
    lib = _lib.load(os.path.abspath(o.lib))
    for ep in o.entry_points:
        run(lib, ep, o.skip_unrefused_plain)


if __name__ == "__main__":
    main()

"""Batched latent optimiser: the host-side operator over the C ABI (include/dragposer.h).

`LatentOptimizer.optimize` runs, for B independent frames at once, what the reference's
``DragPose.run`` does per frame in its while loop (python/src/drag_pose.py:296-355): decode ->
FK -> tracker loss -> backward -> Adam on z, `n_iter` times, entirely inside one HIP kernel
launch.  PyTorch is used for device memory and streams only: tensors are handed to the library as
raw device pointers on torch's current stream.  There is no CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .model import DEFAULT_MODEL, NJ, HostModel

LATENT = 24

_OUT_SPECS = {  # name -> (trailing shape, dtype)
    "z": ((LATENT,), torch.float32),
    "z_pre": ((LATENT,), torch.float32),
    "pose": ((88,), torch.float32),
    "disp": ((3,), torch.float32),
    "world_disp": ((3,), torch.float32),
    "world_rot": ((4,), torch.float32),
    "pos": ((NJ, 3), torch.float32),
    "rot": ((NJ, 9), torch.float32),
    "loss": ((3,), torch.float32),
    "iters": ((), torch.int32),
    "status": ((), torch.int32),  # DP_STATUS_* bits (include/dragposer.h)
}
_GRAD_NAMES = ("pose", "disp", "world_disp", "world_rot", "pos", "rot")  # the outputs forward_vjp takes gradients of
_LAUNCH_SPECS = {  # results that are per launch, not per frame; only on request
    "clock": ((2,), torch.int64),  # shader cycles / 100 MHz ticks of workgroup 0's iteration loop: sclk_ghz()
}


def sclk_ghz(clock):
    """the shader clock (GHz) a launch ran at, from the `clock` result (a host synchronisation)"""
    c = clock.cpu()
    return float(c[0]) / float(c[1]) * 0.1 if int(c[1]) > 0 else float("nan")


def _check(t, name, shape, dtype, device):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor on {device}")
    if t.device != device:
        raise ValueError(f"{name}: tensor is on {t.device}, the optimiser is on {device}")
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name}: expected contiguous {dtype} of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t.data_ptr()


def _traced(trace, shape, dtype, device):
    """a layer's `*_trace` argument: True means a zeroed tensor allocated here"""
    return torch.zeros(shape, dtype=dtype, device=device) if trace is True else trace


_TERMS_NEED_GLOBAL_POS = "optimize_terms: an active PLANE or point-DISTANCE term needs global_pos [B,3]"


def _own_output(name, width, B, dev, out, tensors, global_pos, gp_error, wanted=True):
    """What the launches with extra loss terms share: their per-frame output `name` [B, width] (from `out` or allocated here, registered in
    `tensors`; not `wanted`: none) and the root positions some terms need (`gp_error`: what to say when those are missing, or None).
    -> (global_pos's pointer or None, the output's pointer or None)"""
    t = None
    if wanted:
        t = out[name] if out is not None and name in out else torch.empty(B, width, dtype=torch.float32, device=dev)
        tensors[name] = t
    gp = None
    if global_pos is not None:
        gp = _check(global_pos, "global_pos", (B, 3), torch.float32, dev)
    elif gp_error:
        raise ValueError(gp_error)
    return gp, _check(t, name, (B, width), torch.float32, dev) if t is not None and width else None


def _seq_state(S, global_pos, global_rot, latent_buf, disp_buf, heights_buf, height_joints, adjust, dev):
    """-> (dp_seq_state, dp_seq_step with its adjust_* words) of S sequences, every tensor checked; `adjust` = (joint, target_joint, weight) or None"""
    H, NH = int(latent_buf.shape[1]), len(height_joints)
    st = _lib.DpSeqState()
    st.global_pos = _check(global_pos, "global_pos", (S, 3), torch.float32, dev)
    st.global_rot = _check(global_rot, "global_rot", (S, 4), torch.float32, dev)
    st.latent_buf = _check(latent_buf, "latent_buf", (S, H, LATENT), torch.float32, dev)
    st.disp_buf = _check(disp_buf, "disp_buf", (S, H, 3), torch.float32, dev)
    st.heights_buf = _check(heights_buf, "heights_buf", (S, H, NH), torch.float32, dev)
    st.history, st.n_heights = H, NH
    for i, j in enumerate(height_joints):
        st.height_joints[i] = int(j)
    step = _lib.DpSeqStep()
    step.adjust_joint = -1
    if adjust is not None:
        step.adjust_joint, step.adjust_target_joint, step.adjust_weight = int(adjust[0]), int(adjust[1]), float(adjust[2])
    return st, step


def _step_outputs(specs, res, scratch, scratch_shape, dev, outputs=None):
    """The per-step results of a whole-sequence launch.  `specs`: (name, given, shape, dtype, struct) per output -- storage the caller gave is
    used and means the output is produced; any other output is allocated here when `outputs` (None: all) names it, and its pointer stays NULL
    otherwise.  `scratch` (given or allocated) becomes res.hist_scratch.  -> ({name: tensor} of what is produced, the scratch: the caller keeps it
    alive until it has launched)"""
    outs = {}
    for name, t, shape, dtype, struct in specs:
        if outputs is not None and name not in outputs and t is None:
            continue
        t = t if t is not None else torch.empty(shape, dtype=dtype, device=dev)
        setattr(struct, name, _check(t, name, shape, dtype, dev))
        outs[name] = t
    scratch = scratch if scratch is not None else torch.empty(scratch_shape, device=dev)
    res.hist_scratch = _check(scratch, "scratch", scratch_shape, torch.float32, dev)
    return outs, scratch


# optimize_sequence's layers above the term table, lowest rung of the ladder first.  Per layer: its argument; its trace's argument, shape after
# [T,S] and dtype; the entry point that takes the layers up to it; and (its struct, what that keeps alive) from the call's arguments `a` and the trace.
_SEQ_LAYERS = (
    ("holds", "hold_trace", lambda a: (len(a["holds"]), 4), torch.float32, "dp_optimize_sequence_holds",
     lambda a, trace: a["holds"].to_struct(a["terms"], a["S"], a["dev"], a["hold_state"], trace, steps=a["T"])),
    ("ar", "z_tgt_trace", lambda a: (LATENT,), torch.float32, "dp_optimize_sequence_ar",
     lambda a, trace: a["ar"].to_struct(a["dev"], trace, (a["T"], a["S"], LATENT))),
    ("gaps", "gap_trace", lambda a: (NJ,), torch.uint8, "dp_optimize_sequence_gaps",  # (dp_live_step with live=: the same rung in one launch)
     lambda a, trace: (a["gaps"].to_struct(a["S"], a["dev"], a["gap_state"], a["present"], trace, steps=a["T"]), None)),
    ("tethers", "tether_trace", lambda a: (len(a["tethers"]), 8), torch.float32, "dp_optimize_sequence_tethers",
     lambda a, trace: a["tethers"].to_struct(a["terms"], a["S"], a["dev"], a["tether_state"], trace, steps=a["T"], holds=a["holds"])),
)


def _sequence_refusals(tgt_pos, latent_buf, z_tgt, constraints, terms, loss_extra, loss_terms, joint_pos, holds, hold_state, hold_trace, ar, z_tgt_trace,
                       gaps, gap_state, present, gap_trace, live, tethers, tether_state, tether_trace):
    """what optimize_sequence refuses of a combination of layers, before it touches the library; -> `terms` (an empty table where `gaps` or `ar`
    came without one)"""
    if terms is not None and terms.has_points:
        for name, given in (("holds", holds is not None), ("gaps", gaps is not None), ("ar", ar is not None), ("tethers", tethers is not None),
                            ("live", live)):
            if given:
                raise ValueError(f"optimize_sequence: a table with points does not go with {name}= (include/dragposer_points.h, Not in)")
    if tethers is None and (tether_state is not None or tether_trace is not None):
        raise ValueError("optimize_sequence: tether_state / tether_trace belong to tethers=")
    if tethers is not None:
        if live:
            raise ValueError("optimize_sequence: tethers= are not part of dp_live_step (include/dragposer_tethers.h, Not covered)")
        if terms is None or constraints is not None:
            raise ValueError("optimize_sequence: tethers= refer to a table, pass terms= (Terms.from_constraints turns constraints into one)")
        if gaps is None:
            raise ValueError("optimize_sequence: tethers= is dp_optimize_sequence_gaps with tethers, pass gaps= (Gaps(0, 1.0) for none to hold)")
        if tether_state is None:
            raise ValueError("optimize_sequence: tethers= needs tether_state [S,len(tethers),8]")
        tethers.check(terms, holds)
    if live and gaps is None:
        raise ValueError("optimize_sequence: live= is the one-launch form of gaps= (pass Gaps(0, 1.0) for none to hold)")
    if live and int(tgt_pos.shape[0]) != 1:
        raise ValueError("optimize_sequence: live= is one frame, tgt_pos holds " + str(int(tgt_pos.shape[0])))
    if gaps is None and (gap_state is not None or present is not None or gap_trace is not None):
        raise ValueError("optimize_sequence: gap_state / present / gap_trace belong to gaps=")
    if gaps is not None:
        gaps.check()
        if gap_state is None:
            raise ValueError("optimize_sequence: gaps= needs gap_state [S,22,16]")
        if constraints is not None:
            raise ValueError("optimize_sequence: gaps= takes a table, pass terms= (Terms.from_constraints turns constraints into one)")
        if terms is None:
            from .terms import Terms

            terms = Terms()
    if ar is None and z_tgt_trace is not None:
        raise ValueError("optimize_sequence: z_tgt_trace belongs to ar=")
    if ar is not None:
        if z_tgt is not None:
            raise ValueError("optimize_sequence: ar= forms the targets itself, pass z_tgt=None")
        if constraints is not None:
            raise ValueError("optimize_sequence: ar= takes a table, pass terms= (Terms.from_constraints turns constraints into one)")
        if ar.order > int(latent_buf.shape[1]):
            raise ValueError(f"optimize_sequence: latent_buf holds {int(latent_buf.shape[1])} rows, fewer than ar.order = {ar.order}")
        if terms is None:
            from .terms import Terms

            terms = Terms()
    if holds is not None and (terms is None or constraints is not None):
        raise ValueError("optimize_sequence: holds= refer to a table, pass terms= (Terms.from_constraints turns constraints into one)")
    if holds is None and (hold_state is not None or hold_trace is not None):
        raise ValueError("optimize_sequence: hold_state / hold_trace belong to holds=")
    if holds is not None and hold_state is None:
        raise ValueError("optimize_sequence: holds= needs hold_state [S,len(holds),4]")
    if constraints is not None and terms is not None:
        raise ValueError("optimize_sequence: pass constraints or terms, not both")
    if constraints is None and terms is None and (loss_extra is not None or loss_terms is not None or joint_pos is not None):
        raise ValueError("optimize_sequence: loss_extra / loss_terms / joint_pos are outputs of constraints= / terms=")
    return terms


class LaunchPlan:
    """A dp_optimize call with its arguments already checked and marshalled (LatentOptimizer.plan).  Holds the input and result
    tensors alive; `plan()` launches on torch's current stream of the optimiser's device and returns the result tensors."""

    __slots__ = ("_opt", "_b", "_p", "_r", "results", "_inputs", "_fn", "_args")

    def __init__(self, opt, batch, params, res, tensors, inputs, skel=None):
        self._opt, self.results, self._inputs = opt, tensors, inputs
        self._b, self._p, self._r = C.byref(batch), C.byref(params), C.byref(res)  # (byref objects keep their structs alive)
        self._fn, self._args = opt.lib.dp_optimize, (self._b, self._p, self._r)
        if skel is not None:  # per-frame skeletons (include/dragposer_skeleton.h)
            self._fn, self._args = opt.lib.dp_optimize_skeleton, (self._b, self._p, C.byref(skel), self._r)

    def __call__(self):
        # (the context is read per call: after LatentOptimizer.close() it is NULL and the library refuses, instead of a freed context being used)
        if not self._opt.ctx.value:
            raise _lib.DragPoserError(_lib.DP_ERR_INVALID, "LaunchPlan: the optimiser it was made by has been closed")
        self._opt._call(self._fn, *self._args)
        return self.results


class LatentOptimizer:
    """One context per device.  Not thread-safe (same contract as the C ABI)."""

    def __init__(self, model_path=DEFAULT_MODEL, device="cuda:0", weight_dtype="fp32", arrays=None, _lib_path=None):
        self.lib = _lib.load(_lib_path)  # (_lib_path: tests only -- the second implementation kept for cross-checks)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("LatentOptimizer needs a ROCm device (cuda:N); there is no CPU fallback")
        if not torch.cuda.is_available():
            raise RuntimeError("no ROCm device visible to PyTorch; dragposer_amd has no CPU fallback")
        self.host_model = HostModel(model_path, weight_dtype, arrays=arrays)
        self.ctx = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        rc = self.lib.dp_create(C.byref(self.ctx), C.byref(self.host_model.struct), idx)
        if rc != _lib.DP_OK:
            msg = self.lib.dp_last_error(None)
            raise _lib.DragPoserError(rc, msg.decode() if msg else "")
        fpb, tpb, lds = C.c_int(), C.c_int(), C.c_int()
        self.lib.dp_kernel_geometry(self.ctx, C.byref(fpb), C.byref(tpb), C.byref(lds))
        self.frames_per_block, self.threads_per_block, self.lds_bytes = fpb.value, tpb.value, lds.value

    def kernel_geometry(self):
        """(frames per workgroup, threads per workgroup, LDS bytes) of the kernel the last launch used"""
        fpb, tpb, lds = C.c_int(), C.c_int(), C.c_int()
        self.lib.dp_kernel_geometry(self.ctx, C.byref(fpb), C.byref(tpb), C.byref(lds))
        return fpb.value, tpb.value, lds.value

    def auto_kernel(self, n_frames):
        """"w4" | "w16": what kernel="auto" launches for a batch of `n_frames` on this device (dp_auto_kernel).  The two kernels
        differ in the last bits of their arithmetic, so a caller that cuts one batch into several launches and wants a frame's
        result not to depend on the cut pins the answer for the deciding size (dragposer_amd.sharding.pick_kernel)."""
        k = self.lib.dp_auto_kernel(self.ctx, int(n_frames))
        if k < 0:
            self._fail(k)
        return {_lib.DP_KERNEL_W4: "w4", _lib.DP_KERNEL_W16: "w16"}[k]

    def close(self):
        if getattr(self, "ctx", None) is not None and self.ctx.value:
            self.lib.dp_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _fail(self, rc):
        msg = self.lib.dp_last_error(self.ctx)
        raise _lib.DragPoserError(rc, msg.decode() if msg else "")

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _call(self, fn, *args):
        """fn(ctx, *args, torch's current stream), raising what the library reports"""
        rc = fn(self.ctx, *args, self._stream())
        if rc != _lib.DP_OK:
            self._fail(rc)

    def _batch(self, z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked, positions_only=False):
        """positions_only: the launch reads neither z_tgt nor tgt_rot (dp_fit_bones), which then stay NULL"""
        B, dev = int(z0.shape[0]), self.device
        batch = _lib.DpBatch()
        batch.n_frames = B
        batch.z0 = _check(z0, "z0", (B, LATENT), torch.float32, dev)
        batch.z_tgt = None if positions_only else _check(z_tgt, "z_tgt", (B, LATENT), torch.float32, dev)
        batch.cur_rot = _check(cur_rot, "cur_rot", (B, 4), torch.float32, dev)
        batch.tgt_pos = _check(tgt_pos, "tgt_pos", (B, NJ, 3), torch.float32, dev)
        batch.tgt_rot = None if positions_only else _check(tgt_rot, "tgt_rot", (B, NJ, 9), torch.float32, dev)
        batch.w = _check(w, "w", (B, NJ, 2), torch.float32, dev)
        batch.tracked = _check(tracked, "tracked", (B, NJ), torch.uint8, dev)
        return batch

    @staticmethod
    def _params(n_iter, lr, betas, eps, lambda_rot, lambda_tmp, stop_eps_pos, stop_eps_rot, min_loss_incr, max_trackers=0,
                kernel=_lib.DP_KERNEL_AUTO, early=None):
        """`early` None: the while-condition runs when any of its three thresholds is given"""
        if early is None:
            early = min_loss_incr is not None or stop_eps_pos > 0 or stop_eps_rot > 0
        return _lib.DpParams(n_iter=int(n_iter), lr=lr, beta1=betas[0], beta2=betas[1], eps=eps, lambda_rot=lambda_rot,
                             lambda_tmp=lambda_tmp, early_stop=int(early), stop_eps_pos=stop_eps_pos, stop_eps_rot=stop_eps_rot,
                             min_loss_incr=float("-inf") if min_loss_incr is None else min_loss_incr,
                             max_trackers=int(max_trackers), kernel=kernel)

    def allocate_outputs(self, B, names=None):
        """a reusable set of result tensors for `optimize(..., out=...)`"""
        return {n: torch.empty((B,) + _OUT_SPECS[n][0], dtype=_OUT_SPECS[n][1], device=self.device) for n in (names or _OUT_SPECS)}

    def _outputs(self, B, names, out):
        res = _lib.DpResult()
        tensors = {}
        for name in names:
            if name in _LAUNCH_SPECS:
                shape, dtype = _LAUNCH_SPECS[name]
            else:
                shape, dtype = (B,) + _OUT_SPECS[name][0], _OUT_SPECS[name][1]
            t = out[name] if out is not None and name in out else torch.empty(shape, dtype=dtype, device=self.device)
            setattr(res, name, _check(t, name, shape, dtype, self.device))
            tensors[name] = t
        return res, tensors

    def _skeleton(self, offsets, n, who):
        """`offsets` -> (dp_skeleton_in, the tensor it points to): [22,3] = one skeleton for the launch (stride 0), [n,22,3] = one per frame
        (per sequence in a sequence launch; stride 66); contiguous fp32 on the optimiser's device (include/dragposer_skeleton.h)"""
        if not isinstance(offsets, torch.Tensor):
            raise TypeError(f"{who}: offsets must be a torch.Tensor on {self.device}, [22,3] or [{n},22,3]")
        if offsets.dim() == 2:
            shape, stride = (NJ, 3), 0
        elif offsets.dim() == 3:
            shape, stride = (n, NJ, 3), _lib.DP_SKELETON_STRIDE
        else:
            raise ValueError(f"{who}: offsets must be [22,3] (one skeleton) or [{n},22,3] (one per frame / sequence), got {tuple(offsets.shape)}")
        s = _lib.DpSkeletonIn()
        s.offsets = _check(offsets, "offsets", shape, torch.float32, self.device)
        s.stride = stride
        return s

    def optimize(self, z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked, n_iter=50, lr=1e-2, betas=(0.9, 0.999),
                 eps=1e-8, lambda_rot=1.0, lambda_tmp=0.02, stop_eps_pos=0.0, stop_eps_rot=0.0, min_loss_incr=None,
                 max_trackers=0, outputs=None, out=None, validate_targets=False, kernel="auto", _debug=None, offsets=None):
        """All inputs are device tensors: z0/z_tgt [B,24], cur_rot [B,4], tgt_pos [B,22,3],
        tgt_rot [B,22,9], w [B,22,2] (fp32) and tracked [B,22] (uint8).  Returns a dict of device
        tensors (see include/dragposer.h: dp_result).  Asynchronous on torch's current stream.
        With stop_eps_* > 0 or min_loss_incr given, every frame runs the reference's own while-condition
        (drag_pose.py:300-304) and `iters` reports how many iterations it took (n_iter = max_iter).
        `max_trackers`: ignored (a kernel-selection hint of version 1; kept so that old callers keep working).
        `kernel`: "auto" | "w4" (4 frames per wave, fp32 MFMA) | "w16" (16 frames per wave, decoder on bf16 MFMA in split
        precision; what "auto" picks beyond 8192 frames: two rounds of "w4") -- include/dragposer.h: DP_KERNEL_*.
        `validate_targets`: check that every tracked joint's tgt_rot is a rotation matrix (the kernel evaluates the
        reference's |R - T|^2 in its quaternion form, equal only for orthonormal det +1 targets: include/dragposer.h) --
        costs a device reduction and a host synchronisation, so it is off by default.
        `offsets`: the performers' bone offsets, [22,3] for every frame or [B,22,3] one per frame (contiguous fp32 on the device; row 0
        ignored): dp_optimize_skeleton (include/dragposer_skeleton.h), on the "w4" kernel at every batch size; None = the context's skeleton
        (dp_optimize, unchanged)."""
        plan = self.plan(z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked, n_iter, lr, betas, eps, lambda_rot, lambda_tmp, stop_eps_pos,
                         stop_eps_rot, min_loss_incr, max_trackers, outputs, out, validate_targets, kernel, offsets=offsets)
        if _debug is not None:
            if offsets is not None:
                raise ValueError("optimize: the debug dump has no per-frame-skeleton form (offsets)")
            self._call(self.lib.dp_optimize_debug, plan._b, plan._p, plan._r, C.c_void_p(_debug.data_ptr()))
            return plan.results
        return plan()

    def plan(self, z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked, n_iter=50, lr=1e-2, betas=(0.9, 0.999),
             eps=1e-8, lambda_rot=1.0, lambda_tmp=0.02, stop_eps_pos=0.0, stop_eps_rot=0.0, min_loss_incr=None,
             max_trackers=0, outputs=None, out=None, validate_targets=False, kernel="auto", offsets=None):
        """`optimize`'s arguments checked and marshalled ONCE: returns a LaunchPlan whose call launches dp_optimize (dp_optimize_skeleton with
        `offsets`, as in `optimize`) over the same
        tensors (read at launch time: refill them in place between calls) into the same result tensors, on torch's current stream --
        a caller that steps the same buffers every frame pays one ctypes call per launch instead of the checks and struct filling."""
        B = int(z0.shape[0])
        skel = None
        if offsets is not None:
            if kernel == "w16":
                raise ValueError('optimize: kernel="w16" has no per-frame skeletons (its slot map keeps the bone offsets in per-slot constants); '
                                 'use "w4" or "auto" with offsets')
            skel = self._skeleton(offsets, B, "optimize")
        if validate_targets:
            check_rotation_targets(tgt_rot, tracked)
        batch = self._batch(z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked)
        p = self._params(n_iter, lr, betas, eps, lambda_rot, lambda_tmp, stop_eps_pos, stop_eps_rot, min_loss_incr, max_trackers,
                         {"auto": _lib.DP_KERNEL_AUTO, "w4": _lib.DP_KERNEL_W4, "w16": _lib.DP_KERNEL_W16}[kernel])
        names = tuple(outputs) if outputs is not None else tuple(_OUT_SPECS)
        res, tensors = self._outputs(B, names, out)
        inputs = (z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked)
        return LaunchPlan(self, batch, p, res, tensors, inputs if skel is None else inputs + (offsets,), skel=skel)

    def forward(self, z, cur_rot, outputs=("pose", "disp", "world_disp", "world_rot", "pos", "rot"), out=None, offsets=None):
        """decode + FK of z [B,24] under cur_rot [B,4] (no loss, no update).  `offsets` [22,3] / [B,22,3]: per-frame skeletons as in
        `optimize` (dp_forward_skeleton)."""
        B = int(z.shape[0])
        skel = self._skeleton(offsets, B, "forward") if offsets is not None else None
        zp = _check(z, "z", (B, LATENT), torch.float32, self.device)
        cp = _check(cur_rot, "cur_rot", (B, 4), torch.float32, self.device)
        res, tensors = self._outputs(B, tuple(outputs), out)
        fn, tail = (self.lib.dp_forward, (C.byref(res),)) if skel is None else (self.lib.dp_forward_skeleton, (C.byref(skel), C.byref(res)))
        self._call(fn, B, C.c_void_p(zp), C.c_void_p(cp), *tail)
        return tensors

    def _optimize_extra(self, fn, inputs, pargs, global_pos, outputs, out, validate_targets, extra, width, gp_error, to_struct, skel=None, mid=()):
        """What optimize_constrained and optimize_terms share: `optimize`'s batch, parameters and results, the per-frame output of their own
        (`extra` [B, width]) and the root positions some of their terms need (`gp_error`: what to say when those are missing, or None).
        to_struct(global_pos pointer, `extra`'s pointer) -> (the extension struct, what it keeps alive).  `skel`: the dp_skeleton_in of the
        per-frame-skeleton form of `fn`, which takes it after the extension struct; `mid`: what `fn` takes between the two."""
        z0, tgt_rot, tracked = inputs[0], inputs[4], inputs[6]
        B, dev = int(z0.shape[0]), self.device
        if validate_targets:
            check_rotation_targets(tgt_rot, tracked)
        batch = self._batch(*inputs)
        p = self._params(*pargs)
        names = tuple(outputs) if outputs is not None else tuple(_OUT_SPECS)
        res, tensors = self._outputs(B, [n for n in names if n != extra], out)
        s, keep = to_struct(*_own_output(extra, width, B, dev, out, tensors, global_pos, gp_error))
        self._call(fn, C.byref(batch), C.byref(p), C.byref(s), *mid, *(() if skel is None else (C.byref(skel),)), C.byref(res))
        del keep
        return tensors

    def optimize_constrained(self, z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked, constraints, global_pos=None, n_iter=50, lr=1e-2,
                             betas=(0.9, 0.999), eps=1e-8, lambda_rot=1.0, lambda_tmp=0.02, stop_eps_pos=0.0, stop_eps_rot=0.0,
                             min_loss_incr=None, max_trackers=0, outputs=None, out=None, validate_targets=False, kernel="auto", offsets=None):
        """`optimize` with the reference's extra loss terms (`constraints`: a dragposer_amd.Constraints) added to the loss and to the
        while-condition's total: include/dragposer_constraints.h, dp_optimize_constrained (one launch).  `global_pos` [B,3] (device,
        fp32): the root position before the frame (the reference's current_global_pos), required when the feet_floor term is on.
        Returns `optimize`'s dict plus `loss_extra` [B,4] (the four weighted terms of the last forward pass).  `kernel` is ignored
        (one kernel implements this operator); `validate_targets` as in `optimize`.
        `offsets`: the performers' bone offsets, [22,3] for every frame or [B,22,3] one per frame (contiguous fp32 on the device; row 0
        ignored): dp_optimize_constrained_skeleton; None = the context's skeleton (dp_optimize_constrained, unchanged)."""
        skel = self._skeleton(offsets, int(z0.shape[0]), "optimize_constrained") if offsets is not None else None
        return self._optimize_extra(
            self.lib.dp_optimize_constrained if skel is None else self.lib.dp_optimize_constrained_skeleton, (z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked),
            (n_iter, lr, betas, eps, lambda_rot, lambda_tmp, stop_eps_pos, stop_eps_rot, min_loss_incr, max_trackers), global_pos, outputs, out,
            validate_targets, "loss_extra", 4, "optimize_constrained: the feet_floor term needs global_pos [B,3]" if constraints.needs_global_pos else None,
            lambda gp, le: (constraints.to_struct(gp, le), None), skel=skel)

    def optimize_terms(self, z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked, terms, global_pos=None, n_iter=50, lr=1e-2,
                       betas=(0.9, 0.999), eps=1e-8, lambda_rot=1.0, lambda_tmp=0.02, stop_eps_pos=0.0, stop_eps_rot=0.0, min_loss_incr=None,
                       max_trackers=0, outputs=None, out=None, validate_targets=False, kernel="auto", offsets=None):
        """`optimize` with a table of user-defined terms (`terms`: a dragposer_amd.Terms) added to the loss and to the while-condition's
        total: include/dragposer_terms.h, dp_optimize_terms (one launch).  `global_pos` [B,3] (device, fp32): the root position before
        the frame, required when an active PLANE or point-DISTANCE term exists.  A term's per-frame rows are its `per_frame` [B,4]
        device tensor.  Returns `optimize`'s dict plus `loss_terms` [B, len(terms)] (each weighted term of the last forward pass).
        `kernel` is ignored; `validate_targets` as in `optimize`.  `offsets` [22,3] / [B,22,3]: per-frame skeletons as in
        `optimize_constrained` (dp_optimize_terms_skeleton); None = the context's skeleton (dp_optimize_terms, unchanged).
        A table with points (`Terms(..., points=Points([...]))`: terms on weighted joint combinations, include/dragposer_points.h) runs
        through dp_optimize_terms_points / dp_optimize_terms_points_skeleton, everything else alike."""
        skel = self._skeleton(offsets, int(z0.shape[0]), "optimize_terms") if offsets is not None else None
        terms.check()
        fn, mid, keep_p = (self.lib.dp_optimize_terms if skel is None else self.lib.dp_optimize_terms_skeleton), (), None
        if terms.has_points:
            ps, keep_p = terms.points.to_struct()
            fn, mid = (self.lib.dp_optimize_terms_points if skel is None else self.lib.dp_optimize_terms_points_skeleton), (C.byref(ps),)
        return self._optimize_extra(
            fn, (z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked),
            (n_iter, lr, betas, eps, lambda_rot, lambda_tmp, stop_eps_pos, stop_eps_rot, min_loss_incr, max_trackers), global_pos, outputs, out,
            validate_targets, "loss_terms", len(terms),
            _TERMS_NEED_GLOBAL_POS if terms.needs_global_pos else None,
            lambda gp, lt: terms.to_struct(int(z0.shape[0]), self.device, gp, lt), skel=skel, mid=mid)

    def optimize_lm(self, z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked, lm=None, lambda_rot=1.0, lambda_tmp=0.02, mu=None, stop_eps_pos=0.0,
                    stop_eps_rot=0.0, outputs=None, out=None, terms=None, global_pos=None, offsets=None):
        """`optimize`'s problem solved by Levenberg-Marquardt steps instead of Adam (`lm`: a dragposer_amd.LM; None = LM()):
        include/dragposer_lm.h, dp_optimize_lm (one launch).  Inputs as in `optimize`.  `mu` [B] fp32 on the device: the damping of every
        frame, read and updated IN PLACE (a caller keeps it from frame to frame); None: every frame starts at lm.mu0.  Returns `optimize`'s
        dict (every array belongs to the returned z; z_pre = z; iters = the steps executed) plus `n_accepted` [B] int32, `loss0` [B,3] (the
        loss at z0) and `mu` [B] (the damping after the call).  `stop_eps_pos` / `stop_eps_rot`: the early stop's thresholds unless `lm`
        carries its own.  Asynchronous on torch's current stream.
        `terms` (a dragposer_amd.Terms without points): the table's terms in the LM loss, include/dragposer_lm_terms.h,
        dp_optimize_lm_terms (one launch); `global_pos` [B,3] as in `optimize_terms`, required when an active PLANE or point-DISTANCE term
        exists.  The dict then also holds `loss_terms` [B, len(terms)], each weighted term at the returned z.  terms=None: dp_optimize_lm,
        unchanged.
        `offsets` [22,3] / [B,22,3]: the performers' bone offsets, one skeleton for the launch or one per frame, as in `optimize`:
        dp_optimize_lm_skeleton (include/dragposer_clip_skeleton.h).  Not together with `terms`.  None: the context's skeleton."""
        from .lm import LM

        if offsets is not None and terms is not None:
            raise ValueError("optimize_lm: offsets does not go with terms (include/dragposer_clip_skeleton.h, \"Not covered\")")
        B, dev = int(z0.shape[0]), self.device
        skel = self._skeleton(offsets, B, "optimize_lm") if offsets is not None else None
        lm = (lm if lm is not None else LM()).check()
        batch = self._batch(z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked)
        p = lm.to_struct(lambda_rot, lambda_tmp, stop_eps_pos, stop_eps_rot)
        own = {"n_accepted": ((B,), torch.int32), "loss0": ((B, 3), torch.float32), "mu": ((B,), torch.float32)}
        names = tuple(outputs) if outputs is not None else tuple(_OUT_SPECS) + tuple(own)
        res, tensors = self._outputs(B, [n for n in names if n not in own and n not in ("clock", "loss_terms")], out)
        ex = _lib.DpLmExtra()
        for name, (shape, dtype) in own.items():
            if name == "mu":
                t = mu if mu is not None else torch.full(shape, float(lm.mu0), dtype=dtype, device=dev)
            elif name in names:
                t = out[name] if out is not None and name in out else torch.empty(shape, dtype=dtype, device=dev)
            else:
                continue
            setattr(ex, name, _check(t, name, shape, dtype, dev))
            tensors[name] = t
        if skel is not None:
            self._call(self.lib.dp_optimize_lm_skeleton, C.byref(batch), C.byref(p), C.byref(skel), C.byref(res), C.byref(ex))
            return tensors
        if terms is None:
            self._call(self.lib.dp_optimize_lm, C.byref(batch), C.byref(p), C.byref(res), C.byref(ex))
            return tensors
        if terms.has_points:
            raise ValueError("optimize_lm: a table with points does not go with the LM solver (include/dragposer_lm_terms.h, \"Not covered\")")
        terms.check()
        s, keep = terms.to_struct(B, dev, *_own_output("loss_terms", len(terms), B, dev, out, tensors, global_pos,
                                                       _TERMS_NEED_GLOBAL_POS if terms.needs_global_pos else None, wanted=outputs is None or "loss_terms" in names))
        self._call(self.lib.dp_optimize_lm_terms, C.byref(batch), C.byref(p), C.byref(s), C.byref(res), C.byref(ex))
        del keep
        return tensors

    def optimize_clip_lm(self, z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked, n_sequences, clip=None, lambda_rot=1.0, lambda_tmp=0.0, mu=None,
                         outputs=None, out=None, offsets=None):
        """A clip solved jointly (`clip`: a dragposer_amd.ClipLM; None = ClipLM()): include/dragposer_clip_lm.h, dp_optimize_clip_lm.  The B rows
        are `n_sequences` sequences of T = B / n_sequences frames, frame t of sequence s in row t * n_sequences + s; each row is `optimize_lm`'s
        frame, and the latents of a sequence are tied frame to frame by clip.smooth |z_t - z_(t-1)|^2 / 24 inside the loss.  `mu` [S] fp32 on the
        device: the damping of every sequence, read and updated IN PLACE; None: every sequence starts at clip.mu0.  Returns `optimize_lm`'s
        per-frame dict (every array belongs to the returned z; iters = the steps run; loss = the fp32 pass's numbers; no loss0) plus
        `clip_loss` [S,2] float64 (the sequence's loss at the returned latents, its coupling part), `loss_hist` [S, steps+1] float64,
        `n_accepted` [S] int32, `mu` [S] and `info` [S] int32 (DP_CLIP_* flags).  With clip.accel a number the call is
        dp_optimize_clip_lm_accel (include/dragposer_clip_accel.h): clip.accel |z_(t+1) - 2 z_t + z_(t-1)|^2 / 24 joins the loss, clip_loss[:, 1]
        is both coupling sums and `accel_loss` [S] float64, the second-difference one, is one more output.  The workspace is a buffer this
        optimiser keeps, by size.
        `offsets` [22,3] / [S,22,3]: the performers' bone offsets, one skeleton for the launch or one per SEQUENCE, held for all its frames
        (what `fit_bones` / dragposer_amd.calibrate return goes here): dp_optimize_clip_lm_skeleton (include/dragposer_clip_skeleton.h), with
        or without clip.accel.  The tensor is read during the launch.  None: the context's skeleton, the plain calls, unchanged.
        Asynchronous on torch's current stream, no host synchronisation."""
        from .clip import ClipLM

        clip = (clip if clip is not None else ClipLM()).check()
        B, dev, S = int(z0.shape[0]), self.device, int(n_sequences)
        if S <= 0 or B % S != 0:
            raise ValueError(f"optimize_clip_lm: n_sequences {n_sequences!r} must be positive and divide the {B} rows")
        skel = self._skeleton(offsets, S, "optimize_clip_lm") if offsets is not None else None
        batch = self._batch(z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked)
        p = clip.to_struct(lambda_rot, lambda_tmp)
        own = {"clip_loss": ((S, 2), torch.float64), "loss_hist": ((S, clip.steps + 1), torch.float64), "n_accepted": ((S,), torch.int32),
               "mu": ((S,), torch.float32), "info": ((S,), torch.int32)}
        accel = clip.accel_struct() if clip.accel is not None else None
        if accel is not None:
            own["accel_loss"] = ((S,), torch.float64)
        names = tuple(outputs) if outputs is not None else tuple(_OUT_SPECS) + tuple(own)
        unknown = [n for n in names if n not in own and n not in _OUT_SPECS]
        if unknown:
            raise ValueError(f"optimize_clip_lm: unknown output {unknown[0]!r}")
        res, tensors = self._outputs(B, [n for n in names if n not in own], out)
        ex = _lib.DpClipLmExtra()
        for name, (shape, dtype) in own.items():
            if name == "mu":
                t = mu if mu is not None else torch.full(shape, float(clip.mu0), dtype=dtype, device=dev)
            elif name in names:
                t = out[name] if out is not None and name in out else torch.empty(shape, dtype=dtype, device=dev)
            else:
                continue
            setattr(accel if name == "accel_loss" else ex, name, _check(t, name, shape, dtype, dev))
            tensors[name] = t
        need = int((self.lib.dp_clip_lm_workspace_bytes if accel is None else self.lib.dp_clip_lm_accel_workspace_bytes)(S, B))
        cache = self.__dict__.setdefault("_clip_workspaces", {})
        ws = cache.get(need)
        if ws is None:
            ws = cache[need] = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
        ex.workspace, ex.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        if skel is not None:
            self._call(self.lib.dp_optimize_clip_lm_skeleton, C.byref(batch), S, C.byref(p), C.byref(accel) if accel is not None else None, C.byref(skel),
                       C.byref(res), C.byref(ex))
        elif accel is None:
            self._call(self.lib.dp_optimize_clip_lm, C.byref(batch), S, C.byref(p), C.byref(res), C.byref(ex))
        else:
            self._call(self.lib.dp_optimize_clip_lm_accel, C.byref(batch), S, C.byref(p), C.byref(accel), C.byref(res), C.byref(ex))
        return tensors

    def fit_bones(self, z, cur_rot, tgt_pos, w, tracked, groups, base=None, prior=None, ridge=1e-3, outputs=None, out=None):
        """Per-group bone scales from B frames of tracker data in one call (include/dragposer_calibration.h, dp_fit_bones): with the joint
        rotations fixed at decode + FK of `z` [B,24] under `cur_rot` [B,4], the scales s of off_b = s[group(b)] * base_b that minimise the
        frames' summed loss_pos + ridge |s - prior|^2.  `tgt_pos`, `w`, `tracked` as in `optimize` (no rotation targets, no z_tgt).
        `groups`: a dragposer_amd.BoneGroups; `base` [22,3] host values (None: the context's bones); `prior` [K] host values (None: ones).
        Returns dict(scales [K], offsets [22,3] -- pass it as `offsets=` to the next launch --, normal [K+1,K+1] float64, rms [2] (at the
        prior, at the scales), info [2] int32 (frames used, DP_FIT_* flags), status [B] int32); `outputs`: the subset to produce (scales
        always), `out`: storage for any of them.  The workspace is a buffer this optimiser keeps.  Asynchronous on torch's current stream,
        no host synchronisation."""
        B, dev, K = int(z.shape[0]), self.device, len(groups)
        batch = self._batch(z, None, cur_rot, tgt_pos, None, w, tracked, positions_only=True)
        fit, keep = groups.to_struct(base, prior, ridge)
        need = int(self.lib.dp_fit_bones_workspace_bytes(B))
        ws = getattr(self, "_fit_workspace", None)
        if ws is None or ws.numel() * 4 < need:
            ws = self._fit_workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
        fit.workspace, fit.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        specs = {"scales": ((K,), torch.float32), "offsets": ((NJ, 3), torch.float32), "normal": ((K + 1, K + 1), torch.float64),
                 "rms": ((2,), torch.float32), "info": ((2,), torch.int32), "status": ((B,), torch.int32)}
        names = tuple(specs) if outputs is None else tuple(outputs)
        unknown = [n for n in names if n not in specs]
        if unknown:
            raise ValueError(f"fit_bones: unknown output {unknown[0]!r}")
        res, tensors = _lib.DpBoneFitResult(), {}
        for name, (shape, dtype) in specs.items():
            if name != "scales" and name not in names and not (out is not None and name in out):
                continue
            t = out[name] if out is not None and name in out else torch.empty(shape, dtype=dtype, device=dev)
            setattr(res, name, _check(t, name, shape, dtype, dev))
            tensors[name] = t
        self._call(self.lib.dp_fit_bones, C.byref(batch), C.byref(fit), C.byref(res))
        del keep
        return tensors

    def forward_vjp(self, z, cur_rot, grads, out=None, offsets=None, doffsets=False):
        """dL/dz [B,24] and dL/dcur_rot [B,4] of decode + FK at (z, cur_rot) for upstream gradients `grads` = {output name: dL/d(that
        output)} over any subset of pose, disp, world_disp, world_rot, pos, rot (shapes as `forward` returns them; missing = zero):
        include/dragposer_grad.h, dp_forward_vjp.  Returns dict(dz, dcur_rot, status) -- status: DP_STATUS_* bits per frame.
        `offsets` [22,3] / [B,22,3]: per-frame skeletons as in `forward` (dp_forward_vjp_skeleton); with them, `doffsets=True` (or a
        "doffsets" tensor in `out`) adds "doffsets" [B,22,3], dL/d(offsets) of each frame (row 0 zero; for one [22,3] skeleton the
        caller sums over the frames).  `out`: a dict of preallocated result tensors (any of these).  Asynchronous on torch's current
        stream."""
        B = int(z.shape[0])
        dev = self.device
        skel = self._skeleton(offsets, B, "forward_vjp") if offsets is not None else None
        if doffsets and skel is None:
            raise ValueError("forward_vjp: doffsets is the gradient of the offsets passed in the same call (offsets=None)")
        want_doff = skel is not None and (bool(doffsets) or (out is not None and "doffsets" in out))
        zp = _check(z, "z", (B, LATENT), torch.float32, dev)
        cp = _check(cur_rot, "cur_rot", (B, 4), torch.float32, dev)
        g = _lib.DpGradIn()
        for name, t in grads.items():
            if name not in _GRAD_NAMES:
                raise ValueError(f"grads: unknown output {name!r} (one of {', '.join(_GRAD_NAMES)})")
            if t is not None:
                setattr(g, name, _check(t, "grads[" + name + "]", (B,) + _OUT_SPECS[name][0], torch.float32, dev))
        res = {}
        specs = (("dz", (B, LATENT), torch.float32), ("dcur_rot", (B, 4), torch.float32), ("status", (B,), torch.int32))
        for name, shape, dtype in specs + ((("doffsets", (B, NJ, 3), torch.float32),) if want_doff else ()):
            t = out[name] if out is not None and name in out else torch.empty(shape, dtype=dtype, device=dev)
            _check(t, name, shape, dtype, dev)
            res[name] = t
        ptr = {name: C.c_void_p(t.data_ptr()) for name, t in res.items()}
        if skel is None:
            fn, args = self.lib.dp_forward_vjp, (C.byref(g), ptr["dz"], ptr["dcur_rot"], ptr["status"])
        else:
            fn, args = self.lib.dp_forward_vjp_skeleton, (C.byref(skel), C.byref(g), ptr["dz"], ptr["dcur_rot"], ptr.get("doffsets"), ptr["status"])
        self._call(fn, B, C.c_void_p(zp), C.c_void_p(cp), *args)
        return res

    def sequence_advance(self, frame, global_pos, global_rot, latent_buf, disp_buf, heights_buf, height_joints, pose_ret=None,
                         pos_ret=None, adjust=None, tgt_pos=None):
        """The reference's per-frame epilogue (drag_pose.py:369-402) for S sequences in one launch: updates
        `global_pos`, `global_rot` and the three history buffers IN PLACE from `frame` (the dict `optimize` returned:
        z_pre, pose, disp, world_disp, world_rot, pos) and fills `pose_ret` / `pos_ret`.
        `adjust` = (joint, target_joint, weight) or None; `tgt_pos` = this frame's dense [S,22,3] targets."""
        S = int(global_pos.shape[0])
        dev = self.device
        res = _lib.DpResult()
        for name in ("z_pre", "pose", "disp", "world_disp", "world_rot", "pos"):
            shape, dtype = _OUT_SPECS[name]
            setattr(res, name, _check(frame[name], name, (S,) + shape, dtype, dev))
        st, step = _seq_state(S, global_pos, global_rot, latent_buf, disp_buf, heights_buf, height_joints, adjust, dev)
        if adjust is not None:
            step.tgt_pos = _check(tgt_pos, "tgt_pos", (S, NJ, 3), torch.float32, dev)
        if pose_ret is not None:
            step.pose_ret = _check(pose_ret, "pose_ret", (S, 88), torch.float32, dev)
        if pos_ret is not None:
            step.pos_ret = _check(pos_ret, "pos_ret", (S, 3), torch.float32, dev)
        self._call(self.lib.dp_sequence_advance, S, C.byref(res), C.byref(st), C.byref(step))

    def _sequence_structs(self, tgt_pos, tgt_rot, tgt_root, w, tracked, z_tgt, z_tgt_strides, global_pos, global_rot, latent_buf, disp_buf,
                          heights_buf, height_joints, adjust, own_targets=False):
        """-> (dp_seq_frames, dp_seq_state, dp_seq_step) of a whole-sequence launch, every tensor checked; own_targets: the launch forms its z_tgt rows"""
        T, S = int(tgt_pos.shape[0]), int(tgt_pos.shape[1])
        dev = self.device
        fr = _lib.DpSeqFrames()
        fr.n_steps = T
        fr.tgt_pos = _check(tgt_pos, "tgt_pos", (T, S, NJ, 3), torch.float32, dev)
        fr.tgt_rot = _check(tgt_rot, "tgt_rot", (T, S, NJ, 9), torch.float32, dev)
        fr.tgt_root = _check(tgt_root, "tgt_root", (T, S, 3), torch.float32, dev) if tgt_root is not None else None
        fr.w = _check(w, "w", (S, NJ, 2), torch.float32, dev)
        fr.tracked = _check(tracked, "tracked", (S, NJ), torch.uint8, dev)
        if own_targets:
            fr.z_tgt, fr.z_tgt_step, fr.z_tgt_seq = None, 0, 0
        else:
            if z_tgt.device != dev or z_tgt.dtype != torch.float32:
                raise ValueError("z_tgt: expected an fp32 tensor on the optimiser's device")
            fr.z_tgt, fr.z_tgt_step, fr.z_tgt_seq = z_tgt.data_ptr(), int(z_tgt_strides[0]), int(z_tgt_strides[1])
        return (fr,) + _seq_state(S, global_pos, global_rot, latent_buf, disp_buf, heights_buf, height_joints, adjust, dev)

    def optimize_sequence(self, latent, tgt_pos, tgt_rot, tgt_root, w, tracked, z_tgt, z_tgt_strides, global_pos, global_rot, latent_buf, disp_buf,
                          heights_buf, height_joints, n_iter=100, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, lambda_rot=1.0, lambda_tmp=0.0,
                          stop_eps_pos=1e-4, stop_eps_rot=1e-2, min_loss_incr=1e-5, adjust=None, pose_ret=None, pos_ret=None, iters=None,
                          loss=None, scratch=None, status=None, offsets=None, constraints=None, terms=None, loss_extra=None, loss_terms=None,
                          joint_pos=None, holds=None, hold_state=None, hold_trace=None, ar=None, z_tgt_trace=None, gaps=None, gap_state=None,
                          present=None, gap_trace=None, live=False, tethers=None, tether_state=None, tether_trace=None):
        """T consecutive frames of S sequences in one launch (include/dragposer.h: dp_optimize_sequence): the optimise loop with the
        reference's while-condition and run()'s epilogue per frame, state carried on the device.  tgt_pos [T,S,22,3] / tgt_rot
        [T,S,22,9] dense per joint; tgt_root [T,S,3] or None (position targets are then tgt_pos + (tgt_root[t] - running global
        position), eval_drag.py:186-199); w [S,22,2], tracked [S,22]; z_tgt any fp32 device tensor addressed with `z_tgt_strides` =
        (floats between steps, floats between sequences).  `latent` [S,24], `global_pos`, `global_rot` and the three history
        buffers are updated IN PLACE.  Returns dict(pose_ret [T,S,88], pos_ret [T,S,3], iters [T,S], loss [T,S,3], status [T,S]: DP_STATUS_* bits).
        `offsets` [22,3] / [S,22,3]: one skeleton for every sequence / one per sequence, kept for every step (dp_optimize_sequence_skeleton,
        include/dragposer_skeleton.h); None = the context's.
        `constraints` (a dragposer_amd.Constraints) or `terms` (a dragposer_amd.Terms; a term's `per_frame` [S,4] held for all frames or
        [T,S,4]): the extra loss terms in every frame's loss, the frame loop still in one launch -- dp_optimize_sequence_constrained /
        dp_optimize_sequence_terms (include/dragposer_sequence_constraints.h), bit for bit what optimize_constrained / optimize_terms,
        sequence_advance and a copy of the latent give frame by frame; the floor, PLANE and point-DISTANCE terms read `global_pos` as it
        runs.  The dict then also holds `loss_extra` [T,S,4] / `loss_terms` [T,S,len(terms)] and `joint_pos` [T,S,22,3] (storage for them
        may be passed).  Both None: dp_optimize_sequence, unchanged.
        `holds` (a dragposer_amd.Holds, with `terms`): joints held where they touched down, dp_optimize_sequence_holds
        (include/dragposer_holds.h).  `hold_state` [S,len(holds),4] is updated IN PLACE (required); `hold_trace` [T,S,len(holds),4] or True
        (allocated here) receives the state after every step and is returned as `hold_trace`.
        `ar` (a dragposer_amd.LatentAR): every step's z_tgt row is formed in the launch from the sequence's last history rows,
        dp_optimize_sequence_ar (include/dragposer_latent_ar.h) -- `z_tgt` must then be None (`z_tgt_strides` is ignored), `terms` / `holds`
        are optional (`constraints` is not taken: Terms.from_constraints turns them into a table) and `latent_buf` holds at least
        `ar.order` rows.  `z_tgt_trace` [T,S,24] or True (allocated here) receives the row every step used and is returned as `z_tgt_trace`.
        `gaps` (a dragposer_amd.Gaps): trackers that drop out and come back, dp_optimize_sequence_gaps (include/dragposer_gaps.h), with or
        without `ar` (without: `z_tgt` as usual); `terms` / `holds` are optional, `constraints` is not taken.  `gap_state` [S,22,16] is
        updated IN PLACE (required); `present` [T,S,22] uint8 or None (NaN samples alone mark gaps); `gap_trace` [T,S,22] uint8 or True
        (allocated here) receives every joint's code of every step and is returned as `gap_trace`.  `status` then also carries
        DP_STATUS_TRACKER_HELD / _LOST / DP_STATUS_NO_TRACKER.
        `live` (with `gaps`, T = 1): the same frame as ONE launch, dp_live_step (include/dragposer_live.h) -- the kernel appends the step's row
        to the three history buffers itself; the bits of the call without it.
        `tethers` (a dragposer_amd.Tethers, with `terms` and `gaps`): joints tied to their own recent path, dp_optimize_sequence_tethers
        (include/dragposer_tethers.h), with or without `holds` and `ar`; pass Gaps(0, 1.0) for none to hold.  `tether_state`
        [S,len(tethers),8] is updated IN PLACE (required); `tether_trace` [T,S,len(tethers),8] or True (allocated here) receives the state
        after every step and is returned as `tether_trace`.  Not together with `live`.
        A `terms` table with points (include/dragposer_points.h) runs through dp_optimize_sequence_terms_points, `offsets` allowed; not
        together with `holds`, `gaps`, `ar`, `tethers` or `live`."""
        live = bool(live)
        terms = _sequence_refusals(tgt_pos, latent_buf, z_tgt, constraints, terms, loss_extra, loss_terms, joint_pos, holds, hold_state, hold_trace, ar,
                                   z_tgt_trace, gaps, gap_state, present, gap_trace, live, tethers, tether_state, tether_trace)
        T, S = int(tgt_pos.shape[0]), int(tgt_pos.shape[1])
        dev = self.device
        skel = self._skeleton(offsets, S, "optimize_sequence") if offsets is not None else None
        fr, st, step = self._sequence_structs(tgt_pos, tgt_rot, tgt_root, w, tracked, z_tgt, z_tgt_strides, global_pos, global_rot, latent_buf,
                                              disp_buf, heights_buf, height_joints, adjust, own_targets=ar is not None)
        res = _lib.DpSeqResults()
        res.world_rot = None
        specs = (("pose_ret", pose_ret, (T, S, 88), torch.float32, res), ("pos_ret", pos_ret, (T, S, 3), torch.float32, res),
                 ("iters", iters, (T, S), torch.int32, res), ("loss", loss, (T, S, 3), torch.float32, res), ("status", status, (T, S), torch.int32, res))
        outs, scratch = _step_outputs(specs, res, scratch, (T, S, LATENT + 3 + len(height_joints)), dev)
        p = self._params(n_iter, lr, betas, eps, lambda_rot, lambda_tmp, stop_eps_pos, stop_eps_rot, min_loss_incr, early=True)
        lp = C.c_void_p(_check(latent, "latent", (S, LATENT), torch.float32, dev))
        tail = (C.byref(st), C.byref(step), C.byref(res))
        if constraints is not None or terms is not None:
            ex = _lib.DpSeqExtra()
            per_step = ("loss_extra", loss_extra, (T, S, 4)) if terms is None else ("loss_terms", loss_terms, (T, S, len(terms)))
            for field, given, shape in (per_step, ("joint_pos", joint_pos, (T, S, NJ, 3))):
                buf = given if given is not None else torch.empty(shape, dtype=torch.float32, device=dev)
                setattr(ex, field, _check(buf, field, shape, torch.float32, dev) if buf.numel() else None)
                outs[field] = buf
            if terms is None:
                own, keep, fn = constraints.to_struct(), None, self.lib.dp_optimize_sequence_constrained
            else:
                own, keep = terms.to_struct(S, dev, steps=T)
                ex.row_step[:len(terms)] = terms.row_steps(S)
                fn = self.lib.dp_optimize_sequence_terms
            mid = ()
            if terms is not None and terms.has_points:
                ps, keep_p = terms.points.to_struct()
                fn, mid = self.lib.dp_optimize_sequence_terms_points, (C.byref(ps),)
            # the layers above the table: the highest one present names the entry point, which takes every layer up to it (absent ones as NULL)
            a = dict(T=T, S=S, dev=dev, terms=terms, holds=holds, hold_state=hold_state, hold_trace=hold_trace, ar=ar, z_tgt_trace=z_tgt_trace, gaps=gaps,
                     gap_state=gap_state, present=present, gap_trace=gap_trace, tethers=tethers, tether_state=tether_state, tether_trace=tether_trace)
            slots, keeps = [], []
            for layer, trace_name, trace_shape, dtype, entry, to_struct in _SEQ_LAYERS:
                if a[layer] is None:
                    slots.append(None)
                    continue
                trace = _traced(a[trace_name], (T, S) + trace_shape(a), dtype, dev)
                s, keep_s = to_struct(a, trace)
                keeps.append(keep_s)
                slots.append(C.byref(s))
                fn, mid = getattr(self.lib, entry), tuple(slots)
                if trace is not None:
                    outs[trace_name] = trace
            if live:
                fn = self.lib.dp_live_step
            self._call(fn, S, lp, C.byref(fr), C.byref(p), C.byref(own), *mid, C.byref(skel) if skel is not None else None, *tail, C.byref(ex))
            del keep, keeps
            return outs
        fn, args = (self.lib.dp_optimize_sequence, tail) if skel is None else (self.lib.dp_optimize_sequence_skeleton, (C.byref(skel),) + tail)
        self._call(fn, S, lp, C.byref(fr), C.byref(p), *args)
        return outs

    def optimize_sequence_lm(self, latent, tgt_pos, tgt_rot, tgt_root, w, tracked, z_tgt, z_tgt_strides, global_pos, global_rot, latent_buf, disp_buf,
                             heights_buf, height_joints, lm=None, lambda_rot=1.0, lambda_tmp=0.0, stop_eps_pos=0.0, stop_eps_rot=0.0, mu=None, ar=None,
                             adjust=None, pose_ret=None, pos_ret=None, iters=None, loss=None, scratch=None, status=None, world_rot=None,
                             mu_trace=None, n_accepted=None, loss0=None, joint_pos=None, z_tgt_trace=None, outputs=None, terms=None, loss_terms=None):
        """T consecutive frames of S sequences solved by Levenberg-Marquardt steps in one launch (include/dragposer_sequence_lm.h:
        dp_optimize_sequence_lm): bit for bit what optimize_lm, sequence_advance and a copy of the latent give frame by frame.  Inputs and
        state as in `optimize_sequence`; `lm`: a dragposer_amd.LM (None = LM(); its `predictor` is not read here).  `mu` [S] fp32: the damping
        of every sequence, read and updated IN PLACE; None: every sequence starts at lm.mu0.  `ar` (a dragposer_amd.LatentAR): every step's
        z_tgt row is formed in the launch from the sequence's last history rows -- `z_tgt` must then be None, and `z_tgt_trace` [T,S,24] or
        True (allocated here) receives the rows.  Returns dict(pose_ret, pos_ret, iters [T,S] = the steps executed, loss [T,S,3], status, world_rot
        [T,S,4], mu_trace [T,S], n_accepted [T,S], loss0 [T,S,3], joint_pos [T,S,22,3]) and `mu` when given; `outputs`: the subset of those
        names to produce (the others' pointers are NULL; `loss` and `loss0` each cost a pass in double per frame).  Asynchronous on torch's
        current stream.
        `terms` (a dragposer_amd.Terms without points; a term's `per_frame` [S,4] held for all frames or [T,S,4]): the table's terms in every
        step's LM loss, the frame loop still in one launch -- dp_optimize_sequence_lm_terms (include/dragposer_sequence_lm_terms.h), bit for
        bit what optimize_lm(terms=, global_pos=the running position), sequence_advance and a copy of the latent give frame by frame.  The
        dict then also holds `loss_terms` [T,S,len(terms)] (storage may be passed; with `outputs`, only when named there).  terms=None:
        dp_optimize_sequence_lm, unchanged."""
        from .lm import LM

        lm = (lm if lm is not None else LM()).check()
        if terms is None and loss_terms is not None:
            raise ValueError("optimize_sequence_lm: loss_terms is an output of terms=")
        if terms is not None:
            if terms.has_points:
                raise ValueError("optimize_sequence_lm: a table with points does not go with the LM solver (include/dragposer_sequence_lm_terms.h, "
                                 "\"Not covered\")")
            terms.check()
        if ar is None and z_tgt_trace is not None:
            raise ValueError("optimize_sequence_lm: z_tgt_trace belongs to ar=")
        if ar is not None and z_tgt is not None:
            raise ValueError("optimize_sequence_lm: ar= forms the targets itself, pass z_tgt=None")
        if ar is None and z_tgt is None:
            raise ValueError("optimize_sequence_lm: pass z_tgt or ar=")
        T, S = int(tgt_pos.shape[0]), int(tgt_pos.shape[1])
        dev = self.device
        H, NH = int(latent_buf.shape[1]), len(height_joints)
        if ar is not None and ar.order > H:
            raise ValueError(f"optimize_sequence_lm: latent_buf holds {H} rows, fewer than ar.order = {ar.order}")
        fr, st, step = self._sequence_structs(tgt_pos, tgt_rot, tgt_root, w, tracked, z_tgt, z_tgt_strides, global_pos, global_rot, latent_buf,
                                              disp_buf, heights_buf, height_joints, adjust, own_targets=ar is not None)
        res, ex = _lib.DpSeqResults(), _lib.DpSeqLmExtra()
        specs = (("pose_ret", pose_ret, (T, S, 88), torch.float32, res), ("pos_ret", pos_ret, (T, S, 3), torch.float32, res),
                 ("iters", iters, (T, S), torch.int32, res), ("loss", loss, (T, S, 3), torch.float32, res), ("status", status, (T, S), torch.int32, res),
                 ("world_rot", world_rot, (T, S, 4), torch.float32, res), ("mu_trace", mu_trace, (T, S), torch.float32, ex),
                 ("n_accepted", n_accepted, (T, S), torch.int32, ex), ("loss0", loss0, (T, S, 3), torch.float32, ex),
                 ("joint_pos", joint_pos, (T, S, NJ, 3), torch.float32, ex))
        if outputs is not None:
            unknown = [n for n in outputs if n not in [sp[0] for sp in specs] + (["loss_terms"] if terms is not None else [])]
            if unknown:
                raise ValueError(f"optimize_sequence_lm: unknown output {unknown[0]!r}")
        if mu is not None:  # (storage given means produced: `mu` is returned when given and never allocated here)
            specs += (("mu", mu, (S,), torch.float32, ex),)
        outs, scratch = _step_outputs(specs, res, scratch, (T, S, LATENT + 3 + NH), dev, outputs)
        rs, keep = None, None
        if ar is not None:
            z_tgt_trace = _traced(z_tgt_trace, (T, S, LATENT), torch.float32, dev)
            rs, keep = ar.to_struct(dev, z_tgt_trace, (T, S, LATENT))
            if z_tgt_trace is not None:
                outs["z_tgt_trace"] = z_tgt_trace
        p = lm.to_struct(lambda_rot, lambda_tmp, stop_eps_pos, stop_eps_rot)
        lp = C.c_void_p(_check(latent, "latent", (S, LATENT), torch.float32, dev))
        fn, head, last, keep_t = self.lib.dp_optimize_sequence_lm, (), (), None
        if terms is not None:  # (the table goes in before the predictor, its per-step output and row steps after everything else)
            tx = _lib.DpSeqExtra()
            if loss_terms is not None or outputs is None or "loss_terms" in outputs:
                lt = loss_terms if loss_terms is not None else torch.empty(T, S, len(terms), dtype=torch.float32, device=dev)
                tx.loss_terms = _check(lt, "loss_terms", (T, S, len(terms)), torch.float32, dev) if lt.numel() else None
                outs["loss_terms"] = lt
            own, keep_t = terms.to_struct(S, dev, steps=T)
            tx.row_step[:len(terms)] = terms.row_steps(S)
            fn, head, last = self.lib.dp_optimize_sequence_lm_terms, (C.byref(own),), (C.byref(tx),)
        self._call(fn, S, lp, C.byref(fr), C.byref(p), *head, C.byref(rs) if rs is not None else None, C.byref(st), C.byref(step), C.byref(res),
                   C.byref(ex), *last)
        del keep, keep_t
        return outs


def check_rotation_targets(tgt_rot, tracked, tol=1e-3):
    """Raises ValueError unless every tracked joint's 3x3 target is orthonormal with determinant +1 (within `tol`)."""
    R = tgt_rot.reshape(-1, NJ, 3, 3)
    m = tracked.reshape(-1, NJ).bool()
    if not bool(m.any()):
        return
    Rt = R[m].double()
    dev_orth = (Rt @ Rt.transpose(-1, -2) - torch.eye(3, dtype=Rt.dtype, device=Rt.device)).abs().amax()
    dev_det = (torch.linalg.det(Rt) - 1.0).abs().amax()
    worst = float(torch.maximum(dev_orth, dev_det))
    if not worst <= tol:
        raise ValueError(f"tgt_rot: tracked targets must be rotation matrices (orthonormal, det +1); worst deviation {worst:.3g} > {tol}")


def to_device_batch(np_batch, device):
    """numpy dict (z0, z_tgt, cur_rot, tgt_pos, tgt_rot, w, tracked) -> device tensors."""
    out = {}
    for k in ("z0", "z_tgt", "cur_rot", "tgt_pos", "tgt_rot", "w"):
        out[k] = torch.from_numpy(np.ascontiguousarray(np_batch[k], dtype=np.float32)).to(device)
    out["tracked"] = torch.from_numpy(np.ascontiguousarray(np_batch["tracked"], dtype=np.uint8)).to(device)
    return out

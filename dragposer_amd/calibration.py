"""Bone lengths from tracker data (include/dragposer_calibration.h): `BoneGroups` says which bones share a scale,
`LatentOptimizer.fit_bones(...)` fits the scales at given latents in one call, and `calibrate(...)` alternates that fit with
`LatentOptimizer.optimize(offsets=...)` -- block coordinate descent on the optimiser's own loss -- for a performer whose poses are unknown
too.  The result's `offsets` [22,3] go wherever per-frame skeletons are taken (include/dragposer_skeleton.h)."""
import ctypes as C
import math

import numpy as np

from . import _lib
from .model import NJ


class BoneGroups:
    """`groups`: 22 ints, entry j = the group of bone j (the offset of joint j from its parent) in -1..K-1; -1: the bone keeps its base
    length; entry 0 (the root has no bone) is ignored.  Every group 0..K-1 owns at least one bone, K <= 24."""

    def __init__(self, groups):
        g = [int(x) for x in groups]
        if len(g) != NJ:
            raise ValueError(f"BoneGroups: {len(g)} entries, expected {NJ} (one per joint; entry 0 is ignored)")
        g[0] = -1
        self.groups = tuple(g)
        self.check()

    def __len__(self):
        return max(self.groups) + 1

    def check(self):
        """raises ValueError for what dp_fit_bones would refuse of the groups, in its order"""
        K = len(self)
        if not 1 <= K <= _lib.DP_FIT_MAX_GROUPS:
            raise ValueError(f"BoneGroups: {K} groups, outside 1..{_lib.DP_FIT_MAX_GROUPS}")
        for j, x in enumerate(self.groups[1:], 1):
            if x < -1:
                raise ValueError(f"BoneGroups: groups[{j}] is {x}, outside -1..{K - 1}")
        for k in range(K):
            if k not in self.groups[1:]:
                raise ValueError(f"BoneGroups: group {k} owns no bone")
        return self

    @classmethod
    def uniform(cls):
        """one scale for the whole skeleton"""
        return cls([-1] + [0] * (NJ - 1))

    @classmethod
    def limbs(cls):
        """legs / spine + neck / arms: joints 1-8 / 9-13 / 14-21 of the shipped tree"""
        return cls([-1] + [0] * 8 + [1] * 5 + [2] * 8)

    @classmethod
    def symmetric(cls):
        """13 groups of the shipped tree, left = right: the four leg bones (hip, knee, ankle, toe: joints 1-4 = 5-8), the five bones of the
        spine, neck and head (9-13), the four arm bones (14-17 = 18-21)"""
        return cls([-1, 0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 9, 10, 11, 12])

    @classmethod
    def per_bone(cls):
        """a scale per bone: 21 groups"""
        return cls([-1] + list(range(NJ - 1)))

    def members(self, k):
        """the bones (joint indices) of group k"""
        return [j for j in range(1, NJ) if self.groups[j] == k]

    def to_struct(self, base=None, prior=None, ridge=1e-3):
        """-> (dp_bone_fit without its workspace, the host arrays its pointers refer to: keep them alive until the call has returned)"""
        K = len(self)
        if not (math.isfinite(float(ridge)) and float(ridge) >= 0.0):
            raise ValueError("fit_bones: ridge is negative or not finite")
        keep = [(C.c_int * NJ)(*self.groups)]
        fit = _lib.DpBoneFit(n_groups=K, ridge=float(ridge))
        fit.groups = C.cast(keep[0], C.c_void_p)
        if base is not None:
            b = np.ascontiguousarray(np.asarray(base, dtype=np.float32))
            if b.shape != (NJ, 3):
                raise ValueError(f"fit_bones: base must be [22,3] host values, got {b.shape}")
            keep.append(b)
            fit.base = b.ctypes.data
        if prior is not None:
            p = np.ascontiguousarray(np.asarray(prior, dtype=np.float32))
            if p.shape != (K,):
                raise ValueError(f"fit_bones: prior must hold {K} values, got {p.shape}")
            keep.append(p)
            fit.prior = p.ctypes.data
        return fit, keep


class Calibration:
    """what `calibrate` returns: `offsets` [22,3] and `scales` [K] (device tensors of the last round), `z` [B,24] (the last round's latents)
    and `trace`: per round dict(scales [K], rms [2], frames, flags) as host values"""

    def __init__(self, offsets, scales, z, trace):
        self.offsets, self.scales, self.z, self.trace = offsets, scales, z, trace


def calibrate(opt, batch, groups, rounds=6, n_iter=50, ridge=1e-3, base=None, **optimize_kw):
    """Bone scales of a performer from `batch` (the dict of `optimize`'s seven device tensors: frames of tracker data, independent of each
    other) when the poses are unknown too.  Round r runs opt.optimize(offsets = the offsets of round r-1, z0 = the latents of round r-1) --
    round 1 from `base` (None: the context's skeleton) and batch["z0"] -- and then opt.fit_bones at the latents it returned; each half-step
    lowers the same loss.  `optimize_kw` goes to opt.optimize (lambda_tmp=0.0 for frames that are not consecutive).  Every launch is
    asynchronous on torch's current stream and nothing is read back inside the loop: the trace is copied to the host once, at the end."""
    import torch

    if rounds < 1:
        raise ValueError("calibrate: rounds must be at least 1")
    K = len(groups)
    b = dict(batch)
    z = b.pop("z0")
    offsets = None if base is None else torch.as_tensor(np.ascontiguousarray(np.asarray(base, dtype=np.float32))).to(opt.device)
    scales_t = torch.empty(rounds, K, dtype=torch.float32, device=opt.device)
    rms_t = torch.empty(rounds, 2, dtype=torch.float32, device=opt.device)
    info_t = torch.empty(rounds, 2, dtype=torch.int32, device=opt.device)
    for r in range(rounds):
        z = opt.optimize(z0=z, **b, n_iter=n_iter, offsets=offsets, outputs=("z",), **optimize_kw)["z"]
        fit = opt.fit_bones(z, b["cur_rot"], b["tgt_pos"], b["w"], b["tracked"], groups, base=base, ridge=ridge,
                            outputs=("offsets",), out=dict(scales=scales_t[r], rms=rms_t[r], info=info_t[r]))
        offsets = fit["offsets"]
    scales_h, rms_h, info_h = scales_t.cpu().numpy(), rms_t.cpu().numpy(), info_t.cpu().numpy()  # (the one synchronisation)
    trace = [dict(scales=scales_h[r], rms=rms_h[r], frames=int(info_h[r, 0]), flags=int(info_h[r, 1])) for r in range(rounds)]
    return Calibration(offsets, scales_t[rounds - 1], z, trace)

"""Holds: joints held where they touched down (foot lock) -- include/dragposer_holds.h, dp_optimize_sequence_holds.  A `Hold` refers to a
point-DISTANCE `Term` of a `Terms` table and turns its point into a per-sequence state (x, y, z, held): latched to the joint's world
position when the joint comes down to `level + contact_lo`, fed to the term while held, released when the joint rises above
`level + contact_hi`.  Used by `LatentOptimizer.optimize_sequence(terms=..., holds=...)`, `DragPose.run_frames(terms=..., holds=...)`
(one launch per stretch) and `DragPose.run(terms=..., holds=...)` (the same arithmetic frame by frame); semantics in the header's comment."""
import math
from dataclasses import dataclass, field, replace

from . import _lib
from .terms import DISTANCE, Terms

MAX_HOLDS = _lib.DP_MAX_HOLDS


@dataclass
class Hold:
    """One hold (dp_hold): `term` indexes the table; heights are along the table's up axis, relative to `level`."""
    term: int
    contact_lo: float
    contact_hi: float
    level: float = 0.0

    def check(self, terms=None, i=0):
        """ValueError for what dp_optimize_sequence_holds refuses of this hold (`terms`: the table it refers to, for the term's rules)"""
        def bad(msg):
            raise ValueError(f"hold {i}: {msg}")

        if not all(math.isfinite(float(x)) for x in (self.level, self.contact_lo, self.contact_hi)):
            bad("non-finite level, contact_lo or contact_hi")
        if self.contact_lo > self.contact_hi:
            bad("contact_lo is above contact_hi")
        if terms is None:
            return
        if not 0 <= int(self.term) < len(terms):
            bad(f"term {self.term} outside the table of {len(terms)}")
        t = terms.terms[int(self.term)]
        if t.type != DISTANCE:
            bad(f"term {self.term} is not a DISTANCE term")
        if t.joint_b != -1:
            bad(f"term {self.term} has a joint_b (a hold needs a point-DISTANCE term)")
        if t.per_frame is not None:
            bad(f"term {self.term} has a per_frame array (the hold's state is its row)")


@dataclass
class Holds:
    """The holds of a table (dp_holds): up to 4.  The state is a [S, len(holds), 4] fp32 device tensor of (x, y, z, held) the caller owns
    (DragPose keeps it in `drag.hold_state`); zeros = nothing held."""
    holds: list = field(default_factory=list)

    def __len__(self):
        return len(self.holds)

    def check(self, terms=None):
        if len(self.holds) > MAX_HOLDS:
            raise ValueError(f"Holds: at most {MAX_HOLDS} holds, got {len(self.holds)}")
        seen = {}
        for i, h in enumerate(self.holds):
            h.check(terms, i)
            if int(h.term) in seen:
                raise ValueError(f"hold {i}: term {h.term} is already held by hold {seen[int(h.term)]}")
            seen[int(h.term)] = i

    def to_struct(self, terms, S, device, state, trace=None, steps=None):
        """-> (_lib.DpHolds, the DpHold array it points to: keep both alive for the call)"""
        import torch

        from .optimizer import _check

        self.check(terms)
        n = len(self.holds)
        arr = (_lib.DpHold * max(n, 1))(*[_lib.DpHold(term=int(h.term), level=float(h.level), contact_lo=float(h.contact_lo),
                                                      contact_hi=float(h.contact_hi)) for h in self.holds])
        s = _lib.DpHolds(n_holds=n)
        s.holds = _lib.C.cast(arr, _lib.C.c_void_p) if n else None
        s.state = _check(state, "hold_state", (S, n, 4), torch.float32, device) if n else None
        s.trace = _check(trace, "hold_trace", (steps, S, n, 4), torch.float32, device) if trace is not None and n else None
        return s, arr

    def new_state(self, S, device):
        import torch

        return torch.zeros(S, len(self.holds), 4, dtype=torch.float32, device=device)

    def frame_terms(self, terms, state):
        """the table of ONE frame of the per-frame composition: every active held term reads its row from a copy of its slice of `state` [S, n, 4]"""
        ts = list(terms.terms)
        for i, h in enumerate(self.holds):
            if ts[h.term].active:
                ts[h.term] = replace(ts[h.term], per_frame=state[:, i].contiguous())
        return Terms(ts, terms.up_axis)

    def update(self, terms, state, pos, global_pos):
        """the header's update after one frame, in place on `state`, with torch fp32 ops on the device and no synchronisation: `pos`
        [S,22,3] the frame's joint positions, `global_pos` [S,3] the advanced global position"""
        import torch

        import numpy as np

        f32 = lambda x: float(np.float32(x))  # (the fp32 value the library compares with, whatever torch does with a Python scalar)
        up = int(terms.up_axis)
        for i, h in enumerate(self.holds):
            t = terms.terms[h.term]
            if not t.active:
                continue
            W = global_pos + (pos[:, t.joint_a] - pos[:, 0])
            hgt = W[:, up] - f32(h.level)
            st = state[:, i]
            free = st[:, 3] == 0
            latch = free & (hgt <= f32(h.contact_lo))
            release = ~free & (hgt > f32(h.contact_hi))
            st[:, :3] = torch.where(latch[:, None], W, st[:, :3])
            st[:, 3] = torch.where(latch, torch.ones_like(hgt), torch.where(release, torch.zeros_like(hgt), st[:, 3]))

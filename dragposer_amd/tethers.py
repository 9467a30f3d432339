"""Tethers: joints tied to their own recent path -- include/dragposer_tethers.h, dp_optimize_sequence_tethers.  A `Tether` refers to a
point-DISTANCE `Term` of a `Terms` table and turns its point into a per-sequence state that follows the joint's own reconstructed world
position: after every frame the point becomes W + alpha * (W - Wprev), W being where the frame put the joint.  The term's band [lo, hi]
is then a speed limit (hi metres per frame move for free; lo = hi = 0: quadratic velocity damping; alpha = 1: acceleration damping).
Used by `LatentOptimizer.optimize_sequence(terms=..., tethers=...)`, `DragPose.run_frames(terms=..., tethers=...)` (one launch per
stretch) and `DragPose.run(terms=..., tethers=...)` (the same arithmetic frame by frame); semantics in the header's comment."""
import math
from dataclasses import dataclass, field, replace

from . import _lib
from .terms import DISTANCE, Terms

MAX_TETHERS = _lib.DP_MAX_TETHERS
STATE_FLOATS = _lib.DP_TETHER_STATE_FLOATS
INPUT_LIMIT = 1.0e4  # DP_INPUT_LIMIT


@dataclass
class Tether:
    """One tether (dp_tether): `term` indexes the table; `alpha` in [0, 1] extrapolates the point by the last frame's motion."""
    term: int
    alpha: float = 0.0

    def check(self, terms=None, i=0):
        """ValueError for what dp_optimize_sequence_tethers refuses of this tether (`terms`: the table it refers to, for the term's rules)"""
        def bad(msg):
            raise ValueError(f"tether {i}: {msg}")

        if terms is not None:
            if not 0 <= int(self.term) < len(terms):
                bad(f"term {self.term} outside the table of {len(terms)}")
            t = terms.terms[int(self.term)]
            if t.type != DISTANCE:
                bad(f"term {self.term} is not a DISTANCE term")
            if t.joint_b != -1:
                bad(f"term {self.term} has a joint_b (a tether needs a point-DISTANCE term)")
            if t.per_frame is not None:
                bad(f"term {self.term} has a per_frame array (the tether's state is its row)")
        a = float(self.alpha)
        if not (math.isfinite(a) and 0.0 <= a <= 1.0):
            bad("alpha must be a finite number in [0, 1]")


@dataclass
class Tethers:
    """The tethers of a table (dp_tethers): up to 4.  The state is a [S, len(tethers), 8] fp32 device tensor the caller owns (DragPose keeps
    it in `drag.tether_state`): (x, y, z, live) the term's row, (wx, wy, wz, have) the joint's last world position; zeros = no path yet."""
    tethers: list = field(default_factory=list)

    def __len__(self):
        return len(self.tethers)

    def check(self, terms=None, holds=None):
        """the header's refusals, in its order: the count, then per tether the term's rules, another tether or a hold on the term, alpha"""
        if len(self.tethers) > MAX_TETHERS:
            raise ValueError(f"Tethers: at most {MAX_TETHERS} tethers, got {len(self.tethers)}")
        held = {int(h.term): i for i, h in enumerate(holds.holds)} if holds is not None else {}
        seen = {}
        for i, t in enumerate(self.tethers):
            Tether(t.term, 0.0).check(terms, i)
            if int(t.term) in seen:
                raise ValueError(f"tether {i}: term {t.term} is already tethered by tether {seen[int(t.term)]}")
            if int(t.term) in held:
                raise ValueError(f"tether {i}: term {t.term} is held by hold {held[int(t.term)]}")
            t.check(None, i)
            seen[int(t.term)] = i

    def to_struct(self, terms, S, device, state, trace=None, steps=None, holds=None):
        """-> (_lib.DpTethers, the DpTether array it points to: keep both alive for the call)"""
        import torch

        from .optimizer import _check

        self.check(terms, holds)
        n = len(self.tethers)
        arr = (_lib.DpTether * max(n, 1))(*[_lib.DpTether(term=int(t.term), alpha=float(t.alpha)) for t in self.tethers])
        s = _lib.DpTethers(n_tethers=n)
        s.tethers = _lib.C.cast(arr, _lib.C.c_void_p) if n else None
        s.state = _check(state, "tether_state", (S, n, STATE_FLOATS), torch.float32, device) if n else None
        s.trace = _check(trace, "tether_trace", (steps, S, n, STATE_FLOATS), torch.float32, device) if trace is not None and n else None
        return s, arr

    def new_state(self, S, device):
        import torch

        return torch.zeros(S, len(self.tethers), STATE_FLOATS, dtype=torch.float32, device=device)

    def frame_terms(self, terms, state):
        """the table of ONE frame of the per-frame composition: every active tethered term reads its row from a copy of words 0..3 of its
        slice of `state` [S, n, 8]"""
        ts = list(terms.terms)
        for i, t in enumerate(self.tethers):
            if ts[t.term].active:
                ts[t.term] = replace(ts[t.term], per_frame=state[:, i, :4].contiguous())
        return Terms(ts, terms.up_axis)

    def update(self, terms, state, pos, global_pos):
        """the header's update after one frame, in place on `state`, with torch fp32 ops on the device, one op per rounding and no
        synchronisation: `pos` [S,22,3] the frame's joint positions, `global_pos` [S,3] the advanced global position"""
        import torch

        import numpy as np

        for i, te in enumerate(self.tethers):
            t = terms.terms[te.term]
            if not t.active:
                continue
            st = state[:, i]
            W = global_pos + (pos[:, t.joint_a] - pos[:, 0])
            ok = (W.abs() <= INPUT_LIMIT).all(dim=1)  # (the comparison form: a NaN fails it)
            alpha = torch.full((), float(np.float32(te.alpha)), dtype=torch.float32, device=W.device)
            ext = W + alpha * (W - st[:, 4:7])
            point = torch.where((st[:, 7] != 0)[:, None], ext, W)
            one = torch.ones_like(W[:, :1])
            new = torch.cat((point, one, W, one), dim=1)
            st.copy_(torch.where(ok[:, None], new, st))

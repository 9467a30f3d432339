"""Gaps: trackers that drop out and come back -- include/dragposer_gaps.h, dp_optimize_sequence_gaps.  A joint whose sample is absent in a
step (marked so through `present`, or refused by the screening: not finite, or beyond DP_INPUT_LIMIT) is held at its last good sample for up
to `max_hold` steps at a weight that decays by `decay` per step, and leaves the step's loss after that until a sample arrives again; the
sequence goes on.  Used by `LatentOptimizer.optimize_sequence(gaps=..., gap_state=...)`, `DragPose.run_frames(gaps=...)` and
`DragPose.run(gaps=...)`; `Gaps.step` is the header's rule in elementwise torch, for the per-frame composition."""
import math
from dataclasses import dataclass

from . import _lib

STATE_FLOATS = _lib.DP_GAP_STATE_FLOATS
INPUT_LIMIT = 1.0e4  # DP_INPUT_LIMIT
PRESENT, HELD, LOST = 1, 2, 3  # a joint's code of a step (0: not tracked by configuration)
NJ = 22


@dataclass
class Gaps:
    """dp_gaps' two numbers.  The state is a [S, 22, 16] fp32 tensor the caller owns (DragPose keeps it in `drag.gap_state`): per joint the
    world position (0-2) and rotation target (3-11) of the last good sample, valid (12), age (13), factor (14), 0 (15); zeros = nothing held."""
    max_hold: int
    decay: float = 1.0

    def check(self):
        if int(self.max_hold) != self.max_hold or not 0 <= int(self.max_hold) <= _lib.DP_GAP_MAX_HOLD:
            raise ValueError(f"Gaps: max_hold {self.max_hold} outside 0..{_lib.DP_GAP_MAX_HOLD}")
        d = float(self.decay)
        if not (math.isfinite(d) and 0.0 < d <= 1.0):
            raise ValueError(f"Gaps: decay {self.decay} must be a finite number in (0, 1]")

    def new_state(self, S, device):
        import torch

        return torch.zeros(S, NJ, STATE_FLOATS, dtype=torch.float32, device=device)

    def to_struct(self, S, device, state, present=None, trace=None, steps=None):
        """-> _lib.DpGaps pointing at the three tensors (keep them alive for the call)"""
        import torch

        from .optimizer import _check

        self.check()
        s = _lib.DpGaps(max_hold=int(self.max_hold), decay=float(self.decay))
        s.state = _check(state, "gap_state", (S, NJ, STATE_FLOATS), torch.float32, device)
        s.present = _check(present, "present", (steps, S, NJ), torch.uint8, device) if present is not None else None
        s.trace = _check(trace, "gap_trace", (steps, S, NJ), torch.uint8, device) if trace is not None else None
        return s

    def step(self, state, tgt_pos_eff, tgt_rot, w, tracked, gpos, present=None):
        """The header's rule for ONE step, in elementwise fp32 torch on the tensors' device, without synchronisation.  `state` [S,22,16] is
        advanced IN PLACE; tgt_pos_eff [S,22,3] the step's effective position targets (tgt_pos + (tgt_root - gpos) where a root is
        given), tgt_rot [S,22,9], w [S,22,2], tracked [S,22] uint8, gpos [S,3] the global position before the step, present [S,22] uint8
        or None.  -> (tgt_pos [S,22,3], tgt_rot [S,22,9], w [S,22,2], tracked [S,22] uint8, codes [S,22] uint8): what the step runs with.
        Rows of joints that are not in the step (code 0 or 3) are zero, with w as given."""
        import torch

        self.check()
        S = state.shape[0]
        cfg = tracked.reshape(S, NJ) != 0
        tp, tr = tgt_pos_eff.reshape(S, NJ, 3), tgt_rot.reshape(S, NJ, 9)
        refused = ~(torch.cat((tp, tr), dim=2).abs() <= INPUT_LIMIT)  # NaN, Inf or beyond the limit
        absent = refused.any(dim=2)
        if present is not None:
            absent = absent | (present.reshape(S, NJ) == 0)
        valid, age1 = state[:, :, 12] != 0, state[:, :, 13] + 1.0
        here = cfg & ~absent
        held = cfg & absent & valid & (age1 <= float(self.max_hold))
        lost = cfg & absent & ~held
        codes = (here * PRESENT + held * HELD + lost * LOST).to(torch.uint8)
        g = gpos.reshape(S, 1, 3)
        zero, one = torch.zeros_like(age1), torch.ones_like(age1)
        decay = torch.tensor(float(self.decay), dtype=torch.float32, device=state.device)
        h3, h9 = here[:, :, None], here[:, :, None]
        new = state.clone()
        new[:, :, 0:3] = torch.where(h3, tp + g, state[:, :, 0:3])
        new[:, :, 3:12] = torch.where(h9, tr, state[:, :, 3:12])
        new[:, :, 12] = torch.where(here, one, torch.where(lost, zero, state[:, :, 12]))
        new[:, :, 13] = torch.where(here, zero, torch.where(held, age1, state[:, :, 13]))
        new[:, :, 14] = torch.where(here, one, torch.where(held, state[:, :, 14] * decay, state[:, :, 14]))
        state.copy_(new)
        on = here | held
        tp_eff = torch.where(here[:, :, None], tp, torch.where(held[:, :, None], state[:, :, 0:3] - g, torch.zeros_like(tp)))
        tr_eff = torch.where(on[:, :, None], state[:, :, 3:12], torch.zeros_like(tr))
        w_eff = torch.where(on[:, :, None], w.reshape(S, NJ, 2) * state[:, :, 14:15], w.reshape(S, NJ, 2))
        return tp_eff.contiguous(), tr_eff.contiguous(), w_eff.contiguous(), on.to(torch.uint8), codes

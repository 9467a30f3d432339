"""The Levenberg-Marquardt solver's settings (include/dragposer_lm.h, include/dragposer_sequence_lm.h): LatentOptimizer.optimize_lm(lm=LM(...)),
LatentOptimizer.optimize_sequence_lm(lm=LM(...)) and DragPose.run / run_frames(solver=LM(...)).  Adam stays the default solver everywhere; an LM is asked for by name."""
import math
from dataclasses import dataclass

from . import _lib


@dataclass
class LM:
    """`steps` trials per frame (1..64), each one Gauss-Newton step damped by mu: accepted when the loss falls (mu <- max(mu mu_down, mu_min)),
    rejected otherwise (mu <- min(mu mu_up, mu_max)).  `early_stop`: a frame ends before a step once loss_pos <= stop_eps_pos and
    lambda_rot loss_rot <= stop_eps_rot, or after a rejection at mu_max.  The two thresholds given here win over the caller's
    (DragPose.run passes its own stop_eps_pos / stop_eps_rot when these are None).  `predictor` (a dragposer_amd.LatentAR, not part of the C
    struct): DragPose.run / run_frames then form every frame's pull target from the sequence's own last latents inside the launch,
    dp_optimize_sequence_lm, weighed by lambda_temporal.  `terms` (a dragposer_amd.Terms without points, not part of the C struct either): the
    table's terms join the LM loss of DragPose.run / run_frames(solver=) -- include/dragposer_lm_terms.h, include/dragposer_sequence_lm_terms.h;
    the table belongs to the solver as the predictor does, and terms= beside solver= stays refused.  LatentOptimizer's calls take their table
    as an argument of their own and do not read this one."""
    steps: int = 3
    mu0: float = 1e-2
    mu_up: float = 4.0
    mu_down: float = 1.0 / 3.0
    mu_min: float = 1e-6
    mu_max: float = 1e6
    early_stop: bool = True
    stop_eps_pos: float = None
    stop_eps_rot: float = None
    terms: object = None      # a dragposer_amd.Terms without points: the table in the LM loss (include/dragposer_sequence_lm_terms.h)
    predictor: object = None  # a dragposer_amd.LatentAR: the pull term's target formed inside the launch (include/dragposer_sequence_lm.h)

    def check(self):
        """raises ValueError for what dp_optimize_lm would refuse, in its order"""
        if not isinstance(self.steps, int) or not 1 <= self.steps <= _lib.DP_LM_MAX_STEPS:
            raise ValueError(f"LM: steps {self.steps!r} outside 1..{_lib.DP_LM_MAX_STEPS}")
        for name in ("mu0", "mu_up", "mu_down", "mu_min", "mu_max"):
            if not math.isfinite(float(getattr(self, name))):
                raise ValueError(f"LM: {name} is not finite")
        if not 0.0 < self.mu_down < 1.0:
            raise ValueError("LM: mu_down must lie in (0, 1)")
        if not self.mu_up > 1.0:
            raise ValueError("LM: mu_up must be greater than 1")
        if not 0.0 < self.mu_min <= self.mu_max:
            raise ValueError("LM: need 0 < mu_min <= mu_max")
        if not self.mu_min <= self.mu0 <= self.mu_max:
            raise ValueError("LM: mu0 outside [mu_min, mu_max]")
        if self.terms is not None:
            from .terms import Terms

            if not isinstance(self.terms, Terms):
                raise ValueError(f"LM: terms must be a dragposer_amd.Terms, got {type(self.terms).__name__}")
            if self.terms.has_points:
                raise ValueError("LM: a table with points does not go with the LM solver (include/dragposer_sequence_lm_terms.h, Not covered)")
            self.terms.check()
        if self.predictor is not None:
            from .ar import LatentAR

            if not isinstance(self.predictor, LatentAR):
                raise ValueError(f"LM: predictor must be a dragposer_amd.LatentAR, got {type(self.predictor).__name__}")
        return self

    def to_struct(self, lambda_rot, lambda_tmp, stop_eps_pos=0.0, stop_eps_rot=0.0):
        eps_p = self.stop_eps_pos if self.stop_eps_pos is not None else stop_eps_pos
        eps_r = self.stop_eps_rot if self.stop_eps_rot is not None else stop_eps_rot
        return _lib.DpLmParams(n_steps=int(self.steps), lambda_rot=float(lambda_rot), lambda_tmp=float(lambda_tmp), mu0=self.mu0, mu_up=self.mu_up,
                               mu_down=self.mu_down, mu_min=self.mu_min, mu_max=self.mu_max, early_stop=int(bool(self.early_stop)),
                               stop_eps_pos=float(eps_p), stop_eps_rot=float(eps_r))

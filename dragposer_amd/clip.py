"""The joint clip solver's settings (include/dragposer_clip_lm.h, include/dragposer_clip_accel.h): LatentOptimizer.optimize_clip_lm(clip=ClipLM(...)).  Every other call solves
a frame on its own; this one is asked for by name."""
import math
from dataclasses import dataclass
from typing import Optional

from . import _lib


@dataclass
class ClipLM:
    """`steps` trials per sequence (1..64), each one Gauss-Newton step on the whole sequence damped by mu: accepted when the sequence's loss
    falls (mu <- max(mu mu_down, mu_min)), rejected otherwise (mu <- min(mu mu_up, mu_max)).  `smooth`: lambda_smooth, the weight of
    |z_t - z_(t-1)|^2 / 24 in the loss (0 decouples the frames; the decision stays per sequence).  `accel`: lambda_accel, the weight of
    |z_(t+1) - 2 z_t + z_(t-1)|^2 / 24; None: dp_optimize_clip_lm, any number (0.0 included): dp_optimize_clip_lm_accel.  There is no early stop."""
    steps: int = 4
    smooth: float = 1.0
    mu0: float = 1e-2
    mu_up: float = 4.0
    mu_down: float = 1.0 / 3.0
    mu_min: float = 1e-6
    mu_max: float = 1e6
    accel: Optional[float] = None

    def check(self):
        """raises ValueError for what dp_optimize_clip_lm (with `accel`: dp_optimize_clip_lm_accel) would refuse of its parameters"""
        if not isinstance(self.steps, int) or not 1 <= self.steps <= _lib.DP_LM_MAX_STEPS:
            raise ValueError(f"ClipLM: steps {self.steps!r} outside 1..{_lib.DP_LM_MAX_STEPS}")
        for name in ("mu0", "mu_up", "mu_down", "mu_min", "mu_max"):
            if not math.isfinite(float(getattr(self, name))):
                raise ValueError(f"ClipLM: {name} is not finite")
        if not 0.0 < self.mu_down < 1.0:
            raise ValueError("ClipLM: mu_down must lie in (0, 1)")
        if not self.mu_up > 1.0:
            raise ValueError("ClipLM: mu_up must be greater than 1")
        if not 0.0 < self.mu_min <= self.mu_max:
            raise ValueError("ClipLM: need 0 < mu_min <= mu_max")
        if not self.mu_min <= self.mu0 <= self.mu_max:
            raise ValueError("ClipLM: mu0 outside [mu_min, mu_max]")
        if not (math.isfinite(float(self.smooth)) and self.smooth >= 0.0):
            raise ValueError("ClipLM: smooth is negative or not finite")
        if self.accel is not None and not (math.isfinite(float(self.accel)) and self.accel >= 0.0):
            raise ValueError("ClipLM: accel is negative or not finite")
        return self

    def to_struct(self, lambda_rot, lambda_tmp):
        return _lib.DpClipLmParams(n_steps=int(self.steps), lambda_rot=float(lambda_rot), lambda_tmp=float(lambda_tmp), lambda_smooth=float(self.smooth),
                                   mu0=self.mu0, mu_up=self.mu_up, mu_down=self.mu_down, mu_min=self.mu_min, mu_max=self.mu_max)

    def accel_struct(self):
        """dp_clip_accel_params of the settings (`accel` is a number)"""
        return _lib.DpClipAccelParams(lambda_accel=float(self.accel))

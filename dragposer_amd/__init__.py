from .autograd import decode_fk  # noqa: F401  (differentiable decode + FK: include/dragposer_grad.h)
from .constraints import Constraints  # noqa: F401  (the reference's extra loss terms: include/dragposer_constraints.h)
from .terms import Term, Terms  # noqa: F401  (user-defined constraint terms: include/dragposer_terms.h)
from .points import Point, Points  # noqa: F401  (terms on weighted joint combinations: include/dragposer_points.h)
from .holds import Hold, Holds  # noqa: F401  (joints held where they touched down: include/dragposer_holds.h)
from .gaps import Gaps  # noqa: F401  (trackers that drop out and come back: include/dragposer_gaps.h)
from .tethers import Tether, Tethers  # noqa: F401  (joints tied to their own recent path: include/dragposer_tethers.h)
from .lm import LM  # noqa: F401  (a Levenberg-Marquardt solver for the per-frame problem: include/dragposer_lm.h)
from .clip import ClipLM  # noqa: F401  (a clip solved jointly, latents tied frame to frame: include/dragposer_clip_lm.h)
from .encoder import NativePoseEncoder  # noqa: F401  (the pose encoder in one HIP launch: include/dragposer_encoder.h)
from .calibration import BoneGroups, Calibration, calibrate  # noqa: F401  (bone lengths from tracker data: include/dragposer_calibration.h)


def __getattr__(name):
    """LatentAR (a training-free predictor for the pull term: include/dragposer_latent_ar.h), imported on first use so that
    `python -m dragposer_amd.ar` runs the module once"""
    if name == "LatentAR":
        from .ar import LatentAR

        return LatentAR
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

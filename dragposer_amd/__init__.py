from .autograd import decode_fk  # noqa: F401  (differentiable decode + FK: include/dragposer_grad.h)
from .constraints import Constraints  # noqa: F401  (the reference's extra loss terms: include/dragposer_constraints.h)
from .terms import Term, Terms  # noqa: F401  (user-defined constraint terms: include/dragposer_terms.h)
from .encoder import NativePoseEncoder  # noqa: F401  (the pose encoder in one HIP launch: include/dragposer_encoder.h)

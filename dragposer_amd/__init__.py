from .autograd import decode_fk  # noqa: F401  (differentiable decode + FK: include/dragposer_grad.h)
from .constraints import Constraints  # noqa: F401  (the reference's extra loss terms: include/dragposer_constraints.h)

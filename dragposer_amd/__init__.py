from .autograd import decode_fk  # noqa: F401  (differentiable decode + FK: include/dragposer_grad.h)
from .constraints import Constraints  # noqa: F401  (the reference's extra loss terms: include/dragposer_constraints.h)
from .terms import Term, Terms  # noqa: F401  (user-defined constraint terms: include/dragposer_terms.h)

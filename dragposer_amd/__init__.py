from .autograd import decode_fk  # noqa: F401  (differentiable decode + FK: include/dragposer_grad.h)

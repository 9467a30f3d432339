"""ORACLE (test infrastructure): the term table with points (include/dragposer_points.h) restated on tests/terms_oracle.py -- the
points' positions P_(22+k) = sum_j m_k[j] P_j are appended to the joints' as rows 22.. of the position array, and terms_oracle's own
term_values / optimize_terms, which index positions by joint_a / joint_b, run on that.  Nothing of the terms is restated here: the
gradient through a point is torch autograd's through the sum.  Any dtype (the tests use fp64 and, for the twin, fp32)."""
import torch

import terms_oracle as TO


def coeff_matrix(points, dt, dev="cpu"):
    """[n_points, 22] of a dragposer_amd.Points (None: no row)"""
    rows = [list(p.coeffs) for p in points.points] if points is not None else []
    return torch.tensor(rows, dtype=dt, device=dev).reshape(len(rows), 22)


def extend(points, pos, rot):
    """pos [B,22,3] -> [B,22+n,3] with the points' positions behind the joints'; rot padded with identities (no term reads them: an
    ALIGN term cannot name a point)"""
    M = coeff_matrix(points, pos.dtype, pos.device)
    if M.shape[0] == 0:
        return pos, rot
    eye = torch.eye(3, dtype=rot.dtype, device=rot.device).expand(rot.shape[0], M.shape[0], 3, 3)
    return torch.cat((pos, torch.einsum("kj,bjc->bkc", M, pos)), 1), torch.cat((rot, eye), 1)


def term_values(terms, pos, rot, gp):
    """terms_oracle.term_values of a table whose terms may name points (terms.points)"""
    return TO.term_values(terms, *extend(getattr(terms, "points", None), pos, rot), gp)


def optimize_terms(model, batch, terms, global_pos, n_iter, **kw):
    """terms_oracle.optimize_terms with its term_values (looked up by that loop at call time) replaced by the one above for the call"""
    inner = TO.term_values
    TO.term_values = lambda t, pos, rot, gp: inner(t, *extend(getattr(t, "points", None), pos, rot), gp)
    try:
        return TO.optimize_terms(model, batch, terms, global_pos, n_iter, **kw)
    finally:
        TO.term_values = inner


def joints_reached(terms, i, pos, rot, gp):
    """[B] the number of joints with a non-zero dL/dP_j of term i alone, at these positions (autograd)"""
    p = pos.clone().requires_grad_()
    vals, _ = term_values(terms, p, rot, gp)
    (g,) = torch.autograd.grad(vals[:, i].sum(), p)
    return (g.abs().sum(-1) > 0).sum(1)

"""CPU: the fp64 restatement of the term table (tests/terms_oracle.py) against the restatement of the four reference terms
(tests/constraints_oracle.py) on Terms.from_constraints, and each term type's analytic gradient (what the kernel accumulates) against
torch autograd."""
import numpy as np
import pytest
import torch

import constraints_oracle as CO
import terms_oracle as TO
from oracle import ref_torch as R
from test_hip_constraints import TERMS, _inputs  # (the GPU file's cases; its tests are not collected from here)


@pytest.mark.parametrize("name", list(TERMS))
def test_from_constraints_reproduces_the_four_term_oracle(name):
    from dragposer_amd import Constraints, Terms

    model = R.OracleModel(dtype=torch.float64)
    b, gp = _inputs(model, 48, seed=3 + len(name))
    c = Constraints(**TERMS[name])
    t = Terms.from_constraints(c)
    for kw in (dict(n_iter=8), dict(n_iter=12, stop_eps_pos=1e-4, stop_eps_rot=1e-2, min_loss_incr=1e-5)):
        ref = CO.optimize_constrained(model, b, c, gp, lam_tmp=0.02, **kw)
        got = TO.optimize_terms(model, b, t, gp, lam_tmp=0.02, **kw)
        np.testing.assert_array_equal(got["iters"], ref["iters"])
        for k in ("pos", "rot", "z_final", "z_pre", "loss"):
            np.testing.assert_allclose(got[k], ref[k], rtol=1e-9, atol=1e-12, err_msg=k)
        np.testing.assert_allclose(got["loss_terms"].sum(1), ref["loss_extra"].sum(1), rtol=1e-9, atol=1e-14)
        assert got["loss_terms"].shape[1] == len(t)


def _rot(B, g):
    q = torch.randn(B, 22, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(B, 22, 3, 3)


def gradient_cases(B, g):
    """one table per type and flag, with per-frame rows (some frames at s = 0) and same-joint terms"""
    from dragposer_amd import Term, Terms

    row = lambda vec, scale=1.0: torch.cat([torch.as_tensor(vec, dtype=torch.float64).expand(B, 3) + 0.05 * torch.randn(B, 3, generator=g,
                                                                                                                      dtype=torch.float64),
                                           (scale * torch.rand(B, 1, generator=g, dtype=torch.float64)) * (torch.arange(B) % 3 != 0).unsqueeze(1)], 1)
    s = 0.5 ** 0.5
    return {
        "plane": Terms([Term.plane(4, (0, 1, 0), (0, 0.1, 0), weight=2.0)]),
        "plane_one_sided_tilted": Terms([Term.plane(8, (s, s, 0), (0.1, 0.0, 0.0), weight=1.5, one_sided=True, per_frame=row((0.0, 0.2, 0.0)))]),
        "band": Terms([Term.distance(3, 7, lo=0.3, hi=0.5, weight=3.0), Term.distance(13, 0, lo=0.1, hi=0.2, drop_up=True)], up_axis=2),
        "point_distance": Terms([Term.distance(21, point=(0.3, 1.2, 0.1), lo=0.05, hi=0.1, weight=2.0, per_frame=row((0.3, 1.2, 0.1), 2.0))]),
        "world_align": Terms([Term.align(13, (0, 0, 1), dir=(1, 0, 0), threshold=0.1, margin=0.1, weight=1.2, drop_up=True,
                                         per_frame=row((0.0, 0.0, 1.0)))]),
        "joint_align": Terms([Term.align(17, (1, 0, 0), 21, (0, 1, 0), margin=-0.2, weight=0.7)]),
        "same_joint": Terms([Term.distance(5, 5, hi=0.0), Term.align(9, (1, 0, 0), 9, (0, 1, 0), margin=0.3, weight=2.0),
                             Term.align(9, (0, 0, 1), 9, (0, 0, 1), drop_up=True)]),
    }


@pytest.mark.parametrize("case", ["plane", "plane_one_sided_tilted", "band", "point_distance", "world_align", "joint_align", "same_joint"])
def test_analytic_gradient_matches_autograd(case):
    B = 64
    g = torch.Generator().manual_seed(len(case))
    terms = gradient_cases(B, g)[case]
    pos = (0.4 * torch.randn(B, 22, 3, generator=g, dtype=torch.float64)).requires_grad_()
    rot = _rot(B, g).requires_grad_()
    gp = torch.randn(B, 3, generator=g, dtype=torch.float64) * 0.2
    vals, _ = TO.term_values(terms, pos, rot, gp)
    assert vals.abs().sum() > 0.0, case
    gP, gG = torch.autograd.grad(vals.sum(), (pos, rot), allow_unused=True)
    aP, aG = TO.term_grads(terms, pos.detach(), rot.detach(), gp)
    np.testing.assert_allclose(aP.numpy(), (gP if gP is not None else torch.zeros_like(pos)).numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(aG.numpy(), (gG if gG is not None else torch.zeros_like(rot)).numpy(), rtol=1e-10, atol=1e-12)

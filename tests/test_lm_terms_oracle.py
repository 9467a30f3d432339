"""CPU: the oracle of dp_optimize_lm_terms (tests/lm_terms_oracle.py) held to autograd, and the conditions tests/test_hip_lm_terms.py's inputs
are chosen for: J^T r is half of the gradient of L; few frames sit on a margin or a switch; the fp32 and fp64 oracles accept alike; every
table has its terms active on a quarter of the frames; the terms' rows move the step; the square-root row beats zero curvature."""
import functools

import numpy as np
import pytest
import torch

import lm_oracle as LO
import lm_terms_oracle as LT
import terms_oracle as TO
from oracle import ref_torch as R

B = 41
MARGIN, SWITCH = 1e-3, 1e-4
TABLES = ("plane_one_sided", "plane_tilted_rows", "band", "point_distance_rows", "world_align_rows", "same_joint", "custom", "pins", "mixed16")


@functools.lru_cache(maxsize=None)
def _models():
    return R.OracleModel(dtype=torch.float64), R.OracleModel(dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _inputs(warm):
    m64 = _models()[0]
    return (LO.warm_inputs(m64, B, seed=11) if warm else R.synth_inputs(m64, B, seed=11)), LT.global_pos(B)


def _mus(n):  # tests/test_hip_lm.py's
    return np.asarray([1e-4, 1e-2, 1.0], np.float32)[np.random.default_rng(5).integers(0, 3, n)]


@functools.lru_cache(maxsize=None)
def _pair(table, warm):
    """one step of both oracles and of the fp64 one without the terms' rows"""
    m64, m32 = _models()
    b, gp = _inputs(warm)
    terms = LT.tables(B, "cpu")[table]
    mu = _mus(B)
    return (LT.lm_terms(m64, b, terms, gp, 1, mu=mu.astype(np.float64)), LT.lm_terms(m32, b, terms, gp, 1, mu=mu),
            LT.lm_terms(m64, b, terms, gp, 1, mu=mu.astype(np.float64), drop_rows=True))


@pytest.mark.parametrize("warm", [True, False])
@pytest.mark.parametrize("table", TABLES)
def test_jtr_is_half_of_autograds_gradient(table, warm):
    m64 = _models()[0]
    b, gp = _inputs(warm)
    terms = LT.tables(B, "cpu")[table]
    t = LO._conv(m64, b)
    gpt = torch.as_tensor(gp).double()
    z = t["z0"].clone().requires_grad_()
    motion, disp = R.decoder_forward(m64, z)
    lp, lr, lt, fk = R.frame_losses(m64, z, motion, disp, t["cur_rot"], t["z_tgt"], t["tgt_pos"], t["tgt_rot"], t["w"], t["tracked"], 1.0, 0.02)
    ex, sw = TO.term_values(terms, fk["pos"], fk["rot"], gpt)
    (grad,) = torch.autograd.grad((lp + lr + lt + ex.sum(1)).sum(), z)
    _, g, _ = LT.normal_equations(m64, terms, t["z0"], t, gpt, LT._all_rows(terms, B, torch.float64), 1.0, 0.02)
    ok = (sw > 1e-6).numpy()
    assert ok.sum() >= 0.9 * B
    # (lo^2 and hi^2 are float32 products in the rows and doubles in term_values: the same active set away from a switch, the same gradient)
    np.testing.assert_allclose(g.numpy()[ok], 0.5 * grad.numpy()[ok], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("warm", [True, False])
@pytest.mark.parametrize("table", TABLES)
def test_the_gpu_tests_inputs_are_decided_clearly(table, warm):
    ref, r32, bare = _pair(table, warm)
    keep = (ref["margin"][:, 0] >= MARGIN) & (ref["switch"][:, 0] >= SWITCH)
    active = (ref["kinds0"] != 0).any(1)
    print(f"{table} {'warm' if warm else 'cold'}: kept {int(keep.sum())}/{B}, active {int(active.sum())}/{B}, accepted {int(ref['accepted'].sum())}")
    assert (~keep).sum() <= 0.1 * B
    np.testing.assert_array_equal(ref["accepted"][keep], r32["accepted"][keep])
    assert active.sum() >= 0.25 * B
    # power: without the terms' rows the trial latent of an active frame lies elsewhere, by far more than the GPU test's bar
    both = active & keep & ref["accepted"][:, 0] & bare["accepted"][:, 0]
    bar = max(4.0 * np.abs(r32["z"] - ref["z"])[keep].max(), 1e-6)
    moved = np.abs(bare["z"] - ref["z"]).max(1)
    print(f"  power: {int(both.sum())} frames accepted both ways, moved by {moved[both].min() if both.any() else float('nan'):.3e} .. "
          f"{moved[both].max() if both.any() else float('nan'):.3e}, bar {bar:.3e}")
    assert both.any() and moved[both].min() > 10.0 * bar


@pytest.mark.parametrize("table", ["band", "custom"])
def test_the_square_root_row_beats_zero_curvature(table):
    m64 = _models()[0]
    share = {}
    for warm in (True, False):
        b, gp = _inputs(warm)
        terms = LT.tables(B, "cpu")[table]
        for rows in ("sqrt", "zero"):
            share[warm, rows] = LT.lm_terms(m64, b, terms, gp, 1, lo_rows=rows)["accepted"][:, 0].mean()
    print(f"{table}: first step accepted, warm / cold: square-root row {share[True, 'sqrt']:.0%} / {share[False, 'sqrt']:.0%}, "
          f"zero curvature {share[True, 'zero']:.0%} / {share[False, 'zero']:.0%}")
    assert share[True, "sqrt"] > share[True, "zero"] and share[False, "sqrt"] > share[False, "zero"]

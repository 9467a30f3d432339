"""CPU: the conditions the GPU inputs of tests/test_hip_fit_bones.py were chosen for, on the oracle alone (tests/fit_bones_oracle.py), so that
a GPU failure cannot be blamed on them: exact recovery at the source latents, the conditioning of `limbs` with six trackers, the leg group
that three trackers leave without a row, and the alternation's six rounds for one group."""
import functools

import numpy as np
import torch

import fit_bones_oracle as FO
from oracle import ref_torch as R


@functools.lru_cache(maxsize=None)
def _models():
    return R.OracleModel(dtype=torch.float64), R.OracleModel(dtype=torch.float32)


def _scaled_batch(model, groups, factors, B=64, trackers=6, seed=3):
    """recipe S with the targets made on the skeleton base * factors[group]"""
    return R.synth_inputs(FO.scaled_model(model, groups, factors), B, trackers=trackers, seed=seed)


def test_the_fit_at_the_source_latents_returns_the_true_scales():
    m64 = _models()[0]
    for groups, K, true in ((FO.UNIFORM, 1, [1.12]), (FO.LIMBS, 3, [1.15, 0.92, 1.08])):
        b = _scaled_batch(m64, groups, true)
        f = FO.fit(m64, b, groups, K, ridge=0.0, z=b["z_src"])
        err = np.abs(f["scales"] - np.asarray(true)).max()
        print(f"K={K}: scales {f['scales']}, max error {err:.2e}, rms {f['rms']}")
        assert f["flags"] == 0 and f["frames"] == 64
        assert err < 1e-6  # (the targets are stored in fp32: 6e-8 relative)
        assert f["rms"][1] < 1e-6 < f["rms"][0]


def test_limbs_with_six_trackers_is_well_conditioned():
    m64 = _models()[0]
    b = _scaled_batch(m64, FO.LIMBS, [1.15, 0.92, 1.08])
    M = FO.fit(m64, b, FO.LIMBS, 3, ridge=0.0, z=b["z_src"])["normal"]
    cond = np.linalg.cond(M[:3, :3])
    print(f"limbs, 6 trackers: condition number {cond:.2f}")
    assert cond < 10.0


def test_three_trackers_leave_the_legs_without_a_row():
    m64 = _models()[0]
    b = _scaled_batch(m64, FO.LIMBS, [1.15, 0.92, 1.08], trackers=3)
    f0 = FO.fit(m64, b, FO.LIMBS, 3, ridge=0.0, z=b["z_src"])
    assert (f0["normal"][0, :] == 0).all() and (f0["normal"][:, 0] == 0).all()  # no tracker sits on or below a leg bone
    assert f0["flags"] == FO.SINGULAR and (f0["scales"] == 1.0).all()
    prior = np.array([1.05, 0.97, 1.1], np.float32)
    f1 = FO.fit(m64, b, FO.LIMBS, 3, ridge=1e-3, prior=prior, z=b["z_src"])
    print(f"limbs, 3 trackers, ridge 1e-3: scales {f1['scales']}")
    assert f1["flags"] == 0 and abs(f1["scales"][0] - float(prior[0])) < 1e-12
    assert np.abs(f1["scales"][1:] - [0.92, 1.08]).max() < 0.01  # (the ridge pulls the two observed groups by about 1e-3 x their distance)
    # the symmetric groups with the recipe's ankle trackers: nothing below the ankles, the toe group (3) has no row
    fs = FO.fit(m64, _scaled_batch(m64, FO.SYMMETRIC, [1.0] * 13), FO.SYMMETRIC, 13, ridge=0.0)
    assert (fs["normal"][3, :] == 0).all() and fs["flags"] == FO.SINGULAR


def test_six_rounds_for_one_group_come_within_half_a_percent():
    m32 = _models()[1]
    b = _scaled_batch(m32, FO.UNIFORM, [1.12])
    trace, rms = FO.calibrate(m32, b, FO.UNIFORM, 1, rounds=6, n_iter=50, ridge=1e-3)
    print("one group, true 1.12, 6 trackers:", np.round(trace[:, 0], 4), "rms", rms[:, 1])
    assert abs(trace[-1, 0] - 1.12) < 0.005
    assert (np.diff(np.abs(trace[:, 0] - 1.12)) < 0).all()  # every round comes closer
    assert (rms[:, 1] <= rms[:, 0]).all()

"""CPU: what the GPU tests of Adam's knobs and of the loop versions rest on (tests/adam_reference.py, tests/test_hip_adam.py,
tests/test_hip_w4_loop_versions.py) -- the reference itself, the bars, and the conditions those tests need to mean anything:

* the fp64 recursion is torch.optim.Adam on the smooth loss, and its fp32 twin stays near it: the bar of every case, printed (`-s`);
* every kept case tells each knob it sets from that knob's default by at least 100 bars, and every case left out does not;
* the short real-path cases: the C oracle's own f32 / f64 pair leaves out no frame, and under the while-condition both stop the same frames,
  at least four of them inside the five iterations;
* the loop-version batches: every wave takes the version written beside its batch, and the f32 oracle's first gradient is within
  test_hip_parity.py's bar of the f64 oracle's on the frames the debug-route test compares;
* Adam parameters the library refuses are refused by the return code before anything is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_reference as A  # tests/adam_reference.py
from dragposer_amd import _lib
from oracle import ref_torch as R
from oracle.analytic import AnalyticOracle


@pytest.mark.parametrize("name", ["fast", "slow_corrections", "beta1_0", "beta2_0"])
def test_the_recursion_is_torch_adam_on_the_smooth_loss(name):
    k, lam, n = A.SETS[name], 0.15, 40
    z0 = torch.tensor(A.start_latents(), dtype=torch.float64)
    zt = torch.tensor(A.smooth_targets(A.start_latents(), n, k["lr"], k["b1"], seed=3), dtype=torch.float64)
    z = z0.clone().requires_grad_()
    opt = torch.optim.Adam([z], lr=k["lr"], betas=(k["b1"], k["b2"]), eps=k["eps"])
    for _ in range(n):
        opt.zero_grad()
        (lam * ((z - zt) ** 2).mean(dim=1)).sum().backward()
        opt.step()
    want = A.recursion(z0.numpy(), zt.numpy(), n, lam=lam, **k)
    np.testing.assert_allclose(z.detach().numpy(), want, rtol=0, atol=1e-12)
    twin = A.recursion_f32(z0.numpy(), zt.numpy(), n, lam=lam, **k)
    assert twin.dtype == np.float32 and np.abs(twin - want).max() < 2e-6


def _all_cases():
    return [(name, lam, n) for name in A.SETS for lam in A.LAMS for n in A.STEPS]


def test_bars_and_the_condition_that_a_case_tells_its_knobs():
    """prints the table DESIGN.md quotes; the bar is 4 x the twin's distance and at least 2e-6"""
    print(f"\n{'set':18s} {'lam':>5s} {'N':>4s} {'twin':>9s} {'bar':>9s}  margins (bars) with one knob at its default")
    for name, lam, n in _all_cases():
        c = A.case(name, lam, n)
        kept = n in A.KEPT_STEPS[name]
        twin = float(np.abs(c["twin"] - c["want"]).max())
        print(f"{name:18s} {lam:5.2f} {n:4d} {twin:9.2e} {c['bar']:9.2e}  " + " ".join(f"{x}:{m:.3g}" for x, m in c["margins"].items()) + ("" if kept else "   (left out)"))
        assert c["bar"] == max(A.BAR_FACTOR * twin, A.BAR_FLOOR) and c["bar"] <= 5e-5, (name, lam, n, c["bar"])
        assert set(c["margins"]) == {x for x in A.KNOBS if A.SETS[name][x] != A.DEFAULT[x]}
        if kept:
            assert all(m >= A.MARGIN for m in c["margins"].values()), (name, lam, n, c["margins"])
    for name in A.SETS:  # a case is left out only because it fails the condition at one of the two lam
        for n in set(A.STEPS) - set(A.KEPT_STEPS[name]):
            assert any(m < A.MARGIN for lam in A.LAMS for m in A.case(name, lam, n)["margins"].values()), (name, n)
    assert all(set(A.KEPT_STEPS[name]) <= set(A.STEPS) for name in A.SETS)
    # every knob is told from its default beyond the argument table by some kept case, and beta1 by one whose beta1^256 is far from 0
    for knob in A.KNOBS:
        assert any(A.SETS[name][knob] != A.DEFAULT[knob] and 257 in A.KEPT_STEPS[name] for name in A.SETS), knob
    assert A.SETS["slow_beta1"]["b1"] ** 256 > 0.25 and A.SETS["slow_beta1"]["b2"] ** 256 > 0.75 and 257 in A.KEPT_STEPS["slow_beta1"]


def test_sequence_cases_tell_their_knobs():
    print()
    for name, n in A.SEQUENCE_CASES:
        c = A.case(name, A.SEQUENCE_LAM, n, A.SEQUENCE_STEPS)
        print(f"sequence {name:10s} N {n:3d} x {A.SEQUENCE_STEPS}: bar {c['bar']:.2e}  " + " ".join(f"{x}:{m:.3g}" for x, m in c["margins"].items()))
        assert c["want"].shape == (A.SEQUENCE_STEPS, A.N_FRAMES, 24) and c["bar"] <= 1e-4
        assert all(m >= A.MARGIN for m in c["margins"].values()), (name, n, c["margins"])
    assert any(n > 256 for _, n in A.SEQUENCE_CASES)


def test_targets_stay_out_of_reach():
    """no component comes nearer to its target than a third of the way it started from it: the gradient never changes sign"""
    for name, lam, n in _all_cases():
        c = A.case(name, lam, n)
        d0, d1 = c["z_tgt"] - c["z0"].astype(np.float64), c["z_tgt"] - c["want"]
        assert (np.sign(d0) == np.sign(d1)).all() and (np.abs(d1) >= np.abs(d0) / 3).all(), (name, lam, n)


# ---------------------------------------------------------------- the short real path of tests/test_hip_adam.py
@pytest.mark.parametrize("name", ["fast", "eps"])
@pytest.mark.parametrize("trackers", ["six", "three"])
def test_real_path_cases_are_ones_the_oracle_pair_agrees_on(trackers, name):
    import test_hip_adam as T  # tests/test_hip_adam.py (its GPU tests are not collected from here)

    for early in (False, True):
        b, r32, r64 = T.real_reference(trackers, name, early)
        pair = np.linalg.norm(r32["pos"] - r64["pos"], axis=-1).max(axis=1) * 1000.0
        print(f"{trackers} {name} early={early}: the oracle's f32 / f64 pair max {pair.max():.5f} mm, iterations {r32['iters'].tolist()}")
        assert pair.max() <= 0.02  # the seed leaves out no frame
        assert np.array_equal(r32["iters"], r64["iters"])
        if early:
            assert (r32["iters"] < T.REAL_ITERS).sum() >= 4 and r32["iters"].max() == T.REAL_ITERS
        else:
            assert (r32["iters"] == T.REAL_ITERS).all()
    # the knobs matter on this path: with the default set every frame ends more than ten times the latent's bar away
    b, r32, _ = T.real_reference(trackers, name, False)
    dflt = AnalyticOracle(precision="f32").optimize(*[b[x] for x in T.KEYS], T.REAL_ITERS, lam_tmp=T.TRACKER_LAM[trackers])
    assert np.abs(dflt["z_final"] - r32["z_final"]).max(axis=1).min() > 10 * 5e-5 * A.SETS[name]["lr"] / 1e-2


@pytest.mark.parametrize("name", ["fast", "eps"])
@pytest.mark.parametrize("unit", ["constrained", "terms"])
def test_constraint_cases_have_the_extra_term_in_the_gradient(unit, name):
    import test_hip_adam as T

    b, extra, ref, plain = T.constraint_reference(unit, name)
    assert (ref["iters"] == T.REAL_ITERS).all() and np.abs(plain["z_final"] - ref["z_final"]).max() > 1e-3
    key = "loss_extra" if unit == "constrained" else "loss_terms"
    assert np.abs(ref[key]).sum() > 0


# ---------------------------------------------------------------- the batches of tests/test_hip_w4_loop_versions.py
def test_loop_version_batches_take_the_versions_written_beside_them():
    import test_hip_w4_loop_versions as L

    parents = np.load(R.DEFAULT_MODEL)["parents"]
    items = np.zeros((2, 16), np.int32)
    groups = np.zeros((2, 15), np.int32)
    assert _lib.load().dp_debug_w4_bp_layout(items.ctypes.data_as(C.c_void_p), groups.ctypes.data_as(C.c_void_p)) == 0
    assert items[0, :9].tolist() == list(range(9))  # side-A item b of quads 0..8 is joint b: what the skip patterns' bits name
    for j in range(1, 9):  # ... and joints 1..8 are the two legs, the toes (4, 8) their ends
        assert int(parents[j]) == (0 if j in (1, 5) else j - 1)
    assert not any(int(parents[j]) in (4, 8) for j in range(22))
    for name, (recipes, versions) in L.BATCHES.items():
        b = L.mixed_batch(name)
        assert len(recipes) <= 20 and len(b["z0"]) == len(recipes)
        assert [int(x) for x in b["tracked"].sum(axis=1)] == [len(r) for r in recipes]
        assert L.expected_versions(b["tracked"], parents) == versions, (name, L.expected_versions(b["tracked"], parents))
    assert set(L.BATCHES["mixed_workgroup"][1]) == {0, 1, 2, "general"} and len(L.BATCHES["mixed_workgroup"][0]) % 4 == 2
    six = L.mixed_batch("six_elsewhere")
    assert (six["tracked"].sum(axis=1) == 6).all() and not six["tracked"][:, 1:9].any()


@pytest.mark.parametrize("rounding", ["none", "bf16"])
@pytest.mark.parametrize("name", ["mixed_workgroup", "unlike_frames_in_a_wave"])
def test_loop_version_batches_have_a_first_gradient_both_oracles_agree_on(name, rounding):
    import test_hip_w4_loop_versions as L

    b = L.mixed_batch(name)
    has = b["tracked"].sum(axis=1) > 0
    g32, g64 = (AnalyticOracle(precision=p, weight_rounding=rounding).grad(*[b[k][has] for k in L.KEYS], 1.0, L.MIXED_LAM)[1] for p in ("f32", "f64"))
    print(f"{name} ({rounding}), seed {L.MIXED_SEED}: f32 against f64 gradient, max |difference| {np.abs(g32 - g64).max():.2e}")
    np.testing.assert_allclose(g32, g64, atol=2e-6, rtol=2e-5)


# ---------------------------------------------------------------- refusals
def test_bad_adam_parameters_are_refused_before_anything_is_launched():
    """eps = 0, beta1 = 1, beta2 < 0 and lr = 0 through dp_optimize, dp_optimize_constrained and dp_optimize_terms: DP_ERR_INVALID, on a context
    with no device behind it -- where the same call with good parameters gets as far as the launch and is refused there (DP_ERR_DEVICE)"""
    lib = _lib.load()
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    b = _lib.DpBatch(n_frames=1, z0=p, z_tgt=p, cur_rot=p, tgt_pos=p, tgt_rot=p, w=p, tracked=p)
    r = _lib.DpResult()
    r.z = p
    cons, terms = _lib.DpConstraints(), _lib.DpTerms(n_terms=0, terms=None)
    ctx = C.c_void_p()
    assert lib.dp_debug_host_ctx(C.byref(ctx)) == _lib.DP_OK and ctx.value
    try:
        calls = {"dp_optimize": lambda prm: lib.dp_optimize(ctx, C.byref(b), C.byref(prm), C.byref(r), None),
                 "dp_optimize_constrained": lambda prm: lib.dp_optimize_constrained(ctx, C.byref(b), C.byref(prm), C.byref(cons), C.byref(r), None),
                 "dp_optimize_terms": lambda prm: lib.dp_optimize_terms(ctx, C.byref(b), C.byref(prm), C.byref(terms), C.byref(r), None)}
        good = dict(n_iter=10, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, lambda_rot=1.0)
        for who, call in calls.items():
            assert call(_lib.DpParams(**good)) == _lib.DP_ERR_DEVICE, who
            for edge in (dict(beta1=0.0), dict(beta2=0.0)):  # (accepted: tests/test_hip_adam.py runs them)
                assert call(_lib.DpParams(**{**good, **edge})) == _lib.DP_ERR_DEVICE, (who, edge)
            for bad, word in ((dict(eps=0.0), "eps"), (dict(beta1=1.0), "Adam"), (dict(beta2=-0.1), "Adam"), (dict(lr=0.0), "Adam"),
                              (dict(beta2=1.0), "Adam"), (dict(eps=float("nan")), "eps")):
                assert call(_lib.DpParams(**{**good, **bad})) == _lib.DP_ERR_INVALID, (who, bad)
                assert word in lib.dp_last_error(ctx).decode(), (who, bad, lib.dp_last_error(ctx))
    finally:
        lib.dp_destroy(ctx)

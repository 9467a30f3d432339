"""GPU (MI355X): dp_optimize_lm (include/dragposer_lm.h) on the paths tests/test_hip_lm.py does not reach, with that file's bars (its
_forward_bars, MARGIN and one-step bar: z within max(4 x the fp32 oracle's own deviation from the fp64 one, 1e-6)):
  1. every joint's rows of J (tests/lm_oracle.py, every_joint_inputs: each joint tracked alone, all 22, odd counts up to 21) on the shipped
     tree and on tests/test_hip_topology.py's two, one step against the fp64 oracle of that tree;
  2. k launches of one step against one launch of k steps, bit for bit: "keep A and g, repeat the solve" against "recompute everything";
  3. rejections that are certain (every pivot 0; L' == L), the clamps at mu_min and mu_max, hit_max, other factors;
  4. the mu array's contract: invalid entries read as mu0, the two bounds used as given, refused frames leave theirs alone;
  5. subsets of the outputs, and one step through a bf16 context against the bf16-rounded oracle.
The conditions the inputs were chosen for (margins, certain rejections) are checked on the CPU in tests/test_lm_oracle.py."""
import functools
import itertools

import numpy as np
import pytest
import torch

import lm_oracle as LO
from oracle import ref_torch as R
from test_hip_lm import MARGIN, _forward_bars, _inputs, _lm, _models, _mus, _run  # (helpers and bars; its tests are not collected from here)
from test_hip_topology import TREES, _model_arrays

pytestmark = pytest.mark.gpu
RESULTS = ("z", "pose", "pos", "rot", "world_rot", "world_disp", "disp", "loss")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def opts(dev):
    from dragposer_amd.optimizer import LatentOptimizer

    return {"fp32": LatentOptimizer(device=dev), "bf16": LatentOptimizer(device=dev, weight_dtype="bf16")}


@pytest.fixture(scope="module")
def trees(dev, opts, tmp_path_factory):
    """name -> (optimizer, fp64 oracle model, fp32 oracle model): the shipped tree and test_hip_topology.py's two"""
    from dragposer_amd.optimizer import LatentOptimizer

    out = {"xsens": (opts["fp32"],) + _models()}
    for name, parents in TREES.items():
        raw = _model_arrays(parents, seed=len(name))
        out[name] = (LatentOptimizer(device=dev, arrays=raw),) + LO.tree_models(raw, str(tmp_path_factory.mktemp(name) / "model.npz"))
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(a, b, what):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=str(what))


def _one_step(opt, dev, b, mu, m64, m32, label, every_frame=False, **factors):
    """tests/test_hip_lm.py's test_one_step_against_the_fp64_oracle on (b, mu) with the oracle pair (m64, m32); a failure names the frames"""
    ref = LO.lm(m64, b, 1, mu=mu.astype(np.float64), **factors)
    r32 = LO.lm(m32, b, 1, mu=mu, **factors)
    got = _run(opt, b, dev, mu=mu, lm=_lm(1, early_stop=False, **factors))
    B = len(mu)
    pair = np.abs(r32["z"] - ref["z"]).max()
    bar = max(4.0 * pair, 1e-6)
    dz = np.abs(got["z"] - ref["z"]).max(1)
    sure = ref["margin"][:, 0] >= MARGIN
    same = got["n_accepted"] == ref["n_accepted"]
    print(f"{label} B={B}: kernel max |dz| {dz[same].max():.3e}, fp32 oracle {pair:.3e}, bar {bar:.3e}, smallest oracle margin "
          f"{np.nanmin(ref['margin']):.3e}, accepted {int(ref['accepted'].sum())}/{B} (kernel {int(got['n_accepted'].sum())}), "
          f"rejected frames {np.nonzero(~ref['accepted'][:, 0])[0].tolist()}")
    if every_frame:
        assert sure.all(), np.nonzero(~sure)[0]
    wrong = np.nonzero((sure & ~same) | (same & (dz > bar)))[0]
    assert wrong.size == 0, f"{label}: frames {wrong.tolist()}: |dz| {dz[wrong]}, bar {bar:.3e}, accepted {got['n_accepted'][wrong]} (oracle {ref['n_accepted'][wrong]})"
    assert (got["status"] == 0).all() and (got["iters"] == 1).all()
    np.testing.assert_array_equal(got["z"], got["z_pre"])
    np.testing.assert_allclose(got["mu"], ref["mu"], rtol=1e-6)
    _forward_bars(got, b, got["z"], None, model=m64)
    return got, ref


# ---- 1. every joint's rows of J, on three trees
@pytest.mark.parametrize("tree,warm", [("xsens", True), ("xsens", False), ("arms_at_two_levels", False), ("four_limbs_on_one_joint", False)])
def test_every_joint_one_step_against_the_fp64_oracle(trees, dev, tree, warm):
    """frame f < 22 tracks joint f alone (a failure's frame number is the joint), 22 all joints (11 pair rounds), 23..27 7, 9, 11, 15, 21"""
    opt, m64, m32 = trees[tree]
    b = LO.every_joint_inputs(m64, warm)
    _one_step(opt, dev, b, _mus(28), m64, m32, f"every joint, {tree} {'warm' if warm else 'cold'}", every_frame=True)


# ---- 2. k launches of one step = one launch of k steps
def _composed(opt, dev, b, k, **kw):
    """k launches of LM(1), z fed back as z0, one mu tensor kept in place, z_tgt fixed -> the launches' results (numpy), in order"""
    from dragposer_amd.optimizer import to_device_batch

    d = to_device_batch(b, dev)
    mu = torch.full((len(b["z0"]),), 1e-2, device=dev)
    runs = []
    for _ in range(k):
        out = opt.optimize_lm(**d, mu=mu, **kw)
        torch.cuda.synchronize()
        assert out["mu"] is mu
        runs.append({n: v.cpu().numpy().copy() for n, v in out.items()})
        d["z0"] = out["z"].clone()
    return runs


@pytest.mark.parametrize("early_stop", [False, True])
@pytest.mark.parametrize("recipe", ["3cold", "6warm"])
def test_k_launches_of_one_step_are_one_launch_of_k_steps(opts, dev, recipe, early_stop):
    """The only state a frame carries between steps is z, mu, the kept loss, and A and g, and a fresh launch at the same z forms the last
    three with the same instructions: bit equality, after rejections (the fused run repeats only the solve) and accepts alike.  mu_max is
    the default, out of reach in 6 steps: hit_max is not carried between launches."""
    B, k = 41, 6
    b = _inputs(recipe, B)
    eps = {}
    if early_stop:  # (thresholds as in tests/test_hip_lm.py's test_several_steps: half the oracle's median final loss)
        half = 0.5 * float(np.median(LO.lm(_models()[0], b, k)["loss"].sum(1)))
        eps = dict(stop_eps_pos=half, stop_eps_rot=half)
        ref = LO.lm(_models()[0], b, k, early_stop=True, **eps)
        print(f"{recipe}: oracle iters histogram under early stop {np.bincount(ref['iters'], minlength=k + 1).tolist()}")
        assert (ref["iters"] < k).any() and len(np.unique(ref["iters"])) > 1  # (frames stop, and not all at the same step)
    fused = _run(opts["fp32"], b, dev, mu=np.full(B, 1e-2, np.float32), lm=_lm(k, early_stop=early_stop), **eps)
    runs = _composed(opts["fp32"], dev, b, k, lm=_lm(1, early_stop=early_stop), **eps)
    rej = [int((r["iters"] - r["n_accepted"]).sum()) for r in runs]
    after = sum(int(((p["iters"] > p["n_accepted"]) & (r["n_accepted"] > 0)).sum()) for p, r in zip(runs, runs[1:]))
    print(f"{recipe} early_stop={early_stop}: rejections per launch {rej}, accepts that follow a rejection {after}, fused iters histogram "
          f"{np.bincount(fused['iters'], minlength=k + 1).tolist()}")
    for r in runs:
        assert (r["status"] == 0).all()
    last = runs[-1]
    for n in RESULTS + ("mu", "z_pre"):
        _same_bits(last[n], fused[n], n)
    np.testing.assert_array_equal(sum(r["iters"] for r in runs), fused["iters"])
    np.testing.assert_array_equal(sum(r["n_accepted"] for r in runs), fused["n_accepted"])
    _same_bits(runs[0]["loss0"], fused["loss0"], "loss0")
    for i in range(1, k):
        _same_bits(runs[i]["loss0"], runs[i - 1]["loss"], f"loss0 of launch {i}")
    if early_stop:
        assert (fused["iters"] < k).any()
        for i in range(1, k):
            was = runs[i - 1]["iters"] == 0
            assert (runs[i]["iters"][was] == 0).all(), i  # (a frame that has stopped stays stopped ...)
            for n in RESULTS + ("mu",):  # (... and its bits no longer move)
                _same_bits(runs[i][n][was], runs[i - 1][n][was], (i, n))
    else:
        acc = LO.lm(_models()[0], b, k)["accepted"]
        assert (fused["iters"] == k).all() and (~acc).any() and (~acc[:, :-1] & acc[:, 1:]).any()  # (the oracle takes the paths this test is about)


# ---- 3. rejections that are certain, the clamps, hit_max
@pytest.mark.parametrize("problem", ["zero", "at_target"])
def test_rejections_that_are_certain_end_at_mu_max(opts, dev, problem):
    """zero: every weight 0 and lambda_tmp 0, so every pivot is 0 and the Cholesky refuses; at_target: z_tgt = z0 as well, lambda_tmp 0.02, so
    delta = 0, L' == L == 0 and the strict `<` rejects.  Exact in any arithmetic (both oracles: tests/test_lm_oracle.py).  Five rejections
    take mu 0.01 -> 10 = mu_max, the sixth is at mu_max and ends the frame; the thresholds are -1 because loss_pos = 0 would end it at once."""
    B = 41
    b, lam_tmp = (LO.zero_problem if problem == "zero" else LO.at_target_problem)(_models()[0], B)
    for early_stop, iters in ((True, 6), (False, 12)):
        got = _run(opts["fp32"], b, dev, lm=_lm(12, mu_max=10.0, early_stop=early_stop, stop_eps_pos=-1.0, stop_eps_rot=-1.0), lambda_tmp=lam_tmp)
        print(f"{problem} early_stop={early_stop}: iters {np.unique(got['iters']).tolist()}, accepted {np.unique(got['n_accepted']).tolist()}, mu {np.unique(got['mu']).tolist()}")
        np.testing.assert_array_equal(got["iters"], iters)
        np.testing.assert_array_equal(got["n_accepted"], 0)
        np.testing.assert_array_equal(got["mu"], np.float32(10.0))
        np.testing.assert_array_equal(got["status"], 0)
        _same_bits(got["z"], b["z0"].astype(np.float32), "z")
        _same_bits(got["z_pre"], got["z"], "z_pre")
        for n, v in got.items():
            assert np.isfinite(v).all(), n
        assert (got["loss"] == 0).all() and (got["loss0"] == 0).all()
        _forward_bars(got, b, b["z0"], None, lam_tmp=lam_tmp)


def test_mu_min_clamps_the_accepted_steps(opts, dev):
    """6 warm: the oracle accepts both steps on every frame, so mu = max(mu0 / 3, mu_min) = mu_min after the first and stays there"""
    B = 41
    b = _inputs("6warm", B)
    ref = LO.lm(_models()[0], b, 2, mu_min=5e-3)
    got = _run(opts["fp32"], b, dev, lm=_lm(2, mu_min=5e-3, early_stop=False))
    sure = (ref["margin"] >= MARGIN).all(1)
    print(f"mu_min 5e-3: compared on {int(sure.sum())}/{B} frames, kernel mu {np.unique(got['mu']).tolist()}, accepted {np.unique(got['n_accepted']).tolist()}")
    assert int((~sure).sum()) <= 2 and (ref["n_accepted"] == 2).all() and (ref["mu"] == 5e-3).all()
    assert (got["status"] == 0).all() and (got["iters"] == 2).all()
    np.testing.assert_array_equal(got["n_accepted"][sure], ref["n_accepted"][sure])
    np.testing.assert_allclose(got["mu"][sure], ref["mu"][sure], rtol=1e-6)


def test_other_factors_on_both_branches(opts, dev):
    """3 cold rejects about a quarter of its frames at step 1: mu x 10 there, mu x 0.5 on the others"""
    m64, m32 = _models()
    B = 41
    got, ref = _one_step(opts["fp32"], dev, _inputs("3cold", B), _mus(B), m64, m32, "3cold, mu_up 10, mu_down 0.5", mu_up=10.0, mu_down=0.5)
    assert 4 <= int((~ref["accepted"][:, 0]).sum()) <= B - 4  # (both branches run)
    ratio = got["mu"].astype(np.float64) / _mus(B)
    assert set(np.round(ratio, 4).tolist()) == {0.5, 10.0}


# ---- 4. the mu array's contract
def _rule(mu, flags, p, early_stop):
    """the header's damping rule from `mu` over the accept flags of the steps that ran -> mu after, or None when the frame would have ended
    before the last of them (a rejection at mu_max under early_stop)"""
    for i, acc in enumerate(flags):
        hit = not acc and mu >= p["mu_max"]
        mu = max(mu * p["mu_down"], p["mu_min"]) if acc else min(mu * p["mu_up"], p["mu_max"])
        if hit and early_stop and i + 1 < len(flags):
            return None
    return mu


def test_mu_entries_that_are_not_valid_are_read_as_mu0(opts, dev):
    B = 9
    b = _inputs("6cold", B)
    mu = np.full(B, 1e-2, np.float32)
    clean = _run(opts["fp32"], b, dev, mu=mu, lm=_lm(3))
    mu[:6] = [np.nan, np.inf, 0.0, -1.0, 1e-7, 1e7]
    got = _run(opts["fp32"], b, dev, mu=mu, lm=_lm(3))
    assert (clean["status"] == 0).all() and (clean["iters"] == 3).all()
    for n in clean:
        _same_bits(got[n], clean[n], n)


def test_mu_min_and_mu_max_are_used_as_given(opts, dev):
    """frames 0..3 enter at mu_min, 4..7 at mu_max, frame 8 at mu0.  From mu_max a step is 1e-6 of a Gauss-Newton step and its margin is below
    MARGIN (the oracle: 3e-6 .. 3e-5), so those frames' flags may fall either way: every frame's mu is held to the header's rule for the
    flags the kernel reports (read as mu0, no sequence of flags gives it), and to the oracle's wherever every step is sure."""
    m64, m32 = _models()
    B = 9
    b = _inputs("6cold", B)
    p = LO.DEFAULTS
    mu = np.full(B, p["mu0"], np.float32)
    mu[:4], mu[4:8] = p["mu_min"], p["mu_max"]
    ref = LO.lm(m64, b, 3, mu=mu.astype(np.float64), early_stop=True)
    r32 = LO.lm(m32, b, 3, mu=mu, early_stop=True)
    got = _run(opts["fp32"], b, dev, mu=mu, lm=_lm(3))
    assert (got["status"] == 0).all()
    bar = max(4.0 * np.abs(r32["z"] - ref["z"]).max(), 1e-6)
    sure = ~(ref["ran"] & (ref["margin"] < MARGIN)).any(1)
    dz = np.abs(got["z"] - ref["z"]).max(1)
    print(f"mu at its bounds: kernel mu {got['mu'].tolist()}, oracle {ref['mu'].tolist()}, accepted {got['n_accepted'].tolist()} (oracle "
          f"{ref['n_accepted'].tolist()}), sure frames {np.nonzero(sure)[0].tolist()}, |dz| {dz.tolist()}, bar {bar:.3e}")
    assert sure[:4].all()  # (from mu_min the steps are full Gauss-Newton steps, decided by a wide margin)
    for f in range(B):
        n, a = int(got["iters"][f]), int(got["n_accepted"][f])
        reach = [_rule(float(mu[f]), fl, p, True) for fl in itertools.product((False, True), repeat=n) if sum(fl) == a]
        assert any(r is not None and abs(float(got["mu"][f]) - r) <= 1e-6 * r for r in reach), (f, got["mu"][f], reach)
    np.testing.assert_array_equal(got["iters"][sure], ref["iters"][sure])
    np.testing.assert_array_equal(got["n_accepted"][sure], ref["n_accepted"][sure])
    np.testing.assert_allclose(got["mu"][sure], ref["mu"][sure], rtol=1e-6)
    assert dz[sure].max() <= bar, (dz, bar)


def test_refused_frames_leave_their_mu_alone(opts, dev):
    B = 9
    b = {k: np.array(v) for k, v in _inputs("6cold", B).items()}
    mu = np.full(B, 1e-2, np.float32)
    mu[[2, 4]] = 0.37
    clean = _run(opts["fp32"], b, dev, mu=mu, lm=_lm(3))
    b["z0"][2, 5] = np.nan  # BAD_STATE: no step runs
    b["tgt_pos"][4, 13, 1] = np.nan  # BAD_TARGETS, on a tracked joint
    got = _run(opts["fp32"], b, dev, mu=mu, lm=_lm(3))
    from dragposer_amd import _lib

    assert got["status"][2] & _lib.DP_STATUS_BAD_STATE and got["status"][4] & _lib.DP_STATUS_BAD_TARGETS
    _same_bits(got["mu"][[2, 4]], np.full(2, 0.37, np.float32), "mu")
    assert (got["n_accepted"][[2, 4]] == 0).all() and (got["iters"][[2, 4]] == 0).all()
    assert (clean["mu"][[2, 4]] != np.float32(0.37)).all()  # (a frame that runs does move it)
    rest = ~np.isin(np.arange(B), [2, 4])
    for n in clean:
        _same_bits(got[n][rest], clean[n][rest], n)


# ---- 5. subsets of the outputs, and a bf16 step
@pytest.mark.parametrize("outputs", [("z",), ("loss",), ("loss0", "n_accepted"), ("pos", "rot", "status", "iters")])
def test_a_subset_of_the_outputs_has_the_bits_of_the_whole(opts, dev, outputs):
    """every pointer may be NULL: the double-precision reporting pass runs only for loss / loss0, each store only for its pointer"""
    b = _inputs("3warm", 9)
    whole = _run(opts["fp32"], b, dev, lm=_lm(3))
    got = _run(opts["fp32"], b, dev, lm=_lm(3), outputs=outputs)
    assert set(got) == set(outputs) | {"mu"}
    assert (whole["status"] == 0).all() and (whole["n_accepted"] > 0).any()
    for n in got:
        _same_bits(got[n], whole[n], n)


@functools.lru_cache(maxsize=None)
def _bf16_models():
    return R.OracleModel(dtype=torch.float64, weight_rounding="bf16"), R.OracleModel(dtype=torch.float32, weight_rounding="bf16")


@pytest.mark.parametrize("recipe", ["6cold", "3warm"])
def test_one_step_through_a_bf16_context(opts, dev, recipe):
    """against the fp64 oracle on bf16-rounded weights, the bar from the fp32 oracle on the same weights.  The rounding itself moves the
    one-step latent by far more than the bar (printed), so an fp32 context in the bf16 one's place would fail."""
    mb64, mb32 = _bf16_models()
    B = 41
    b, mu = _inputs(recipe, B), _mus(B)
    _, ref = _one_step(opts["bf16"], dev, b, mu, mb64, mb32, f"bf16 context, {recipe}")
    plain = LO.lm(_models()[0], b, 1, mu=mu.astype(np.float64))
    agree = plain["n_accepted"] == ref["n_accepted"]
    print(f"  the weights' rounding moves the oracle's z by {np.abs(plain['z'] - ref['z'])[agree].max():.3e}")

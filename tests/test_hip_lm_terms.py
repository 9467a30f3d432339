"""GPU (MI355X): dp_optimize_lm_terms (include/dragposer_lm_terms.h) -- dp_optimize_lm with a term table in its loss -- against the fp64
oracle (tests/lm_terms_oracle.py): the empty table's bits, one step per table and per primitive (tests/test_hip_lm.py's bars), several
steps, k launches against one, the status word and isolation, determinism, output subsets, graph capture, a bf16 context."""
import functools

import numpy as np
import pytest
import torch

import lm_oracle as LO
import lm_terms_oracle as LT
from oracle import ref_torch as R
from test_hip_lm import MARGIN, _forward_bars, _lm, _models, _mus, _sub

pytestmark = pytest.mark.gpu
SWITCH = 1e-4  # a frame whose nearest switch of a term is closer than this may take either active set
TABLES = ("plane_one_sided", "plane_tilted_rows", "band", "point_distance_rows", "world_align_rows", "same_joint", "custom", "pins", "mixed16")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def opts(dev):
    from dragposer_amd.optimizer import LatentOptimizer

    return {"fp32": LatentOptimizer(device=dev), "bf16": LatentOptimizer(device=dev, weight_dtype="bf16")}


@functools.lru_cache(maxsize=None)
def _inputs(warm, B):
    m64 = _models()[0]
    return (LO.warm_inputs(m64, B, seed=11) if warm else R.synth_inputs(m64, B, seed=11)), LT.global_pos(B)


def _sub_terms(terms, n):
    from dataclasses import replace

    from dragposer_amd import Terms

    return Terms([replace(t, per_frame=t.per_frame[:n].contiguous()) if t.per_frame is not None else t for t in terms.terms], terms.up_axis)


def _run(opt, b, gp, terms, dev, mu=None, **kw):
    from dragposer_amd.optimizer import to_device_batch

    d = to_device_batch(b, dev)
    out = opt.optimize_lm(**d, mu=torch.from_numpy(mu.copy()).to(dev) if mu is not None else None, terms=terms,
                          global_pos=torch.from_numpy(np.ascontiguousarray(gp)).to(dev) if gp is not None else None, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _one_step(opt, dev, b, gp, terms, mu, models=None, who=""):
    """one step of the kernel against the oracle pair: the accept flag on the frames that are kept, z within max(4 x the fp32 oracle's largest
    deviation on the same frames, 1e-6), mu, the forward bars and loss_terms at the kernel's own latent.

    loss_terms is held to term_values in fp64 (rtol 1e-5 / atol 1e-9) on the joints of the fp64 forward pass over the weights the CONTEXT
    holds, the folded fp32 matrices (lm_terms_oracle.folded_model): that is the function the kernel's pass in double evaluates and the header
    documents.  On the oracle's own weights, folded in double, a joint lies 1e-7 m elsewhere, which moves a band's slot c (lo^2 - q) by up to
    7.4e-8 whatever its size -- measured on an MI355X: CUSTOM()'s knee band was off by 7.4e-8 on a slot of 4.4e-3 (warm) and by 3.6e-8 on one
    of 1.5e-4 (cold) against those weights, and by less than the bar on every slot of every table against the context's.  The forward bars
    (positions, rotations, the three loss numbers) stay on the oracle's own weights, as in tests/test_hip_lm.py.  `models`: a bf16 context is
    held to the bf16-rounded oracle throughout."""
    m64, m32 = models or _models()
    ct = LT.cpu_terms(terms)
    ref = LT.lm_terms(m64, b, ct, gp, 1, mu=mu.astype(np.float64))
    r32 = LT.lm_terms(m32, b, ct, gp, 1, mu=mu)
    got = _run(opt, b, gp, terms, dev, mu=mu, lm=_lm(1, early_stop=False))
    keep = (ref["margin"][:, 0] >= MARGIN) & (ref["switch"][:, 0] >= SWITCH)
    assert len(keep) == 1 or keep.sum() >= 0.9 * len(keep), keep.sum()  # (tests/test_lm_terms_oracle.py holds the cap for these inputs)
    assert (got["status"] == 0).all() and (got["iters"] == 1).all()
    np.testing.assert_array_equal(got["n_accepted"][keep], ref["n_accepted"][keep])
    bar = max(4.0 * np.abs(r32["z"] - ref["z"])[keep].max(), 1e-6) if keep.any() else 1e-6
    dz = np.abs(got["z"] - ref["z"])[keep].max() if keep.any() else 0.0
    print(f"{who}: kernel max |dz| {dz:.3e}, bar {bar:.3e}, kept {int(keep.sum())}/{len(keep)}, accepted {int(ref['accepted'].sum())}, "
          f"active at z0 {int((ref['kinds0'] != 0).any(1).sum())}")
    assert dz <= bar, (dz, bar)
    np.testing.assert_allclose(got["mu"][keep], ref["mu"][keep], rtol=1e-6)
    _forward_bars(got, b, got["z"], got["loss"], model=m64)
    want = LT.terms_np(LT.folded_model(opt.host_model) if models is None else m64, ct, got["z"].astype(np.float64), b, gp)
    np.testing.assert_allclose(got["loss_terms"], want, rtol=1e-5, atol=1e-9)
    return got, ref


@pytest.mark.parametrize("warm", [True, False])
@pytest.mark.parametrize("lm", [dict(steps=3), dict(steps=6, early_stop=False)])
def test_empty_table_and_all_zero_weights_have_dp_optimize_lms_bits(opts, dev, warm, lm):
    from dataclasses import replace

    from dragposer_amd import Terms

    for B in (41, 1):
        b, gp = _inputs(warm, 41)
        b, gp, mu = _sub(b, B), gp[:B], _mus(41)[:B]
        plain = _run(opts["fp32"], b, None, None, dev, mu=mu, lm=_lm(**lm))
        assert "loss_terms" not in plain
        table = _sub_terms(LT.tables(41, dev)["mixed16"], B)
        off = Terms([replace(t, weight=0.0) for t in table.terms], table.up_axis)
        for terms, g in ((Terms(), None), (off, None), (off, gp)):
            got = _run(opts["fp32"], b, g, terms, dev, mu=mu, lm=_lm(**lm))
            assert got["loss_terms"].shape == (B, len(terms)) and (got["loss_terms"] == 0).all()
            for k in plain:
                np.testing.assert_array_equal(got[k], plain[k], err_msg=k)


@pytest.mark.parametrize("B", [41, 1])
@pytest.mark.parametrize("warm", [True, False])
@pytest.mark.parametrize("table", TABLES)
def test_one_step_against_the_fp64_oracle(opts, dev, table, warm, B):
    b, gp = _inputs(warm, 41)
    terms = _sub_terms(LT.tables(41, dev)[table], B)
    _one_step(opts["fp32"], dev, _sub(b, B), gp[:B], terms, _mus(41)[:B], who=f"{table} {'warm' if warm else 'cold'} B={B}")


def _primitives():
    from dragposer_amd import Term

    far, near = (0.0, 5.0, 0.0), (0.0, -5.0, 0.0)
    return {  # name -> (term, active at z0)
        "plane_two_sided": (Term.plane(8, (0, 1, 0), (0, 0.3, 0), weight=1.5), True),
        "plane_one_sided_active": (Term.plane(8, (0, 1, 0), far, weight=0.05, one_sided=True), True),
        "plane_one_sided_inactive": (Term.plane(8, (0, 1, 0), near, weight=1.5, one_sided=True), False),
        "distance_above_hi": (Term.distance(3, 7, lo=0.0, hi=0.05, weight=3.0), True),
        "distance_below_lo": (Term.distance(3, 7, lo=2.0, hi=3.0, weight=0.3), True),
        "distance_inside": (Term.distance(3, 7, lo=0.0, hi=5.0, weight=3.0), False),
        "pin_drop_up": (Term.distance(13, 0, drop_up=True, weight=2.0), True),
        "same_joint_twice": (Term.distance(5, 5, lo=0.1, hi=0.2, weight=2.0), True),
        "world_align": (Term.align(13, (0, 0, 1), dir=(1, 0, 0), margin=-0.5, weight=1.2, drop_up=True), True),
        "joint_align": (Term.align(17, (1, 0, 0), 21, (0, 1, 0), margin=-0.5, weight=0.7), True),
        "align_below_threshold": (Term.align(13, (0, 0, 1), dir=(1, 0, 0), threshold=5.0, weight=1.2), False),
    }


@pytest.mark.parametrize("name", list(_primitives()))
def test_each_primitive_alone_on_a_single_frame(opts, dev, name):
    from dragposer_amd import Terms

    term, active = _primitives()[name]
    b, gp = _inputs(True, 41)
    b, gp, mu = _sub(b, 1), gp[:1], _mus(41)[:1]
    terms = Terms([term])
    if active:
        got, ref = _one_step(opts["fp32"], dev, b, gp, terms, mu, who=name)
        assert (ref["kinds0"] != 0).all(), ref["kinds0"]
        assert (ref["loss_terms0"] > 0).all()
    else:
        ref = LT.lm_terms(_models()[0], b, terms, gp, 1, mu=mu.astype(np.float64))
        assert (ref["kinds0"] == 0).all() and (ref["loss_terms0"] == 0).all() and ref["switch"][0, 0] > SWITCH
        got = _run(opts["fp32"], b, gp, terms, dev, mu=mu, lm=_lm(1, early_stop=False))
        plain = _run(opts["fp32"], b, None, None, dev, mu=mu, lm=_lm(1, early_stop=False))
        for k in plain:
            np.testing.assert_array_equal(got[k], plain[k], err_msg=k)
        assert (got["loss_terms"] == 0).all()


@pytest.mark.parametrize("steps", [4, 8])
@pytest.mark.parametrize("table", TABLES)
def test_several_steps(opts, dev, table, steps):
    m64, m32 = _models()
    b, gp = _inputs(True, 64)
    terms = LT.tables(64, dev)[table]
    ct = LT.cpu_terms(terms)
    ref, r32 = LT.lm_terms(m64, b, ct, gp, steps), LT.lm_terms(m32, b, ct, gp, steps)
    got = _run(opts["fp32"], b, gp, terms, dev, lm=_lm(steps, early_stop=False))
    assert (got["status"] == 0).all() and (got["iters"] == steps).all()
    t0 = LT.terms_np(m64, ct, np.asarray(b["z0"], np.float64), b, gp).sum(1)
    tot = got["loss"].sum(1).astype(np.float64) + got["loss_terms"].sum(1)
    # (both sides are fp32 numbers of a pass in double, and the terms at z0 are the fp64 oracle's: equal up to a few fp32 roundings where no
    #  step was accepted, hence the 1e-6)
    assert (tot <= (got["loss0"].sum(1) + t0) * (1 + 1e-6)).all()
    assert (np.diff(ref["loss_hist"], axis=1) <= 0).all()
    want = ref["loss_hist"][:, -1]
    pair = np.abs(r32["loss_hist"][:, -1] - want) / want
    rel = np.abs(tot - want) / want
    unsure = ((ref["ran"] & (ref["margin"] < MARGIN)).any(1)) | (ref["switch"] < SWITCH).any(1)
    # the bar comes from the frames whose oracle trajectory was decided clearly; EVERY frame is held to it, and the tenth that may lie beyond
    # is spent first on the unsure ones (a trajectory that ends on a term's boundary, as a foot on its floor does, is unsure by nature)
    bar = 4.0 * (pair[~unsure].max() if (~unsure).any() else pair.max())
    out = int((rel > bar).sum())
    print(f"{table} {steps} steps: kernel max rel difference {rel.max():.3e} (median {np.median(rel):.3e}), oracle pair max {pair[~unsure].max():.3e}, "
          f"bar {bar:.3e}, unsure {int(unsure.sum())}, beyond {out}/64 ({int(((rel > bar) & ~unsure).sum())} of them sure), "
          f"accepted mean {got['n_accepted'].mean():.2f} (oracle {ref['n_accepted'].mean():.2f})")
    assert out <= 0.1 * len(rel), (np.sort(rel)[-4:], bar)


@pytest.mark.parametrize("table", ["band", "custom"])
def test_k_launches_of_one_step_are_one_launch_of_k_steps(opts, dev, table):
    from dragposer_amd.optimizer import to_device_batch

    opt, k = opts["fp32"], 4
    b, gp = _inputs(False, 41)
    terms = LT.tables(41, dev)[table]
    whole = _run(opt, b, gp, terms, dev, mu=_mus(41), lm=_lm(k, early_stop=False))
    d = to_device_batch(b, dev)
    g = torch.from_numpy(gp).to(dev)
    mu = torch.from_numpy(_mus(41).copy()).to(dev)
    z, nacc, iters = d["z0"], 0, 0
    for _ in range(k):
        out = opt.optimize_lm(**dict(d, z0=z), mu=mu, terms=terms, global_pos=g, lm=_lm(1, early_stop=False))
        z, nacc, iters = out["z"].clone(), nacc + out["n_accepted"].cpu().numpy(), iters + out["iters"].cpu().numpy()
    torch.cuda.synchronize()
    for name in ("z", "pose", "pos", "rot", "disp", "world_disp", "world_rot", "loss", "loss_terms", "mu", "status"):
        np.testing.assert_array_equal(out[name].cpu().numpy(), whole[name], err_msg=name)
    np.testing.assert_array_equal(nacc, whole["n_accepted"])
    np.testing.assert_array_equal(iters, whole["iters"])


def test_status_and_isolation(opts, dev):
    from dataclasses import replace

    from dragposer_amd import Terms, _lib

    opt = opts["fp32"]
    b, gp = _inputs(False, 41)
    b, gp = _sub(b, 9), gp[:9].copy()
    terms = _sub_terms(LT.tables(41, dev)["mixed16"], 9)
    mu = _mus(41)[:9]
    clean = _run(opt, b, gp, terms, dev, mu=mu, lm=_lm(3))
    assert (clean["status"] == 0).all()

    def with_row(term, frame, col, value):
        ts = list(terms.terms)
        pf = ts[term].per_frame.clone()
        pf[frame, col] = value
        ts[term] = replace(ts[term], per_frame=pf)
        return Terms(ts, terms.up_axis)

    for bad, frame in ((with_row(2, 4, 1, float("nan")), 4), (with_row(6, 5, 3, -1.0), 5)):
        got = _run(opt, b, gp, bad, dev, mu=mu, lm=_lm(3))
        assert got["status"][frame] == _lib.DP_STATUS_BAD_TARGETS | _lib.DP_STATUS_NONFINITE_RESULT
        for k in ("z", "loss", "loss0", "loss_terms"):
            assert np.isnan(got[k][frame]).all(), k
        assert got["iters"][frame] == 0 and got["mu"][frame] == mu[frame] and np.isfinite(got["pos"][frame]).all()
        rest = np.arange(9) != frame
        for k in clean:
            np.testing.assert_array_equal(got[k][rest], clean[k][rest], err_msg=k)
    g2 = gp.copy()
    g2[2, 0] = np.nan
    got = _run(opt, b, g2, terms, dev, mu=mu, lm=_lm(3))
    assert got["status"][2] == _lib.DP_STATUS_BAD_STATE | _lib.DP_STATUS_NONFINITE_RESULT
    assert np.isnan(got["pos"][2]).all() and np.isnan(got["loss_terms"][2]).all() and got["mu"][2] == mu[2]
    rest = np.arange(9) != 2
    for k in clean:
        np.testing.assert_array_equal(got[k][rest], clean[k][rest], err_msg=k)
    # s = 0 on a frame: the term is off there -- a zero loss slot and the bits of the table without that term
    s0 = terms.terms[6].per_frame[:, 3].cpu().numpy() == 0
    assert s0.any() and (clean["loss_terms"][s0, 6] == 0).all()
    less = Terms([t for i, t in enumerate(terms.terms) if i != 6], terms.up_axis)
    other = _run(opt, b, gp, less, dev, mu=mu, lm=_lm(3))
    for k in clean:
        if k == "loss_terms":
            np.testing.assert_array_equal(np.delete(clean[k], 6, axis=1)[s0], other[k][s0])
        else:
            np.testing.assert_array_equal(clean[k][s0], other[k][s0], err_msg=k)


def test_determinism_output_subsets_and_graph_capture(opts, dev):
    from dragposer_amd.optimizer import to_device_batch

    opt = opts["fp32"]
    b, gp = _inputs(False, 41)
    terms = LT.tables(41, dev)["mixed16"]
    a = _run(opt, b, gp, terms, dev, lm=_lm(3))
    c = _run(opt, b, gp, terms, dev, lm=_lm(3))
    for k in a:
        np.testing.assert_array_equal(a[k], c[k], err_msg=k)
    for subset in (("z", "loss_terms"), ("loss_terms",), ("pos", "loss", "mu"), ("z", "n_accepted")):
        part = _run(opt, b, gp, terms, dev, lm=_lm(3), outputs=subset)
        assert set(part) == set(subset) | {"mu"}
        for k in part:
            np.testing.assert_array_equal(part[k], a[k], err_msg=k)
    d = to_device_batch(b, dev)
    g = torch.from_numpy(gp).to(dev)
    out = opt.allocate_outputs(41)
    out.update(n_accepted=torch.empty(41, dtype=torch.int32, device=dev), loss0=torch.empty(41, 3, device=dev),
               loss_terms=torch.empty(41, len(terms), device=dev))
    mu = torch.full((41,), 1e-2, device=dev)
    rows = terms.terms[6].per_frame
    kept = rows.clone()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        opt.optimize_lm(**d, lm=_lm(3), mu=mu, out=out, outputs=tuple(out), terms=terms, global_pos=g)
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.optimize_lm(**d, lm=_lm(3), mu=mu, out=out, outputs=tuple(out), terms=terms, global_pos=g)
    for v in out.values():
        v.fill_(-1)
    mu.fill_(1e-2)
    graph.replay()
    torch.cuda.synchronize()
    for k in out:
        np.testing.assert_array_equal(out[k].cpu().numpy(), a[k], err_msg=k)
    np.testing.assert_array_equal(mu.cpu().numpy(), a["mu"])
    # the second replay reads mu and the rows as they are then
    rows[:, 3] = 0.0
    mu.fill_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    second = {k: v.cpu().numpy() for k, v in out.items()}
    assert (second["loss_terms"][:, 6] == 0).all() and not np.array_equal(second["z"], a["z"])
    fresh = _run(opt, b, gp, terms, dev, mu=np.full(41, 1.0, np.float32), lm=_lm(3))
    rows.copy_(kept)
    for k in second:
        np.testing.assert_array_equal(second[k], fresh[k], err_msg=k)


def test_a_bf16_context_meets_the_one_step_bar_of_the_bf16_rounded_oracles(opts, dev):
    mb = (R.OracleModel(dtype=torch.float64, weight_rounding="bf16"), R.OracleModel(dtype=torch.float32, weight_rounding="bf16"))
    b, gp = _inputs(True, 41)
    _one_step(opts["bf16"], dev, b, gp, LT.tables(41, dev)["custom"], _mus(41), models=mb, who="bf16 custom")

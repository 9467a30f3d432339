"""GPU: Adam's knobs -- dp_params.lr / beta1 / beta2 / eps -- on every kernel that implements Adam.

The smooth case (tests/adam_reference.py): a frame whose tracker term is exactly zero has the loss lam * mean((z - z_tgt)^2), and its latent after N
steps is a scalar recursion per component, with no decoder and no LeakyReLU kink for two correct implementations to part ways at.  The tracker
term is zeroed two ways -- frames that track nothing (the dp_optimize units: the project defines that case there) and frames with the reference's
six trackers and every weight 0 (all units) --, the targets are drawn out of reach (adam_reference.smooth_targets), and every unit's latent is
held to the fp64 recursion at the case's bar: 4 x the distance of the recursion's own fp32 twin, never below 2e-6 (the kernels take sqrt and the
reciprocal from the 1-ulp hardware instructions where the twin rounds them correctly).  A case is run only if it can tell every knob it sets from
that knob's default: the fp64 result with the one knob put back lies at least 100 bars away (tests/test_adam_reference.py holds the table to
that, and this file asserts it again per case).  The four routes the knobs take -- the host's table of Adam scalars, its continuation on the device
beyond iteration 256, the loop's own scalars (1 - beta1, beta2, 1 - beta2, eps) and the double-precision continuation of dp_cons_body.h -- all
end in that latent.

The real path, short: 16 tracked frames x 5 iterations with the "fast" and the "eps" set against the oracles, which take lr, betas and eps."""
import numpy as np
import pytest
import torch

import adam_reference as A  # tests/adam_reference.py
from instantiations import UNIT_W4, UNIT_W4_BP, UNIT_W4_BP_LV, UNIT_W16, last_launch, set_layout  # tests/instantiations.py
from oracle import ref_torch as R
from oracle.analytic import AnalyticOracle
from skeleton_cases import UNIT_W4_BP_SKEL, UNIT_W4_SKEL  # tests/skeleton_cases.py
from test_hip_w4_loop_versions import LAM as TRACKER_LAM, SETS as TRACKER_SETS, _batch  # tests/test_hip_w4_loop_versions.py

pytestmark = pytest.mark.gpu

KEYS = ("z0", "z_tgt", "cur_rot", "tgt_pos", "tgt_rot", "w", "tracked")
OUT = ("z", "pos", "loss", "iters", "status")
# the while-condition with a threshold that is never met: the tracker losses of a smooth case are exactly 0 and the loop goes on while one of them
# is ABOVE its threshold -- so the threshold is below zero --, and every decrement of the loss is above -inf
NEVER = dict(stop_eps_pos=-1.0, stop_eps_rot=-1.0, min_loss_incr=float("-inf"))
# unit -> (dp_debug_set_w4_layout's argument, what dp_debug_last_launch must report (unit, waves, early) or None, the ways the tracker term is zeroed)
UNITS = {
    "w4_dense": (0, (UNIT_W4, 4, 0), ("w0", "untracked")),
    "w4_bp_debug": (1, (UNIT_W4_BP, 4, 0), ("w0", "untracked")),
    "w4_bplv": (1, (UNIT_W4_BP_LV, 4, 0), ("w0", "untracked")),
    "w16_4w": (1, (UNIT_W16, 4, 0), ("w0", "untracked")),
    "w4sk": (0, (UNIT_W4_SKEL, 4, 0), ("w0", "untracked")),
    "w4sk_bp": (1, (UNIT_W4_BP_SKEL, 4, 0), ("w0", "untracked")),
    "w4_dense_while": (0, (UNIT_W4, 4, 1), ("w0", "untracked")),
    "w4_bp_while": (1, (UNIT_W4_BP, 4, 1), ("w0", "untracked")),
    "w16_4w_while": (1, (UNIT_W16, 4, 1), ("w0", "untracked")),
    "w4sk_while": (0, (UNIT_W4_SKEL, 4, 1), ("w0", "untracked")),
    "w4sk_bp_while": (1, (UNIT_W4_BP_SKEL, 4, 1), ("w0", "untracked")),
    "constrained": (1, None, ("w0",)),
    "terms": (1, None, ("w0",)),
}


@pytest.fixture(scope="module")
def opt():
    from dragposer_amd.optimizer import LatentOptimizer

    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    o = LatentOptimizer(device="cuda:0")
    assert set_layout(o, -1) == 1
    yield o
    set_layout(o, 1)
    o.close()


_BASE = {}


def smooth_batch(c, way):
    """the eight frames of a smooth case: recipe S's rotations and targets, the case's z0 and z_tgt, the tracker term zeroed `way`"""
    if "b" not in _BASE:
        _BASE["b"] = R.synth_inputs(R.OracleModel(), A.N_FRAMES, seed=515)
    b = {k: _BASE["b"][k].copy() for k in KEYS}
    b["z0"], b["z_tgt"] = c["z0"].copy(), c["z_tgt"].copy()
    b["w"][:] = 0
    if way == "untracked":
        b["tracked"][:] = 0
        b["tgt_pos"][:] = 0
        b["tgt_rot"][:] = 0
    else:
        assert way == "w0" and (b["tracked"].sum(1) == 6).all()
    return b


def _adam(k):
    return dict(lr=k["lr"], betas=(k["b1"], k["b2"]), eps=k["eps"])


def run_unit(opt, unit, b, n_iter, k, lam, stop=None, constraints=None, terms=None):
    """one launch of `unit` -> its results as numpy arrays; the unit is asserted through dp_debug_last_launch where the launcher records it.
    `stop`: the while-condition's settings of a *_while unit (default: NEVER)"""
    from dragposer_amd import Constraints, Terms
    from dragposer_amd.optimizer import to_device_batch

    layout, pick, _ = UNITS[unit]
    assert set_layout(opt, layout) == layout
    d = to_device_batch(b, opt.device)
    kw = dict(n_iter=n_iter, lambda_tmp=lam, outputs=OUT, **_adam(k))
    if unit.endswith("_while"):
        kw.update(NEVER if stop is None else stop)
    if unit == "constrained":
        out = opt.optimize_constrained(**d, constraints=constraints or Constraints(), **kw)
    elif unit == "terms":
        out = opt.optimize_terms(**d, terms=terms or Terms(), **kw)
    else:
        kw["kernel"] = "w16" if unit.startswith("w16") else "w4"
        if unit == "w4_bp_debug":
            kw["_debug"] = torch.zeros(len(b["z0"]), 240, device=opt.device)
        if unit.startswith("w4sk"):  # the context's own skeleton, passed per frame
            base = np.asarray(np.load(R.DEFAULT_MODEL)["offsets"], np.float32)
            kw["offsets"] = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(base, (len(b["z0"]), 22, 3)))).to(opt.device)
        out = opt.optimize(**d, **kw)
    torch.cuda.synchronize()
    if pick is not None:
        ran = last_launch(opt)
        assert tuple(ran) == pick + (0, int(n_iter > 256)), (unit, ran)
    return {x: v.cpu().numpy() for x, v in out.items()}


def _tells_its_knobs(c):
    return all(m >= A.MARGIN for m in c["margins"].values())


@pytest.mark.parametrize("name", [n for n, steps in A.KEPT_STEPS.items() if steps])
@pytest.mark.parametrize("unit", list(UNITS))
def test_smooth_case_latent_against_the_fp64_recursion(opt, unit, name):
    k = A.SETS[name]
    for lam in A.LAMS:
        for n_iter in A.KEPT_STEPS[name]:
            c = A.case(name, lam, n_iter)
            assert _tells_its_knobs(c), (name, lam, n_iter, c["margins"])
            for way in UNITS[unit][2]:
                o = run_unit(opt, unit, smooth_batch(c, way), n_iter, k, lam)
                err = float(np.abs(o["z"].astype(np.float64) - c["want"]).max())
                print(f"{unit} {name} lam {lam} N {n_iter} {way}: |z - fp64| max {err:.2e}, bar {c['bar']:.2e}")
                assert (o["status"] == 0).all() and (o["iters"] == n_iter).all(), (unit, name, lam, n_iter, way, o["status"], o["iters"])
                assert (o["loss"][:, :2] == 0).all(), (unit, name, way)  # the tracker term was exactly zero on the last pass
                assert err <= c["bar"], (unit, name, lam, n_iter, way, err, c["bar"])


@pytest.mark.parametrize("layout", [1, 0], ids=["body_part", "dense"])
@pytest.mark.parametrize("name,n_iter", A.SEQUENCE_CASES, ids=[f"{n}-{i}" for n, i in A.SEQUENCE_CASES])
def test_smooth_case_through_a_whole_sequence_launch(opt, name, n_iter, layout):
    """dp_optimize_sequence over T = 3 steps with the while-condition never met: Adam is re-created per step, so step k's latent is the recursion
    restarted from step k - 1's; the latent after the last step carries all three.  n_iter 257: the LONG sequence kernel."""
    from dragposer_amd.drag_pose import DragPose

    T, S, lam, k = A.SEQUENCE_STEPS, A.N_FRAMES, A.SEQUENCE_LAM, A.SETS[name]
    c = A.case(name, lam, n_iter, T)
    assert _tells_its_knobs(c), (name, n_iter, c["margins"])
    b = smooth_batch(c, "w0")
    assert set_layout(opt, layout) == layout
    dev = opt.device
    dp = DragPose(opt, None, np.zeros(24), np.ones(24), n_sequences=S)
    dp.set_initial_state(b["z0"], np.zeros((S, 3), np.float32), b["cur_rot"], np.zeros((S, 6), np.float32))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tp, tr = t(np.broadcast_to(b["tgt_pos"], (T, S, 22, 3))), t(np.broadcast_to(b["tgt_rot"], (T, S, 22, 9)))
    heights = (0, 4, 8, 13, 17, 21)
    scratch = torch.empty(T, S, 24 + 3 + len(heights), device=dev)
    r = opt.optimize_sequence(dp.latent, tp, tr, None, t(b["w"]), t(b["tracked"]), t(b["z_tgt"]), (0, 24), dp.current_global_pos, dp.current_global_rot,
                              dp.latent_buffer, dp.displacement_buffer, dp.heights_buffer, heights, n_iter=n_iter, lambda_rot=1.0, lambda_tmp=lam,
                              scratch=scratch, **_adam(k), **NEVER)
    torch.cuda.synchronize()
    ran = last_launch(opt)
    assert tuple(ran) == (UNIT_W4_BP if layout else UNIT_W4, 4, 1, 1, int(n_iter > 256)), ran
    assert (r["status"] == 0).all() and (r["iters"] == n_iter).all(), (r["status"], r["iters"])
    z = dp.latent.cpu().numpy().astype(np.float64)
    err = float(np.abs(z - c["want"][-1]).max())
    # every step's last forward pass read the latent one Adam step before the step's end
    pre = scratch[..., :24].cpu().numpy().astype(np.float64)
    start = np.concatenate([c["z0"][None].astype(np.float64), c["want"][:-1]])
    want_pre = np.stack([A.recursion(start[s], c["z_tgt"], n_iter - 1, lam=lam, **k) for s in range(T)])
    err_pre = float(np.abs(pre - want_pre).max())
    print(f"sequence {name} N {n_iter} layout {layout}: |z - fp64| max {err:.2e}, per step (z_pre) {err_pre:.2e}, bar {c['bar']:.2e}")
    assert err <= c["bar"] and err_pre <= c["bar"], (name, n_iter, err, err_pre, c["bar"])


# ---------------------------------------------------------------- the real path, short
REAL_SETS = ("fast", "eps")
REAL_SEED, REAL_FRAMES, REAL_ITERS = 31, 16, 5
# min_loss_incr per (trackers, set): the geometric middle of the widest gap between two decrements of the f64 oracle's loss over these five
# iterations that stops at least four frames before the fifth (tests/test_adam_reference.py asserts the stops and that the f32 oracle agrees)
REAL_WHILE = {("six", "fast"): 0.0065, ("six", "eps"): 0.0029, ("three", "fast"): 0.037, ("three", "eps"): 0.017}
_REAL = {}


def real_reference(trackers, name, early):
    """(batch, the C oracle's f32 run, its f64 run) of a short real-path case: computed once, shared, left unchanged"""
    key = (trackers, name, early)
    if key not in _REAL:
        b, _ = _batch(REAL_FRAMES, TRACKER_SETS[trackers], seed=REAL_SEED)
        kw = dict(lam_tmp=TRACKER_LAM[trackers], **_adam(A.SETS[name]))
        if early:
            kw["min_loss_incr"] = REAL_WHILE[trackers, name]
        pair = [AnalyticOracle(precision=p).optimize(*[b[x] for x in KEYS], REAL_ITERS, **kw) for p in ("f32", "f64")]
        for r in pair:
            for v in r.values():
                v.setflags(write=False)
        _REAL[key] = (b, pair[0], pair[1])
    return _REAL[key]


def _check_real(what, o, ref_pos, ref_z, ref_loss, ref_iters, keep, lr):
    """test_hip_w4_loop_versions.py::test_each_version_against_the_c_oracle's bars, the latent's scaled with the step size"""
    err = np.linalg.norm(o["pos"] - ref_pos, axis=-1).max(axis=1) * 1000.0
    dz = np.abs(o["z"] - ref_z).max(axis=1)
    print(f"{what}: max joint error {err[keep].max():.5f} mm, |dz| {dz[keep].max():.2e}, iterations {o['iters'].tolist()}")
    assert (o["status"] == 0).all() and keep.sum() >= len(keep) - 1
    assert err[keep].max() <= 0.05, (what, err)
    assert dz[keep].max() <= 5e-5 * lr / 1e-2, (what, dz)
    np.testing.assert_allclose(o["loss"][keep], ref_loss[keep], rtol=2e-3, atol=1e-8, err_msg=what)
    np.testing.assert_array_equal(o["iters"][keep], ref_iters[keep], err_msg=what)


REAL_UNITS = {False: ("w4_dense", "w4_bp_debug", "w4_bplv", "w16_4w", "w4sk", "w4sk_bp"),
              True: ("w4_dense_while", "w4_bp_while", "w16_4w_while", "w4sk_while", "w4sk_bp_while")}


@pytest.mark.parametrize("early", [False, True], ids=["fixed_count", "while_condition"])
@pytest.mark.parametrize("name", REAL_SETS)
@pytest.mark.parametrize("trackers", ["six", "three"])
def test_tracked_frames_with_other_knobs_against_the_c_oracle(opt, trackers, name, early):
    b, r32, r64 = real_reference(trackers, name, early)
    keep = np.linalg.norm(r32["pos"] - r64["pos"], axis=-1).max(axis=1) * 1000.0 <= 0.02  # (the oracle's own pair: leaves out none, asserted on the CPU)
    k, lam = A.SETS[name], TRACKER_LAM[trackers]
    if early:
        assert (r32["iters"] < REAL_ITERS).sum() >= 4 and np.array_equal(r32["iters"], r64["iters"])
    for unit in REAL_UNITS[early]:
        o = run_unit(opt, unit, b, REAL_ITERS, k, lam, stop=dict(min_loss_incr=REAL_WHILE[trackers, name]) if early else None)
        _check_real(f"{unit} {trackers} {name}", o, r32["pos"], r32["z_final"], r32["loss"], r32["iters"], keep, k["lr"])


def constraint_reference(unit, name):
    """(batch, the extra term as Constraints / Terms, the fp64 oracle's run, the plain fp64 run without the term) of the constraint kernels' short case"""
    import constraints_oracle as CO
    import terms_oracle as TO
    from dragposer_amd import Constraints, Terms

    key = (unit, name)
    if key not in _REAL:
        b, _ = _batch(REAL_FRAMES, TRACKER_SETS["six"], seed=REAL_SEED)
        k = A.SETS[name]
        cons = Constraints(w_head_hips_colinear=1.0)
        model = R.OracleModel(dtype=torch.float64)
        kw = dict(lam_tmp=TRACKER_LAM["six"], **_adam(k))
        if unit == "constrained":
            extra, ref = cons, CO.optimize_constrained(model, b, cons, np.zeros((REAL_FRAMES, 3), np.float32), REAL_ITERS, **kw)
        else:
            extra = Terms.from_constraints(cons)
            ref = TO.optimize_terms(model, b, extra, None, REAL_ITERS, **kw)
        plain = AnalyticOracle(precision="f64").optimize(*[b[x] for x in KEYS], REAL_ITERS, **kw)
        _REAL[key] = (b, extra, ref, plain)
    return _REAL[key]


@pytest.mark.parametrize("name", REAL_SETS)
@pytest.mark.parametrize("unit", ["constrained", "terms"])
def test_constraint_kernels_with_other_knobs_against_their_oracles(opt, unit, name):
    """dp_optimize_constrained / dp_optimize_terms (dp_cons_body.h's Adam: the bias corrections continued in double per iteration) on the six-tracker
    frames with the head over the hips as the one extra term, against tests/constraints_oracle.py / tests/terms_oracle.py in fp64"""
    b, extra, ref, plain = constraint_reference(unit, name)
    k, lam = A.SETS[name], TRACKER_LAM["six"]
    assert np.abs(plain["z_final"] - ref["z_final"]).max() > 1e-3  # the extra term is in the gradient
    o = run_unit(opt, unit, b, REAL_ITERS, k, lam, **{"constraints" if unit == "constrained" else "terms": extra})
    _check_real(f"{unit} {name}", o, ref["pos"], ref["z_final"], ref["loss"], ref["iters"], np.ones(REAL_FRAMES, bool), k["lr"])

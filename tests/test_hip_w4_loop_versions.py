"""GPU: the loop versions of the body-part fixed-count kernel (dp_w4_bp_lv.hip; dp_w4_impl.h, W4_LOOP_VERSIONS) against its general loop, bit for bit.

A wave of that kernel picks one version of the iteration loop behind its set-up: the common one (with the wave's bL2 skip pattern compiled in) when
it optimises and none of its four frames tracks more than six joints, the general one otherwise.  A frame's arithmetic does not depend on its
wave-mates (the transposes multiply the other frames' values with exact zeros, and bL2's skipped K-groups multiply exact zeros), so the same
frame must come out with the same bits whichever version its wave runs.  The test makes the SAME frames run both: batch X gives every frame
one tracker set; batch Y is batch X except that frame 3 of every wave tracks seven joints, which sends the wave to the general loop.  Frames
0..2 of every wave are then compared array by array, as bytes.

The three tracker sets select the three compiled skip patterns: the reference's six trackers (the toes are dead: mode 1), its three (both
legs are dead: mode 2) and six with a toe instead of a foot (nothing to skip: mode 0).

Three kernels, one answer (BATCHES below): the same inputs through the plain call (dp_w4_bplv_kernel: a version per wave), through the call with
the debug dump (dp_w4_bp_kernel: the loop standing once) and through the dense layout (dp_w4_kernel, which tests/test_hip_instantiations.py holds to
the oracle at 256 / 257 / 300 iterations) must agree in every byte of every per-frame result, at 1 ... 300 iterations -- beyond 256 the LONG
kernels, whose Adam scalars come from adam_beyond inside the version's lambda -- on batches whose waves take unlike versions in one workgroup, whose
mode comes from the union of unlike frames, and whose last wave is ragged."""
import numpy as np
import pytest
import torch

from adam_reference import temporal_only  # tests/adam_reference.py
from instantiations import UNIT_W4, UNIT_W4_BP, UNIT_W4_BP_LV, Inst, last_launch, set_layout  # tests/instantiations.py
from oracle import ref_torch as R
from oracle.analytic import AnalyticOracle

pytestmark = pytest.mark.gpu

KEYS = ("z0", "z_tgt", "cur_rot", "tgt_pos", "tgt_rot", "w", "tracked")
PER_FRAME = ("z", "z_pre", "pose", "disp", "world_disp", "world_rot", "pos", "rot", "loss", "iters", "status")
TOE = 4  # the left toe: below the left foot (joint 3), item 4 of bL2's first skip pattern
SETS = {
    "six": dict(R.W6),                                                          # mode 1
    "three": dict(R.W3),                                                        # mode 2
    "toe": {**{j: w for j, w in R.W6.items() if j != 3}, TOE: R.W6[3]},         # mode 0
}
LAM = {"six": 0.02, "three": 0.15, "toe": 0.02}
SEVENTH = (10, 5, 9, 1)  # joints added to frame 3 of a wave until it tracks seven (none of them in any of the sets)
B = 20                   # five waves: one workgroup of four and a ragged one of one


def _batch(n, wtab, seed=977):
    """recipe S (oracle/ref_torch.py: synth_inputs) with any tracker set; `full` keeps the targets of EVERY joint"""
    m = R.OracleModel()
    b = R.synth_inputs(m, n, seed=seed)
    with torch.no_grad():
        mo, d = R.decoder_forward(m, torch.tensor(b["z_src"]))
        _, _, pos, rot, _ = R.pose_fk(m, mo, d, torch.tensor(b["cur_rot"]))
    full = dict(pos=pos.float().numpy(), rot=rot.reshape(n, R.NJ, 9).float().numpy())
    b["tracked"][:] = 0
    b["w"][:] = 0
    for j, wj in wtab.items():
        b["tracked"][:, j] = 1
        b["w"][:, j] = wj
    _retarget(b, full)
    return b, full


def _retarget(b, full):
    trk = b["tracked"].astype(bool)[..., None]
    b["tgt_pos"] = (full["pos"] * trk).astype(np.float32)
    b["tgt_rot"] = (full["rot"] * trk).astype(np.float32)


def _seven_on_frame_3(b, full):
    y = {k: b[k].copy() for k in KEYS}
    for f in range(3, len(y["z0"]), 4):
        for j in SEVENTH:
            if y["tracked"][f].sum() >= 7:
                break
            assert not y["tracked"][f, j]
            y["tracked"][f, j] = 1
            y["w"][f, j] = (5.0, 0.01)
        assert y["tracked"][f].sum() == 7
    _retarget(y, full)
    return y


@pytest.fixture(scope="module")
def opts():
    from dragposer_amd.optimizer import LatentOptimizer

    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    o = {dt: LatentOptimizer(device="cuda:0", weight_dtype=dt) for dt in ("fp32", "bf16")}
    yield o
    for x in o.values():  # (the three-way tests switch to the dense layout and back)
        set_layout(x, 1)
        x.close()


@pytest.fixture(scope="module")
def batches():
    out = {}
    for name, wtab in SETS.items():
        x, full = _batch(B, wtab)
        out[name] = (x, _seven_on_frame_3(x, full))
    return out


def _run(o, b, n_iter, lam, **kw):
    from dragposer_amd.optimizer import to_device_batch

    out = o.optimize(**to_device_batch({k: b[k] for k in KEYS}, o.device), n_iter=n_iter, lambda_tmp=lam, kernel="w4", outputs=PER_FRAME, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("n_iter", [1, 2, 3, 50])
@pytest.mark.parametrize("trackers", ["six", "three", "toe"])
def test_common_and_general_loop_give_the_same_bits(opts, batches, trackers, n_iter, dtype):
    x, y = batches[trackers]
    keep = np.array([f for f in range(B) if f % 4 != 3])
    assert (x["tracked"][keep] == y["tracked"][keep]).all() and (y["tracked"][3::4].sum(1) == 7).all() and (x["tracked"].sum(1) <= 6).all()
    ox, oy = _run(opts[dtype], x, n_iter, LAM[trackers]), _run(opts[dtype], y, n_iter, LAM[trackers])
    assert (ox["status"] == 0).all() and (oy["status"] == 0).all() and (ox["iters"] == n_iter).all()
    for k in PER_FRAME:
        a, b = np.ascontiguousarray(ox[k][keep]), np.ascontiguousarray(oy[k][keep])
        assert np.isfinite(a.astype(np.float64)).all(), k
        assert a.tobytes() == b.tobytes(), (k, np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    # (the seven-tracker frames did run: their result differs from the six-tracker twin's)
    assert not np.array_equal(ox["z"][3::4], oy["z"][3::4])


@pytest.mark.parametrize("trackers", ["six", "three", "toe"])
def test_each_version_against_the_c_oracle(opts, trackers):
    """16 frames x 3 iterations of one tracker set per skip pattern against the C restatement, at test_hip_parity.py's bar: 0.05 mm at
    every joint; latent, losses and iteration count beside it."""
    b, _ = _batch(16, SETS[trackers], seed=31)
    o = _run(opts["fp32"], b, 3, LAM[trackers])
    ref = AnalyticOracle(precision="f32").optimize(*[b[k] for k in KEYS], 3, lam_tmp=LAM[trackers])
    err = np.linalg.norm(o["pos"] - ref["pos"], axis=-1).max() * 1000.0
    print(f"{trackers}: max joint error against the C oracle {err:.5f} mm")
    assert err <= 0.05, err
    np.testing.assert_allclose(o["z"], ref["z_final"], atol=5e-5)
    np.testing.assert_allclose(o["loss"], ref["loss"], rtol=2e-3, atol=1e-8)
    assert (o["iters"] == 3).all()


def test_forward_only_launch_is_unchanged(opts):
    """dp_forward (dp_w4_bp.hip's kernel: the general loop alone, left after its first forward pass) on 5 frames against the C oracle, at
    test_hip_parity.py's tolerances"""
    dev = torch.device("cuda:0")
    b = R.synth_inputs(R.OracleModel(), 5)
    o = opts["fp32"].forward(torch.from_numpy(b["z_src"]).to(dev), torch.from_numpy(b["cur_rot"]).to(dev))
    torch.cuda.synchronize()
    f = AnalyticOracle(precision="f64").forward(b["z_src"], b["cur_rot"])
    assert (np.linalg.norm(o["pos"].cpu().numpy() - f["pos"], axis=-1) * 1000.0).max() < 0.005
    np.testing.assert_allclose(o["rot"].cpu().numpy(), f["rot"], atol=1e-5)
    np.testing.assert_allclose(o["world_rot"].cpu().numpy(), f["world_rot"], atol=2e-6)
    np.testing.assert_allclose(o["world_disp"].cpu().numpy(), f["world_disp"], atol=2e-7)
    np.testing.assert_allclose(o["pose"].cpu().numpy(), f["pose"], atol=1e-3)


def test_a_nan_target_in_a_common_wave(opts):
    """test_hip_status.py's expectations at 8 frames: frame 5's wave runs the common loop on the frame's neutral stand-ins -- the frame
    reports NONFINITE | BAD_TARGETS and returns NaN, its three wave-mates and the other wave keep their bits and a zero status"""
    ST_NONFINITE, ST_BAD_TARGETS = 1, 4
    b = R.synth_inputs(R.OracleModel(), 8, seed=4321)
    clean = _run(opts["fp32"], b, 50, 0.02)
    bad = {k: b[k].copy() for k in KEYS}
    bad["tgt_pos"][5, 13, 1] = float("nan")  # a tracked joint (left hand) of frame 5
    out = _run(opts["fp32"], bad, 50, 0.02)
    others = [f for f in range(8) if f != 5]
    for k in PER_FRAME:
        assert np.ascontiguousarray(out[k][others]).tobytes() == np.ascontiguousarray(clean[k][others]).tobytes(), k
    assert (out["status"][others] == 0).all() and (clean["status"] == 0).all()
    assert int(out["status"][5]) == ST_NONFINITE | ST_BAD_TARGETS
    assert np.isnan(out["z"][5]).all() and np.isnan(out["loss"][5]).all() and int(out["iters"][5]) == 50
    for k in ("pose", "pos", "rot", "world_rot", "disp", "z_pre"):  # fifty passes: the NaN latent of the second pass onwards decodes to NaN
        assert np.isnan(out[k][5]).all(), k


# ---------------------------------------------------------------- three kernels, one answer
# Which version a wave takes (dp_w4_impl.h, behind the set-up): the general loop when one of its four frames tracks more than six joints; else the common
# loop with bL2's skip mode, from the side-A items that are live in the UNION of the four frames' tracker masks -- an item is live when its joint, or
# a joint below it, is tracked.  B2_SKIP_2 = 0x1FE (items 1..8: both legs) all dead -> mode 2; else B2_SKIP_1 = 0x110 (items 4 and 8: the toes) dead
# -> mode 1; else mode 0.  Side-A item b of quads 0..8 is joint b (dp_w4.h: bp_item_of; dp_debug_w4_bp_layout).  `expected_versions` restates that
# from the skeleton's parents, and tests/test_adam_reference.py holds the versions written beside each batch below to it on the CPU.
B2_SKIP_1, B2_SKIP_2 = (1 << 4) | (1 << 8), 0x1FE
TOE_ALONE = {TOE: (5.0, 0.01)}
ROOT_ALONE = {0: (10.0, 10.0)}
NOTHING = {}
SEVEN = {**SETS["six"], SEVENTH[0]: (5.0, 0.01)}
SIX_ELSEWHERE = {0: (10.0, 10.0), 11: (5.0, 0.01), 13: (5.0, 0.01), 15: (5.0, 0.01), 17: (5.0, 0.01), 21: (5.0, 0.01)}  # none on or below a leg
SEVENTEEN = {j: (5.0, 0.01) for j in range(17)}
# name -> (tracker set per frame, the version every wave must take: 0 / 1 / 2 = the common loop with that skip mode, "general")
BATCHES = {
    # one workgroup whose four waves run the four versions, and a ragged fifth wave of two frames (its two clamped copies repeat the last valid
    # frame: the union, and so the mode, is that of `three`)
    "mixed_workgroup": ([SETS["six"]] * 4 + [SETS["three"]] * 4 + [SETS["toe"]] * 4 + [SETS["six"]] * 3 + [SEVEN] + [SETS["three"]] * 2,
                        (1, 2, 0, "general", 2)),
    # the union of unlike frames: the feet of ONE frame keep the legs alive for the wave (mode 1); one left toe takes both skip patterns away
    # (mode 0); the root alone and a frame that tracks nothing leave the legs dead (mode 2); nothing tracked at all (mode 2)
    "unlike_frames_in_a_wave": ([SETS["six"]] + [SETS["three"]] * 3 + [SETS["three"]] * 3 + [TOE_ALONE]
                                + [SETS["three"], ROOT_ALONE, NOTHING, SETS["three"]] + [NOTHING] * 4, (1, 0, 2, 2)),
    # mode 2 with six trackers per frame (Emax == 6); and the same frames with a 17-tracker frame in the second wave: stage T's second pass
    # inside the loop-version kernel's general loop
    "six_elsewhere": ([SIX_ELSEWHERE] * 8, (2, 2)),
    "six_elsewhere_17": ([SIX_ELSEWHERE] * 5 + [SEVENTEEN] + [SIX_ELSEWHERE] * 2, (2, "general")),
}
MIXED_SEED = 977  # (the f32 oracle's gradient is within test_hip_parity.py's bar of the f64 oracle's on every tracked frame of both batches with
                  #  this seed, the file's first: tests/test_adam_reference.py)
MIXED_LAM = 0.02


def expected_versions(tracked, parents):
    """the version each wave of a launch takes, from the rule above; a ragged wave's missing frames repeat its last one (same union)"""
    below = {j: {j} for j in range(len(parents))}  # joint -> itself and every joint below it
    for j in range(len(parents) - 1, 0, -1):
        below[int(parents[j])] |= below[j]
    out = []
    for f0 in range(0, len(tracked), 4):
        wave = tracked[f0:f0 + 4].astype(bool)
        if wave.sum(axis=1).max() > 6:
            out.append("general")
            continue
        union = set(np.nonzero(wave.any(axis=0))[0].tolist())
        live = sum(1 << b for b in range(9) if below[b] & union)
        out.append(2 if not live & B2_SKIP_2 else 1 if not live & B2_SKIP_1 else 0)
    return tuple(out)


_MIXED = {}


def mixed_batch(name, seed=MIXED_SEED):
    """a batch of BATCHES: recipe S with a tracker set per frame (computed once, shared, left unchanged)"""
    if (name, seed) not in _MIXED:
        recipes = BATCHES[name][0]
        b, full = _batch(len(recipes), {}, seed=seed)
        for f, wtab in enumerate(recipes):
            for j, wj in wtab.items():
                b["tracked"][f, j] = 1
                b["w"][f, j] = wj
        _retarget(b, full)
        _MIXED[name, seed] = {k: b[k] for k in KEYS}
    return _MIXED[name, seed]


def _three_routes(o, b, n_iter, dbg=None):
    """the batch through the loop-version kernel, dp_w4_bp.hip's kernel (debug dump) and the dense kernel, each asserted through dp_debug_last_launch"""
    lng = int(n_iter > 256)
    assert set_layout(o, 1) == 1
    lv = _run(o, b, n_iter, MIXED_LAM)
    assert last_launch(o) == Inst(UNIT_W4_BP_LV, 4, 0, 0, lng), last_launch(o)
    one = _run(o, b, n_iter, MIXED_LAM, _debug=dbg if dbg is not None else torch.zeros(len(b["z0"]), 240, device=o.device))
    assert last_launch(o) == Inst(UNIT_W4_BP, 4, 0, 0, lng), last_launch(o)
    assert set_layout(o, 0) == 0
    try:
        dense = _run(o, b, n_iter, MIXED_LAM)
        assert last_launch(o) == Inst(UNIT_W4, 4, 0, 0, lng), last_launch(o)
    finally:
        assert set_layout(o, 1) == 1
    return lv, one, dense


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("n_iter", [1, 2, 50, 256, 257, 300])
@pytest.mark.parametrize("name", list(BATCHES))
def test_three_kernels_one_answer(opts, name, n_iter, dtype):
    b = mixed_batch(name)
    lv, one, dense = _three_routes(opts[dtype], b, n_iter)
    assert (dense["status"] == 0).all() and (dense["iters"] == n_iter).all()
    for k in PER_FRAME:
        want = np.ascontiguousarray(dense[k])
        assert np.isfinite(want.astype(np.float64)).all(), k
        for route, got in (("loop versions", lv), ("debug dump", one)):
            got = np.ascontiguousarray(got[k])
            assert got.tobytes() == want.tobytes(), (name, n_iter, dtype, route, k, np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0])


@pytest.mark.parametrize("n_iter", [50, 300])
def test_a_frame_does_not_depend_on_the_version_of_its_wave(opts, n_iter):
    """six_elsewhere with and without the 17-tracker frame: the three wave-mates of that frame move from mode 2 to the general loop and keep their bits"""
    a, b = mixed_batch("six_elsewhere"), mixed_batch("six_elsewhere_17")
    keep = np.array([f for f in range(8) if f != 5])
    assert all(np.array_equal(a[k][keep], b[k][keep]) for k in KEYS) and b["tracked"][5].sum() == 17
    oa, ob = _run(opts["fp32"], a, n_iter, MIXED_LAM), _run(opts["fp32"], b, n_iter, MIXED_LAM)
    for k in PER_FRAME:
        assert np.ascontiguousarray(oa[k][keep]).tobytes() == np.ascontiguousarray(ob[k][keep]).tobytes(), k
    assert not np.array_equal(oa["z"][5], ob["z"][5])


@pytest.mark.parametrize("name", ["mixed_workgroup", "unlike_frames_in_a_wave"])
def test_mixed_waves_against_the_c_oracle(opts, name):
    """the loop-version kernel on a batch of unlike waves, 3 iterations against the C restatement at test_each_version_against_the_c_oracle's bars;
    a frame that tracks nothing (the oracle's mean over no tracker is 0 / 0) against the pull term alone, at test_hip_w4_early_reads.py's atol for
    one iteration -- three steps of at most lr each, formed to a few ulp of a latent of size 0.3, stay within it"""
    b = mixed_batch(name)
    o = _run(opts["fp32"], b, 3, MIXED_LAM)
    assert last_launch(opts["fp32"]) == Inst(UNIT_W4_BP_LV, 4, 0, 0, 0)
    ref = AnalyticOracle(precision="f32").optimize(*[b[k] for k in KEYS], 3, lam_tmp=MIXED_LAM)
    has = b["tracked"].sum(axis=1) > 0
    err = np.linalg.norm(o["pos"] - ref["pos"], axis=-1).max(axis=1) * 1000.0
    print(f"{name}: max joint error against the C oracle {err[has].max():.5f} mm on {int(has.sum())} tracked frames")
    assert err[has].max() <= 0.05, err
    np.testing.assert_allclose(o["z"][has], ref["z_final"][has], atol=5e-5)
    np.testing.assert_allclose(o["loss"][has], ref["loss"][has], rtol=2e-3, atol=1e-8)
    assert (o["iters"] == 3).all() and (o["status"] == 0).all()
    for f in np.nonzero(~has)[0]:
        np.testing.assert_allclose(o["z"][f], temporal_only(b, f, 3, lam=MIXED_LAM), atol=2e-6)
        assert (o["loss"][f, :2] == 0).all() and np.isfinite(o["pos"][f]).all()
    assert name == "mixed_workgroup" or (~has).sum() == 5


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["mixed_workgroup", "unlike_frames_in_a_wave"])
def test_first_gradient_of_the_kernel_left_to_the_debug_route(opts, name, dtype):
    """dp_w4_bp.hip's fixed-count kernel is reached through the debug dump alone: its dL/dz of the first iteration (columns 208:232 of the dump) on the
    frames that track something, against the f64 oracle's gradient at test_hip_parity.py's bar"""
    b = mixed_batch(name)
    o = opts[dtype]
    dbg = torch.zeros(len(b["z0"]), 240, device=o.device)
    assert set_layout(o, 1) == 1
    _run(o, b, 1, MIXED_LAM, _debug=dbg)
    assert last_launch(o) == Inst(UNIT_W4_BP, 4, 0, 0, 0)
    has = b["tracked"].sum(axis=1) > 0
    _, gr = AnalyticOracle(precision="f64", weight_rounding="bf16" if dtype == "bf16" else "none").grad(*[b[k][has] for k in KEYS], 1.0, MIXED_LAM)
    np.testing.assert_allclose(dbg.cpu().numpy()[has, 208:232], gr, atol=2e-6, rtol=2e-5)

"""GPU: the loop versions of the body-part fixed-count kernel (dp_w4_bp_lv.hip; dp_w4_impl.h, W4_LOOP_VERSIONS) against its general loop, bit for bit.

A wave of that kernel picks one version of the iteration loop behind its set-up: the common one (with the wave's bL2 skip pattern compiled in) when
it optimises and none of its four frames tracks more than six joints, the general one otherwise.  A frame's arithmetic does not depend on its
wave-mates (the transposes multiply the other frames' values with exact zeros, and bL2's skipped K-groups multiply exact zeros), so the same
frame must come out with the same bits whichever version its wave runs.  The test makes the SAME frames run both: batch X gives every frame
one tracker set; batch Y is batch X except that frame 3 of every wave tracks seven joints, which sends the wave to the general loop.  Frames
0..2 of every wave are then compared array by array, as bytes.

The three tracker sets select the three compiled skip patterns: the reference's six trackers (the toes are dead: mode 1), its three (both
legs are dead: mode 2) and six with a toe instead of a foot (nothing to skip: mode 0)."""
import numpy as np
import pytest
import torch

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
    return {dt: LatentOptimizer(device="cuda:0", weight_dtype=dt) for dt in ("fp32", "bf16")}


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

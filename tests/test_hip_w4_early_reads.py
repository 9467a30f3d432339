"""GPU (MI355X): dp_w4's kinematics with their LDS reads issued ahead of their waits (csrc/dp_w4_impl.h: W4_EARLY_READS), against the
C oracle (oracle.analytic.AnalyticOracle, fp32) at the smallest shapes at which the re-ordered reads can go wrong:

* stage T's reads now run in EVERY lane, from inside stage J: lanes without a tracker (a frame that tracks nothing, frames that track only
  the root: the QS_IDENT / WT_TRASH slots) must address their own frame block and store nothing;
* ragged launches (3 frames: one wave with a clamped copy; 17: a second workgroup of one frame);
* the paths that keep the old shape (stage G beyond 6 trackers, stage T's second pass beyond 16) in ONE wave, next to a 6-tracker wave of
  the same workgroup;
* one iteration (fp32 rounding, every frame), 50 at a fixed count and 50 under the while-condition (0.05 mm off flagged frames:
  tests/sensitivity.py), in both layouts of layer 2 and once through the per-frame-skeleton unit.

The seeds were chosen on the CPU so that the oracle's own fp32 / fp64 pair flags no frame of any case (a case may still leave out one)."""
import numpy as np
import pytest
import torch

from adam_reference import temporal_only  # tests/adam_reference.py: the latent of a frame that tracks nothing (lam = LAM is its default)
from oracle import ref_torch as R
from oracle.analytic import AnalyticOracle

pytestmark = pytest.mark.gpu

KEYS = ("z0", "z_tgt", "cur_rot", "tgt_pos", "tgt_rot", "w", "tracked")
LAM = 0.02
WHILE = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2, min_loss_incr=1e-5)
STD6 = -6  # a frame with the reference's six trackers and their weights
ROOT = -1  # a frame that tracks the root alone
# per-frame tracker counts (>= 0: that many joints, drawn; STD6; ROOT) and the seed of the draw
CASES = {
    "lanes_without_a_tracker": ([0, 1, 6, 22], 11),
    "root_only": ([ROOT] * 8, 12),
    "ragged_3": ([STD6] * 3, 13),
    "ragged_17": ([STD6] * 17, 14),
    "old_shape_paths": ([7, 16, 17, 22, STD6, STD6, STD6, STD6], 15),
}


def _mm(a, b):
    return np.linalg.norm(a - b, axis=-1) * 1000.0


def build_case(name):
    counts, seed = CASES[name]
    B = len(counts)
    m = R.OracleModel()
    b = R.synth_inputs(m, B, seed=seed)
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        mo, dd = R.decoder_forward(m, torch.tensor(b["z_src"]))
        _, _, pos, rot, _ = R.pose_fk(m, mo, dd, torch.tensor(b["cur_rot"]))
    b["tracked"][:] = 0
    b["w"][:] = 0
    for f, n in enumerate(counts):
        if n == STD6:
            for j, wj in R.W6.items():
                b["tracked"][f, j] = 1
                b["w"][f, j] = wj
            continue
        js = np.array([0]) if n == ROOT else np.sort(rs.permutation(22)[:n])
        b["tracked"][f, js] = 1
        b["w"][f, js, 0] = rs.uniform(1, 10, len(js))
        b["w"][f, js, 1] = rs.uniform(0.01, 2, len(js))
    trk = b["tracked"].astype(bool)[..., None]
    b["tgt_pos"] = (pos.numpy() * trk).astype(np.float32)
    b["tgt_rot"] = (rot.numpy().reshape(B, 22, 9) * trk).astype(np.float32)
    return b


_REF = {}


def reference(name, n_iter, early):
    """(batch, fp32 oracle, fp64 oracle) of a case: computed once, shared, never modified"""
    key = (name, n_iter, early)
    if key not in _REF:
        b = build_case(name)
        kw = WHILE if early else {}
        o = [AnalyticOracle(precision=p).optimize(*[b[k] for k in KEYS], n_iter, lam_tmp=LAM, **kw) for p in ("f32", "f64")]
        for r in o:
            for v in r.values():
                v.setflags(write=False)
        _REF[key] = (b, o[0], o[1])
    return _REF[key]


def flagged_frames(b, r32, r64):
    """frames on which the oracle's own fp32 and fp64 runs part ways (the project's rule), among the frames that track something"""
    has = b["tracked"].sum(axis=1) > 0
    return has & ((_mm(r32["pos"], r64["pos"]).max(axis=1) > 0.02) | (r32["iters"] != r64["iters"]))


@pytest.fixture(scope="module")
def opt():
    from dragposer_amd.optimizer import LatentOptimizer
    from instantiations import set_layout  # tests/instantiations.py

    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    o = LatentOptimizer(device=torch.device("cuda:0"))
    yield o
    set_layout(o, 1)
    o.close()


def _run(opt, b, bp, n_iter, early, skeleton=False):
    from dragposer_amd.optimizer import to_device_batch
    from instantiations import UNIT_W4, UNIT_W4_BP, UNIT_W4_BP_LV, last_launch, set_layout
    from skeleton_cases import UNIT_W4_BP_SKEL, UNIT_W4_SKEL  # tests/skeleton_cases.py

    assert set_layout(opt, bp) == bp
    kw = dict(WHILE) if early else {}
    if skeleton:  # the context's own skeleton, passed per frame: the per-frame-skeleton unit on the oracle's model
        base = np.asarray(np.load(R.DEFAULT_MODEL)["offsets"], np.float32)
        kw["offsets"] = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(base, (len(b["z0"]), 22, 3)))).cuda()
    out = opt.optimize(**to_device_batch(b, opt.device), n_iter=n_iter, lambda_tmp=LAM, kernel="w4", **kw)
    torch.cuda.synchronize()
    ran = last_launch(opt)
    assert ran.unit == ((UNIT_W4_BP_SKEL if bp else UNIT_W4_SKEL) if skeleton else ((UNIT_W4_BP if early else UNIT_W4_BP_LV) if bp else UNIT_W4)) and ran.early == int(early), ran
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert (out["status"] == 0).all()
    return out


def _check_untracked(b, o, n_iter, ztol):
    """a frame that tracks nothing: only the temporal term moves it, and its tracker losses are exactly zero"""
    for f in np.nonzero(b["tracked"].sum(axis=1) == 0)[0]:
        np.testing.assert_allclose(o["z"][f], temporal_only(b, f, n_iter), atol=ztol)
        assert (o["loss"][f, :2] == 0).all() and np.isfinite(o["pos"][f]).all()


def _check_one_iteration(b, r32, o):
    """the tolerances of tests/test_hip_w4.py::test_first_step_and_forward_agree_tightly, no frame left out"""
    has = b["tracked"].sum(axis=1) > 0  # (the oracle's mean over zero trackers is 0/0, like the reference's)
    np.testing.assert_allclose(o["z"][has], r32["z_final"][has], atol=2e-6)
    for k, tol in (("pos", 2e-6), ("rot", 5e-6), ("world_rot", 2e-6), ("world_disp", 2e-7), ("loss", 1e-6)):
        np.testing.assert_allclose(o[k][has], r32[k][has], atol=tol, rtol=2e-5, err_msg=k)
    np.testing.assert_allclose(o["pose"][has], r32["pose"][has], atol=2e-3)  # normalised space (/sigma ~ 1700x)
    assert (o["iters"] == 1).all()
    _check_untracked(b, o, 1, 2e-6)


def _check_fifty(name, b, r32, r64, o, early):
    has = b["tracked"].sum(axis=1) > 0
    flagged = flagged_frames(b, r32, r64)
    err = _mm(o["pos"], r32["pos"]).max(axis=1)
    print(f"{name} early={early}: flagged {np.nonzero(flagged)[0].tolist()}, max error off them {err[has & ~flagged].max():.4f} mm, "
          f"iterations {o['iters'].tolist()} (oracle {r32['iters'].tolist()})")
    assert flagged.sum() <= 1
    cmp = has & ~flagged
    assert err[cmp].max() <= 0.05
    np.testing.assert_array_equal(o["iters"][cmp], r32["iters"][cmp])
    np.testing.assert_allclose(o["loss"][cmp], r32["loss"][cmp], rtol=2e-3, atol=1e-8)
    assert np.isfinite(o["z"]).all() and np.isfinite(o["loss"]).all()
    if not early:
        _check_untracked(b, o, 50, 5e-5)


@pytest.mark.parametrize("bp", [1, 0], ids=["body_part", "dense"])
@pytest.mark.parametrize("name", list(CASES))
def test_one_iteration_matches_the_oracle_on_every_frame(opt, name, bp):
    b, r32, _ = reference(name, 1, False)
    _check_one_iteration(b, r32, _run(opt, b, bp, 1, False))


@pytest.mark.parametrize("early", [False, True], ids=["fixed_count", "while_condition"])
@pytest.mark.parametrize("bp", [1, 0], ids=["body_part", "dense"])
@pytest.mark.parametrize("name", list(CASES))
def test_fifty_iterations_match_the_oracle(opt, name, bp, early):
    b, r32, r64 = reference(name, 50, early)
    _check_fifty(name, b, r32, r64, _run(opt, b, bp, 50, early), early)


@pytest.mark.parametrize("bp", [1, 0], ids=["body_part", "dense"])
def test_the_per_frame_skeleton_unit_compiles_the_same_stages(opt, bp):
    """dp_w4_skel.hip / dp_w4_bp_skel.hip include the same header: the wave with lanes without a tracker and the old-shape paths through them"""
    for name in ("lanes_without_a_tracker", "old_shape_paths"):
        b, r32, _ = reference(name, 1, False)
        _check_one_iteration(b, r32, _run(opt, b, bp, 1, False, skeleton=True))
        b, r32, r64 = reference(name, 50, False)
        _check_fifty(name, b, r32, r64, _run(opt, b, bp, 50, False, skeleton=True), False)

"""GPU: libDragPoserDLL.so's additions (include/dragposer_unity.h) -- terms, holds, gaps and the latent AR predictor in the plug-in's live
step -- against DragPose.run(terms=, holds=, ar=, gaps=, present=), the two-launch route, driven with the same targets.  40 frames, 6
trackers, the reference's six-row constraint table plus two held pins, a damped constant-velocity predictor, Gaps(5, 0.9); one hand is
blanked for 8 frames through `present` and another joint for 3 frames through NaN -- the input that ends a session without the gaps.
The latent, the iteration counts, the status words, the gap codes and the hold rows are compared exactly: both sides run the same
instructions on the same inputs.  The returned pose and position go through different host arithmetic (C++ float against numpy double) and
are held to test_unity_abi.py's own bars."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from test_unity_abi import CLIP, DATA, F2, F3, Qt, _load

pytestmark = pytest.mark.gpu

T, DAMPING = 40, 0.6
HELD_BIT, LOST_BIT = 16, 32


def _exact_quaternions():
    """the 24 unit quaternions with components in {0, +-1} or all +-1/2: every product in their rotation matrices is 0, 1/4 or 1 and the
    entries are 0 and +-1 whatever the order of evaluation, so the plug-in's float qmat and numpy's double to_matrix hand over identical targets"""
    q = []
    for i in range(4):
        for s in (1.0, -1.0):
            v = [0.0] * 4
            v[i] = s
            q.append(v)
    q += [list(v) for v in itertools.product((0.5, -0.5), repeat=4)]
    return np.array(q)


def _bind(lib):
    from dragposer_amd import _lib as L

    lib.drag_poser_set_terms.argtypes = [C.c_void_p, C.c_int, C.POINTER(L.DpTerm), C.c_int]
    lib.drag_poser_set_holds.argtypes = [C.c_void_p, C.c_int, C.POINTER(L.DpHold)]
    lib.drag_poser_set_gaps.argtypes = [C.c_void_p, C.c_int, C.c_float]
    lib.drag_poser_set_latent_ar.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.drag_pose_present.argtypes = [C.c_void_p, C.c_int, C.POINTER(F3), C.POINTER(Qt), C.POINTER(C.c_ubyte), C.POINTER(Qt), C.POINTER(F3)]
    lib.drag_poser_last_status.argtypes = [C.c_void_p]
    lib.drag_poser_get_gap_codes.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte)]
    lib.drag_poser_get_hold_state.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    return lib


def _handle(lib, cr0):
    h = lib.init_drag_poser()
    lib.set_reference_skeleton(h, CLIP.encode())
    lib.load_models(h, DATA.encode())
    assert lib.drag_poser_last_error(h) == b"", lib.drag_poser_last_error(h)
    mask = np.zeros(22, np.float32)
    mask[R.TRACK6] = 1
    w = np.ones((22, 2), np.float32)
    for j, wj in R.W6.items():
        w[j] = wj
    lib.set_mask_and_weights(h, mask.ctypes.data_as(C.POINTER(C.c_float)), w.ctypes.data_as(C.POINTER(F2)))
    lib.set_optim_params(h, 1e-4, 1e-2, 10, 1e-2)
    lib.init_drag_model(h, F3(0.1, 0.2, 0.3), Qt(*[float(v) for v in cr0]))
    return h


def _table():
    from dragposer_amd import Constraints
    from dragposer_amd.terms import Term, Terms

    ref = Terms.from_constraints(Constraints.reference())
    assert len(ref) == 6
    pins = [Term.distance(4, point=(0.0, 0.0, 0.0), lo=0.0, hi=0.0, weight=0.8, drop_up=True),
            Term.distance(8, point=(0.0, 0.0, 0.0), lo=0.0, hi=0.02, weight=0.6)]
    return Terms(ref.terms + pins, ref.up_axis)


def _inputs():
    m = R.OracleModel()
    b = R.synth_inputs(m, T, seed=5)
    idx = np.array(R.TRACK6)
    quats = _exact_quaternions()
    assert quats.shape == (24, 4)
    g = np.random.default_rng(3)
    tq = quats[g.integers(0, 24, size=(T, 6))]
    tp = b["tgt_pos"][:, idx].astype(np.float32).copy()
    present = np.ones((T, 6), np.uint8)
    present[10:18, list(idx).index(17)] = 0                 # one hand blanked for 8 frames: held 5, lost 3
    tp[25:28, list(idx).index(13), 2] = np.float32("nan")   # another joint for 3 frames through a NaN component
    return b, idx, tp, tq, present


def _configure(lib, h, table, holds, ar, gaps):
    arr = (type(table.terms[0].to_struct()) * len(table))(*[t.to_struct() for t in table.terms])
    lib.drag_poser_set_terms(h, len(table), arr, table.up_axis)
    assert lib.drag_poser_last_error(h) == b"", lib.drag_poser_last_error(h)
    from dragposer_amd import _lib as L

    harr = (L.DpHold * len(holds.holds))(*[L.DpHold(term=x.term, level=x.level, contact_lo=x.contact_lo, contact_hi=x.contact_hi) for x in holds.holds])
    lib.drag_poser_set_holds(h, len(holds.holds), harr)
    assert lib.drag_poser_last_error(h) == b"", lib.drag_poser_last_error(h)
    A, c = np.ascontiguousarray(ar.A, np.float32), np.ascontiguousarray(ar.c, np.float32)
    lib.drag_poser_set_latent_ar(h, ar.order, A.ctypes.data_as(C.POINTER(C.c_float)), c.ctypes.data_as(C.POINTER(C.c_float)))
    assert lib.drag_poser_last_error(h) == b"", lib.drag_poser_last_error(h)
    if gaps is not None:
        lib.drag_poser_set_gaps(h, gaps.max_hold, gaps.decay)
        assert lib.drag_poser_last_error(h) == b"", lib.drag_poser_last_error(h)


@pytest.mark.parametrize("gaps_set", (True, False))
def test_the_plugin_equals_the_operator_through_dropouts(gaps_set):
    from dragposer_amd import Gaps, Hold, Holds, LatentAR
    from dragposer_amd import quat_np as Q
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.optimizer import LatentOptimizer

    lib = _bind(_load())
    b, idx, tp, tq, present = _inputs()
    cr0 = b["cur_rot"][0]
    table, holds, ar = _table(), Holds([Hold(6, 0.0, 0.1, level=10.0), Hold(7, 0.0, 0.1, level=10.0)]), LatentAR.constant_velocity(DAMPING)
    gaps = Gaps(5, 0.9) if gaps_set else Gaps(0, 1.0)  # never set: max_hold 0, decay 1
    h = _handle(lib, cr0)
    _configure(lib, h, table, holds, ar, gaps if gaps_set else None)
    lib.set_lambdas(h, 1.0, 0.02, 0)
    assert lib.drag_poser_last_error(h) == b""  # a predictor is configured: lambdaTemporal takes effect, nothing to report
    z0 = np.zeros(24, np.float32)
    lib.drag_poser_get_latent(h, z0.ctypes.data_as(C.POINTER(C.c_float)))

    opt = LatentOptimizer(device="cuda:0")
    dp = DragPose(opt, None, np.zeros(24), np.ones(24), n_sequences=1)
    dp.set_initial_state(z0, np.array([0.1, 0.2, 0.3], np.float32), cr0, np.zeros(6))
    wj = np.array([R.W6[j] for j in R.TRACK6], np.float32)
    raw = np.load(R.DEFAULT_MODEL)
    statuses = []
    for t in range(T):
        res_pose, res_pos = (Qt * 22)(), (F3 * 1)()
        prs = (C.c_ubyte * 6)(*present[t].tolist())
        lib.drag_pose_present(h, 6, (F3 * 6)(*[F3(*map(float, p)) for p in tp[t]]), (Qt * 6)(*[Qt(*map(float, q)) for q in tq[t]]), prs, res_pose, res_pos)
        assert lib.drag_poser_last_error(h) == b"", (t, lib.drag_poser_last_error(h))
        pose, gpos = dp.run(torch.tensor(tp[t]), torch.tensor(Q.to_matrix(tq[t]).astype(np.float32)), idx, wj, stop_eps_pos=1e-4, stop_eps_rot=1e-2,
                            max_iter=10, learning_rate=1e-2, lambda_rot=1.0, lambda_temporal=0.02, temporal_future_window=0, terms=table, holds=holds,
                            ar=ar, gaps=gaps, present=torch.tensor(present[t][None]))
        z = np.zeros(24, np.float32)
        lib.drag_poser_get_latent(h, z.ctypes.data_as(C.POINTER(C.c_float)))
        assert np.array_equal(z, dp.latent[0].cpu().numpy()), t
        assert lib.drag_poser_last_iterations(h) == int(dp.last["iters"][0]), t
        assert lib.drag_poser_last_status(h) == int(dp.last["status"][0]), t
        statuses.append(lib.drag_poser_last_status(h))
        codes = (C.c_ubyte * 22)()
        lib.drag_poser_get_gap_codes(h, codes)
        assert list(codes) == dp.last["gap_trace"][0].cpu().tolist(), t
        rows = (C.c_float * 8)()
        lib.drag_poser_get_hold_state(h, rows)
        assert np.array_equal(np.array(rows, np.float32).reshape(2, 4), dp.hold_state[0].cpu().numpy()), t
        np.testing.assert_allclose([res_pos[0].x, res_pos[0].y, res_pos[0].z], gpos.cpu().numpy(), atol=1e-6)
        qs = (pose.cpu().numpy().astype(np.float64) * opt.host_model.arrays["std_q"] + opt.host_model.arrays["mean_q"]).reshape(1, 22, 4)
        got = np.array([[q.w, q.x, q.y, q.z] for q in res_pose])
        np.testing.assert_allclose(got, Q.from_root_space(qs, raw["parents"])[0], atol=2e-6)
    # the session lived through both dropouts, and they were what the script says
    assert np.isfinite(z).all() and not any(s & (1 | 2 | 4) for s in statuses)
    if gaps_set:
        assert [s & (HELD_BIT | LOST_BIT) for s in statuses[10:18]] == [HELD_BIT] * 5 + [LOST_BIT] * 3
        assert [s & (HELD_BIT | LOST_BIT) for s in statuses[25:28]] == [HELD_BIT] * 3
    else:
        assert [s & (HELD_BIT | LOST_BIT) for s in statuses[10:18]] == [LOST_BIT] * 8 and [s & LOST_BIT for s in statuses[25:28]] == [LOST_BIT] * 3
    assert dp.hold_state[0, :, 3].tolist() == [1.0, 1.0]
    lib.destroy_drag_poser(h)


def test_a_table_the_library_refuses_surfaces_at_the_next_frame_and_commits_nothing():
    from dragposer_amd import _lib as L

    lib = _bind(_load())
    b, idx, tp, tq, present = _inputs()
    h = _handle(lib, b["cur_rot"][0])
    frame = lambda t, pose, pos: lib.drag_pose(h, 6, (F3 * 6)(*[F3(*map(float, p)) for p in tp[t]]), (Qt * 6)(*[Qt(*map(float, q)) for q in tq[t]]), pose, pos)
    res_pose, res_pos = (Qt * 22)(), (F3 * 1)()
    frame(0, res_pose, res_pos)
    assert lib.drag_poser_last_error(h) == b""
    z0, z1 = np.zeros(24, np.float32), np.zeros(24, np.float32)
    lib.drag_poser_get_latent(h, z0.ctypes.data_as(C.POINTER(C.c_float)))
    bad = (L.DpTerm * 1)(L.DpTerm(type=L.DP_TERM_PLANE, joint_a=22, weight=1.0))  # joint_a outside 0..21: dp_terms' own check, at the launch
    lib.drag_poser_set_terms(h, 1, bad, 1)
    assert lib.drag_poser_last_error(h) == b""
    pose2, pos2 = (Qt * 22)(), (F3 * 1)()
    frame(1, pose2, pos2)
    assert b"term 0" in lib.drag_poser_last_error(h)
    lib.drag_poser_get_latent(h, z1.ctypes.data_as(C.POINTER(C.c_float)))
    assert np.array_equal(z0, z1) and bytes(pose2) == bytes((Qt * 22)()) and lib.drag_poser_last_status(h) == 0  # nothing committed, nothing returned
    lib.drag_poser_set_terms(h, 0, None, 1)  # cleared: the frame is a live step with an empty table, and the session goes on
    frame(1, pose2, pos2)
    assert lib.drag_poser_last_error(h) == b""
    lib.drag_poser_get_latent(h, z1.ctypes.data_as(C.POINTER(C.c_float)))
    assert not np.array_equal(z0, z1) and np.isfinite(z1).all()
    codes = (C.c_ubyte * 22)()
    lib.drag_poser_get_gap_codes(h, codes)
    assert [j for j in range(22) if codes[j] == 1] == sorted(R.TRACK6) and set(codes) == {0, 1}
    lib.destroy_drag_poser(h)


def test_a_handle_with_nothing_configured_is_the_plain_call():
    """the same frames through a handle that never saw a setter and through one whose setters were all refused: identical results, and the
    frame that carries a NaN ends both sessions as before"""
    lib = _bind(_load())
    b, idx, tp, tq, present = _inputs()
    cr0 = b["cur_rot"][0]
    a, c = _handle(lib, cr0), _handle(lib, cr0)
    lib.drag_poser_set_gaps(c, -1, 0.5)
    assert b"maxHold" in lib.drag_poser_last_error(c)
    lib.drag_poser_set_terms(c, 1, None, 1)
    assert b"NULL terms" in lib.drag_poser_last_error(c)
    for t in range(12):
        out = []
        for h in (a, c):
            res_pose, res_pos = (Qt * 22)(), (F3 * 1)()
            lib.drag_pose(h, 6, (F3 * 6)(*[F3(*map(float, p)) for p in tp[t]]), (Qt * 6)(*[Qt(*map(float, q)) for q in tq[t]]), res_pose, res_pos)
            assert lib.drag_poser_last_error(h) == b""
            z = np.zeros(24, np.float32)
            lib.drag_poser_get_latent(h, z.ctypes.data_as(C.POINTER(C.c_float)))
            out.append((z.tobytes(), bytes(res_pose), bytes(res_pos), lib.drag_poser_last_iterations(h), lib.drag_poser_last_status(h)))
        assert out[0] == out[1] and out[0][4] == 0, t
    res_pose, res_pos = (Qt * 22)(), (F3 * 1)()
    prs = (C.c_ubyte * 6)(1, 1, 1, 1, 1, 1)
    lib.drag_pose_present(a, 6, (F3 * 6)(*[F3(*map(float, p)) for p in tp[12]]), (Qt * 6)(*[Qt(*map(float, q)) for q in tq[12]]), prs, res_pose, res_pos)
    assert b"present" in lib.drag_poser_last_error(a)  # `present` belongs to the gaps: nothing is configured on this handle
    lib.drag_pose(a, 6, (F3 * 6)(*[F3(*map(float, p)) for p in tp[25]]), (Qt * 6)(*[Qt(*map(float, q)) for q in tq[25]]), res_pose, res_pos)
    assert lib.drag_poser_last_status(a) & 4  # DP_STATUS_BAD_TARGETS: the plain call still refuses a NaN sample
    for h in (a, c):
        lib.destroy_drag_poser(h)

"""CPU: dragposer_amd.Tether / Tethers (include/dragposer_tethers.h) -- what check() refuses, in the header's order, and the update rule
on hand-written states: torch fp32 on the CPU, every expected value computed here with numpy float32 one rounding at a time."""
import numpy as np
import pytest
import torch

from dragposer_amd import Hold, Holds, Tether, Tethers
from dragposer_amd.terms import Term, Terms

F = np.float32


def _table(w_knee=0.6):
    return Terms([Term.plane(4, (0.0, 1.0, 0.0)), Term.distance(3, 7, lo=0.1, hi=0.3),
                  Term.distance(8, point=(0.0, 0.0, 0.0), weight=0.8, drop_up=True),
                  Term.distance(6, point=(0.0, 0.0, 0.0), lo=0.0, hi=0.02, weight=w_knee),
                  Term.distance(19, point=(0.0, 0.0, 0.0), weight=0.8),
                  Term.distance(5, per_frame=torch.zeros(2, 4))])


def test_check_refuses_what_the_header_lists():
    table = _table()
    Tethers([Tether(3), Tether(4, 1.0)]).check(table, Holds([Hold(2, 0.0, 0.1)]))
    Tethers([]).check(table)
    Tether(3, 0.5).check(table)
    for tether, word in ((Tether(-1), "term -1 outside the table of 6"), (Tether(6), "term 6 outside the table of 6"),
                         (Tether(0), "term 0 is not a DISTANCE term"), (Tether(1), "term 1 has a joint_b"),
                         (Tether(5), "term 5 has a per_frame array"), (Tether(3, -0.1), "alpha"), (Tether(3, 1.5), "alpha"),
                         (Tether(3, float("nan")), "alpha"), (Tether(3, float("inf")), "alpha")):
        with pytest.raises(ValueError, match="tether 0: " + word):
            tether.check(table)
        with pytest.raises(ValueError, match="tether 1: " + word):
            Tethers([Tether(4), tether]).check(table)
    with pytest.raises(ValueError, match="at most 4 tethers, got 5"):
        Tethers([Tether(3)] * 5).check(table)
    with pytest.raises(ValueError, match="tether 1: term 3 is already tethered by tether 0"):
        Tethers([Tether(3), Tether(3)]).check(table)
    with pytest.raises(ValueError, match="tether 1: term 2 is held by hold 0"):
        Tethers([Tether(3), Tether(2)]).check(table, Holds([Hold(2, 0.0, 0.1)]))
    with pytest.raises(ValueError, match="tether 0: term 0 is not a DISTANCE term"):  # (the term's rules come before alpha)
        Tethers([Tether(0, 2.0)]).check(table)
    with pytest.raises(ValueError, match="tether 0: alpha"):                          # (a tether's own checks before the next tether's)
        Tethers([Tether(3, 2.0), Tether(3)]).check(table)


def _frame(S=4):
    """joint positions and an advanced global position with fp32 values that round in every operation"""
    g = torch.Generator().manual_seed(3)
    return torch.randn(S, 22, 3, generator=g) * 0.37, torch.randn(S, 3, generator=g) * 1.3


def _world(pos, gpos, joint):
    p, gp = pos.numpy(), gpos.numpy()
    return (gp + (p[:, joint] - p[:, 0]).astype(F)).astype(F)


def test_update_first_frame_extrapolation_refusal_and_the_inert_tether():
    table, tethers = _table(), Tethers([Tether(3, 0.0), Tether(4, 0.75)])
    pos, gpos = _frame()
    state = tethers.new_state(4, "cpu")
    assert tuple(state.shape) == (4, 2, 8) and not state.any()
    # the first frame: have = 0, the point is W itself, whatever alpha
    tethers.update(table, state, pos, gpos)
    for k, j in ((0, 6), (1, 19)):
        W = _world(pos, gpos, j)
        assert np.array_equal(state[:, k, :3].numpy(), W) and np.array_equal(state[:, k, 4:7].numpy(), W)
        assert bool((state[:, k, 3] == 1).all()) and bool((state[:, k, 7] == 1).all())
    # the second frame: point = W + alpha * (W - Wprev), add(mul(sub)), each rounded to fp32
    before = state.clone()
    pos2, gpos2 = pos + 0.013, gpos * 1.01
    tethers.update(table, state, pos2, gpos2)
    for k, j, alpha in ((0, 6, F(0.0)), (1, 19, F(0.75))):
        W, Wp = _world(pos2, gpos2, j), before[:, k, 4:7].numpy()
        point = (W + (alpha * (W - Wp).astype(F)).astype(F)).astype(F)
        assert np.array_equal(state[:, k, :3].numpy(), point) and np.array_equal(state[:, k, 4:7].numpy(), W)
    assert np.array_equal(state[:, 0, :3].numpy(), state[:, 0, 4:7].numpy())      # alpha 0: the last position
    assert not np.array_equal(state[:, 1, :3].numpy(), state[:, 1, 4:7].numpy())  # alpha 0.75: ahead of it
    # a frame whose W is NaN, infinite or beyond DP_INPUT_LIMIT in one component leaves that sequence's state as it was
    before = state.clone()
    pos3, gpos3 = pos2.clone(), gpos2.clone()
    pos3[0, 6, 1] = float("nan")      # sequence 0: the knee alone
    gpos3[1, 2] = float("inf")        # sequence 1: both joints
    gpos3[2, 0] = 1.0001e4            # sequence 2: finite, beyond the limit
    tethers.update(table, state, pos3, gpos3)
    assert torch.equal(state[0, 0], before[0, 0]) and not torch.equal(state[0, 1], before[0, 1])
    assert torch.equal(state[1], before[1]) and torch.equal(state[2], before[2])
    assert not torch.equal(state[3], before[3]) and bool(torch.isfinite(state).all())
    # a joint 0 that is NaN: every W of that sequence is
    pos4 = pos2.clone()
    pos4[3, 0, 0] = float("nan")
    before = state.clone()
    tethers.update(table, state, pos4, gpos2)
    assert torch.equal(state[3], before[3])
    # the inert tether: weight 0, its rows are not touched
    inert = _table(w_knee=0.0)
    state = torch.full((4, 2, 8), -7.5e8)
    tethers.update(inert, state, pos, gpos)
    assert bool((state[:, 0] == -7.5e8).all()) and np.array_equal(state[:, 1, 4:7].numpy(), _world(pos, gpos, 19))
    assert not inert.terms[3].active and tethers.frame_terms(inert, state).terms[3].per_frame is None


def test_frame_terms_hands_the_rows_over():
    table, tethers = _table(), Tethers([Tether(3), Tether(4, 1.0)])
    state = torch.arange(4 * 2 * 8, dtype=torch.float32).reshape(4, 2, 8)
    ft = tethers.frame_terms(table, state)
    assert torch.equal(ft.terms[3].per_frame, state[:, 0, :4]) and torch.equal(ft.terms[4].per_frame, state[:, 1, :4])
    assert ft.terms[3].per_frame.is_contiguous() and table.terms[3].per_frame is None and ft.terms[0] is table.terms[0]
    state[0, 0, 0] = -1.0
    assert float(ft.terms[3].per_frame[0, 0]) == 0.0  # a copy: the frame reads the state as it stood before the step


def test_the_jitter_metric_on_a_hand_computed_example():
    """three joints, five frames: joint 0 stands still and joint 1 moves on a line at constant speed (second difference 0); joint 2 leaves
    the origin for (3, 4, 0) at frame 2 alone: |W(t+1) - 2 W(t) + W(t-1)| = 5, 10, 5 at t = 1, 2, 3 -- the mean over 3 frames x 3 joints is
    20 / 9; with joint 1 on x = t^2 instead (second difference 2 at every inner frame) it is 26 / 9"""
    from dragposer_amd.eval_drag import motion_jitter, parse_tethers, tether_terms

    w = np.zeros((5, 3, 3))
    w[:, 0] = (0.5, -1.0, 2.0)
    w[:, 1, 1] = 0.25 * np.arange(5)
    w[2, 2] = (3.0, 4.0, 0.0)
    assert motion_jitter(w) == pytest.approx(20.0 / 9.0, rel=1e-12)
    w[:, 1, 1] = np.arange(5) ** 2
    assert motion_jitter(w) == pytest.approx(26.0 / 9.0, rel=1e-12)
    assert motion_jitter(w[:3]) == pytest.approx((0.0 + 2.0 + 5.0) / 3.0, rel=1e-12) and np.isnan(motion_jitter(w[:2]))
    assert motion_jitter(w + 7.0) == pytest.approx(26.0 / 9.0, rel=1e-12)  # a translation does not change it
    # the command line's J:HI:WEIGHT[:ALPHA] and the table it builds
    specs = parse_tethers(["5:0.02:1", "19:0:0.1:1"])
    assert specs == [(5, 0.02, 1.0, 0.0), (19, 0.0, 0.1, 1.0)]
    terms, tethers = tether_terms(specs, Terms([Term.plane(4, (0.0, 1.0, 0.0))]))
    tethers.check(terms)
    assert [(t.term, t.alpha) for t in tethers.tethers] == [(1, 0.0), (2, 1.0)]
    assert [(t.joint_a, t.joint_b, t.p0, t.p1, t.weight) for t in terms.terms[1:]] == [(5, -1, 0.0, 0.02, 1.0), (19, -1, 0.0, 0.0, 0.1)]
    for bad in (["5:0.02"], ["22:0:1"], ["5:-1:1"], ["5:0:1:2"], ["5:x:1"], ["1:0:1"] * 5):
        with pytest.raises(SystemExit):
            parse_tethers(bad)

"""CPU: dragposer_amd.Gaps.step, the rule of include/dragposer_gaps.h in elementwise torch, against a plain numpy float32 loop over
(sequence, joint) that follows the header line by line.  A 40-step script per joint covers: present throughout; held to exactly max_hold
and expiring one step later; returning; absent from step 0 with a zero state; a sample with one Inf component and present = 1; present = 0
with a garbage sample; a value beyond DP_INPUT_LIMIT; a joint that is not tracked.  Run with max_hold = 3 / decay = 0.7, max_hold = 0, and
decay = 1.  Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

from dragposer_amd import Gaps
from dragposer_amd.gaps import HELD, LOST, PRESENT

T, S, NJ = 40, 3, 22
F = np.float32
LIMIT = F(1.0e4)


def _script(seed=5):
    """targets, weights, the tracker set, the global positions and `present` of 40 steps; what each joint's script is for is said inline"""
    g = np.random.default_rng(seed)
    tp = g.standard_normal((T, S, NJ, 3)).astype(F)
    tr = g.standard_normal((T, S, NJ, 9)).astype(F)
    w = (0.5 + g.random((S, NJ, 2))).astype(F)
    gpos = g.standard_normal((T, S, 3)).astype(F)
    tracked = np.ones((S, NJ), np.uint8)
    tracked[:, 5] = 0                                  # joint 5: not tracked by configuration (its samples are NaN and never looked at)
    tp[:, :, 5] = np.nan
    present = np.ones((T, S, NJ), np.uint8)
    present[10:14, :, 1] = 0                           # joint 1: absent for 4 steps (max_hold 3: held 3, lost 1), returns at 14
    present[20:23, :, 1] = 0                           # ... and for exactly 3 (held to exactly max_hold, never lost)
    present[0:6, :, 2] = 0                             # joint 2: absent from step 0 with a zero state: lost until it appears at 6
    tp[8, :, 3, 1] = np.inf                            # joint 3: one Inf component with present = 1
    tr[9, :, 3, 4] = np.nan                            # ... and a NaN rotation component the step after
    present[15:18, :, 4] = 0                           # joint 4: present = 0 with a garbage sample
    tp[15:18, :, 4] = F(3.0e38)
    tr[15:18, :, 4] = np.nan
    tp[25, :, 6, 2] = F(1.0001e4)                      # joint 6: beyond DP_INPUT_LIMIT (finite)
    tp[26, :, 6, 0] = F(-1.0e4)                        # ... and exactly at it: accepted
    present[30:40, 1, :] = 0                           # sequence 1: every tracker gone for the last 10 steps
    return tp, tr, w, tracked, gpos, present


def _numpy_rule(max_hold, decay, tp, tr, w, tracked, gpos, present):
    """the header, one (s, j) at a time, every operation a float32 one"""
    state = np.zeros((S, NJ, 16), F)
    out = dict(tp=np.zeros_like(tp), tr=np.zeros_like(tr), w=np.zeros((T, S, NJ, 2), F), on=np.zeros((T, S, NJ), np.uint8),
               code=np.zeros((T, S, NJ), np.uint8), state=np.zeros((T, S, NJ, 16), F))
    refused = lambda x: not (np.abs(x) <= LIMIT)
    with np.errstate(all="ignore"):
        for t in range(T):
            for s in range(S):
                for j in range(NJ):
                    out["w"][t, s, j] = w[s, j]
                    if tracked[s, j] == 0:
                        continue
                    row = state[s, j]
                    absent = present is not None and present[t, s, j] == 0
                    if not absent:
                        absent = any(refused(x) for x in tp[t, s, j]) or any(refused(x) for x in tr[t, s, j])
                    if not absent:
                        code = PRESENT
                        for k in range(3):
                            row[k] = F(tp[t, s, j, k] + gpos[t, s, k])
                        row[3:12] = tr[t, s, j]
                        row[12], row[13], row[14] = F(1), F(0), F(1)
                        out["tp"][t, s, j] = tp[t, s, j]
                    elif row[12] != 0 and F(row[13] + F(1)) <= F(max_hold):
                        code = HELD
                        row[13] = F(row[13] + F(1))
                        row[14] = F(row[14] * F(decay))
                        for k in range(3):
                            out["tp"][t, s, j, k] = F(row[k] - gpos[t, s, k])
                    else:
                        code = LOST
                        row[12] = F(0)
                    out["code"][t, s, j] = code
                    if code != LOST:
                        out["on"][t, s, j] = 1
                        out["tr"][t, s, j] = row[3:12]
                        out["w"][t, s, j] = [F(w[s, j, 0] * row[14]), F(w[s, j, 1] * row[14])]
            out["state"][t] = state
    return out


def _torch_rule(gaps, tp, tr, w, tracked, gpos, present, device="cpu"):
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    state = gaps.new_state(S, device)
    keys = ("tp", "tr", "w", "on", "code")
    out = {k: [] for k in keys + ("state",)}
    for t in range(T):
        r = gaps.step(state, f(tp[t]), f(tr[t]), f(w), f(tracked), f(gpos[t]), f(present[t]) if present is not None else None)
        for k, v in zip(keys, r):
            out[k].append(v.cpu().numpy())
        out["state"].append(state.cpu().numpy().copy())
    return {k: np.stack(v) for k, v in out.items()}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("max_hold,decay", [(3, 0.7), (0, 0.7), (3, 1.0), (65535, 0.999)])
def test_step_equals_the_numpy_loop(max_hold, decay):
    sc = _script()
    exp = _numpy_rule(max_hold, decay, *sc)
    got = _torch_rule(Gaps(max_hold, decay), *sc)
    for k in exp:
        assert _same(got[k], exp[k]), (k, max_hold, decay)
    code = exp["code"]
    assert (code[:, :, 5] == 0).all() and (code[:, :, 0][:30] == PRESENT).all()
    if max_hold == 3:
        assert code[10:15, 0, 1].tolist() == [HELD, HELD, HELD, LOST, PRESENT]          # held to exactly max_hold, expired one step later, back
        assert code[19:24, 0, 1].tolist() == [PRESENT, HELD, HELD, HELD, PRESENT]
        assert exp["state"][12, 0, 1, 13] == 3 and exp["state"][13, 0, 1, 12] == 0
        assert code[0:7, 0, 2].tolist() == [LOST] * 6 + [PRESENT]                       # never seen: nothing to hold
        assert code[8:11, 0, 3].tolist() == [HELD, HELD, PRESENT]                       # the Inf and the NaN sample, present = 1
        assert code[15:18, 0, 4].tolist() == [HELD] * 3 and np.isfinite(exp["tp"][15:18, :, 4]).all()
        assert code[25:27, 0, 6].tolist() == [HELD, PRESENT]                            # beyond the limit / exactly at it
        assert (code[33:, 1][:, exp["on"][29, 1] == 1] == LOST).all() and exp["on"][33:, 1].sum() == 0  # E == 0 from step 33 on
        f = exp["state"][12, 0, 1, 14]
        assert f == (F(decay) * F(decay)) * F(decay) if decay != 1.0 else f == 1
        assert _same(exp["w"][12, 0, 1], np.array([F(sc[2][0, 1, 0] * f), F(sc[2][0, 1, 1] * f)], F))
    if max_hold == 0:
        assert not (code == HELD).any() and (code[10:14, :, 1] == LOST).all()
    if max_hold == 65535:
        assert (code[30:, 1][:, sc[3][1] == 1] == HELD).all()
    assert np.isfinite(exp["tp"]).all() and np.isfinite(exp["tr"]).all() and (exp["state"][..., 15] == 0).all()


def test_without_present_only_refused_samples_mark_gaps():
    tp, tr, w, tracked, gpos, _ = _script()
    exp = _numpy_rule(3, 0.7, tp, tr, w, tracked, gpos, None)
    got = _torch_rule(Gaps(3, 0.7), tp, tr, w, tracked, gpos, None)
    for k in exp:
        assert _same(got[k], exp[k]), k
    assert (exp["code"][:, :, 1] == PRESENT).all() and exp["code"][8:11, 0, 3].tolist() == [HELD, HELD, PRESENT]
    assert exp["code"][15:19, 0, 4].tolist() == [HELD, HELD, HELD, PRESENT]  # (the garbage sample is refused on its own)


def test_what_gaps_refuses():
    for bad in (dict(max_hold=-1), dict(max_hold=65536), dict(max_hold=1.5), dict(max_hold=3, decay=0.0), dict(max_hold=3, decay=1.5),
                dict(max_hold=3, decay=float("nan")), dict(max_hold=3, decay=float("inf")), dict(max_hold=3, decay=-0.1)):
        with pytest.raises(ValueError, match="Gaps:"):
            Gaps(**bad).check()
    Gaps(0, 1.0).check()
    Gaps(65535, 1e-30).check()

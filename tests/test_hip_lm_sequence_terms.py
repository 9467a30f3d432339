"""GPU (MI355X): dp_optimize_sequence_lm_terms (include/dragposer_sequence_lm_terms.h) -- dp_optimize_lm_terms' frame with the step loop of a
sequence on the device -- against the per-frame composition the header names, done by hand: optimize_lm(terms=, global_pos=the running
position) with the carried latent, global rotation and mu, the step's (shifted) targets and the step's rows of every term, then
sequence_advance, then the latent copy.  The per-frame kernels are the yardstick: the same arithmetic in the same order, so every comparison
is bit for bit (NaN where NaN) and no tolerance is involved.  Then the special cases and faults the contract names, and the routes through
DragPose.  The clip, its state and the helpers are tests/test_hip_lm_sequence.py's; the tables are tests/lm_terms_oracle.py's."""
import functools
import types
from dataclasses import replace

import numpy as np
import pytest
import torch

import lm_terms_oracle as LT
import test_hip_lm_sequence as LS
import test_hip_terms as HT
from test_hip_lm_sequence import ADJ, BAD_STATE, BAD_TARGETS, EPS, HJ, LAM, NONFINITE, STATE_KEYS, T, _ar, _assert_same, _cat, _lms, _opt, _same, _state

pytestmark = pytest.mark.gpu

OUT_KEYS = LS.OUT_KEYS + ("loss_terms",)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device(DEV)


@functools.lru_cache(maxsize=None)
def _clip(recipe, S):
    """tests/test_hip_lm_sequence.py's clip with the start position drawn as lm_terms_oracle.global_pos draws it (y near 0.9), so that the
    plane at PLANE_Y cuts through the feet"""
    c = LS._clip(recipe, S)
    return types.SimpleNamespace(**dict(vars(c), gpos=torch.from_numpy(LT.global_pos(S)).to(DEV)))


def _rows_T(S, vec, seed, **kw):
    """[T,S,4] rows, HT._rows' draw over T * S frames: vec + noise, and s = 0 on every third (step, sequence) pair"""
    return HT._rows(T * S, vec, DEV, seed, **kw).reshape(T, S, 4).contiguous()


@functools.lru_cache(maxsize=None)
def _table(name, S):
    from dragposer_amd import Term, Terms

    tb = LT.tables(S, DEV)
    if name == "mixed9":  # one term alone in the second round of the term pass
        return Terms(tb["mixed16"].terms[:9], up_axis=1)
    if name == "pins_T":  # pins with a row per step: row step S * 4
        return Terms([Term.distance(17, weight=2.0, per_frame=_rows_T(S, (0.3, 1.0, 0.2), 4, scale=2.0, noise=0.1)),
                      Term.distance(4, weight=1.0, per_frame=_rows_T(S, (0.1, 0.05, 0.0), 5, noise=0.1))])
    if name == "joints":  # joint to joint: no term reads the global position
        return Terms([Term.distance(3, 7, lo=0.25, hi=0.5, weight=3.0), Term.align(9, (1, 0, 0), 9, (0, 1, 0), margin=0.3, weight=2.0)])
    if name == "empty":
        return Terms()
    if name == "dead":
        return Terms([replace(t, weight=0.0) for t in tb["mixed16"].terms], up_axis=1)
    return tb[name]


def _at(terms, t):
    """the table the composition hands dp_optimize_lm_terms at step t: every [T,S,4] per_frame cut to that step's [S,4]"""
    from dragposer_amd import Terms

    return Terms([replace(x, per_frame=x.per_frame[t].contiguous()) if x.per_frame is not None and x.per_frame.dim() == 3 else x for x in terms.terms],
                 terms.up_axis)


def _per_frame(opt, c, st, lm, terms, t0=0, n=T, ar=None, root=True, adj=ADJ, tgt_pos=None, table_at=_at):
    """the composition, frame by frame on the host -> the outputs of frames t0 .. t0 + n (with the z_tgt rows used); st is advanced in place.
    table_at(terms, t): the table handed over at step t; when the steps' tables differ in length, loss_terms is the list of the steps' arrays"""
    S, d = c.S, opt.device
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    o = {k: [] for k in OUT_KEYS + ("z_tgt",)}
    nan = torch.full((S, 24), float("nan"), device=d)
    for t in range(t0, t0 + n):
        zt = ar.predict(st.lbuf) if ar is not None else c.z_tgt[t].contiguous()
        tp = (tgt_pos[t] + (c.root[t] - st.gpos).unsqueeze(1)).contiguous() if root else tgt_pos[t]
        fr = opt.optimize_lm(st.latent, zt, st.grot, tp, c.tgt_rot[t], c.w, c.tracked, lm=lm, lambda_rot=1.0, lambda_tmp=LAM, mu=st.mu,
                             terms=table_at(terms, t), global_pos=st.gpos, **EPS)
        pose, pos = torch.empty(S, 88, device=d), torch.empty(S, 3, device=d)
        opt.sequence_advance(fr, st.gpos, st.grot, st.lbuf, st.dbuf, st.hbuf, HJ, pose_ret=pose, pos_ret=pos, adjust=adj,
                             tgt_pos=tp if adj is not None else None)
        st.latent.copy_(fr["z"])
        bad_state = (fr["status"] & BAD_STATE) != 0
        for k, v in (("pose_ret", pose), ("pos_ret", pos), ("world_rot", fr["world_rot"]), ("iters", fr["iters"]), ("loss", fr["loss"]),
                     ("status", fr["status"]), ("scratch", torch.cat((st.lbuf[:, -1], st.dbuf[:, -1], st.hbuf[:, -1]), dim=1)), ("mu_trace", st.mu),
                     ("n_accepted", fr["n_accepted"]), ("loss0", fr["loss0"]), ("joint_pos", fr["pos"]), ("loss_terms", fr["loss_terms"]),
                     ("z_tgt", torch.where(bad_state[:, None], nan, zt))):
            o[k].append(v.clone())
    return {k: (torch.stack(v) if k != "loss_terms" or len({x.shape for x in v}) == 1 else v) for k, v in o.items()}


def _launch(opt, c, st, lm, terms, t0=0, n=T, ar=None, root=True, adj=ADJ, tgt_pos=None, outputs=None, null_mu=False):
    """one launch over frames t0 .. t0 + n -> its outputs; st is advanced in place"""
    tgt_pos = c.tgt_pos if tgt_pos is None else tgt_pos
    sl = slice(t0, t0 + n)
    scratch = torch.empty(n, c.S, 24 + 3 + len(HJ), device=opt.device)
    zt, strides = (None, (0, 0)) if ar is not None else (c.z_tgt[sl].contiguous(), (c.S * 24, 24))
    o = opt.optimize_sequence_lm(st.latent, tgt_pos[sl].contiguous(), c.tgt_rot[sl].contiguous(), c.root[sl].contiguous() if root else None, c.w,
                                 c.tracked, zt, strides, st.gpos, st.grot, st.lbuf, st.dbuf, st.hbuf, HJ, lm=lm, lambda_rot=1.0, lambda_tmp=LAM,
                                 mu=None if null_mu else st.mu, ar=ar, adjust=adj, scratch=scratch, z_tgt_trace=True if ar is not None else None,
                                 outputs=outputs, terms=terms.frames(t0, t0 + n) if terms is not None else None, **EPS)
    o["scratch"] = scratch
    if ar is not None:
        o["z_tgt"] = o.pop("z_tgt_trace")
    return o


def _case(recipe, S, which, table, dtype="fp32", **kw):
    opt, c, lm, terms = _opt(dtype), _clip(recipe, S), _lms()[which], _table(table, S)
    if "ar" in kw:
        kw["ar"] = _ar(kw["ar"])
    keys = OUT_KEYS + (("z_tgt",) if "ar" in kw else ())
    est = _state(c)
    exp = _per_frame(opt, c, est, lm, terms, **kw)
    gst = _state(c)
    got = _launch(opt, c, gst, lm, terms, **kw)
    cst = _state(c)
    chained = _cat(_launch(opt, c, cst, lm, terms, 0, 3, **kw), _launch(opt, c, cst, lm, terms, 3, 4, **kw))
    torch.cuda.synchronize()
    what = (recipe, S, which, table, dtype)
    assert got["loss_terms"].shape == (T, S, len(terms))
    _assert_same(got, exp, keys, what)
    _assert_same(gst, est, STATE_KEYS, what)
    _assert_same(chained, exp, keys, what + ("3 + 4",))
    _assert_same(cst, est, STATE_KEYS, what + ("3 + 4",))
    assert int(exp["status"].max()) == 0 and bool(torch.isfinite(exp["pose_ret"]).all())
    assert _same(got["scratch"][-LS.H:, :, :24], gst.lbuf.transpose(0, 1))  # the second launch appended what the steps handed over
    return exp


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("table", ["plane_one_sided", "custom", "pins", "mixed16", "mixed9"])
@pytest.mark.parametrize("recipe,which", [("6warm", "six"), ("6warm", "three"), ("3cold", "six"), ("3cold", "three")])
def test_one_launch_equals_the_composition(dev, recipe, which, table, S):
    """S = 1 (one wave alone) and S = 5 (two workgroups, the second partly filled), T = 7 in one launch and as 3 + 4 steps, with tgt_root and the
    joint adjustment: every per-step output, loss_terms, the whole state, mu and its trace.  `pins` has per-frame rows [S,4], held; mixed16
    fills both rounds of the term pass, mixed9 leaves one term alone in the second"""
    _case(recipe, S, which, table)


def _on_and_off(lt):
    """[n] per term: the sequences in which the slot is > 0 on some step and exactly 0 on another"""
    return [int((((lt[:, :, k] > 0).any(0)) & ((lt[:, :, k] == 0).any(0))).sum()) for k in range(lt.shape[2])]


def test_the_clip_is_not_vacuous(dev):
    """Asserted on the COMPOSITION's outputs (the per-frame kernels), S = 5, LM(6) without early stop, both recipes: for plane_one_sided and
    for a band of mixed16, loss_terms is > 0 on some step and exactly 0 on another step of the same sequence -- the active set changes inside a
    wave's lifetime --, some trial is rejected and some accepted, and mu moves and is carried.  Measured on an MI355X with the tables and
    PLANE_Y as tests/lm_terms_oracle.py has them, nothing had to be moved (profiles/lm_seq_terms_tests.txt) -- sequences of 5 with a slot on
    and off: 6warm plane_one_sided [4]; 6warm mixed16 [5, 5, 0, 5, 4, 3, 0, 0, 0, 4, 4, 3, 0, 0, 0, 0] (the bands are terms 3, 4, 5, 6, 9);
    3cold plane_one_sided [5]; 3cold mixed16 [5, 4, 0, 5, 4, 5, 0, 0, 0, 4, 4, 3, 0, 0, 0, 0].  Trials rejected / accepted: 99 / 111,
    101 / 109, 95 / 115, 102 / 108; mu moves in 5 of 5 sequences in each."""
    opt, lm = _opt(), _lms()["six"]
    for recipe in ("6warm", "3cold"):
        c = _clip(recipe, 5)
        for table in ("plane_one_sided", "mixed16"):
            terms = _table(table, 5)
            exp = _per_frame(opt, c, _state(c), lm, terms)
            torch.cuda.synchronize()
            flips = _on_and_off(exp["loss_terms"])
            rejected, accepted = int((exp["iters"] - exp["n_accepted"]).sum()), int(exp["n_accepted"].sum())
            mt = exp["mu_trace"]
            moved = sum(bool((mt[:, s] != 1e-2).any() and (mt[1:, s] != mt[:-1, s]).any()) for s in range(5))
            print(f"not vacuous: {recipe} {table}: sequences with a slot on and off, per term {flips}; trials rejected {rejected}, accepted {accepted}; "
                  f"sequences whose mu moves {moved}/5")
            if table == "plane_one_sided":
                assert flips[0] >= 1, flips
            else:  # the bands of mixed16: terms 3, 4, 5, 6 and 9
                assert any(flips[k] >= 1 for k in (3, 4, 5, 6, 9)), flips
            assert rejected > 0 and accepted > 0 and moved >= 1


def test_rows_per_step(dev):
    """pins with [T,S,4] rows (row step S * 4): the launch against the composition fed row t at step t.  (The same table with [S,4] rows is
    `pins` above.)  Then a term whose s is 0 on steps 2 and 5 only, and positive on the others: on those steps the launch has the bits of the
    table WITHOUT that term, the composition being handed the shorter table there"""
    from dragposer_amd import Terms

    exp = _case("6warm", 5, "six", "pins_T")
    s = exp["loss_terms"]
    assert bool(((_table("pins_T", 5).terms[0].per_frame[..., 3] == 0) == (s[..., 0] == 0)).all())  # a slot is 0 exactly where its row's s is
    opt, c, lm = _opt(), _clip("6warm", 5), _lms()["six"]
    base = _table("pins_T", 5)
    rows = base.terms[0].per_frame.clone()
    rows[..., 3] = 1.5
    rows[2, :, 3] = rows[5, :, 3] = 0.0
    terms = Terms([replace(base.terms[0], per_frame=rows), base.terms[1]])
    without = Terms([base.terms[1]])
    est, gst = _state(c), _state(c)
    exp = _per_frame(opt, c, est, lm, terms, table_at=lambda tb, t: _at(without if t in (2, 5) else tb, t))
    got = _launch(opt, c, gst, lm, terms)
    torch.cuda.synchronize()
    lt = exp.pop("loss_terms")
    _assert_same(got, exp, LS.OUT_KEYS, "a term off on steps 2 and 5")
    _assert_same(gst, est, STATE_KEYS)
    for t in range(T):
        if t in (2, 5):
            assert bool((got["loss_terms"][t, :, 0] == 0).all()) and _same(got["loss_terms"][t, :, 1:], lt[t])
        else:
            assert bool((got["loss_terms"][t, :, 0] > 0).all()) and _same(got["loss_terms"][t], lt[t])


@pytest.mark.parametrize("table", ["empty", "dead"])
@pytest.mark.parametrize("recipe,which", [("6warm", "three"), ("3cold", "six")])
def test_empty_and_dead_tables_have_the_plain_launchs_bits(dev, recipe, which, table):
    """Terms([]) and mixed16 with every weight 0: dp_optimize_sequence_lm's bits on every common output and on the state"""
    opt, c, lm, terms = _opt(), _clip(recipe, 5), _lms()[which], _table(table, 5)
    pst, gst = _state(c), _state(c)
    plain = LS._launch(opt, c, pst, lm)
    got = _launch(opt, c, gst, lm, terms)
    torch.cuda.synchronize()
    assert got["loss_terms"].shape == (T, 5, len(terms)) and bool((got["loss_terms"] == 0).all())
    _assert_same(got, plain, LS.OUT_KEYS, table)
    _assert_same(gst, pst, STATE_KEYS, table)


@pytest.mark.parametrize("order", [1, 2])
def test_the_predictor_beside_a_table(dev, order):
    """orders 1 (hold) and 2 (a fixed random A) beside `custom`: also the z_tgt row every step used"""
    exp = _case("3cold", 5, "three", "custom", ar=order, adj=None if order == 2 else ADJ)
    assert bool((exp["loss"][..., 2] > 0).any()) and not torch.equal(exp["z_tgt"][1], exp["z_tgt"][0])
    _case("6warm", 5, "six", "mixed16", ar=order)


def _fault(c, lm, terms, clean_terms=None, tgt_pos=None, state=lambda st: None):
    """the launch and the composition on a faulty input (a table, a target array or a state that differs from the clean one's), the clean
    launch beside them -> (got, its state, clean, its state)"""
    opt = _opt()
    cst = _state(c)
    clean = _launch(opt, c, cst, lm, clean_terms if clean_terms is not None else terms)
    gst, est = _state(c), _state(c)
    state(gst), state(est)
    got = _launch(opt, c, gst, lm, terms, tgt_pos=tgt_pos)
    exp = _per_frame(opt, c, est, lm, terms, tgt_pos=tgt_pos)
    torch.cuda.synchronize()
    _assert_same(got, exp, OUT_KEYS)
    _assert_same(gst, est, STATE_KEYS)
    return got, gst, clean, cst


def test_a_nan_per_frame_row_of_an_active_term(dev):
    """a NaN in term 1's row at (t = 3, s = 1): that step DP_STATUS_BAD_TARGETS with the warm start's pose and NaN z and loss_terms, every later
    step DP_STATUS_BAD_STATE, mu untouched, the other four sequences bit-equal to the clean launch -- all of it the composition's bits"""
    from dragposer_amd import Terms

    c, lm, base = _clip("6warm", 5), _lms()["six"], _table("pins_T", 5)
    rows = base.terms[1].per_frame.clone()
    rows[3, 1, 1] = float("nan")
    got, gst, clean, cst = _fault(c, lm, Terms([base.terms[0], replace(base.terms[1], per_frame=rows)]), clean_terms=base)
    LS._fault_checks(got, gst, clean, cst, OUT_KEYS, 3)
    assert bool(torch.isnan(got["loss_terms"][3:, 1]).all()) and bool(torch.isfinite(got["loss_terms"][:3, 1]).all())


def test_a_nan_tracker_sample_beside_a_table(dev):
    c, lm = _clip("6cold", 5), _lms()["six"]
    tp = c.tgt_pos.clone()
    tp[2, 1, 17, 1] = float("nan")
    got, gst, clean, cst = _fault(c, lm, _table("pins_T", 5), tgt_pos=tp)
    LS._fault_checks(got, gst, clean, cst, OUT_KEYS, 2)
    assert bool(torch.isnan(got["loss_terms"][2:, 1]).all())


def test_a_refused_global_position_at_entry(dev):
    """with plane_one_sided, which reads it: every step of that sequence DP_STATUS_BAD_STATE, results NaN, mu untouched.  With a joint-to-joint
    table, which does not: the position is not screened, and the sequence goes the way dp_optimize_sequence_lm takes it (tgt_root shifts the
    targets by a NaN: DP_STATUS_BAD_TARGETS at step 0).  Both the composition's bits; the other sequences keep the clean launch's"""
    c, lm = _clip("6warm", 5), _lms()["three"]

    def poison(st):
        st.gpos[1, 2] = float("inf")

    got, gst, clean, cst = _fault(c, lm, _table("plane_one_sided", 5), state=poison)
    st = got["status"].cpu()
    assert bool((st[:, 1] == (BAD_STATE | NONFINITE)).all()) and bool((st[:, [0, 2, 3, 4]] == 0).all())
    for k in ("pose_ret", "pos_ret", "world_rot", "joint_pos", "scratch", "loss", "loss0", "loss_terms"):
        assert bool(torch.isnan(got[k][:, 1]).all()), k
    assert bool((got["iters"][:, 1] == 0).all()) and bool((got["mu_trace"][:, 1] == 1e-2).all()) and float(gst.mu[1]) == float(np.float32(1e-2))
    assert bool(torch.isnan(gst.latent[1]).all()) and bool(torch.isnan(gst.gpos[1]).all()) and bool(torch.isnan(gst.grot[1]).all())
    rest = [0, 2, 3, 4]
    for k in OUT_KEYS:
        assert _same(got[k][:, rest], clean[k][:, rest]), k
    for k in STATE_KEYS:
        assert _same(getattr(gst, k)[rest], getattr(cst, k)[rest]), k
    got, gst, clean, cst = _fault(c, lm, _table("joints", 5), state=poison)
    st = got["status"].cpu()
    assert int(st[0, 1]) == BAD_TARGETS | NONFINITE and bool((st[1:, 1] == (BAD_STATE | NONFINITE)).all())
    for k in OUT_KEYS:
        assert _same(got[k][:, rest], clean[k][:, rest]), k


def test_output_subsets_a_bf16_context_and_two_launches(dev):
    opt, c, lm, terms = _opt(), _clip("3cold", 5), _lms()["six"], _table("mixed16", 5)
    wst = _state(c)
    whole = _launch(opt, c, wst, lm, terms)
    again_st = _state(c)
    again = _launch(opt, c, again_st, lm, terms)
    torch.cuda.synchronize()
    _assert_same(again, whole, OUT_KEYS)  # no atomics: two calls, identical bits
    _assert_same(again_st, wst, STATE_KEYS)
    for names in (("pose_ret",), ("loss_terms",), ("iters", "mu_trace"), ("loss0", "status"), ("loss", "joint_pos", "world_rot"),
                  ("pos_ret", "n_accepted", "loss_terms"), ()):
        st = _state(c)
        part = _launch(opt, c, st, lm, terms, outputs=names)
        torch.cuda.synchronize()
        assert set(part) == set(names) | {"scratch", "mu"}
        _assert_same(part, whole, names + ("scratch",), names)
        _assert_same(st, wst, STATE_KEYS, names)
    st = _state(c)  # mu = NULL: every sequence starts at mu0, the damping is carried inside the launch and not returned
    part = _launch(opt, c, st, lm, terms, null_mu=True)
    torch.cuda.synchronize()
    _assert_same(part, whole, OUT_KEYS, "mu NULL")
    _case("6warm", 5, "three", "mixed16", dtype="bf16")
    _case("3cold", 5, "six", "pins_T", dtype="bf16")


def test_a_captured_launch_replayed_with_rows_and_mu_rewritten(dev):
    """one launch of 3 steps captured into a graph and replayed twice, the per-frame rows and mu rewritten between the replays: rows, mu,
    latent and state are read at replay time -- the bits of two eager launches with those rows and that mu"""
    from dragposer_amd import Terms

    opt, c, lm, base = _opt(), _clip("6warm", 5), _lms()["three"], _table("pins_T", 5)
    rows_a = [t.per_frame[:3].contiguous() for t in base.terms]
    rows_b = [t.per_frame[3:6].contiguous() for t in base.terms]
    with_rows = lambda rows: Terms([replace(t, per_frame=r) for t, r in zip(base.terms, rows)])
    est = _state(c)
    e1 = _launch(opt, c, est, lm, with_rows(rows_a), 0, 3)
    est.mu.fill_(0.5)
    e2 = _launch(opt, c, est, lm, with_rows(rows_b), 0, 3)
    torch.cuda.synchronize()
    assert not _same(e1["loss_terms"], e2["loss_terms"])
    gst = _state(c)
    init = {k: getattr(gst, k).clone() for k in STATE_KEYS}
    buf = [r.clone() for r in rows_a]
    terms = with_rows(buf)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        o = _launch(opt, c, gst, lm, terms, 0, 3)  # (warm-up, and the launch's output tensors)
    torch.cuda.current_stream(dev).wait_stream(s)
    outs = {k: o[k] for k in OUT_KEYS if k != "scratch"}
    args = dict(lm=lm, lambda_rot=1.0, lambda_tmp=LAM, mu=gst.mu, adjust=ADJ, scratch=o["scratch"], terms=terms, **EPS, **outs)
    tp, tr, root, zt = c.tgt_pos[:3].contiguous(), c.tgt_rot[:3].contiguous(), c.root[:3].contiguous(), c.z_tgt[:3].contiguous()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.optimize_sequence_lm(gst.latent, tp, tr, root, c.w, c.tracked, zt, (c.S * 24, 24), gst.gpos, gst.grot, gst.lbuf, gst.dbuf, gst.hbuf, HJ, **args)
    for k, v in init.items():
        getattr(gst, k).copy_(v)
    for exp, rows, mu in ((e1, rows_a, None), (e2, rows_b, 0.5)):
        for b, r in zip(buf, rows):
            b.copy_(r)
        if mu is not None:
            gst.mu.fill_(mu)
        for k in OUT_KEYS:
            o[k].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(o, exp, OUT_KEYS)
    _assert_same(gst, est, STATE_KEYS)


# ---------------------------------------------------------------------------------------------------- through DragPose
def _dragpose_both(solver, lam, temporal=None, window=0, n=12):
    """n frames of tests/data/example_clip.bvh with `custom` and a pin with a row per frame as the solver's table (LM.terms): the loop over
    run(solver=) that shifts the targets by hand and whose solver carries frame t's rows, against run_frames(solver=, target_root=) whose
    solver carries the [n,1,4] rows -> (the DragPose of run_frames, the number of frames of each of its launches)"""
    from dragposer_amd import Term, Terms
    from dragposer_amd.drag_pose import DragPose

    opt, q, mask_idx, weights, kw = LS._bvh_clip()
    kw = dict(kw, temporal_future_window=window)
    g = torch.Generator().manual_seed(31)
    rows = torch.cat((q["gpos"][:n].reshape(n, 1, 3).cpu() + 0.05 * torch.randn(n, 1, 3, generator=g), 0.5 + torch.rand(n, 1, 1, generator=g)), 2)
    rows[4, :, 3] = 0.0  # (off on one frame)
    terms = Terms(HT.CUSTOM().terms + [Term.distance(0, weight=0.5, per_frame=rows.contiguous().to(DEV))])
    both = []
    for _ in range(2):
        dp = DragPose(opt, temporal, np.zeros(24, np.float32), np.ones(24, np.float32), n_sequences=1, native_temporal=temporal is not None)
        dp.set_initial_state(q["z0"], q["m"]["global_pos"][0][None], q["m"]["global_rot"][0][None], q["m"]["heights"][0][None])
        both.append(dp)
    loop, whole = both
    rec = {k: [] for k in ("pose", "gpos", "iters", "status", "loss", "loss_terms")}
    for t in range(n):
        tp = q["tp_rel"][t][None] + (q["gpos"][t] - loop.current_global_pos).unsqueeze(1)
        pose, gpos = loop.run(tp, q["tR"][t][None], mask_idx, weights, solver=replace(solver, terms=_at(terms, t)), lambda_temporal=lam, **kw)
        last = loop.last
        lt = last["loss_terms"] if "loss_terms" in last else loop.last_terms[0]
        for k, v in (("pose", pose), ("gpos", gpos), ("iters", last["iters"]), ("status", last["status"]), ("loss", last["loss"]), ("loss_terms", lt)):
            rec[k].append(v.clone())
    calls = []
    seq = whole.opt.optimize_sequence_lm
    whole.opt.optimize_sequence_lm = lambda *x, **k: (calls.append(int(x[1].shape[0])), seq(*x, **k))[1]
    try:
        ps, gs, its = whole.run_frames(q["tp_rel"][:n].reshape(n, 1, -1, 3), q["tR"][:n].reshape(n, 1, -1, 3, 3), mask_idx, weights,
                                       target_root=q["gpos"][:n].reshape(n, 1, 3), solver=replace(solver, terms=terms), lambda_temporal=lam, **kw)
    finally:
        del whole.opt.optimize_sequence_lm
    torch.cuda.synchronize()
    rec = {k: torch.stack(v) for k, v in rec.items()}
    assert torch.equal(ps, rec["pose"]) and torch.equal(gs, rec["gpos"]) and torch.equal(its, rec["iters"])
    assert torch.equal(whole.last_status, rec["status"]) and int(whole.last_status.max()) == 0
    assert torch.equal(whole.last_loss, rec["loss"]) and torch.equal(whole.last_terms, rec["loss_terms"])
    assert whole.last_terms.shape == (n, 1, 4) and bool((whole.last_terms[:, 0, 3] > 0).sum() == n - 1) and float(whole.last_terms[4, 0, 3]) == 0.0
    assert torch.equal(whole.lm_mu, loop.lm_mu) and torch.equal(whole.latent, loop.latent)
    for k in ("current_global_pos", "current_global_rot", "latent_buffer", "displacement_buffer", "heights_buffer"):
        assert torch.equal(getattr(whole, k), getattr(loop, k)), k
    return whole, calls


def test_dragpose_run_frames_equals_run_across_a_stretch_boundary(dev):
    """run_frames(solver=LM(3, terms=), target_root=) equals run(solver=LM(3, terms=)) frame by frame, bit for bit: with a seeded temporal predictor
    and a window of 8 the 12 frames are cut into stretches of 8 / 4, and the [12,1,4] rows are offset per stretch"""
    from dragposer_amd import LM
    from dragposer_amd.temporal import TemporalPredictor

    torch.manual_seed(5)
    predictor = TemporalPredictor(n_encoder_layers=1, n_decoder_layers=1, dim_feedforward=16)
    whole, calls = _dragpose_both(LM(3), 0.02, temporal=predictor, window=8)
    assert calls == [8, 4]
    assert bool((whole.last_loss[..., 2] > 0).any())  # the pull towards the predictor's targets is in the loss


def test_dragpose_with_the_solvers_predictor_and_a_table(dev):
    """with solver.predictor run_frames is ONE launch, and run() its one-step launch: the same bits"""
    from dragposer_amd import LM, LatentAR

    whole, calls = _dragpose_both(LM(3, predictor=LatentAR.hold()), 0.05)
    assert calls == [12]
    assert bool((whole.last_loss[..., 2] > 0).any())  # the pull is weighed in


def test_dragpose_still_refuses_the_other_layers(dev):
    from dragposer_amd import LM, Hold, Holds, Points, Term, Terms

    opt, q, mask_idx, weights, kw = LS._bvh_clip()
    dp = LS._fresh(opt, q)
    tp, tR = q["tp_rel"][:2].reshape(2, 1, -1, 3), q["tR"][:2].reshape(2, 1, -1, 3, 3)
    with pytest.raises(ValueError, match="solver= does not go with holds="):
        dp.run_frames(tp, tR, mask_idx, weights, solver=LM(3, terms=HT.CUSTOM()), holds=Holds([Hold(0, 0.02, 0.05)]), **kw)
    with pytest.raises(ValueError, match="solver= does not go with terms="):  # the table belongs to the solver
        dp.run_frames(tp, tR, mask_idx, weights, solver=LM(3), terms=HT.CUSTOM(), **kw)
    with pytest.raises(ValueError, match="a table with points does not go with the LM solver"):
        dp.run_frames(tp, tR, mask_idx, weights, solver=LM(3, terms=Terms([Term.distance(4, 8, hi=0.3)], points=Points([]))), **kw)

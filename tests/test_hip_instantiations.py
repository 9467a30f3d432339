"""GPU: every optimise-kernel instantiation of the product library (tests/instantiations.py, held to the library's symbols by
tests/test_instantiation_coverage.py) is launched, is reported by dp_debug_last_launch as what ran, and is checked:

* against the C oracle (oracle/analytic.c, f32 and f64) under the enforced rules of BASELINE.md section 3: a frame more than 0.05 mm
  from the f32 oracle is one the oracle's own f32 / f64 pair parts ways on, or one that shows a mechanism on the oracle's trajectory
  (tests/sensitivity.py); at most 2 x the pair's count + 2 of them, none beyond 5 mm; the loss to 2e-3 everywhere else;
* at the shapes where these kernels break: batches that fill no wave or workgroup (1, 61, 67), n_iter 256 (the last step of the
  argument table of Adam scalars) and 257 / 300 (LONG: the kernels continue the table on the device), and for the two-waves-per-SIMD
  dp_w16 units a batch beyond one wave per SIMD of the chip (n_cu * 64 + 37 frames);
* early stop: iteration counts exact against the oracle on the frames its pair agrees on -- after asserting that the counts spread
  (for LONG: on both sides of 256) -- except for a frame where at most two decisions of the while-condition went the other way, each
  with a stop quantity of the oracle's trajectory within 2e-5 of its threshold (`_stop_flip`), whose results must then be the oracle's
  trajectory at the kernel's count (at most 3 of 67 frames, 9 of 192);
* sequences: dp_optimize_sequence over T steps = T one-step DragPose.run calls, bit for bit, and the first step against the oracle;
* the body-part layout's fixed-count launches: the plain call runs dp_w4_bp_lv.hip's kernel (rows w4_bplv-*), the call with the debug dump --
  the only product route to them -- dp_w4_bp.hip's fixed-count kernels (rows w4_bp-4w-fixed*): the same batches, the same oracle check, and
  the two byte-equal on every per-frame result;
* dp_w4's two row layouts (dense, body-part) on the same model: bit-identical, in fp32 and bf16;
* a model the body-part layout does not fit loads dense, refuses the body-part layout, and matches an oracle built from it;
* dp_w16 with 4 and 8 waves per workgroup: the same bits."""
import numpy as np
import pytest
import torch

from instantiations import INSTANTIATIONS, UNIT_W4, UNIT_W4_BP, UNIT_W4_BP_LV, UNIT_W16, Inst, inst_id, last_launch, set_layout  # tests/instantiations.py
from oracle import ref_torch as R
from oracle.analytic import DEFAULT_MODEL, AnalyticOracle
from sensitivity import kink_distance, tiny_gradient  # tests/sensitivity.py

pytestmark = pytest.mark.gpu

KEYS = ("z0", "z_tgt", "cur_rot", "tgt_pos", "tgt_rot", "w", "tracked")
PER_FRAME = ("z", "z_pre", "pose", "disp", "world_disp", "world_rot", "pos", "rot", "loss", "iters", "status")
LAM = 0.02
# early-stop settings: the reference's eval values (their counts spread over 11 ... 256), and tighter ones whose counts fall on both sides of 256
ES_SHORT = dict(stop_eps_pos=1e-4, stop_eps_rot=1e-2, min_loss_incr=1e-5)
ES_LONG = dict(stop_eps_pos=1e-6, stop_eps_rot=1e-4, min_loss_incr=1e-6)
B_MAIN, B_RAGGED = 67, (1, 61)  # 67 = four workgroups of dp_w4 + 3 frames, one of dp_w16 + 3; 1 and 61 as its leading rows


def _mm(a, b):
    return np.linalg.norm(a - b, axis=-1) * 1000.0


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_against_oracle(out, b, n_iter, es, model_path=DEFAULT_MODEL, what=""):
    """BASELINE.md section 3, with the C oracle's f32 / f64 pair in the reference pair's role"""
    a = [b[k] for k in KEYS]
    o32, o64 = _oracle_pair(b, n_iter, es, model_path)
    sens = _mm(o32["pos"], o64["pos"]).max(axis=1) > 0.02
    if es:
        sens |= o32["iters"] != o64["iters"]
    n_pair = int(sens.sum())
    err = _mm(out["pos"], o32["pos"]).max(axis=1)
    flips = []
    if es:
        off = np.nonzero(~sens & (out["iters"] != o32["iters"]))[0]
        flips = [int(f) for f in off if _stop_flip(out, a, f, int(o32["iters"][f]), n_iter, es, model_path)]
        assert flips == off.tolist() and len(flips) <= max(3, len(err) // 20), (what, off, flips)
    beyond = np.nonzero(err > 0.05)[0]
    print(f"{what}: {len(err)} frames, n_iter {n_iter}: max {err.max():.5f} mm off the pair's {n_pair} frames "
          f"{err[~sens].max() if (~sens).any() else 0:.5f}; beyond 0.05 mm {beyond.tolist()}; "
          f"stop decided the other way within rounding of a threshold: {len(flips)} frames {flips}")
    sens[flips] = True
    others = [int(f) for f in beyond if f not in flips]  # (a frame that stopped elsewhere is not one the pair's allowance counts)
    assert len(others) <= 2 * n_pair + 2 and err.max() <= 5.0, (what, beyond, err[beyond], n_pair, flips)
    rest = [int(f) for f in beyond if not sens[f]]
    if rest:
        kink = kink_distance(b, rest, n_iter, LAM, model_path=model_path)
        tiny = tiny_gradient(b, rest, LAM, model_path=model_path)
        assert all(k < 5e-6 or t < 1e-5 for k, t in zip(kink, tiny)), (what, rest, kink, tiny)
        sens[rest] = True
    ok = ~sens
    np.testing.assert_allclose(out["loss"][ok], o32["loss"][ok], rtol=2e-3, atol=1e-8, err_msg=what)
    if es:
        assert np.array_equal(out["iters"][ok], o32["iters"][ok]), (what, np.nonzero(out["iters"] != o32["iters"])[0])
    else:
        assert (out["iters"] == n_iter).all(), what
    return o32


_PAIRS = {}


def _oracle_pair(b, n_iter, es, model_path):
    """the C oracle's f32 and f64 runs of a batch: computed once per (model, batch, n_iter, stop settings) -- the rows of the dense, the body-part,
    the loop-version and the dp_w16 unit share them -- and left unchanged"""
    key = (model_path, n_iter, tuple(sorted(es.items())), tuple(hash(b[k].tobytes()) for k in KEYS))
    if key not in _PAIRS:
        a = [b[k] for k in KEYS]
        pair = tuple(AnalyticOracle(model_path=model_path, precision=p).optimize(*a, n_iter, lam_tmp=LAM, **es) for p in ("f32", "f64"))
        for r in pair:
            for v in r.values():
                v.setflags(write=False)
        _PAIRS[key] = pair
    return _PAIRS[key]


STOP_ROUNDING = 2e-5  # (relative) how near its threshold a stop quantity must be for two correct implementations to decide it differently


def _stop_flip(out, a, f, it_o, n_iter, es, model_path):
    """Frame f of the kernel stopped at another iteration than the f32 oracle.  Accepted only as decisions of the while-condition
    (oracle/analytic.c: (loss[0] > stop_eps_pos or loss[1] > stop_eps_rot) and incr > min_loss_incr) taken the other way within
    rounding: along the oracle's own trajectory, every decision the kernel took at an iteration from min(counts) to its own count
    must be the trajectory's, or one that a move of a stop quantity by at most STOP_ROUNDING of its size turns over -- loss[0] vs
    stop_eps_pos, loss[1] vs stop_eps_rot, or the decrement of the total loss vs min_loss_incr, measured against the total loss (the
    kernels' losses agree with the f32 oracle's to about 1e-5 relative after a few hundred iterations, and the decrement is the
    difference of two of them).  At most two such decisions per frame; the kernel's results must be the trajectory's at its count."""
    it_g = int(out["iters"][f])
    lo = min(it_g, it_o)
    A = AnalyticOracle(model_path=model_path, precision="f32")
    one = lambda n: A.optimize(*[x[f:f + 1] for x in a], n, lam_tmp=LAM)
    tot = lambda l: float(np.float32(np.float32(l[0] + l[1]) + l[2]))  # (as the loop sums it: fp32, then to double)
    loss = {n: one(n)["loss"][0] for n in range(max(lo - 1, 1), it_g + 1)}
    go = lambda x: (x[0] or x[1]) and x[2]
    flipped = 0
    for k in range(lo, it_g + 1):  # the kernel went on before it_g and stopped at it_g
        lk = loss[k]
        incr = (tot(loss[k - 1]) if k > 1 else 1.0e7) - tot(lk)
        terms = [(float(lk[0]), es["stop_eps_pos"], max(abs(float(lk[0])), es["stop_eps_pos"])),
                 (float(lk[1]), es["stop_eps_rot"], max(abs(float(lk[1])), es["stop_eps_rot"])),
                 (incr, es["min_loss_incr"], tot(lk))]
        above = [v > t for v, t, _ in terms]
        if go(above) == (k < it_g):
            continue
        flipped += 1
        if not any(abs(v - t) <= STOP_ROUNDING * scale and go([not x if j == i else x for j, x in enumerate(above)]) != go(above)
                   for i, (v, t, scale) in enumerate(terms)):
            return False
    at = one(it_g)
    same_path = _mm(out["pos"][f], at["pos"][0]).max() <= 0.05 and np.allclose(out["loss"][f], at["loss"][0], rtol=2e-3, atol=1e-8)
    return 1 <= flipped <= 2 and same_path


def _assert_counts_spread(it, n_iter):
    assert len(np.unique(it)) >= 6 and it.min() < n_iter // 2 and (it < n_iter).sum() >= 3, np.unique(it)
    if n_iter > 256:  # the LONG units: frames that stop inside the argument table, and frames that stop beyond it
        assert (it < 256).sum() >= 3 and ((it > 256) & (it < n_iter)).sum() >= 3, np.unique(it)


@pytest.fixture(scope="module")
def opt():
    from dragposer_amd.optimizer import LatentOptimizer

    o = LatentOptimizer(device="cuda:0")
    assert set_layout(o, -1) == 1  # the shipped checkpoint fits the body-part layout
    yield o
    o.close()


@pytest.fixture(scope="module")
def batch():
    return R.synth_inputs(R.OracleModel(), B_MAIN, seed=11)


def _select(opt, inst):
    if inst.unit in (UNIT_W4, UNIT_W4_BP, UNIT_W4_BP_LV):
        bp = 0 if inst.unit == UNIT_W4 else 1
        assert set_layout(opt, bp) == bp


def _optimize(opt, b, n_iter, es, kernel, outputs=PER_FRAME, dump=False):
    """`dump`: through dp_optimize_debug, with a buffer for the first iteration's dump (what keeps a fixed-count launch of the body-part layout
    on dp_w4_bp.hip's own kernel)"""
    from dragposer_amd.optimizer import to_device_batch

    kw = dict(_debug=torch.zeros(len(b["z0"]), 240, device=opt.device)) if dump else {}
    return _np(opt.optimize(**to_device_batch(b, opt.device), n_iter=n_iter, lambda_tmp=LAM, kernel=kernel, outputs=outputs, **es, **kw))


def _frame_entry(opt, b, inst, model_path=DEFAULT_MODEL):
    """a fixed-count or early-stop entry of a dp_w4 unit or of dp_w16 with 4 waves: 67 frames against the oracle, 1 and 61 frames row-equal.
    dp_w4_bp.hip's fixed-count kernels are reached through the debug dump alone (dp_launch_w4_bp): their rows run the same batches that way, and
    every per-frame result must be, byte for byte, what the plain call -- dp_w4_bp_lv.hip's row -- returns."""
    kernel = "w16" if inst.unit == UNIT_W16 else "w4"
    dump = inst.unit == UNIT_W4_BP and not inst.early
    for n_iter in ((257, 300) if inst.long else (256,)):
        if inst.long and inst.early and n_iter == 257:
            continue  # (early stop beyond the table: 300 iterations, counts on both sides of 256)
        es = (ES_LONG if inst.long else ES_SHORT) if inst.early else {}
        out = _optimize(opt, b, n_iter, es, kernel, dump=dump)
        assert last_launch(opt) == inst, (last_launch(opt), inst)
        o32 = _check_against_oracle(out, b, n_iter, es, model_path, what=f"{inst_id(inst)}")
        if dump:
            lv = _optimize(opt, b, n_iter, es, kernel)
            assert last_launch(opt) == inst._replace(unit=UNIT_W4_BP_LV), last_launch(opt)
            for k in PER_FRAME:
                assert np.ascontiguousarray(lv[k]).tobytes() == np.ascontiguousarray(out[k]).tobytes(), f"{inst_id(inst)} n_iter {n_iter}: {k} differs from the loop-version kernel's"
        if inst.early:
            _assert_counts_spread(o32["iters"], n_iter)
        for B in B_RAGGED:
            sub = _optimize(opt, {k: b[k][:B] for k in KEYS}, n_iter, es, kernel, dump=dump)
            assert last_launch(opt) == inst
            for k in PER_FRAME:
                np.testing.assert_array_equal(sub[k], out[k][:B], err_msg=f"{inst_id(inst)} B={B} {k}")


def _sequence_entry(opt, inst, S=37, T=3, model_path=DEFAULT_MODEL):
    """dp_optimize_sequence (no temporal predictor) over T steps = T one-step DragPose.run calls, bit for bit; step 0 against the oracle"""
    from dragposer_amd.drag_pose import DragPose

    max_iter = 300 if inst.long else 100
    es = ES_LONG if inst.long else ES_SHORT
    s = R.synth_inputs(R.OracleModel(), T * S, seed=21)  # (step 0 of sequence k: frame k of the recipe, from its own warm start)
    idx = np.array(R.TRACK6)
    w = np.array([R.W6[j] for j in R.TRACK6], np.float32)
    tp = torch.tensor(s["tgt_pos"][:, idx]).reshape(T, S, 6, 3).cuda()
    tR = torch.tensor(s["tgt_rot"][:, idx]).reshape(T, S, 6, 3, 3).cuda()
    kw = dict(max_iter=max_iter, learning_rate=1e-2, lambda_rot=1, lambda_temporal=0.0, temporal_future_window=0, **es)

    def fresh():
        dp = DragPose(opt, None, np.zeros(24), np.ones(24), n_sequences=S)
        dp.set_initial_state(s["z0"][:S], np.zeros((S, 3), np.float32), s["cur_rot"][:S], np.zeros((S, 6), np.float32))
        return dp

    a, c = fresh(), fresh()
    pa, ga, ia = a.run_frames(tp, tR, idx, w, **kw)
    assert last_launch(opt) == inst, (last_launch(opt), inst)
    pc, gc, ic, first = [], [], [], None
    for t in range(T):
        p1, g1 = c.run(tp[t], tR[t], idx, w, **kw)
        assert last_launch(opt) == inst
        pc.append(p1.reshape(S, 88).clone()); gc.append(g1.reshape(S, 3).clone()); ic.append(c.last["iters"].clone())
        if t == 0:
            first = {k: c.last[k].clone() for k in ("z", "loss", "iters", "status")}
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(ic), ia) and torch.equal(torch.stack(pc), pa) and torch.equal(torch.stack(gc), ga), inst_id(inst)
    for attr in ("latent", "current_global_pos", "current_global_rot", "latent_buffer", "displacement_buffer", "heights_buffer"):
        assert torch.equal(getattr(a, attr), getattr(c, attr)), (inst_id(inst), attr)
    assert (a.last_status == 0).all() and torch.isfinite(pa).all()
    # step 0 is one optimisation of each sequence's first frame from its initial state: the oracle's, with the pull term off
    trk = np.zeros((S, R.NJ), np.uint8)
    trk[:, idx] = 1
    wd = np.zeros((S, R.NJ, 2), np.float32)
    wd[:, idx] = w
    tpos = np.zeros((S, R.NJ, 3), np.float32)
    tpos[:, idx] = tp[0].cpu().numpy()
    trot = np.zeros((S, R.NJ, 9), np.float32)
    trot[:, idx] = tR[0].reshape(S, 6, 9).cpu().numpy()
    args = (s["z0"][:S], np.zeros((S, 24), np.float32), s["cur_rot"][:S], tpos, trot, wd, trk)
    o32 = AnalyticOracle(model_path=model_path, precision="f32").optimize(*args, max_iter, lam_tmp=0.0, **es)
    o64 = AnalyticOracle(model_path=model_path, precision="f64").optimize(*args, max_iter, lam_tmp=0.0, **es)
    _assert_counts_spread(o32["iters"], max_iter)
    sens = (_mm(o32["pos"], o64["pos"]).max(axis=1) > 0.02) | (o32["iters"] != o64["iters"])
    f = {k: v.cpu().numpy() for k, v in first.items()}
    dz = np.abs(f["z"] - o32["z_final"]).max(axis=1)
    off = np.nonzero(~sens & ((f["iters"] != o32["iters"]) | (dz > 5e-4)))[0]
    print(f"{inst_id(inst)}: step 0 of {S} sequences, max_iter {max_iter}: |dz| max {dz[~sens].max():.2e} off the pair's {int(sens.sum())}; apart {off.tolist()}")
    assert len(off) <= sens.sum() + 2, off  # (with the pair's own: at most 2 x its count + 2 apart)
    if len(off):
        kink = kink_distance(dict(zip(KEYS, args)), off, max_iter, 0.0, model_path=model_path)
        tiny = tiny_gradient(dict(zip(KEYS, args)), off, 0.0, model_path=model_path)
        assert all(k < 5e-6 or t < 1e-5 for k, t in zip(kink, tiny)), (off, kink, tiny)
        sens[off] = True
    assert np.array_equal(f["iters"][~sens], o32["iters"][~sens]) and (f["status"] == 0).all()
    np.testing.assert_allclose(f["loss"][~sens], o32["loss"][~sens], rtol=2e-3, atol=1e-8)


def _w16_two_waves_entry(opt, inst):
    """B = n_cu * 64 + 37: beyond one wave per SIMD.  The oracle on a fixed sample (the first 64 frames, the ragged last 64, 64 seeded
    ones); the same sample through the one-wave-per-SIMD unit: the same bits"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = n_cu * 64 + 37
    big = R.synth_inputs(R.OracleModel(), B, seed=31)
    rng = np.random.default_rng(7)
    sample = np.concatenate([np.arange(64), np.sort(rng.choice(np.arange(64, B - 64), 64, replace=False)), np.arange(B - 64, B)])
    n_iter = 300 if inst.long else 256
    es = (ES_LONG if inst.long else ES_SHORT) if inst.early else {}
    out = _optimize(opt, big, n_iter, es, "w16")
    assert last_launch(opt) == inst, (last_launch(opt), inst)
    got = {k: v[sample] for k, v in out.items()}
    bs = {k: big[k][sample] for k in KEYS}
    o32 = _check_against_oracle(got, bs, n_iter, es, what=f"{inst_id(inst)} (B {B}, sampled)")
    if inst.early:
        _assert_counts_spread(o32["iters"], n_iter)
    one = _optimize(opt, bs, n_iter, es, "w16")
    assert last_launch(opt) == inst._replace(waves=4)
    for k in PER_FRAME:
        np.testing.assert_array_equal(one[k], got[k], err_msg=f"{inst_id(inst)}: 4 vs 8 waves, {k}")


@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=inst_id)
def test_instantiation_runs_and_matches_the_oracle(opt, batch, inst):
    _select(opt, inst)
    try:
        if inst.seq:
            _sequence_entry(opt, inst)
        elif inst.unit == UNIT_W16 and inst.waves == 8:
            _w16_two_waves_entry(opt, inst)
        else:
            _frame_entry(opt, batch, inst)
    finally:
        set_layout(opt, 1)


W4_ENTRIES = [i for i in INSTANTIATIONS if i.unit == UNIT_W4]


def _w4_workloads(opt, b):
    """every dp_w4 instantiation and dp_forward on the same inputs: {name: results}, with the instantiation each ran"""
    from dragposer_amd.drag_pose import DragPose
    from dragposer_amd.optimizer import to_device_batch

    res, ran = {}, []
    for inst in W4_ENTRIES:
        n_iter = 300 if inst.long else (100 if inst.seq else 256)
        es = (ES_LONG if inst.long else ES_SHORT) if inst.early else {}
        if inst.seq:
            S, T = 19, 3
            idx = np.array(R.TRACK6)
            w = np.array([R.W6[j] for j in R.TRACK6], np.float32)
            tp = torch.tensor(b["tgt_pos"][:T * S, idx]).reshape(T, S, 6, 3).cuda()
            tR = torch.tensor(b["tgt_rot"][:T * S, idx]).reshape(T, S, 6, 3, 3).cuda()
            dp = DragPose(opt, None, np.zeros(24), np.ones(24), n_sequences=S)
            dp.set_initial_state(b["z0"][:S], np.zeros((S, 3), np.float32), b["cur_rot"][:S], np.zeros((S, 6), np.float32))
            dev = opt.device
            tpd, trd = torch.zeros(T, S, R.NJ, 3, device=dev), torch.zeros(T, S, R.NJ, 9, device=dev)
            tpd[:, :, idx], trd[:, :, idx] = tp, tR.reshape(T, S, 6, 9)
            trk, wd = torch.zeros(S, R.NJ, dtype=torch.uint8, device=dev), torch.zeros(S, R.NJ, 2, device=dev)
            trk[:, idx], wd[:, idx] = 1, torch.from_numpy(w).to(dev)
            heights = (0, 4, 8, 13, 17, 21)
            scratch = torch.empty(T, S, 24 + 3 + len(heights), device=dev)  # history rows: z_pre | displacement | heights
            r = opt.optimize_sequence(dp.latent, tpd, trd, None, wd, trk, torch.zeros(S, 24, device=dev), (0, 24), dp.current_global_pos,
                                      dp.current_global_rot, dp.latent_buffer, dp.displacement_buffer, dp.heights_buffer, heights, n_iter=n_iter,
                                      lr=1e-2, lambda_rot=1.0, lambda_tmp=0.0, scratch=scratch, **es)
            res[inst_id(inst)] = _np(dict(pose=r["pose_ret"], pos=r["pos_ret"], iters=r["iters"], loss=r["loss"], status=r["status"], z=dp.latent,
                                          z_pre=scratch[..., :24], rot=dp.current_global_rot, world_pos=dp.current_global_pos))
        else:
            res[inst_id(inst)] = _optimize(opt, b, n_iter, es, "w4")
        ran.append(last_launch(opt))
    f = opt.forward(*(torch.from_numpy(b[k]).to(opt.device) for k in ("z0", "cur_rot")), outputs=("pose", "disp", "world_disp", "world_rot", "pos", "rot", "status"))
    res["forward"] = _np(f)
    ran.append(last_launch(opt))
    return res, ran


@pytest.mark.parametrize("wd", ["fp32", "bf16"])
def test_dense_and_body_part_layouts_give_the_same_bits(wd, batch):
    """the body-part unit leaves out only weights that are exactly 0.0 and keeps the dense K order of everything else: every result of
    every dp_w4 instantiation, and of dp_forward, is the dense unit's to the bit"""
    from dragposer_amd.optimizer import LatentOptimizer

    o = LatentOptimizer(device="cuda:0", weight_dtype=wd)
    try:
        assert set_layout(o, -1) == 1
        bp, ran_bp = _w4_workloads(o, batch)
        assert set_layout(o, 0) == 0 and set_layout(o, -1) == 0
        dense, ran_d = _w4_workloads(o, batch)
        assert set_layout(o, 1) == 1
        again, _ = _w4_workloads(o, batch)
    finally:
        o.close()
    assert ran_d == W4_ENTRIES + [Inst(UNIT_W4, 4, 0, 0, 0)], ran_d
    # (body-part: the fixed-count optimising launches go to the loop-version kernel; the while-condition, sequences and dp_forward stay)
    assert ran_bp == [i._replace(unit=UNIT_W4_BP if i.early else UNIT_W4_BP_LV) for i in W4_ENTRIES] + [Inst(UNIT_W4_BP, 4, 0, 0, 0)], ran_bp
    for name in dense:
        for k in dense[name]:
            np.testing.assert_array_equal(bp[name][k], dense[name][k], err_msg=f"{wd} {name} {k}")
            np.testing.assert_array_equal(again[name][k], dense[name][k], err_msg=f"{wd} {name} {k} (switched back)")
    assert all((dense[n]["status"] == 0).all() for n in dense)


def test_a_model_the_body_part_layout_does_not_fit_runs_dense_and_uses_the_weight(tmp_path, batch):
    """tests/test_w4_bp_layout.py's model with one left-out weight of layer 2 at 0.5: dp_create keeps the dense layout, the body-part one is
    refused, and all six dense instantiations and dp_forward match an oracle built from the same weights -- so the dense kernel multiplies
    the weight the body-part unit would drop"""
    from dragposer_amd import _lib
    from dragposer_amd.optimizer import LatentOptimizer, to_device_batch

    raw = dict(np.load(DEFAULT_MODEL))
    U = raw["decoder.layers.2.0.weight"]
    col = int(np.flatnonzero(U[:, 4 * 8])[0])
    W, M = raw["decoder.layers.2.1.weight"].copy(), raw["decoder.layers.2.1.mask"].copy()
    W[1, col, 0], M[1, col, 0] = 0.5, 1.0
    raw["decoder.layers.2.1.weight"], raw["decoder.layers.2.1.mask"] = W, M
    path = str(tmp_path / "model.npz")
    np.savez(path, **raw)
    o = LatentOptimizer(device="cuda:0", arrays=raw)
    try:
        assert set_layout(o, -1) == 0
        assert set_layout(o, 1) == _lib.DP_ERR_UNSUPPORTED and set_layout(o, -1) == 0
        d = to_device_batch(batch, o.device)
        f = _np(o.forward(d["z0"], d["cur_rot"], outputs=("pos", "rot")))
        assert last_launch(o) == Inst(UNIT_W4, 4, 0, 0, 0)
        want = AnalyticOracle(model_path=path, precision="f32").forward(batch["z0"], batch["cur_rot"])
        base = AnalyticOracle(precision="f32").forward(batch["z0"], batch["cur_rot"])
        assert _mm(want["pos"], base["pos"]).max() > 1.0  # the weight moves the pose: a kernel that dropped it could not pass below
        assert _mm(f["pos"], want["pos"]).max() <= 0.01 and np.abs(f["rot"] - want["rot"]).max() <= 2e-5
        for inst in W4_ENTRIES:
            if inst.seq:
                _sequence_entry(o, inst, model_path=path)
            else:
                _frame_entry(o, batch, inst, model_path=path)
    finally:
        o.close()

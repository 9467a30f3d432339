"""GPU (MI355X): dp_forward_vjp_skeleton / decode_fk(offsets=...) (include/dragposer_grad.h) -- dz, dcur_rot and the gradient of the bone
offsets against torch autograd through the fp64 oracle with one skeleton per frame, the bit promises against dp_forward_vjp (the context's own
skeleton; one context per skeleton), refused skeleton rows, determinism, graph capture and a bone-scale fit through torch.optim.Adam.

Frames with a pre-activation within 1e-5 of a LeakyReLU kink (fp64) are excluded from the gradient comparisons and counted, as in
tests/test_hip_vjp.py, with its bar."""
import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from test_hip_skeleton import _raw, _skeletons  # (the four skeletons of test_hip_skeleton.py's xsens fixture)
from test_hip_vjp import NAMES, _check, _inputs

pytestmark = pytest.mark.gpu

NJ = 22


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def opts(dev):
    from dragposer_amd.optimizer import LatentOptimizer

    return {"fp32": LatentOptimizer(device=dev), "bf16": LatentOptimizer(device=dev, weight_dtype="bf16")}


def _base():
    return np.asarray(_raw()["offsets"], np.float32)


def _per_frame(base, B, seed):
    """[B,22,3] fp32: `base` scaled per frame by 0.8..1.25, each bone jittered by a further 0.95..1.05"""
    g = torch.Generator().manual_seed(seed)
    s = 0.8 + 0.45 * torch.rand(B, 1, 1, generator=g)
    jit = 0.95 + 0.1 * torch.rand(B, NJ, 1, generator=g)
    return (torch.from_numpy(base) * s * jit).float().contiguous()


def _fk_world(model, q_root_space, root_pos, O):
    """oracle.ref_torch.fk_world with the bone offsets as a [B,22,3] tensor (one skeleton per frame) instead of the model's"""
    Rm = R.quat_to_rotmat(q_root_space)
    Rinv = R.quat_to_rotmat(R.quat_conj(q_root_space))
    G, P = [Rm[:, 0]], [root_pos]
    for j in range(1, NJ):
        p = model.parents[j]
        local = Rm[:, j] if p == 0 else Rinv[:, p] @ Rm[:, j]
        G.append(G[p] @ local)
        P.append((G[p] @ O[:, j, :, None]).squeeze(-1) + P[p])
    return torch.stack(P, dim=1), torch.stack(G, dim=1)


def _outputs(model, z, cr, O):
    """oracle.ref_torch.pose_fk on decoder_forward, with _fk_world's per-frame skeletons"""
    motion, disp = R.decoder_forward(model, z)
    q = (motion * model.sd4 + model.mu4).reshape(-1, NJ, 4)
    d = disp * model.sd_d + model.mu_d
    wr = R.quat_mul(cr, q[:, 0])
    q = torch.cat((wr.unsqueeze(1), q[:, 1:]), dim=1)
    wd = R.quat_rotate(wr, d)
    pos, rot = _fk_world(model, q, wd, O)
    return dict(pose=motion, disp=d, world_disp=wd, world_rot=wr, pos=pos, rot=rot.reshape(-1, NJ, 9))


def _ref(model, z, cr, O, grads, subsets):
    """fp64 torch autograd: {subset: (dz, dcur, doffsets)} and each frame's smallest |pre-activation| (test_hip_vjp._ref's kink measure)"""
    zt, ct, ot = (t.double().requires_grad_() for t in (z, cr, O))
    outs = _outputs(model, zt, ct, ot)
    res = {}
    for s in subsets:
        L = sum((outs[n] * grads[n].double()).sum() for n in s)
        got = torch.autograd.grad(L, (zt, ct, ot), retain_graph=True, allow_unused=True)
        res[s] = tuple((torch.zeros_like(t) if g_ is None else g_).numpy() for g_, t in zip(got, (zt, ct, ot)))
    with torch.no_grad():
        h = zt @ model.Wf.T + model.bf
        h = (h @ model.U[0].T) @ model.W[0].T + model.b[0]
        k0 = h.abs().amin(1)
        h = torch.nn.functional.leaky_relu(h, 0.2)
        h = (h @ model.U[1].T) @ model.W[1].T + model.b[1]
        kink = torch.minimum(k0, h.abs().amin(1)).numpy()
    return res, kink


def _gpu(opt, z, cr, O, grads, subset, dev):
    r = opt.forward_vjp(z.to(dev), cr.to(dev), {n: grads[n].to(dev) for n in subset}, offsets=O.to(dev), doffsets=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def test_the_restated_fk_is_the_oracles_on_one_skeleton():
    model = R.OracleModel(dtype=torch.float64)
    z, cr, _ = _inputs(64, seed=2)
    motion, disp = R.decoder_forward(model, z.double())
    wd, wr, pos, rot, d = R.pose_fk(model, motion, disp, cr.double())
    o = _outputs(model, z.double(), cr.double(), model.offsets.expand(64, NJ, 3))
    np.testing.assert_allclose(o["pos"].numpy(), pos.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(o["rot"].numpy(), rot.reshape(-1, NJ, 9).numpy(), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(o["world_disp"].numpy(), wd.numpy())


@pytest.mark.parametrize("wd", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 17, 4096, 65537])
def test_vjp_with_per_frame_skeletons_matches_fp64_autograd(opts, dev, wd, B):
    model = R.OracleModel(dtype=torch.float64, weight_rounding="bf16" if wd == "bf16" else "none")
    z, cr, grads = _inputs(B, seed=B + (7 if wd == "bf16" else 0))
    O = _per_frame(_base(), B, seed=B)
    subsets = [(n,) for n in NAMES] + [NAMES] if B <= 4096 else [NAMES]
    ref, kink = _ref(model, z, cr, O, grads, subsets)
    ok = kink >= 1e-5
    assert (~ok).sum() <= max(0.01 * B, 0), ((~ok).sum(), B)
    for s in subsets:
        r = _gpu(opts[wd], z, cr, O, grads, s, dev)
        assert (r["status"] == 0).all()
        _check(r["dz"], ref[s][0], ok)
        _check(r["dcur_rot"], ref[s][1], ok)
        _check(r["doffsets"].reshape(B, -1), ref[s][2].reshape(B, -1), ok)
        assert (r["doffsets"][:, 0] == 0).all()
        if "pos" not in s:  # (only the positions depend on the bones)
            assert (r["doffsets"] == 0).all(), s


def test_the_contexts_own_skeleton_gives_the_plain_bits(opts, dev):
    for wd, opt in opts.items():
        z, cr, grads = _inputs(4096, seed=31)
        z, cr = z.to(dev), cr.to(dev)
        grads = {n: t.to(dev) for n, t in grads.items()}
        own = torch.from_numpy(_base()).to(dev)
        want = opt.forward_vjp(z, cr, grads)
        for off in (own, own.expand(4096, NJ, 3).contiguous()):  # stride 0, stride 66
            for doff in (False, True):
                got = opt.forward_vjp(z, cr, grads, offsets=off, doffsets=doff)
                torch.cuda.synchronize()
                for k in ("dz", "dcur_rot", "status"):
                    assert torch.equal(got[k], want[k]), (wd, off.dim(), doff, k)
                assert ("doffsets" in got) == doff
        assert (want["status"] == 0).all()


def test_a_mixed_batch_equals_one_context_per_skeleton(opts, dev):
    from dragposer_amd.optimizer import LatentOptimizer

    main = opts["fp32"]
    skels = _skeletons(_base())
    B = 1024
    z, cr, grads = _inputs(B, seed=77)
    z, cr = z.to(dev), cr.to(dev)
    grads = {n: t.to(dev) for n, t in grads.items()}
    idx = np.arange(B) % len(skels)  # (every wave holds all four)
    off = torch.from_numpy(np.stack([skels[k] for k in idx])).to(dev)
    got = main.forward_vjp(z, cr, grads, offsets=off, doffsets=True)
    for k, s in enumerate(skels):
        ref = LatentOptimizer(device=dev, arrays=_raw(offsets=s))
        rows = torch.from_numpy(np.nonzero(idx == k)[0]).to(dev)
        want = ref.forward_vjp(z[rows].contiguous(), cr[rows].contiguous(), {n: t[rows].contiguous() for n, t in grads.items()})
        one = main.forward_vjp(z[rows].contiguous(), cr[rows].contiguous(), {n: t[rows].contiguous() for n, t in grads.items()},
                               offsets=torch.from_numpy(s).to(dev), doffsets=True)  # (stride 0 with that skeleton)
        torch.cuda.synchronize()
        for n in ("dz", "dcur_rot", "status"):
            assert torch.equal(got[n][rows], want[n]), (k, n)
            assert torch.equal(one[n], want[n]), (k, n)
        assert torch.equal(got["doffsets"][rows], one["doffsets"]), k
        ref.close()
    assert int(got["status"].abs().sum()) == 0


def test_another_tree_with_mixed_bone_lengths_matches_fp64_autograd(dev, tmp_path):
    from dragposer_amd.optimizer import LatentOptimizer
    from test_hip_topology import TREES, _model_arrays

    raw = _model_arrays(TREES["four_limbs_on_one_joint"], seed=5)
    path = str(tmp_path / "model.npz")
    np.savez(path, **raw)
    model = R.OracleModel(path, dtype=torch.float64)
    opt = LatentOptimizer(device=dev, arrays=raw)
    B = 600
    skels = _skeletons(np.asarray(raw["offsets"], np.float32))
    O = torch.from_numpy(np.stack([skels[f % 4] for f in range(B)]))
    z, cr, grads = _inputs(B, seed=13)
    ref, kink = _ref(model, z, cr, O, grads, [NAMES, ("pos",)])
    ok = kink >= 1e-5
    assert (~ok).sum() <= 6
    for s in ref:
        r = _gpu(opt, z, cr, O, grads, s, dev)
        assert (r["status"] == 0).all()
        _check(r["dz"], ref[s][0], ok)
        _check(r["dcur_rot"], ref[s][1], ok)
        _check(r["doffsets"].reshape(B, -1), ref[s][2].reshape(B, -1), ok)
    opt.close()


@pytest.mark.parametrize("form", ["per_frame", "one", "expanded"])
def test_decode_fk_with_offsets_matches_fp64_autograd(opts, dev, form):
    from dragposer_amd import decode_fk

    opt = opts["fp32"]
    model = R.OracleModel(dtype=torch.float64)
    B = 256
    z, cr, grads = _inputs(B, seed=41)
    base = torch.from_numpy(_base())
    if form == "per_frame":
        leaf = _per_frame(_base(), B, seed=41)
        O_of = lambda t: t  # noqa: E731
    elif form == "one":
        leaf = base * 1.07
        O_of = lambda t: t.expand(B, NJ, 3)  # noqa: E731
    else:
        leaf = base * 0.93
        O_of = lambda t: t.expand(B, NJ, 3)  # noqa: E731
    ref, kink = _ref(model, z, cr, O_of(leaf).contiguous(), grads, [NAMES])
    ok = kink >= 1e-5
    zd, cd = z.to(dev).requires_grad_(), cr.to(dev).requires_grad_()
    ld = leaf.to(dev).requires_grad_()
    off = ld.expand(B, NJ, 3) if form == "expanded" else ld  # (an expanded view: decode_fk makes it contiguous, autograd reduces it)
    o = decode_fk(opt, zd, cd, offsets=off)
    fwd = opt.forward(z.to(dev), cr.to(dev), offsets=O_of(leaf).to(dev).contiguous() if form == "expanded" else leaf.to(dev))
    for n in NAMES:
        assert o[n].grad_fn is not None and torch.equal(o[n].detach(), fwd[n]), n
    L = sum((o[n] * grads[n].to(dev)).sum() for n in NAMES)
    L.backward()
    torch.cuda.synchronize()
    _check(zd.grad.cpu().numpy(), ref[NAMES][0], ok)
    _check(cd.grad.cpu().numpy(), ref[NAMES][1], ok)
    want = ref[NAMES][2]
    if form == "per_frame":
        _check(ld.grad.cpu().numpy().reshape(B, -1), want.reshape(B, -1), ok)
    else:  # one skeleton for every frame: the frames' gradients summed (every frame counted -- a kink frame's gradient is still a gradient)
        got = ld.grad.cpu().numpy()
        s = want.sum(0)
        assert got.shape == (NJ, 3)
        np.testing.assert_allclose(got, s, rtol=0, atol=1e-4 * np.abs(s).max() + 1e-5 * np.abs(want).max() * np.sqrt(B))
    # the same dz, bit for bit, as forward_vjp with these offsets
    r = opt.forward_vjp(z.to(dev), cr.to(dev), {n: t.to(dev) for n, t in grads.items()}, offsets=O_of(ld.detach()).contiguous())
    assert torch.equal(zd.grad, r["dz"]) and torch.equal(cd.grad, r["dcur_rot"])


def test_offsets_without_requires_grad_get_no_gradient(opts, dev):
    from dragposer_amd import decode_fk

    opt = opts["fp32"]
    B = 64
    z, cr, grads = _inputs(B, seed=43)
    zd = z.to(dev).requires_grad_()
    off = _per_frame(_base(), B, seed=43).to(dev)
    asked = []  # (what each backward launch asked for)
    vjp = opt.forward_vjp
    opt.forward_vjp = lambda *a, **k: asked.append(k.get("doffsets", False)) or vjp(*a, **k)
    try:
        o = decode_fk(opt, zd, cr.to(dev), outputs=("pos",), offsets=off)
        (o["pos"] * grads["pos"].to(dev)).sum().backward()
        offg = off.clone().requires_grad_()
        (decode_fk(opt, z.to(dev), cr.to(dev), outputs=("pos",), offsets=offg)["pos"] * grads["pos"].to(dev)).sum().backward()
    finally:
        del opt.forward_vjp
    torch.cuda.synchronize()
    assert asked == [False, True]
    assert off.grad is None and zd.grad is not None and offg.grad is not None
    r = opt.forward_vjp(z.to(dev), cr.to(dev), {"pos": grads["pos"].to(dev)}, offsets=off)
    assert torch.equal(zd.grad, r["dz"]) and "doffsets" not in r
    # the root's OFFSET (row 0) is no input of the function
    base = torch.from_numpy(_base()).to(dev).requires_grad_()
    (decode_fk(opt, z.to(dev), cr.to(dev), outputs=("pos",), offsets=base)["pos"] * grads["pos"].to(dev)).sum().backward()
    assert (base.grad[0] == 0).all() and (base.grad[1:] != 0).any()


def test_refused_rows_poison_their_own_frame_only(opts, dev):
    from dragposer_amd import _lib

    opt = opts["fp32"]
    B = 256
    z, cr, grads = _inputs(B, seed=21)
    z, cr = z.to(dev), cr.to(dev)
    grads = {n: t.to(dev) for n, t in grads.items()}
    skels = _skeletons(_base())
    off = torch.from_numpy(np.stack([skels[f % 4] for f in range(B)])).to(dev)
    clean = opt.forward_vjp(z, cr, grads, offsets=off, doffsets=True)
    bad = off.clone()
    bad[41, 7, 1] = float("nan")   # frame 41: wave 0, lane 41
    bad[130, 1, 0] = 1e5           # frame 130: beyond DP_INPUT_LIMIT (a root child's bone)
    bad[200, 0, :] = float("nan")  # row 0 is never read: frame 200 stays clean
    got = opt.forward_vjp(z, cr, grads, offsets=bad, doffsets=True)
    fwd = opt.forward(z, cr, outputs=("pos", "status"), offsets=bad)
    torch.cuda.synchronize()
    st = got["status"].cpu().numpy()
    assert st[41] == _lib.DP_STATUS_BAD_STATE and st[130] == _lib.DP_STATUS_BAD_STATE and st[200] == 0
    # the same frames as dp_forward_skeleton refuses (which adds DP_STATUS_NONFINITE_RESULT to the word: dp_forward's convention)
    fst = fwd["status"].cpu().numpy()
    assert np.array_equal((st & _lib.DP_STATUS_BAD_STATE) != 0, (fst & _lib.DP_STATUS_BAD_STATE) != 0)
    assert np.count_nonzero(st) == 2
    for f in (41, 130):
        for k in ("dz", "dcur_rot", "doffsets"):
            assert torch.isnan(got[k][f]).all(), (f, k)
    keep = torch.ones(B, dtype=torch.bool, device=dev)
    keep[41] = keep[130] = False
    for k in ("dz", "dcur_rot", "doffsets", "status"):
        assert torch.equal(got[k][keep], clean[k][keep]), k  # (lane neighbours 40, 42 and 129, 131 included)


def test_determinism_and_graph_capture(opts, dev):
    opt = opts["fp32"]
    B = 1000
    z, cr, grads = _inputs(B, seed=3)
    z, cr = z.to(dev), cr.to(dev)
    grads = {n: t.to(dev) for n, t in grads.items()}
    off = _per_frame(_base(), B, seed=3).to(dev)
    a = opt.forward_vjp(z, cr, grads, offsets=off, doffsets=True)
    b = opt.forward_vjp(z, cr, grads, offsets=off, doffsets=True)
    torch.cuda.synchronize()
    for k in ("dz", "dcur_rot", "status", "doffsets"):
        assert torch.equal(a[k], b[k]), k
    assert (a["status"] == 0).all()
    out = {k: torch.full_like(v, -1) for k, v in a.items()}
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        opt.forward_vjp(z, cr, grads, out=out, offsets=off)  # (warm-up outside the capture; "doffsets" in out asks for them)
    torch.cuda.current_stream(dev).wait_stream(s)
    for v in out.values():
        v.fill_(-1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.forward_vjp(z, cr, grads, out=out, offsets=off)
    graph.replay()
    torch.cuda.synchronize()
    for k in ("dz", "dcur_rot", "status", "doffsets"):
        assert torch.equal(out[k], a[k]), k


def test_a_bone_scale_is_fitted_through_decode_fk_with_torch_adam(opts, dev):
    """targets made with every bone 1.1x the model's; a scalar scale fitted from 1.0 through decode_fk(offsets=s * base)"""
    from dragposer_amd import decode_fk

    opt = opts["fp32"]
    B = 64
    z, cr, _ = _inputs(B, seed=9)
    z, cr = z.to(dev), cr.to(dev)
    base = torch.from_numpy(_base()).to(dev)
    tgt = opt.forward(z, cr, outputs=("pos",), offsets=(1.1 * base).contiguous())["pos"]
    s = torch.ones((), device=dev, requires_grad=True)
    adam = torch.optim.Adam([s], lr=1e-2)
    for _ in range(300):
        o = decode_fk(opt, z, cr, outputs=("pos",), offsets=s * base)
        loss = ((o["pos"] - tgt) ** 2).sum(-1).mean()
        adam.zero_grad()
        loss.backward()
        adam.step()
    torch.cuda.synchronize()
    assert abs(float(s.detach()) - 1.1) < 1e-3, float(s.detach())

"""GPU (MI355X): dp_forward_vjp / decode_fk (include/dragposer_grad.h) against torch autograd through the fp64 oracle, against the fused
kernel's own gradient, on other skeletons, through a torch.optim.Adam loop, and for isolation, determinism and graph capture.

Frames with a pre-activation within 1e-5 of a LeakyReLU kink (fp64) are excluded from the gradient comparisons and counted: there
the derivative jumps (slope 1 <-> 0.2) and two correct implementations may pick different sides (tests/test_hip_parity.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_torch as R

pytestmark = pytest.mark.gpu

NAMES = ("pose", "disp", "world_disp", "world_rot", "pos", "rot")
SHAPES = {"pose": (88,), "disp": (3,), "world_disp": (3,), "world_rot": (4,), "pos": (22, 3), "rot": (22, 9)}
KEYS = ("z0", "z_tgt", "cur_rot", "tgt_pos", "tgt_rot", "w", "tracked")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def opts(dev):
    from dragposer_amd.optimizer import LatentOptimizer

    return {"fp32": LatentOptimizer(device=dev), "bf16": LatentOptimizer(device=dev, weight_dtype="bf16")}


def _inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, 24, generator=g) * 0.5
    cr = torch.randn(B, 4, generator=g)
    cr = cr / torch.linalg.norm(cr, dim=-1, keepdim=True) * (0.8 + 0.4 * torch.rand(B, 1, generator=g))  # cur_rot is used unnormalised
    grads = {n: torch.randn((B,) + SHAPES[n], generator=g) for n in NAMES}
    return z, cr, grads


def _ref(model, z, cr, grads, subsets):
    """fp64 torch autograd through oracle.ref_torch: {subset: (dz, dcur)} and each frame's smallest |pre-activation|"""
    zt = z.double().requires_grad_()
    ct = cr.double().requires_grad_()
    motion, disp = R.decoder_forward(model, zt)
    wd, wr, pos, rot, d = R.pose_fk(model, motion, disp, ct)
    outs = dict(pose=motion, disp=d, world_disp=wd, world_rot=wr, pos=pos, rot=rot.reshape(-1, 22, 9))
    res = {}
    for s in subsets:
        L = sum((outs[n] * grads[n].double()).sum() for n in s)
        gz, gc = torch.autograd.grad(L, (zt, ct), retain_graph=True, allow_unused=True)  # (pose alone does not reach cur_rot)
        res[s] = tuple((torch.zeros_like(t) if g_ is None else g_).numpy() for g_, t in ((gz, zt), (gc, ct)))
    with torch.no_grad():
        h = zt @ model.Wf.T + model.bf
        h = (h @ model.U[0].T) @ model.W[0].T + model.b[0]
        k0 = h.abs().amin(1)
        h = torch.nn.functional.leaky_relu(h, 0.2)
        h = (h @ model.U[1].T) @ model.W[1].T + model.b[1]
        kink = torch.minimum(k0, h.abs().amin(1)).numpy()
    return res, kink


def _gpu(opt, z, cr, grads, subset, dev):
    g = {n: grads[n].to(dev) for n in subset}
    r = opt.forward_vjp(z.to(dev), cr.to(dev), g)
    torch.cuda.synchronize()
    return r["dz"].cpu().numpy(), r["dcur_rot"].cpu().numpy(), r["status"].cpu().numpy()


def _check(got, want, ok):
    """|d| <= 1e-4 max|ref| + 1e-6 per frame, on the frames `ok`"""
    scale = np.abs(want).max(axis=1)
    err = np.abs(got - want).max(axis=1)
    bad = ok & ~(err <= 1e-4 * scale + 1e-6)
    assert not bad.any(), (np.nonzero(bad)[0][:8], err[bad][:8], scale[bad][:8])


@pytest.mark.parametrize("wd", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, 17, 4096, 65537])
def test_vjp_matches_fp64_autograd(opts, dev, wd, B):
    model = R.OracleModel(dtype=torch.float64, weight_rounding="bf16" if wd == "bf16" else "none")
    z, cr, grads = _inputs(B, seed=B + (7 if wd == "bf16" else 0))
    subsets = [(n,) for n in NAMES] + [NAMES] if B <= 4096 else [NAMES]
    ref, kink = _ref(model, z, cr, grads, subsets)
    ok = kink >= 1e-5
    assert (~ok).sum() <= max(0.01 * B, 0), ((~ok).sum(), B)
    for s in subsets:
        gz, gc, st = _gpu(opts[wd], z, cr, grads, s, dev)
        assert (st == 0).all()
        _check(gz, ref[s][0], ok)
        _check(gc, ref[s][1], ok)


@pytest.mark.parametrize("name", ["s1", "s3"])
def test_vjp_equals_the_fused_kernels_first_gradient(opts, dev, golden_dir, name):
    from dragposer_amd.optimizer import to_device_batch

    g = R.load_golden(os.path.join(golden_dir, f"{name}.npz"))
    opt = opts["bf16" if g["meta"]["weight_rounding"] == "bf16" else "fp32"]
    b = to_device_batch(g, dev)
    B = len(g["z0"])
    dbg = torch.zeros(B, 240, device=dev)
    opt.optimize(**b, n_iter=1, lambda_tmp=0.0, _debug=dbg)
    o = opt.forward(b["z0"], b["cur_rot"], outputs=("pos", "rot"))
    trk = b["tracked"].float()
    E = trk.sum(1, keepdim=True)
    cp = (2.0 * b["w"][..., 0] * trk / (3.0 * E)).unsqueeze(-1)
    cr_ = (2.0 * 1.0 * b["w"][..., 1] * trk / (9.0 * E)).unsqueeze(-1)
    gr = {"pos": cp * (o["pos"] - b["tgt_pos"]), "rot": cr_ * (o["rot"] - b["tgt_rot"])}
    r = opt.forward_vjp(b["z0"], b["cur_rot"], gr)
    torch.cuda.synchronize()
    np.testing.assert_allclose(r["dz"].cpu().numpy(), dbg.cpu().numpy()[:, 208:232], atol=2e-6, rtol=0)


@pytest.mark.parametrize("tree", ["arms_at_two_levels", "four_limbs_on_one_joint"])
def test_vjp_on_other_skeletons(dev, tmp_path, tree):
    from dragposer_amd.optimizer import LatentOptimizer
    from test_hip_topology import TREES, _model_arrays

    raw = _model_arrays(TREES[tree], seed=len(tree))
    path = str(tmp_path / "model.npz")
    np.savez(path, **raw)
    model = R.OracleModel(path, dtype=torch.float64)
    opt = LatentOptimizer(device=dev, arrays=raw)
    z, cr, grads = _inputs(300, seed=11)
    ref, kink = _ref(model, z, cr, grads, [NAMES, ("pos",), ("rot",)])
    ok = kink >= 1e-5
    assert (~ok).sum() <= 3
    for s in ref:
        gz, gc, _ = _gpu(opt, z, cr, grads, s, dev)
        _check(gz, ref[s][0], ok)
        _check(gc, ref[s][1], ok)


def test_reference_loss_through_decode_fk_with_torch_adam(opts, dev, golden_dir):
    """DragPose.loss (drag_pose.py:66-194) restated on decode_fk, torch.optim.Adam for 10 iterations, against dp_optimize(n_iter=10)"""
    from dragposer_amd import decode_fk
    from dragposer_amd.optimizer import to_device_batch
    from sensitivity import kink_distance

    g = R.load_golden(os.path.join(golden_dir, "s1.npz"))
    lam = g["meta"]["lambda_tmp"]
    opt = opts["fp32"]
    b = to_device_batch(g, dev)
    n_iter = 10
    ref = opt.optimize(**b, n_iter=n_iter, lambda_tmp=lam)
    z = b["z0"].clone().requires_grad_()
    adam = torch.optim.Adam([z], lr=1e-2)
    trk = b["tracked"].float()
    E = trk.sum(1)
    for _ in range(n_iter):
        o = decode_fk(opt, z, b["cur_rot"], outputs=("pos", "rot"))
        lp = (((o["pos"] - b["tgt_pos"]) ** 2).sum(-1) * b["w"][..., 0] * trk).sum(1) / (3.0 * E)
        lr_ = (((o["rot"] - b["tgt_rot"]) ** 2).sum(-1) * b["w"][..., 1] * trk).sum(1) / (9.0 * E)
        lt = lam * ((z - b["z_tgt"]) ** 2).mean(1)
        adam.zero_grad()
        (lp + lr_ + lt).sum().backward()
        adam.step()
    torch.cuda.synchronize()
    err = np.linalg.norm(o["pos"].detach().cpu().numpy() - ref["pos"].cpu().numpy(), axis=-1).max(1) * 1000.0
    off = np.nonzero(err > 0.05)[0]
    if len(off):  # (only where the trajectory passes a LeakyReLU kink, as in tests/test_hip_parity.py)
        kd = kink_distance(g, off, n_iter, lam)
        assert (kd < 1e-5).all() and err[off].max() < 3.0, (off, err[off], kd)
    assert len(off) <= 2, (off, err[off])


def test_isolation_determinism_and_graph_capture(opts, dev):
    opt = opts["fp32"]
    z, cr, grads = _inputs(1000, seed=3)
    z, cr = z.to(dev), cr.to(dev)
    grads = {n: t.to(dev) for n, t in grads.items()}
    a = opt.forward_vjp(z, cr, grads)
    b = opt.forward_vjp(z, cr, grads)
    torch.cuda.synchronize()
    for k in ("dz", "dcur_rot", "status"):
        assert torch.equal(a[k], b[k]), k
    assert (a["status"] == 0).all()
    zb = z.clone()
    zb[417, 5] = float("nan")
    cb = cr.clone()
    cb[3, 0] = 2.0e4  # beyond DP_INPUT_LIMIT
    c = opt.forward_vjp(zb, cb, grads)
    torch.cuda.synchronize()
    from dragposer_amd import _lib

    assert int(c["status"][417]) == _lib.DP_STATUS_BAD_STATE and int(c["status"][3]) == _lib.DP_STATUS_BAD_STATE
    assert torch.isnan(c["dz"][417]).all() and torch.isnan(c["dcur_rot"][417]).all() and torch.isnan(c["dz"][3]).all()
    keep = torch.ones(1000, dtype=torch.bool, device=dev)
    keep[[3, 417]] = False
    for k in ("dz", "dcur_rot", "status"):
        assert torch.equal(c[k][keep], a[k][keep]), k
    # a non-finite upstream gradient: that frame's dz is not finite and says so
    gn = {n: t.clone() for n, t in grads.items()}
    gn["pos"][9, 4, 1] = float("inf")
    d = opt.forward_vjp(z, cr, gn)
    torch.cuda.synchronize()
    assert int(d["status"][9]) == _lib.DP_STATUS_NONFINITE_RESULT and not torch.isfinite(d["dz"][9]).all()
    keep = torch.ones(1000, dtype=torch.bool, device=dev)
    keep[9] = False
    assert torch.equal(d["dz"][keep], a["dz"][keep])
    # one kernel node, captured and replayed
    out = {k: torch.full_like(v, -1) for k, v in a.items()}
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        opt.forward_vjp(z, cr, grads, out=out)  # (warm-up outside the capture)
    torch.cuda.current_stream(dev).wait_stream(s)
    for v in out.values():
        v.fill_(-1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.forward_vjp(z, cr, grads, out=out)
    graph.replay()
    torch.cuda.synchronize()
    for k in ("dz", "dcur_rot", "status"):
        assert torch.equal(out[k], a[k]), k


def test_decode_fk_gradients_and_double_backward(opts, dev):
    from dragposer_amd import decode_fk

    opt = opts["fp32"]
    z, cr, grads = _inputs(64, seed=5)
    zd = z.to(dev).requires_grad_()
    cd = cr.to(dev).requires_grad_()
    o = decode_fk(opt, zd, cd)
    fwd = opt.forward(z.to(dev), cr.to(dev))
    for n in NAMES:
        assert o[n].grad_fn is not None and torch.equal(o[n].detach(), fwd[n]), n
    L = sum((o[n] * grads[n].to(dev)).sum() for n in NAMES)
    gz, gc = torch.autograd.grad(L, (zd, cd), create_graph=True)
    r = opt.forward_vjp(z.to(dev), cr.to(dev), {n: t.to(dev) for n, t in grads.items()})
    assert torch.equal(gz.detach(), r["dz"]) and torch.equal(gc.detach(), r["dcur_rot"])
    # a second derivative: the upstream gradient of a squared output depends on that output
    gz2, = torch.autograd.grad((decode_fk(opt, zd, cd, outputs=("pos",))["pos"] ** 2).sum(), zd, create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice"):
        gz2.sum().backward()

"""ORACLE (test infrastructure): the constrained optimise loop of include/dragposer_constraints.h restated in torch on CPU, built on
oracle.ref_torch's primitives (decoder, FK, tracker losses, Adam as torch computes it).  Any dtype (the tests use fp64).  The four
extra terms follow DragPose.loss's `# Additional Losses` block (drag_pose.py:129-183), batched over frames, with G f for
quat.from_matrix(G) (x) f (G is a rotation)."""
import numpy as np
import torch

from oracle import ref_torch as R


def _h(v, up):
    m = torch.ones(3, dtype=v.dtype)
    m[up] = 0.0
    return v * m


def extra_terms(c, pos, rot, gp):
    """[B,4] unweighted terms: feet_floor, head_hips_forward, head_hips_colinear, hips_feet_colinear (rot: [B,22,3,3])"""
    up = c.up_axis
    B = pos.shape[0]
    fl = torch.zeros(B, dtype=pos.dtype)
    if c.w_feet_floor != 0.0:
        hs = [gp[:, up] + (pos[:, j, up] - c.floor_level) for j in c.floor_joints]
        fl = sum((torch.relu(-h) if c.floor_one_sided else h) ** 2 for h in hs) / len(hs)
    f = torch.tensor(c.fwd_axis, dtype=pos.dtype)
    a = _h(rot[:, c.head_joint] @ f, up)
    na = torch.linalg.norm(a, dim=-1)
    b = _h(rot[:, c.hips_joint] @ f, up)
    b = b / torch.linalg.norm(b, dim=-1, keepdim=True)
    s = (a / na.unsqueeze(-1) * b).sum(-1) + c.fwd_margin
    fw = torch.where(na > c.fwd_threshold, (1.0 - torch.clamp(s, max=1.0)) ** 2, torch.zeros_like(s))
    hc = (_h(pos[:, c.head_joint] - pos[:, c.hips_joint], up) ** 2).sum(-1)
    ft = sum(torch.clamp((_h(pos[:, c.hips_joint] - pos[:, j], up) ** 2).sum(-1) - c.feet_radius ** 2, min=0.0) for j in c.foot_joints)
    return torch.stack((fl, fw, hc, ft), dim=1)


def optimize_constrained(model, batch, c, global_pos, n_iter, lr=1e-2, lam_rot=1.0, lam_tmp=0.02, betas=(0.9, 0.999), eps=1e-8,
                         stop_eps_pos=0.0, stop_eps_rot=0.0, min_loss_incr=None):
    """-> dict(pos, rot, z_final, z_pre, iters, loss [B,3], loss_extra [B,4], kink [B]) of the last forward pass (early stop per frame as
    dp_optimize; `kink`: the smallest |pre-activation| or |distance of a min/max/threshold from its switch| along the trajectory)"""
    dt = model.dtype
    cv = lambda k: torch.as_tensor(np.asarray(batch[k])).to(dt)
    z0, zt, cr, tp, tr, w = (cv(k) for k in ("z0", "z_tgt", "cur_rot", "tgt_pos", "tgt_rot", "w"))
    trk = torch.as_tensor(np.asarray(batch["tracked"])).bool()
    gp = torch.as_tensor(np.asarray(global_pos)).to(dt)
    wk = torch.tensor([c.w_feet_floor, c.w_head_hips_forward, c.w_head_hips_colinear, c.w_hips_feet_colinear], dtype=dt)
    B = z0.shape[0]
    z = z0.clone()
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    active = torch.ones(B, dtype=torch.bool)
    prev = torch.full((B,), 10000000.0, dtype=dt)
    iters = torch.zeros(B, dtype=torch.int32)
    keep = {}
    kink = torch.full((B,), float("inf"), dtype=dt)
    hist = torch.full((B, n_iter, 3), float("nan"), dtype=dt)  # loss_pos, loss_rot (weighted), total of every executed pass
    min_incr = -float("inf") if min_loss_incr is None else min_loss_incr
    for it, (step, bc2s) in enumerate(R.adam_scalars(n_iter, lr, betas)):
        if not bool(active.any()):
            break
        zz = z.clone().requires_grad_()
        motion, disp = R.decoder_forward(model, zz)
        lp, lr_, lt, fk = R.frame_losses(model, zz, motion, disp, cr, zt, tp, tr, w, trk, lam_rot, lam_tmp)
        ex = extra_terms(c, fk["pos"], fk["rot"], gp) * wk
        tot = lp + lr_ + lt + ex[:, [1, 2, 0, 3]].sum(1)
        (g,) = torch.autograd.grad(tot.sum(), zz)
        with torch.no_grad():
            h = zz @ model.Wf.T + model.bf
            h0 = (h @ model.U[0].T) @ model.W[0].T + model.b[0]
            h1 = (torch.nn.functional.leaky_relu(h0, 0.2) @ model.U[1].T) @ model.W[1].T + model.b[1]
            sw = _switch_distance(c, fk, gp)
            kink = torch.where(active, torch.minimum(kink, torch.minimum(torch.minimum(h0.abs().amin(1), h1.abs().amin(1)), sw)), kink)
            for name, val in (("pos", fk["pos"]), ("rot", fk["rot"].reshape(B, 22, 9)), ("z_pre", z), ("loss", torch.stack((lp, lr_, lt), 1)),
                              ("loss_extra", ex)):
                if name not in keep:
                    keep[name] = val.detach().clone()
                else:
                    keep[name][active] = val.detach()[active]
            hist[active, it] = torch.stack((lp, lr_, tot), 1).detach()[active]
            a = active.unsqueeze(1)
            m_new = m + (1.0 - betas[0]) * (g - m)
            v_new = v * betas[1] + (1.0 - betas[1]) * g * g
            z_new = z - step * (m_new / (v_new.sqrt() / bc2s + eps))
            m, v, z = torch.where(a, m_new, m), torch.where(a, v_new, v), torch.where(a, z_new, z)
            iters += active.to(torch.int32)
            t = tot.detach()
            cont = ((lp > stop_eps_pos) | (lr_ > stop_eps_rot)) & (prev - t > min_incr)
            prev = torch.where(active, t, prev)
            active = active & cont
    out = {k: x.numpy() for k, x in keep.items()}
    out.update(z_final=z.numpy(), iters=iters.numpy(), kink=kink.numpy(), hist=hist.numpy())
    return out


def near_stop(ref, f, lo, hi, stop_eps_pos, stop_eps_rot, min_loss_incr, rel=2e-5):
    """whether a decision of the while-condition of frame f, at an iteration in lo..hi of the oracle's trajectory, sits within `rel` of
    its threshold (loss_pos vs stop_eps_pos, loss_rot vs stop_eps_rot, the decrement of the total vs min_loss_incr, against the total):
    where two correct implementations may decide it differently (tests/test_hip_instantiations.py: STOP_ROUNDING)"""
    h = ref["hist"][f]
    for k in range(max(lo, 1), min(hi, h.shape[0]) + 1):
        lp, lr_, tot = h[k - 1]
        if not np.isfinite(tot):
            break
        incr = (h[k - 2, 2] if k > 1 else 10000000.0) - tot
        if (abs(lp - stop_eps_pos) <= rel * max(abs(lp), stop_eps_pos) or abs(lr_ - stop_eps_rot) <= rel * max(abs(lr_), stop_eps_rot)
                or abs(incr - min_loss_incr) <= rel * abs(tot)):
            return True
    return False


def _switch_distance(c, fk, gp):
    """per frame: how close a min / max / relu / threshold of the extra terms sits to its switch"""
    pos, rot, up = fk["pos"], fk["rot"], c.up_axis
    B = pos.shape[0]
    d = torch.full((B,), float("inf"), dtype=pos.dtype)
    if c.w_feet_floor != 0.0 and c.floor_one_sided:
        for j in c.floor_joints:
            d = torch.minimum(d, (gp[:, up] + pos[:, j, up] - c.floor_level).abs())
    if c.w_head_hips_forward != 0.0:
        f = torch.tensor(c.fwd_axis, dtype=pos.dtype)
        a = _h(rot[:, c.head_joint] @ f, up)
        na = torch.linalg.norm(a, dim=-1)
        b = _h(rot[:, c.hips_joint] @ f, up)
        b = b / torch.linalg.norm(b, dim=-1, keepdim=True)
        s = (a / na.unsqueeze(-1) * b).sum(-1) + c.fwd_margin
        d = torch.minimum(d, torch.minimum((na - c.fwd_threshold).abs(), (s - 1.0).abs()))
    if c.w_hips_feet_colinear != 0.0:
        for j in c.foot_joints:
            d = torch.minimum(d, ((_h(pos[:, c.hips_joint] - pos[:, j], up) ** 2).sum(-1) - c.feet_radius ** 2).abs())
    return d

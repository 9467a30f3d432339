"""ORACLE (test infrastructure): the term-table optimise loop of include/dragposer_terms.h restated in torch on CPU, on oracle.ref_torch's
primitives (decoder, FK, tracker losses, Adam as torch computes it) -- tests/constraints_oracle.py's loop with the table's loss in place
of the four fixed terms.  Any dtype (the tests use fp64).  `term_grads` is the analytic upstream gradient the kernel accumulates
(dL/dP_j, dL/dG_j), held to torch autograd by tests/test_terms_oracle.py."""
import numpy as np
import torch

from dragposer_amd.terms import ALIGN, DISTANCE, DROP_UP, ONE_SIDED, PLANE
from oracle import ref_torch as R


def _h(v, up, on):
    if not on:
        return v
    m = torch.ones(3, dtype=v.dtype, device=v.device)
    m[up] = 0.0
    return v * m


def rows_of(t, B, dt, dev="cpu"):
    """[B,4] (vector, s_f) of a term: its per-frame rows, or its own point / dir and s = 1"""
    if t.per_frame is not None and t.weight != 0.0:
        pf = t.per_frame
        return (pf.detach() if isinstance(pf, torch.Tensor) else torch.as_tensor(np.asarray(pf))).to(device=dev, dtype=dt)
    v = t.dir if t.type == ALIGN else t.point
    return torch.tensor([*v, 1.0], dtype=dt, device=dev).expand(B, 4)


def term_values(terms, pos, rot, gp):
    """[B, n] weighted terms weight * s_f * T (pos [B,22,3], rot [B,22,3,3], gp [B,3]); also [B] the distance of the nearest switch.
    Differentiable, on the device of `pos` (the decode_fk loop of tests/test_hip_terms.py uses it on the GPU)"""
    up = terms.up_axis
    B, dt, dev = pos.shape[0], pos.dtype, pos.device
    cst = lambda v: torch.tensor(v, dtype=dt, device=dev)
    vals, sw = [], torch.full((B,), float("inf"), dtype=dt, device=dev)
    for t in terms.terms:
        row = rows_of(t, B, dt, dev)
        ws = t.weight * row[:, 3]
        drop = bool(t.flags & DROP_UP)
        if t.weight == 0.0:
            vals.append(torch.zeros(B, dtype=dt, device=dev))
            continue
        if t.type == PLANE:
            d = ((gp + pos[:, t.joint_a] - row[:, :3]) * cst(t.dir)).sum(-1)
            if t.flags & ONE_SIDED:
                T = torch.relu(-d) ** 2
                sw = torch.minimum(sw, torch.where(ws != 0, d.abs(), torch.full_like(d, float("inf"))))
            else:
                T = d ** 2
        elif t.type == DISTANCE:
            u = pos[:, t.joint_a] - pos[:, t.joint_b] if t.joint_b >= 0 else gp + pos[:, t.joint_a] - row[:, :3]
            q = (_h(u, up, drop) ** 2).sum(-1)
            lo2, hi2 = t.p0 ** 2, t.p1 ** 2
            T = torch.relu(q - hi2) + torch.relu(lo2 - q)
            if not (t.p0 == 0.0 and t.p1 == 0.0):
                sw = torch.minimum(sw, torch.where(ws != 0, torch.minimum((q - hi2).abs(), (q - lo2).abs()),
                                                   torch.full_like(q, float("inf"))))
        else:
            a = _h(rot[:, t.joint_a] @ cst(t.axis_a), up, drop)
            na = torch.linalg.norm(a, dim=-1)
            b = _h(rot[:, t.joint_b] @ cst(t.axis_b) if t.joint_b >= 0 else row[:, :3], up, drop)
            b = b / torch.linalg.norm(b, dim=-1, keepdim=True)
            c = (a / na.unsqueeze(-1) * b).sum(-1) + t.p1
            T = torch.where(na > t.p0, (1.0 - torch.clamp(c, max=1.0)) ** 2, torch.zeros_like(c))
            sw = torch.minimum(sw, torch.where(ws != 0, torch.minimum((na - t.p0).abs(), (c - 1.0).abs()), torch.full_like(c, float("inf"))))
        vals.append(torch.where(ws != 0, ws * T, torch.zeros_like(T)))
    return (torch.stack(vals, 1) if vals else torch.zeros(B, 0, dtype=dt, device=dev)), sw


def term_grads(terms, pos, rot, gp):
    """the analytic dL/dP [B,22,3] and dL/dG [B,22,3,3] of sum(term_values) -- the kernel's formulas (dp_cons_body.h), in torch"""
    up = terms.up_axis
    B, dt = pos.shape[0], pos.dtype
    gP, gG = torch.zeros_like(pos), torch.zeros_like(rot)
    for t in terms.terms:
        if t.weight == 0.0:
            continue
        row = rows_of(t, B, dt)
        ws = (t.weight * row[:, 3]).unsqueeze(-1)
        drop = bool(t.flags & DROP_UP)
        if t.type == PLANE:
            n = torch.tensor(t.dir, dtype=dt)
            d = ((gp + pos[:, t.joint_a] - row[:, :3]) * n).sum(-1, keepdim=True)
            g = torch.clamp(d, max=0.0) if t.flags & ONE_SIDED else d
            gP[:, t.joint_a] += 2.0 * ws * g * n
        elif t.type == DISTANCE:
            u = pos[:, t.joint_a] - pos[:, t.joint_b] if t.joint_b >= 0 else gp + pos[:, t.joint_a] - row[:, :3]
            u = _h(u, up, drop)
            q = (u ** 2).sum(-1, keepdim=True)
            lo2, hi2 = t.p0 ** 2, t.p1 ** 2
            dq = ws * ((q > hi2).to(dt) - (q < lo2).to(dt))
            gP[:, t.joint_a] += 2.0 * dq * u
            if t.joint_b >= 0:
                gP[:, t.joint_b] -= 2.0 * dq * u
        else:
            xa, xb = torch.tensor(t.axis_a, dtype=dt), torch.tensor(t.axis_b, dtype=dt)
            a = _h(rot[:, t.joint_a] @ xa, up, drop)
            na = torch.linalg.norm(a, dim=-1, keepdim=True)
            b = _h(rot[:, t.joint_b] @ xb if t.joint_b >= 0 else row[:, :3], up, drop)
            nb = torch.linalg.norm(b, dim=-1, keepdim=True)
            ah, bh = a / na, b / nb
            cs = (ah * bh).sum(-1, keepdim=True)
            s = cs + t.p1
            on = (na > t.p0) & (s < 1.0)
            ds = torch.where(on, -2.0 * (1.0 - s) * ws, torch.zeros_like(s))
            da = _h((bh - ah * cs) / na, up, drop)
            gG[:, t.joint_a] += (ds * da).unsqueeze(-1) * xa
            if t.joint_b >= 0:
                db = _h((ah - bh * cs) / nb, up, drop)
                gG[:, t.joint_b] += (ds * db).unsqueeze(-1) * xb
    return gP, gG


def optimize_terms(model, batch, terms, global_pos, n_iter, lr=1e-2, lam_rot=1.0, lam_tmp=0.02, betas=(0.9, 0.999), eps=1e-8,
                   stop_eps_pos=0.0, stop_eps_rot=0.0, min_loss_incr=None):
    """-> dict(pos, rot, z_final, z_pre, iters, loss [B,3], loss_terms [B,n], kink [B], hist) of the last forward pass (early stop per
    frame as dp_optimize); constraints_oracle.optimize_constrained's loop and conventions"""
    dt = model.dtype
    cv = lambda k: torch.as_tensor(np.asarray(batch[k])).to(dt)
    z0, zt, cr, tp, tr, w = (cv(k) for k in ("z0", "z_tgt", "cur_rot", "tgt_pos", "tgt_rot", "w"))
    trk = torch.as_tensor(np.asarray(batch["tracked"])).bool()
    B = z0.shape[0]
    gp = torch.zeros(B, 3, dtype=dt) if global_pos is None else torch.as_tensor(np.asarray(global_pos)).to(dt)
    z = z0.clone()
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    active = torch.ones(B, dtype=torch.bool)
    prev = torch.full((B,), 10000000.0, dtype=dt)
    iters = torch.zeros(B, dtype=torch.int32)
    keep = {}
    kink = torch.full((B,), float("inf"), dtype=dt)
    hist = torch.full((B, n_iter, 3), float("nan"), dtype=dt)
    for it, (step, bc2s) in enumerate(R.adam_scalars(n_iter, lr, betas)):
        if not bool(active.any()):
            break
        zz = z.clone().requires_grad_()
        motion, disp = R.decoder_forward(model, zz)
        lp, lr_, lt, fk = R.frame_losses(model, zz, motion, disp, cr, zt, tp, tr, w, trk, lam_rot, lam_tmp)
        ex, sw = term_values(terms, fk["pos"], fk["rot"], gp)
        tot = lp + lr_ + lt + ex.sum(1)
        (g,) = torch.autograd.grad(tot.sum(), zz)
        with torch.no_grad():
            h = zz @ model.Wf.T + model.bf
            h0 = (h @ model.U[0].T) @ model.W[0].T + model.b[0]
            h1 = (torch.nn.functional.leaky_relu(h0, 0.2) @ model.U[1].T) @ model.W[1].T + model.b[1]
            kink = torch.where(active, torch.minimum(kink, torch.minimum(torch.minimum(h0.abs().amin(1), h1.abs().amin(1)), sw.detach())), kink)
            for name, val in (("pos", fk["pos"]), ("rot", fk["rot"].reshape(B, 22, 9)), ("z_pre", z), ("loss", torch.stack((lp, lr_, lt), 1)),
                              ("loss_terms", ex)):
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
            cont = ((lp > stop_eps_pos) | (lr_ > stop_eps_rot)) & (prev - t > (-float("inf") if min_loss_incr is None else min_loss_incr))
            prev = torch.where(active, t, prev)
            active = active & cont
    out = {k: x.numpy() for k, x in keep.items()}
    out.update(z_final=z.numpy(), iters=iters.numpy(), kink=kink.numpy(), hist=hist.numpy())
    return out

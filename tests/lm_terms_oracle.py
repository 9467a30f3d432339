"""ORACLE of dp_optimize_lm_terms (include/dragposer_lm_terms.h, "The algorithm"): tests/lm_oracle.py's Levenberg-Marquardt loop with the
term table's rows in [J | r] and the table's TRUE terms (tests/terms_oracle.py: term_values) in the loss that accepts a trial.  In torch on
the CPU, in the model's dtype (fp64 or fp32).  The rows come from torch.func.jacfwd of the row function with the active set frozen at z.

Rows, with c = weight * s_f:  PLANE, when two-sided or d < 0: sqrt(c) d.  DISTANCE: q > hi^2: sqrt(c) u (three rows); q < lo^2:
sqrt(c (lo^2 - q)); lo^2 and hi^2 the float32 products the library stores.  ALIGN, when |u| > p0 and c < 1: sqrt(c_k) (1 - c)."""
import numpy as np
import torch

import lm_oracle as LO
import terms_oracle as TO
from dragposer_amd.terms import ALIGN, DISTANCE, DROP_UP, ONE_SIDED, PLANE
from oracle import ref_torch as R

NONE, K_PLANE, K_HI, K_LO, K_ALIGN = 0, 1, 2, 3, 4


def _sq32(x):
    """x * x as the library stores it: a float32 product"""
    return float(np.float32(x) * np.float32(x))


def _fk(model, z, cr):
    motion, disp = R.decoder_forward(model, z)
    _, _, pos, rot, _ = R.pose_fk(model, motion, disp, cr)
    return pos, rot


def _all_rows(terms, B, dt):
    """[B, n, 4] every term's (vector, s_f)"""
    return torch.stack([TO.rows_of(t, B, dt) for t in terms.terms], 1) if len(terms) else torch.zeros(B, 0, 4, dtype=dt)


def _geometry(t, up, pos, rot, gp, row):
    """what a term is made of at one frame (pos [22,3], rot [22,3,3], gp [3], row [4]): PLANE d; DISTANCE (u, q); ALIGN (|u|, c)"""
    cst = lambda v: torch.tensor(v, dtype=pos.dtype)
    drop = bool(t.flags & DROP_UP)
    if t.type == PLANE:
        return (((gp + pos[t.joint_a] - row[:3]) * cst(t.dir)).sum(),)
    if t.type == DISTANCE:
        u = pos[t.joint_a] - pos[t.joint_b] if t.joint_b >= 0 else gp + pos[t.joint_a] - row[:3]
        u = TO._h(u, up, drop)
        return u, (u ** 2).sum()
    a = TO._h(rot[t.joint_a] @ cst(t.axis_a), up, drop)
    na = torch.linalg.norm(a)
    b = TO._h(rot[t.joint_b] @ cst(t.axis_b) if t.joint_b >= 0 else row[:3], up, drop)
    return na, (a / na * (b / torch.linalg.norm(b))).sum() + t.p1


def kinds_at(terms, pos, rot, gp, rows):
    """[B, n] int64: the active set at these joints, strict inequalities (NONE, K_PLANE, K_HI, K_LO, K_ALIGN); c = 0 is NONE"""
    B = pos.shape[0]
    out = torch.zeros(B, len(terms), dtype=torch.int64)
    for f in range(B):
        for k, t in enumerate(terms.terms):
            if t.weight == 0.0 or float(rows[f, k, 3]) == 0.0:
                continue
            g = _geometry(t, terms.up_axis, pos[f], rot[f], gp[f], rows[f, k])
            if t.type == PLANE:
                out[f, k] = K_PLANE if not (t.flags & ONE_SIDED) or bool(g[0] < 0) else NONE
            elif t.type == DISTANCE:
                out[f, k] = K_HI if bool(g[1] > _sq32(t.p1)) else K_LO if bool(g[1] < _sq32(t.p0)) else NONE
            else:
                out[f, k] = K_ALIGN if bool(g[0] > t.p0) and bool(g[1] < 1.0) else NONE
    return out


def rows_fn(model, terms):
    """f(z, cur_rot, gp, rows [n,4], kinds [n]) -> the terms' 3n residual rows of one frame, the active set as `kinds` says"""
    def f(z, cr, gp, rows, kinds):
        pos, rot = _fk(model, z[None], cr[None])
        pos, rot = pos[0], rot[0]
        zero = z.new_zeros(())
        out = []
        for k, t in enumerate(terms.terms):
            if t.weight == 0.0:
                out += [zero, zero, zero]
                continue
            c = t.weight * rows[k, 3]
            sc = torch.sqrt(c)
            g = _geometry(t, terms.up_axis, pos, rot, gp, rows[k])
            if t.type == PLANE:
                out += [torch.where(kinds[k] == K_PLANE, sc * g[0], zero), zero, zero]
            elif t.type == DISTANCE:
                u, q = g
                lo = torch.sqrt(torch.where(kinds[k] == K_LO, c * (_sq32(t.p0) - q), torch.ones_like(q)))
                out += [torch.where(kinds[k] == K_HI, sc * u[0], torch.where(kinds[k] == K_LO, lo, zero)),
                        torch.where(kinds[k] == K_HI, sc * u[1], zero), torch.where(kinds[k] == K_HI, sc * u[2], zero)]
            else:
                out += [torch.where(kinds[k] == K_ALIGN, sc * (1.0 - g[1]), zero), zero, zero]
        return torch.stack(out) if out else z.new_zeros(0)

    return f


def total(model, terms, z, t, gp, lam_rot, lam_tmp):
    """-> (loss [B,3], loss_terms [B,n], switch distance [B], fk) at z: the three numbers and the true weighted terms"""
    loss, fk = LO.forward(model, z, t, lam_rot, lam_tmp)
    with torch.no_grad():
        vals, sw = TO.term_values(terms, fk["pos"], fk["rot"], gp)
    return loss, vals, sw, fk


def normal_equations(model, terms, z, t, gp, rows, lam_rot, lam_tmp, drop_rows=False, lo_rows="sqrt"):
    """-> A, g, kinds at z over tracker, term and pull rows.  drop_rows: the terms' rows left out of both (the power check);
    lo_rows="zero": a DISTANCE below lo adds its row to g only (the zero-curvature variant)"""
    A, g = LO.normal_equations(model, z, t, lam_rot, lam_tmp)
    with torch.no_grad():
        pos, rot = _fk(model, z, t["cur_rot"])
        kinds = kinds_at(terms, pos, rot, gp, rows)
    if len(terms) and not drop_rows:
        f = rows_fn(model, terms)
        args = (z, t["cur_rot"], gp, rows, kinds)
        J = torch.func.vmap(torch.func.jacfwd(f))(*args)
        r = torch.func.vmap(f)(*args)
        J, r = J.to(z.dtype), r.to(z.dtype)
        g = g + (J.transpose(1, 2) @ r[..., None])[..., 0]
        if lo_rows == "zero":
            J = J * (kinds != K_LO).repeat_interleave(3, dim=1).to(J.dtype)[..., None]
        A = A + J.transpose(1, 2) @ J
    return A, g, kinds


def lm_terms(model, batch, terms, global_pos, n_steps, lam_rot=1.0, lam_tmp=0.02, mu=None, early_stop=False, stop_eps_pos=0.0, stop_eps_rot=0.0,
             drop_rows=False, lo_rows="sqrt", **kw):
    """n_steps LM steps with the table.  lm_oracle.lm's dict -- `loss`, `loss0` the three numbers; `loss_hist` and `margin` of the TOTAL with
    the terms -- plus loss_terms [B,n] (at z), loss_terms0 (at z0), switch [B,n_steps+1] (the switch distance at every kept latent; [:, 0] is
    z0's), kinds0 [B,n] (the active set at z0)."""
    p = dict(LO.DEFAULTS, **kw)
    dt = model.dtype
    t = LO._conv(model, batch)
    B = t["z0"].shape[0]
    gp = torch.zeros(B, 3, dtype=dt) if global_pos is None else torch.as_tensor(np.asarray(global_pos)).to(dt)
    rows = _all_rows(terms, B, dt)
    z = t["z0"].clone()
    mu_t = torch.full((B,), p["mu0"], dtype=dt) if mu is None else torch.as_tensor(mu).to(dt).clone()
    loss, vals, sw, _ = total(model, terms, z, t, gp, lam_rot, lam_tmp)
    loss0, vals0 = loss.clone(), vals.clone()
    active = torch.ones(B, dtype=torch.bool)
    hit_max = torch.zeros(B, dtype=torch.bool)
    n_acc = torch.zeros(B, dtype=torch.int32)
    iters = torch.zeros(B, dtype=torch.int32)
    accepted = torch.zeros(B, n_steps, dtype=torch.bool)
    ran = torch.zeros(B, n_steps, dtype=torch.bool)
    margin = torch.full((B, n_steps), float("nan"), dtype=dt)
    hist, switch, kinds0 = [loss.sum(1) + vals.sum(1)], [sw.clone()], None
    eye = torch.eye(24, dtype=dt)
    for s in range(n_steps):
        if early_stop:
            active = active & ~((loss[:, 0] <= stop_eps_pos) & (loss[:, 1] <= stop_eps_rot)) & ~hit_max
        A, g, kinds = normal_equations(model, terms, z, t, gp, rows, lam_rot, lam_tmp, drop_rows, lo_rows)
        kinds0 = kinds if kinds0 is None else kinds0
        H = A + mu_t[:, None, None] * (A * eye)
        Lc, info = torch.linalg.cholesky_ex(H)
        ok = (info == 0) & torch.isfinite(Lc).all(dim=(1, 2))
        Lc = torch.where(ok[:, None, None], Lc, eye.expand(B, 24, 24))
        delta = torch.cholesky_solve(-g[..., None], Lc)[..., 0]
        zn = z + delta
        ln, vn, swn, _ = total(model, terms, zn, t, gp, lam_rot, lam_tmp)
        tot, totn = loss.sum(1) + vals.sum(1), ln.sum(1) + vn.sum(1)
        acc = active & ok & (totn < tot)
        rej = active & ~acc
        margin[:, s] = torch.where(active, (totn - tot).abs() / tot, margin[:, s])
        ran[:, s], accepted[:, s] = active, acc
        z = torch.where(acc[:, None], zn, z)
        loss, vals, sw = torch.where(acc[:, None], ln, loss), torch.where(acc[:, None], vn, vals), torch.where(acc, swn, sw)
        hit_max = rej & (mu_t >= p["mu_max"])
        mu_t = torch.where(acc, torch.clamp(mu_t * p["mu_down"], min=p["mu_min"]), torch.where(rej, torch.clamp(mu_t * p["mu_up"], max=p["mu_max"]), mu_t))
        n_acc += acc.to(torch.int32)
        iters += active.to(torch.int32)
        hist.append(loss.sum(1) + vals.sum(1))
        switch.append(sw.clone())
    return dict(z=z.numpy(), loss=loss.numpy(), loss0=loss0.numpy(), n_accepted=n_acc.numpy(), iters=iters.numpy(), mu=mu_t.numpy(),
                accepted=accepted.numpy(), ran=ran.numpy(), margin=margin.numpy(), loss_hist=torch.stack(hist, dim=1).numpy(),
                loss_terms=vals.numpy(), loss_terms0=vals0.numpy(), switch=torch.stack(switch, dim=1).numpy(),
                kinds0=(kinds0 if kinds0 is not None else torch.zeros(B, len(terms), dtype=torch.int64)).numpy())


def terms_np(model, terms, z, batch, global_pos):
    """[B, n] the weighted terms at the latents z, in the model's dtype (the GPU test's reference for loss_terms)"""
    t = LO._conv(model, batch)
    dt = model.dtype
    gp = torch.zeros(len(z), 3, dtype=dt) if global_pos is None else torch.as_tensor(np.asarray(global_pos)).to(dt)
    return total(model, terms, torch.as_tensor(z).to(dt), t, gp, 1.0, 0.0)[1].numpy()


def folded_model(host_model):
    """an fp64 OracleModel whose decoder is the context's folded fp32 matrices (dragposer_amd.model.HostModel.fold), applied in double:
    the function the kernels' pass in double evaluates (include/dragposer_lm.h: "evaluated once more in double on the same fp32 weights").
    The oracle's own weights, folded in double, differ from these by their rounding to fp32: 6e-7 on a decoder output, 1e-7 m on a joint."""
    f, _ = host_model.fold()
    m = R.OracleModel(dtype=torch.float64)
    d = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    m.Wf, m.bf = torch.eye(24, dtype=torch.float64), torch.zeros(24, dtype=torch.float64)
    m.U = [torch.eye(n, dtype=torch.float64) for n in (24, 40, 60)]
    m.W, m.b = [d(f["A0"]), d(f["A1"]), d(f["A2"])], [d(f["c0"]), d(f["b1"]), d(f["b2"])]
    return m


def cpu_terms(terms):
    """`terms` with every per_frame tensor on the CPU (the oracle's copy of a table whose rows live on the device)"""
    from dataclasses import replace

    from dragposer_amd import Terms

    return Terms([replace(t, per_frame=t.per_frame.detach().cpu()) if t.per_frame is not None else t for t in terms.terms], terms.up_axis)


PLANE_Y = 0.55  # plane_one_sided's floor, moved up from tests/test_hip_terms.py's 0.02 until a quarter of the frames have a foot below it


def global_pos(B, seed=11):
    """[B,3] float32, as tests/test_hip_constraints.py::_inputs draws it"""
    g = torch.Generator().manual_seed(seed + 1)
    gp = (torch.randn(B, 3, generator=g) * 0.1).numpy().astype(np.float32)
    gp[:, 1] += 0.9
    return gp


def tables(B, dev):
    """name -> Terms: tests/test_hip_terms.py's six cases (plane_one_sided with its plane at PLANE_Y), CUSTOM(), two pins with per-frame rows,
    and 16 terms of every type, which fill both rounds of the kernel's term pass and all four sub-slots of a half.  The bands of that table
    have lo and hi whose squares are exact in float32 (0.0625 .. 0.75): the library compares q with the float32 products lo^2 and hi^2 its
    table stores, as its header says, terms_oracle.term_values squares them in double, and for lo = 0.6 the two differ by 1.5e-8, more than
    loss_terms' bar allows a slot of 6e-4 (measured: 1.6e-8 on DISTANCE(20, 16, lo=0.6, hi=0.7), on the oracle's and on the folded weights)"""
    import test_hip_terms as HT
    from dragposer_amd import Term, Terms

    s = 0.5 ** 0.5
    c = dict(HT._cases(B, dev))
    c["plane_one_sided"] = Terms([Term.plane(4, (0, 1, 0), (0, PLANE_Y, 0), weight=3.0, one_sided=True)])
    c["custom"] = HT.CUSTOM()
    c["pins"] = Terms([Term.distance(17, weight=2.0, per_frame=HT._rows(B, (0.3, 1.0, 0.2), dev, 4, scale=2.0, noise=0.1)),
                       Term.distance(4, weight=1.0, per_frame=HT._rows(B, (0.1, 0.05, 0.0), dev, 5, noise=0.1))])
    c["mixed16"] = Terms([
        Term.plane(4, (0, 1, 0), (0, PLANE_Y, 0), weight=3.0, one_sided=True), Term.plane(8, (0, 1, 0), (0, PLANE_Y, 0), weight=3.0, one_sided=True),
        Term.plane(17, (s, s, 0), (0.0, 0.6, 0.0), weight=0.5, per_frame=HT._rows(B, (0.0, 0.6, 0.0), dev, 6)),
        Term.distance(3, 7, lo=0.25, hi=0.5, weight=3.0), Term.distance(13, 0, lo=0.125, hi=0.25, drop_up=True),
        Term.distance(2, 6, lo=0.25, hi=10.0, weight=4.0, drop_up=True),
        Term.distance(21, point=(0.3, 1.0, 0.1), lo=0.0625, hi=0.125, weight=2.0, per_frame=HT._rows(B, (0.3, 1.0, 0.1), dev, 7, scale=2.0)),
        Term.distance(17, weight=0.5, per_frame=HT._rows(B, (0.3, 1.0, 0.2), dev, 8, noise=0.1)),
        Term.distance(5, 5, hi=0.0), Term.distance(20, 16, lo=0.5, hi=0.75, weight=1.0),
        Term.align(13, (0, 0, 1), dir=(1, 0, 0), threshold=0.2, margin=0.0, weight=0.5, drop_up=True),
        Term.align(13, (0, 0, 1), dir=(1, 0, 0), threshold=0.1, margin=0.1, weight=1.2, drop_up=True, per_frame=HT._rows(B, (0.0, 0.0, 1.0), dev, 9)),
        Term.align(9, (1, 0, 0), 9, (0, 1, 0), margin=0.3, weight=2.0), Term.align(17, (1, 0, 0), 21, (0, 1, 0), margin=-0.2, weight=0.7),
        Term.align(12, (0, 1, 0), 0, (0, 1, 0), margin=0.0, weight=0.8), Term.plane(0, (0, 0, 1), (0, 0, 0.05), weight=0.0),
    ], up_axis=1)
    return c

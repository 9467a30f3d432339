"""ORACLE of dp_optimize_clip_lm (include/dragposer_clip_lm.h, "The step"): S sequences of T frames solved jointly, the latents of a sequence
tied frame to frame by c |z_t - z_(t-1)|^2 with c = lambda_smooth / 24, by Levenberg-Marquardt steps on the whole sequence.  In torch on the CPU
over tests/lm_oracle.py's normal_equations / forward, in the model's dtype (fp64 or fp32).  Frame t of sequence s is row t * S + s.

Per sequence and step:  H = blockdiag(A_t) + c Lap (x) I_24,  G_t = g_t + c (Lap Z)_t,  M = H + mu diag(H),  M Delta = -G by the block recursion
  S_0 = M_00;  S_t = M_tt - c^2 S_(t-1)^-1;  S_t = L_t L_t^T;  y_t = L_t^-1 (-G_t + c L_(t-1)^-T y_(t-1));  Delta_t = L_t^-T (y_t + c L_t^-1 Delta_(t+1))
(a pivot <= 0 or not finite in any block rejects), Z' = Z + Delta accepted iff L_s(Z') < L_s(Z); mu, one per sequence, moves as in lm_oracle.lm.
`dense=True` solves M Delta = -G by one Cholesky of the dense matrix instead: what the recursion is held against."""
import numpy as np
import torch

import lm_oracle as LO

DEFAULTS = LO.DEFAULTS


def clip_inputs(model, S, T, trackers=6, seed=11):
    """the warm recipe's S * T unrelated frames, read as S sequences of T frames"""
    return LO.warm_inputs(model, S * T, trackers=trackers, seed=seed)


def infill_inputs(model, S, T, keep, trackers=6, seed=11):
    """clip_inputs with every weight 0 except on the frames listed in `keep`: the other frames follow from their neighbours alone"""
    b = clip_inputs(model, S, T, trackers, seed)
    w = np.array(b["w"]).reshape(T, S, *b["w"].shape[1:])
    mask = np.zeros(T, bool)
    mask[list(keep)] = True
    w[~mask] = 0
    return dict(b, w=w.reshape(b["w"].shape))


def laplacian_rows(Z):
    """(Lap Z)_t of Z [T, S, 24] along t: the path graph's Laplacian, 0 for T = 1"""
    out = torch.zeros_like(Z)
    out[1:] += Z[1:] - Z[:-1]
    out[:-1] += Z[:-1] - Z[1:]
    return out


def degrees(T, dtype):
    d = torch.full((T,), 2.0, dtype=dtype)
    d[0] -= 1.0
    d[-1] -= 1.0
    return d if T > 1 else torch.zeros(1, dtype=dtype)


def coupling(Z, c):
    """c sum_t |z_t - z_(t-1)|^2 per sequence, of Z [T, S, 24], summed in double"""
    d = (Z[1:] - Z[:-1]).double()
    return float(c) * (d * d).sum(dim=(0, 2))


def totals(loss, Z, c):
    """-> (L_s [S], its coupling part [S]) in double: the frames' three numbers added frame by frame in index order, then the coupling"""
    T, S = Z.shape[0], Z.shape[1]
    per = ((loss[:, 0] + loss[:, 1]) + loss[:, 2]).double().reshape(T, S)
    tot = torch.zeros(S, dtype=torch.float64)
    for t in range(T):
        tot = tot + per[t]
    cp = coupling(Z, c)
    return tot + cp, cp


def solve_recursion(A, G, c, mu, deg):
    """A [T,24,24], G [T,24] of one sequence -> (Delta [T,24], ok)"""
    T, dt = A.shape[0], A.dtype
    eye = torch.eye(24, dtype=dt)
    Linv, ys = [], []
    ok = True
    for t in range(T):
        H = A[t] + (c * deg[t]) * eye
        M = H + mu * (H * eye)
        if t > 0:
            M = M - (c * c) * (Linv[-1].T @ Linv[-1])
        L, info = torch.linalg.cholesky_ex(M)
        if int(info) != 0 or not bool(torch.isfinite(L).all()):
            ok = False
            break
        Li = torch.linalg.solve_triangular(L, eye, upper=False)
        rhs = -G[t]
        if t > 0:
            rhs = rhs + c * (Linv[-1].T @ ys[-1])
        Linv.append(Li)
        ys.append(Li @ rhs)
    if not ok:
        return torch.zeros(T, 24, dtype=dt), False
    D = [None] * T
    for t in range(T - 1, -1, -1):
        w = ys[t]
        if t < T - 1:
            w = w + c * (Linv[t] @ D[t + 1])
        D[t] = Linv[t].T @ w
    return torch.stack(D), True


def dense_matrix(A, c, mu, deg):
    T, dt = A.shape[0], A.dtype
    eye = torch.eye(24, dtype=dt)
    M = torch.zeros(24 * T, 24 * T, dtype=dt)
    for t in range(T):
        H = A[t] + (c * deg[t]) * eye
        M[24 * t:24 * t + 24, 24 * t:24 * t + 24] = H + mu * (H * eye)
        if t > 0:
            M[24 * t:24 * t + 24, 24 * t - 24:24 * t] = -c * eye
            M[24 * t - 24:24 * t, 24 * t:24 * t + 24] = -c * eye
    return M


def solve_dense(A, G, c, mu, deg):
    T = A.shape[0]
    L, info = torch.linalg.cholesky_ex(dense_matrix(A, c, mu, deg))
    if int(info) != 0 or not bool(torch.isfinite(L).all()):
        return torch.zeros(T, 24, dtype=A.dtype), False
    return torch.cholesky_solve(-G.reshape(-1, 1), L).reshape(T, 24), True


def clip_lm(model, batch, S, n_steps, lam_smooth, lam_rot=1.0, lam_tmp=0.02, mu=None, dense=False, **kw):
    """n_steps joint LM steps on the S sequences of `batch` (B = S * T rows).  Returns numpy arrays: z [B,24], loss [B,3] (at z), n_accepted [S],
    mu [S] (after), accepted [S,n_steps], margin [S,n_steps] (|L' - L| / L), loss_hist [S,n_steps+1] (L_s of the kept latents), clip_loss [S,2]
    (L_s, its coupling part), delta [n_steps][B,24] (every step's Delta, zeros where the solve failed), solved [S,n_steps]."""
    p = dict(DEFAULTS, **kw)
    dt = model.dtype
    t = LO._conv(model, batch)
    B = t["z0"].shape[0]
    assert B % S == 0
    T = B // S
    c = torch.tensor(lam_smooth, dtype=dt) / 24.0
    deg = degrees(T, dt)
    z = t["z0"].clone()
    mu_t = torch.full((S,), p["mu0"], dtype=dt) if mu is None else torch.as_tensor(mu).to(dt).clone()
    loss, _ = LO.forward(model, z, t, lam_rot, lam_tmp)
    tot, cp = totals(loss, z.reshape(T, S, 24), c)
    n_acc = np.zeros(S, np.int32)
    accepted = np.zeros((S, n_steps), bool)
    solved = np.zeros((S, n_steps), bool)
    margin = np.full((S, n_steps), np.nan)
    hist = [tot.clone()]
    deltas = []
    for k in range(n_steps):
        A, g = LO.normal_equations(model, z, t, lam_rot, lam_tmp)
        Z = z.reshape(T, S, 24)
        G = g.reshape(T, S, 24) + c * laplacian_rows(Z)
        A = A.reshape(T, S, 24, 24)
        D = torch.zeros(T, S, 24, dtype=dt)
        for s in range(S):
            D[:, s], ok = (solve_dense if dense else solve_recursion)(A[:, s], G[:, s], c, mu_t[s], deg)
            solved[s, k] = ok
        deltas.append(D.reshape(B, 24).numpy().copy())
        zn = (Z + D).reshape(B, 24)
        ln, _ = LO.forward(model, zn, t, lam_rot, lam_tmp)
        totn, cpn = totals(ln, zn.reshape(T, S, 24), c)
        acc = torch.as_tensor(solved[:, k]) & (totn < tot)
        margin[:, k] = ((totn - tot).abs() / tot).numpy()
        margin[~solved[:, k], k] = np.inf  # (a refused solve is a certain rejection)
        accepted[:, k] = acc.numpy()
        rows = acc.repeat(T)  # row t * S + s
        z = torch.where(rows[:, None], zn, z)
        loss = torch.where(rows[:, None], ln, loss)
        tot, cp = torch.where(acc, totn, tot), torch.where(acc, cpn, cp)
        mu_t = torch.where(acc, torch.clamp(mu_t * p["mu_down"], min=p["mu_min"]), torch.clamp(mu_t * p["mu_up"], max=p["mu_max"]))
        n_acc += acc.numpy().astype(np.int32)
        hist.append(tot.clone())
    return dict(z=z.numpy(), loss=loss.numpy(), n_accepted=n_acc, mu=mu_t.numpy(), accepted=accepted, margin=margin, solved=solved,
                loss_hist=torch.stack(hist, dim=1).numpy(), clip_loss=torch.stack((tot, cp), dim=1).numpy(), delta=deltas)

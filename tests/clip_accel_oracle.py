"""ORACLE of dp_optimize_clip_lm_accel (include/dragposer_clip_accel.h, "The step"): tests/clip_lm_oracle.py's problem with
c2 |z_(t+1) - 2 z_t + z_(t-1)|^2, c2 = lambda_accel / 24, beside its first-difference term.  In torch on the CPU over tests/lm_oracle.py's
normal_equations / forward, in the model's dtype (fp64 or fp32).  Frame t of sequence s is row t * S + s.

K = c1 Lap + c2 D2^T D2 (scalar, T x T, bandwidth 2), built here from D2 itself, not from a table of its entries.  Per sequence and step:
H = blockdiag(A_t) + K (x) I_24,  G_t = g_t + (K Z)_t,  M = H + mu diag(H),  M Delta = -G by the block recursion with k1 = K[t,t-1], k2 = K[t,t-2]
  F_t = (k1 I - k2 L_(t-2)^-T F_(t-1)^T) L_(t-1)^-T;  S_t = M_tt - k2^2 L_(t-2)^-T L_(t-2)^-1 - F_t F_t^T = L_t L_t^T
  y_t = L_t^-1 (-G_t - k2 L_(t-2)^-T y_(t-2) - F_t y_(t-1));  Delta_t = L_t^-T (y_t - F_(t+1)^T Delta_(t+1) - K[t+2,t] L_t^-1 Delta_(t+2))
(a pivot <= 0 or not finite in any block rejects), Z' = Z + Delta accepted iff L_s(Z') < L_s(Z); mu, one per sequence, moves as in lm_oracle.lm.
`dense=True` solves M Delta = -G by one Cholesky of the dense matrix instead: what the recursion is held against."""
import numpy as np
import torch

import clip_lm_oracle as CO
import lm_oracle as LO

DEFAULTS = LO.DEFAULTS


def second_difference(T, dtype):
    """D2 [(T-2), T]: rows (1, -2, 1); no row for T <= 2"""
    D = torch.zeros(max(T - 2, 0), T, dtype=dtype)
    for j in range(T - 2):
        D[j, j], D[j, j + 1], D[j, j + 2] = 1.0, -2.0, 1.0
    return D


def band_matrix(T, c1, c2, dtype):
    """K = c1 Lap + c2 D2^T D2, [T, T]"""
    lap = torch.diag(CO.degrees(T, dtype))
    for t in range(1, T):
        lap[t, t - 1] = lap[t - 1, t] = -1.0
    D = second_difference(T, dtype)
    return c1 * lap + c2 * (D.T @ D)


def accel_rows(Z):
    """(D2^T D2 Z)_t of Z [T, S, 24] along t, formed from the second differences; 0 for T <= 2"""
    out = torch.zeros_like(Z)
    if Z.shape[0] > 2:
        a = Z[2:] - 2.0 * Z[1:-1] + Z[:-2]
        out[:-2] += a
        out[1:-1] -= 2.0 * a
        out[2:] += a
    return out


def accel_coupling(Z, c2):
    """c2 sum_t |z_(t+1) - 2 z_t + z_(t-1)|^2 per sequence, of Z [T, S, 24], summed in double"""
    Zd = Z.double()
    if Z.shape[0] <= 2:
        return torch.zeros(Z.shape[1], dtype=torch.float64)
    a = Zd[2:] - 2.0 * Zd[1:-1] + Zd[:-2]
    return float(c2) * (a * a).sum(dim=(0, 2))


def totals(loss, Z, c1, c2):
    """-> (L_s [S], its coupling part [S] (both sums), the second-difference part [S]) in double"""
    tot, cp = CO.totals(loss, Z, c1)
    ap = accel_coupling(Z, c2)
    return tot + ap, cp + ap, ap


def solve_recursion(A, G, Kb, mu):
    """A [T,24,24], G [T,24] of one sequence, Kb [T,T] -> (Delta [T,24], ok)"""
    T, dt = A.shape[0], A.dtype
    eye = torch.eye(24, dtype=dt)
    zero = torch.zeros(24, 24, dtype=dt)
    Linv, F, ys = [], [], []
    for t in range(T):
        k1 = Kb[t, t - 1] if t >= 1 else 0.0
        k2 = Kb[t, t - 2] if t >= 2 else 0.0
        H = A[t] + Kb[t, t] * eye
        M = H + mu * (H * eye)
        Ft = zero
        if t >= 1:
            W = k1 * eye
            if t >= 2:
                W = W - k2 * (Linv[t - 2].T @ F[t - 1].T)
                M = M - (k2 * k2) * (Linv[t - 2].T @ Linv[t - 2])
            Ft = W @ Linv[t - 1].T
            M = M - Ft @ Ft.T
        L, info = torch.linalg.cholesky_ex(M)
        if int(info) != 0 or not bool(torch.isfinite(L).all()):
            return torch.zeros(T, 24, dtype=dt), False
        Li = torch.linalg.solve_triangular(L, eye, upper=False)
        rhs = -G[t]
        if t >= 1:
            rhs = rhs - Ft @ ys[t - 1]
        if t >= 2:
            rhs = rhs - k2 * (Linv[t - 2].T @ ys[t - 2])
        Linv.append(Li)
        F.append(Ft)
        ys.append(Li @ rhs)
    D = [None] * T
    for t in range(T - 1, -1, -1):
        w = ys[t]
        if t + 1 < T:
            w = w - F[t + 1].T @ D[t + 1]
        if t + 2 < T:
            w = w - Kb[t + 2, t] * (Linv[t] @ D[t + 2])
        D[t] = Linv[t].T @ w
    return torch.stack(D), True


def dense_matrix(A, Kb, mu):
    T, dt = A.shape[0], A.dtype
    eye = torch.eye(24, dtype=dt)
    M = torch.kron(Kb, eye)
    for t in range(T):
        M[24 * t:24 * t + 24, 24 * t:24 * t + 24] += A[t]
    return M + mu * torch.diag(torch.diagonal(M))


def solve_dense(A, G, Kb, mu):
    T = A.shape[0]
    L, info = torch.linalg.cholesky_ex(dense_matrix(A, Kb, mu))
    if int(info) != 0 or not bool(torch.isfinite(L).all()):
        return torch.zeros(T, 24, dtype=A.dtype), False
    return torch.cholesky_solve(-G.reshape(-1, 1), L).reshape(T, 24), True


def coupling_gradient(Z, c1, c2):
    """(K Z)_t of Z [T, S, 24]: -> (both parts together, the second-difference part alone)"""
    ga = c2 * accel_rows(Z)
    return c1 * CO.laplacian_rows(Z) + ga, ga


def clip_lm(model, batch, S, n_steps, lam_smooth, lam_accel, lam_rot=1.0, lam_tmp=0.02, mu=None, dense=False, **kw):
    """n_steps joint LM steps on the S sequences of `batch` (B = S * T rows).  Returns what clip_lm_oracle.clip_lm returns (clip_loss[:, 1]: both
    coupling sums) plus accel_loss [S], the second-difference part of L_s at the returned latents."""
    p = dict(DEFAULTS, **kw)
    dt = model.dtype
    t = LO._conv(model, batch)
    B = t["z0"].shape[0]
    assert B % S == 0
    T = B // S
    c1, c2 = torch.tensor(lam_smooth, dtype=dt) / 24.0, torch.tensor(lam_accel, dtype=dt) / 24.0
    Kb = band_matrix(T, c1, c2, dt)
    z = t["z0"].clone()
    mu_t = torch.full((S,), p["mu0"], dtype=dt) if mu is None else torch.as_tensor(mu).to(dt).clone()
    loss, _ = LO.forward(model, z, t, lam_rot, lam_tmp)
    tot, cp, ap = totals(loss, z.reshape(T, S, 24), c1, c2)
    n_acc = np.zeros(S, np.int32)
    accepted = np.zeros((S, n_steps), bool)
    solved = np.zeros((S, n_steps), bool)
    margin = np.full((S, n_steps), np.nan)
    hist = [tot.clone()]
    deltas = []
    for k in range(n_steps):
        A, g = LO.normal_equations(model, z, t, lam_rot, lam_tmp)
        Z = z.reshape(T, S, 24)
        G = g.reshape(T, S, 24) + coupling_gradient(Z, c1, c2)[0]
        A = A.reshape(T, S, 24, 24)
        D = torch.zeros(T, S, 24, dtype=dt)
        for s in range(S):
            D[:, s], ok = solve_dense(A[:, s], G[:, s], Kb, mu_t[s]) if dense else solve_recursion(A[:, s], G[:, s], Kb, mu_t[s])
            solved[s, k] = ok
        deltas.append(D.reshape(B, 24).numpy().copy())
        zn = (Z + D).reshape(B, 24)
        ln, _ = LO.forward(model, zn, t, lam_rot, lam_tmp)
        totn, cpn, apn = totals(ln, zn.reshape(T, S, 24), c1, c2)
        acc = torch.as_tensor(solved[:, k]) & (totn < tot)
        margin[:, k] = ((totn - tot).abs() / tot).numpy()
        margin[~solved[:, k], k] = np.inf  # (a refused solve is a certain rejection)
        accepted[:, k] = acc.numpy()
        rows = acc.repeat(T)  # row t * S + s
        z = torch.where(rows[:, None], zn, z)
        loss = torch.where(rows[:, None], ln, loss)
        tot, cp, ap = torch.where(acc, totn, tot), torch.where(acc, cpn, cp), torch.where(acc, apn, ap)
        mu_t = torch.where(acc, torch.clamp(mu_t * p["mu_down"], min=p["mu_min"]), torch.clamp(mu_t * p["mu_up"], max=p["mu_max"]))
        n_acc += acc.numpy().astype(np.int32)
        hist.append(tot.clone())
    return dict(z=z.numpy(), loss=loss.numpy(), n_accepted=n_acc, mu=mu_t.numpy(), accepted=accepted, margin=margin, solved=solved,
                loss_hist=torch.stack(hist, dim=1).numpy(), clip_loss=torch.stack((tot, cp), dim=1).numpy(), accel_loss=ap.numpy(), delta=deltas)

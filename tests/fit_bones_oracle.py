"""ORACLE of dp_fit_bones (include/dragposer_calibration.h): per-group bone scales from tracker frames, in torch on the CPU over
oracle.ref_torch's decoder_forward / pose_fk, in the model's dtype (fp64 or fp32: the forward pass, the rows, the sums and the solve).

Per frame f with E tracked joints, rotations G = pose_fk's `rot` at (z, cur_rot), and bones base_b with group groups[b] (-1: not fitted):
    A[f,j,:,g] = sum over b on the path 0 -> j with groups[b] = g of G[f, parent(b)] base_b
    c[f,j]     = world_disp[f] + the same sum over groups[b] = -1
    rows of joint j: sqrt(w_pos / (3E)) [A[f,j] | tgt_pos - c[f,j]]
M = sum over the frames of [A b]^T [A b]; N = M[:K,:K], g = M[:K,K]; scales = solve(N + ridge I, g + ridge prior) by Cholesky, a pivot that
is <= 0 or not finite -> DP_FIT_SINGULAR and scales = prior.  A frame whose z, cur_rot, tracked tgt_pos or tracked weights are not finite
or beyond DP_INPUT_LIMIT is refused, and a frame without a tracked joint is not used."""
import numpy as np
import torch

from oracle import ref_torch as R

NO_FRAMES, SINGULAR = 1, 2
INPUT_LIMIT = 1.0e4
LIMBS = [-1] + [0] * 8 + [1] * 5 + [2] * 8  # legs (joints 1-8) / spine + neck (9-13) / arms (14-21) of the shipped tree
SYMMETRIC = [-1, 0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 9, 10, 11, 12]  # left = right: 4 leg, 5 spine, 4 arm groups
UNIFORM = [-1] + [0] * 21
PER_BONE = [-1] + list(range(21))


def paths(parents):
    """joint -> the bones (joint indices > 0) on its path to the root"""
    out = []
    for j in range(R.NJ):
        p, c = [], j
        while c != 0:
            p.append(c)
            c = parents[c]
        out.append(p)
    return out


def used_frames(z, cur_rot, tgt_pos, w, tracked):
    """(used [B] bool, status [B]) by the header's screening"""
    bad = lambda x: ~(np.abs(np.asarray(x, np.float64)) <= INPUT_LIMIT)
    trk = np.asarray(tracked).astype(bool)
    bs = bad(z).any(1) | bad(cur_rot).any(1)
    bt = ~bs & ((bad(tgt_pos).any(2) | bad(w).any(2)) & trk).any(1)
    status = np.where(bs, 2, np.where(bt, 4, 0)).astype(np.int32)
    return ~bs & ~bt & trk.any(1), status


def normal_matrix(model, z, cur_rot, tgt_pos, w, tracked, groups, K, base=None):
    """-> (M [K+1,K+1] in the model's dtype, frames used, status)"""
    dt = model.dtype
    used, status = used_frames(z, cur_rot, tgt_pos, w, tracked)
    M = torch.zeros(K + 1, K + 1, dtype=dt)
    if not used.any():
        return M, 0, status
    conv = lambda a: torch.as_tensor(np.asarray(a)[used]).to(dt)
    z, cur_rot, tgt_pos, w = map(conv, (z, cur_rot, tgt_pos, w))
    trk = torch.as_tensor(np.asarray(tracked)[used]).bool()
    base = model.offsets if base is None else torch.as_tensor(np.asarray(base)).to(dt)
    with torch.no_grad():
        motion, disp = R.decoder_forward(model, z)
        world_disp, _, _, rot, _ = R.pose_fk(model, motion, disp, cur_rot)
        B = z.shape[0]
        par = model.parents
        bone = torch.stack([torch.zeros(B, 3, dtype=dt)] + [(rot[:, par[b]] @ base[b].reshape(3, 1)).squeeze(-1) for b in range(1, R.NJ)], dim=1)
        D = torch.zeros(B, R.NJ, 3, K + 1, dtype=dt)  # [A | tgt - c]
        for j, path in enumerate(paths(par)):
            c = world_disp.clone()
            for b in path:
                if groups[b] >= 0:
                    D[:, j, :, groups[b]] += bone[:, b]
                else:
                    c = c + bone[:, b]
            D[:, j, :, K] = tgt_pos[:, j] - c
        E = trk.sum(1).to(dt)
        sw = torch.sqrt(w[..., 0] / (3.0 * E[:, None])) * trk.to(dt)
        D = (D * sw[:, :, None, None]).reshape(-1, K + 1)
        M = D.T @ D
    return M, int(used.sum()), status


def solve(M, K, frames, prior=None, ridge=1e-3):
    """-> dict(scales [K], flags, rms [2]) in M's dtype"""
    dt = M.dtype
    prior = torch.ones(K, dtype=dt) if prior is None else torch.as_tensor(np.asarray(prior, np.float32)).to(dt)
    q = lambda s: M[K, K] - 2.0 * (s @ M[:K, K]) + s @ M[:K, :K] @ s
    flags, s = 0, prior
    if frames == 0:
        flags = NO_FRAMES
    else:
        H = M[:K, :K] + ridge * torch.eye(K, dtype=dt)
        L, info = torch.linalg.cholesky_ex(H)
        if int(info) != 0 or not bool(torch.isfinite(L).all()):
            flags = SINGULAR
        else:
            s = torch.cholesky_solve((M[:K, K] + ridge * prior).reshape(K, 1), L).reshape(K)
    rms = [float(torch.sqrt(torch.clamp(q(x), min=0) / frames)) if frames else 0.0 for x in (prior, s)]
    return dict(scales=s.numpy().copy(), flags=flags, rms=np.array(rms))


def scaled_offsets(base, groups, scales):
    """base_j * s_g(j) (fp32 products), base_j for group -1, row 0 zero"""
    base = np.asarray(base, np.float32)
    out = base.copy()
    for j in range(1, R.NJ):
        if groups[j] >= 0:
            out[j] = base[j] * np.float32(scales[groups[j]])
    out[0] = 0
    return out


def fit(model, b, groups, K, base=None, prior=None, ridge=1e-3, z=None):
    """the whole call on a batch dict (z defaults to b["z0"]) -> dict(normal, scales, rms, flags, frames, status, offsets)"""
    z = b["z0"] if z is None else z
    M, frames, status = normal_matrix(model, z, b["cur_rot"], b["tgt_pos"], b["w"], b["tracked"], groups, K, base)
    out = solve(M, K, frames, prior, ridge)
    base_np = model.offsets.numpy() if base is None else base
    out.update(normal=M.numpy().copy(), frames=frames, status=status, offsets=scaled_offsets(base_np, groups, out["scales"]))
    return out


def scaled_model(model, groups, factors):
    """a copy of `model` whose bones are base * factors[group]"""
    import copy

    m = copy.copy(model)
    f = torch.tensor([1.0 if g < 0 else float(factors[g]) for g in groups], dtype=model.dtype)
    m.offsets = model.offsets * f[:, None]
    return m


def calibrate(model, b, groups, K, rounds=6, n_iter=50, ridge=1e-3, lam_tmp=0.0):
    """the alternation on the oracle: round r = ref_torch.optimize on the skeleton base * s_(r-1) from z_(r-1), then the fit at its z_final.
    -> (scales per round [rounds, K], rms per round [rounds, 2])"""
    z, s = np.asarray(b["z0"]), np.ones(K)
    trace, rms = [], []
    for _ in range(rounds):
        m = scaled_model(model, groups, s)
        o = R.optimize(m, z, b["z_tgt"], b["cur_rot"], b["tgt_pos"], b["tgt_rot"], b["w"], b["tracked"], n_iter, lam_tmp=lam_tmp)
        z = o["z_final"]
        f = fit(model, b, groups, K, ridge=ridge, z=z)
        s = f["scales"]
        trace.append(s.copy())
        rms.append(f["rms"])
    return np.array(trace), np.array(rms)

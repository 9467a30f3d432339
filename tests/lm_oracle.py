"""ORACLE of dp_optimize_lm (include/dragposer_lm.h, "The algorithm"): Levenberg-Marquardt on the 24-D latent, in torch on the CPU over
oracle.ref_torch's decoder_forward / pose_fk, in the model's dtype (fp64 or fp32).  J comes from torch.func.jacfwd.

Per frame, E tracked joints:  r_pos,t = sqrt(w_pos,t / (3E)) (P_t - tgt_pos_t);  r_rot,t = sqrt(lam_rot w_rot,t / (9E)) (G_t - tgt_rot_t);
r_tmp = sqrt(lam_tmp / 24) (z - z_tgt);  L = |r|^2 = the reference's total loss.  A = J^T J, g = J^T r, H = A + mu diag(A), H delta = -g by
Cholesky (a pivot <= 0 or not finite rejects), z' = z + delta accepted iff L(z') < L(z); mu <- max(mu mu_down, mu_min) on accept,
min(mu mu_up, mu_max) on reject.  A step is one trial.  With early_stop a frame ends before a step when loss_pos <= stop_eps_pos and
lam_rot loss_rot <= stop_eps_rot, or after a rejection at mu_max."""
import numpy as np
import torch

from oracle import ref_torch as R

DEFAULTS = dict(mu0=1e-2, mu_down=1.0 / 3.0, mu_up=4.0, mu_min=1e-6, mu_max=1e6)


def warm_inputs(model, B, trackers=6, mixed=False, seed=11):
    """the warm recipe: synth_inputs with z0 = z_src + 0.05 N(0,1) and z_tgt = z0"""
    b = R.synth_inputs(model, B, trackers=trackers, mixed=mixed, seed=seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    b["z0"] = (torch.from_numpy(b["z_src"]) + 0.05 * torch.randn(B, 24, generator=g)).numpy()
    b["z_tgt"] = b["z0"].copy()
    return b


EVERY_JOINT_COUNTS = (7, 9, 11, 15, 21)  # frames 23..27 of every_joint_inputs


def every_joint_inputs(model, warm, seed=11):
    """28 frames that between them form every joint's rows of J: frame f < 22 tracks joint f alone, frame 22 all 22 joints, frames 23..27
    the first 7, 9, 11, 15 and 21 joints of np.random.default_rng(3).permutation(22).  Weights of a tracked joint: uniform in [1, 10]
    (position) and [0.01, 10] (rotation), 0 elsewhere; targets = FK(decode(z_src), cur_rot) of `model` (any tree) on the tracked joints;
    z_src, z0, z_tgt and cur_rot are warm_inputs' (warm) or synth_inputs' (cold) draws."""
    B = R.NJ + 1 + len(EVERY_JOINT_COUNTS)
    b = warm_inputs(model, B, seed=seed) if warm else R.synth_inputs(model, B, seed=seed)
    tracked = np.zeros((B, R.NJ), np.uint8)
    tracked[np.arange(R.NJ), np.arange(R.NJ)] = 1
    tracked[R.NJ] = 1
    perm = np.random.default_rng(3).permutation(R.NJ)
    for i, n in enumerate(EVERY_JOINT_COUNTS):
        tracked[R.NJ + 1 + i, perm[:n]] = 1
    rng = np.random.default_rng(seed)
    w = np.stack((rng.uniform(1.0, 10.0, (B, R.NJ)), rng.uniform(0.01, 10.0, (B, R.NJ))), axis=-1) * tracked[..., None]
    return retarget(model, dict(b, tracked=tracked, w=w.astype(np.float32)))


def retarget(model, b):
    """`b` with tgt_pos / tgt_rot = FK(decode(z_src), cur_rot) of `model` on b's tracked joints (fp32, 0 elsewhere), as synth_inputs forms them"""
    dt = model.dtype
    with torch.no_grad():
        motion, disp = R.decoder_forward(model, torch.as_tensor(b["z_src"]).to(dt))
        _, _, pos, rot, _ = R.pose_fk(model, motion, disp, torch.as_tensor(b["cur_rot"]).to(dt))
    trk = torch.as_tensor(b["tracked"]).unsqueeze(-1).to(dt)
    return dict(b, tgt_pos=(pos * trk).float().numpy(), tgt_rot=(rot.reshape(-1, R.NJ, 9) * trk).float().numpy())


def tree_models(raw, path):
    """the model arrays `raw` (another tree: tests/test_hip_topology.py's _model_arrays) saved at `path` -> (fp64, fp32) OracleModel"""
    np.savez(path, **raw)
    return R.OracleModel(path, dtype=torch.float64), R.OracleModel(path, dtype=torch.float32)


def zero_problem(model, B, seed=11):
    """(batch, lambda_tmp) of a problem whose every trial is refused by the Cholesky, in any arithmetic: the 6-tracker warm recipe with every
    weight 0 and lambda_tmp = 0, so A = 0, g = 0 and every pivot is 0"""
    b = warm_inputs(model, B, trackers=6, seed=seed)
    return dict(b, w=np.zeros_like(b["w"])), 0.0


def at_target_problem(model, B, seed=11):
    """(batch, lambda_tmp) of a problem whose every trial is rejected by the strict `<`, in any arithmetic: zero_problem with lambda_tmp =
    0.02 and z_tgt = z0 (warm_inputs sets it), so A = (lambda_tmp / 24) I, g = 0, delta = 0 and L' == L == 0"""
    b, _ = zero_problem(model, B, seed)
    assert np.array_equal(b["z_tgt"], b["z0"])
    return b, 0.02


def _conv(model, b):
    dt = model.dtype
    t = {k: torch.as_tensor(b[k]).to(dt) for k in ("z0", "z_tgt", "cur_rot", "tgt_pos", "tgt_rot", "w")}
    t["tracked"] = torch.as_tensor(b["tracked"]).bool()
    return t


def forward(model, z, t, lam_rot, lam_tmp):
    """-> (loss [B,3], fk dict) at z: the reference's three loss numbers (the second and third already times their lambda)"""
    with torch.no_grad():
        motion, disp = R.decoder_forward(model, z)
        lp, lr, lt, fk = R.frame_losses(model, z, motion, disp, t["cur_rot"], t["z_tgt"], t["tgt_pos"], t["tgt_rot"], t["w"], t["tracked"],
                                        lam_rot, lam_tmp)
    fk = dict(fk, pose=motion)
    return torch.stack((lp, lr, lt), dim=1), fk


def residual_fn(model, lam_rot, lam_tmp):
    def f(z, cr, zt, tp, tr, w, trk):
        motion, disp = R.decoder_forward(model, z[None])
        _, _, pos, rot, _ = R.pose_fk(model, motion, disp, cr[None])
        E = trk.sum()
        sp = torch.sqrt(w[:, 0] / (3.0 * E)) * trk
        sr = torch.sqrt(lam_rot * w[:, 1] / (9.0 * E)) * trk
        rp = (pos[0] - tp) * sp[:, None]
        rr = (rot[0].reshape(R.NJ, 9) - tr) * sr[:, None]
        rt = (z - zt) * (lam_tmp / 24.0) ** 0.5
        return torch.cat((rp.reshape(-1), rr.reshape(-1), rt))

    return f


def normal_equations(model, z, t, lam_rot, lam_tmp, jac_hook=None):
    """-> A [B,24,24], g [B,24] at z.  `jac_hook(J) -> J` (J [B, 66 + 198 + 24, 24]: the position rows of joint j at 3j, its rotation rows at
    66 + 9j, then the latent pull's) lets a test plant an error in J to show that a comparison would notice it."""
    f = residual_fn(model, lam_rot, lam_tmp)
    trk = t["tracked"].to(model.dtype)
    args = (z, t["cur_rot"], t["z_tgt"], t["tgt_pos"], t["tgt_rot"], t["w"], trk)
    J = torch.func.vmap(torch.func.jacfwd(f))(*args)
    r = torch.func.vmap(f)(*args)
    if jac_hook is not None:
        J = jac_hook(J)
    return J.transpose(1, 2) @ J, (J.transpose(1, 2) @ r[..., None])[..., 0]


def lm(model, batch, n_steps, lam_rot=1.0, lam_tmp=0.02, mu=None, early_stop=False, stop_eps_pos=0.0, stop_eps_rot=0.0, jac_hook=None, **kw):
    """n_steps LM steps on every frame of `batch` (a synth_inputs dict).  Returns numpy arrays: z, loss [B,3], loss0 [B,3], n_accepted, iters,
    mu (after), accepted [B,n_steps] (bool), ran [B,n_steps] (bool: the step was executed), margin [B,n_steps] (|L'-L|/L; NaN where not run),
    loss_hist [B,n_steps+1] (total loss of the kept latent)."""
    p = dict(DEFAULTS, **kw)
    dt = model.dtype
    t = _conv(model, batch)
    B = t["z0"].shape[0]
    z = t["z0"].clone()
    mu_t = torch.full((B,), p["mu0"], dtype=dt) if mu is None else torch.as_tensor(mu).to(dt).clone()
    loss, _ = forward(model, z, t, lam_rot, lam_tmp)
    loss0 = loss.clone()
    active = torch.ones(B, dtype=torch.bool)
    hit_max = torch.zeros(B, dtype=torch.bool)
    n_acc = torch.zeros(B, dtype=torch.int32)
    iters = torch.zeros(B, dtype=torch.int32)
    accepted = torch.zeros(B, n_steps, dtype=torch.bool)
    ran = torch.zeros(B, n_steps, dtype=torch.bool)
    margin = torch.full((B, n_steps), float("nan"), dtype=dt)
    hist = [loss.sum(1).clone()]
    eye = torch.eye(24, dtype=dt)
    for s in range(n_steps):
        if early_stop:
            active = active & ~((loss[:, 0] <= stop_eps_pos) & (loss[:, 1] <= stop_eps_rot)) & ~hit_max
        if not bool(active.any()):
            hist.append(loss.sum(1).clone())
            continue
        A, g = normal_equations(model, z, t, lam_rot, lam_tmp, jac_hook)
        H = A + mu_t[:, None, None] * (A * eye)
        Lc, info = torch.linalg.cholesky_ex(H)
        ok = (info == 0) & torch.isfinite(Lc).all(dim=(1, 2))
        Lc = torch.where(ok[:, None, None], Lc, eye.expand(B, 24, 24))
        delta = torch.cholesky_solve(-g[..., None], Lc)[..., 0]
        zn = z + delta
        ln, _ = forward(model, zn, t, lam_rot, lam_tmp)
        tot, totn = loss.sum(1), ln.sum(1)
        acc = active & ok & (totn < tot)
        rej = active & ~acc
        margin[:, s] = torch.where(active, (totn - tot).abs() / tot, margin[:, s])
        ran[:, s], accepted[:, s] = active, acc
        z = torch.where(acc[:, None], zn, z)
        loss = torch.where(acc[:, None], ln, loss)
        hit_max = rej & (mu_t >= p["mu_max"])
        mu_t = torch.where(acc, torch.clamp(mu_t * p["mu_down"], min=p["mu_min"]), torch.where(rej, torch.clamp(mu_t * p["mu_up"], max=p["mu_max"]), mu_t))
        n_acc += acc.to(torch.int32)
        iters += active.to(torch.int32)
        hist.append(loss.sum(1).clone())
    return dict(z=z.numpy(), loss=loss.numpy(), loss0=loss0.numpy(), n_accepted=n_acc.numpy(), iters=iters.numpy(), mu=mu_t.numpy(),
                accepted=accepted.numpy(), ran=ran.numpy(), margin=margin.numpy(), loss_hist=torch.stack(hist, dim=1).numpy())


def forward_np(model, z, batch, lam_rot=1.0, lam_tmp=0.02):
    """the oracle's forward pass at a given latent: dict(loss [B,3], pos, rot [B,22,9], pose, disp, world_disp, world_rot) as numpy"""
    t = _conv(model, batch)
    loss, fk = forward(model, torch.as_tensor(z).to(model.dtype), t, lam_rot, lam_tmp)
    out = {k: v.numpy() for k, v in fk.items()}
    out["rot"] = out["rot"].reshape(len(z), R.NJ, 9)
    out["loss"] = loss.numpy()
    return out

"""Test helper: Adam on a loss that has no kink -- the reference of tests/test_hip_adam.py (GPU), itself tested by tests/test_adam_reference.py (CPU).

A frame whose tracker term is exactly zero (it tracks nothing, or every tracker weight is 0) has the loss lam * mean((z - z_tgt)^2): no decoder, no
LeakyReLU, and its latent after N steps of torch.optim.Adam is a scalar recursion per component.  `recursion` is that recursion in fp64;
`recursion_f32` is its fp32 twin, rounding where the kernels round (dp_host.cpp: fill_loop, fill_adam; dp_w4_iter.h: "bL0 + Adam"): the knobs
arrive as floats, the two bias corrections are formed in double from them and rounded once, and every step is the kernels' sequence of fp32
operations with the products the compiler contracts (-ffp-contract=on) fused.  The twin's own distance from the fp64 recursion measures what fp32
costs on a case; the bar a kernel must meet is 4 x that (the kernels take sqrt and the reciprocal from the 1-ulp hardware instructions, the twin
takes them correctly rounded) and never below 2e-6.

The recursion is smooth only while no component reaches its target (at the target the gradient changes sign and Adam's normalised step turns a
rounding difference into a step of size lr): `smooth_targets` draws z_tgt = z0 +- d with d at least 1.5 N lr / (1 - beta1) per component, further
than N steps of about lr each can travel."""
import functools

import numpy as np

DEFAULT = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8)
KNOBS = ("lr", "b1", "b2", "eps")
SETS = {
    "default": dict(DEFAULT),
    "slow_corrections": dict(lr=3e-3, b1=0.995, b2=0.9995, eps=1e-8),  # both bias corrections still far from 1 beyond the argument table
    "fast": dict(lr=3e-2, b1=0.8, b2=0.95, eps=1e-6),                  # the host table, its continuation and the loop's scalars at once
    "eps": dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-3),                  # an eps that matters: is it forwarded at all
    "beta1_0": dict(lr=1e-2, b1=0.0, b2=0.999, eps=1e-8),              # the edges check_adam accepts
    "beta2_0": dict(lr=1e-2, b1=0.9, b2=0.0, eps=1e-8),
    # three sets of this file's own, in place of the cases the condition below takes out of the six above
    "slow_beta1": dict(lr=3e-3, b1=0.995, b2=0.999, eps=1e-8),         # beta1^256 = 0.28, beta2^256 = 0.77: both corrections far from 1 past the table
    "fast_eps_default": dict(lr=3e-2, b1=0.8, b2=0.95, eps=1e-8),      # "fast" without its eps
    "lr_only": dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8),
}
LAMS = (0.02, 0.15)
STEPS = (1, 8, 256, 257, 300)
N_FRAMES = 8
INPUT_LIMIT = 1.0e4  # include/dragposer.h: DP_INPUT_LIMIT
BAR_FLOOR, BAR_FACTOR, MARGIN = 2e-6, 4.0, 100.0
# The condition: a case is kept only if the fp64 result with ANY ONE knob put back to its default lies at least MARGIN bars from the expected result,
# at both values of lam -- otherwise it cannot tell that knob from its default.  The step counts each set keeps (tests/test_adam_reference.py asserts
# the condition for every kept case, and for every case left out that it does fail):
#   * after ONE step Adam's update is lr g / (|g| + eps) whatever the betas: N = 1 is left to the sets that leave the betas alone;
#   * with targets out of reach the gradient changes by at most (1 - beta1) / 1.5 of itself over a run, and Adam's normalised step depends on the
#     betas only through that change.  "slow_corrections" (beta1 0.995) sees its beta2 (0.9995 against 0.999) at 3 bars at most, at every N;
#     larger N does not help (the targets move out with N, and the twin's distance grows faster than the margin: 8 bars at 1000, 4 at 2000);
#   * "fast" sees its eps (1e-6 against 1e-8) at eps (1 - beta1) / (1.5 ctmp) = 8e-5 = 40 bars of the floor at most, whatever N (the targets move out
#     with N lr, and the gradient with them).
# What the two sets were for is kept by "slow_beta1" (both bias corrections far from 1 beyond the table, beta1 told at > 100 bars) and by
# "fast_eps_default" (the three families at once); eps is told by the "eps" set at every N.
KEPT_STEPS = {
    "default": (1, 8, 256, 257, 300),
    "slow_corrections": (),
    "fast": (),
    "eps": (1, 8, 256, 257, 300),
    "beta1_0": (8, 256, 257, 300),
    "beta2_0": (8, 256, 257, 300),
    "slow_beta1": (256, 257, 300),
    "fast_eps_default": (8, 256, 257, 300),
    "lr_only": (1, 8, 256, 257, 300),
}
# whole-sequence launches: T steps of n_iter iterations each, Adam re-created per step; n_iter 257 is the LONG kernel.  (Three times the way to
# go: the targets are three times as far, the twin's distance grows with them, and fewer cases meet the condition.)
SEQUENCE_STEPS, SEQUENCE_LAM = 3, 0.02
SEQUENCE_CASES = (("default", 8), ("default", 257), ("eps", 8), ("eps", 257), ("beta1_0", 8), ("beta1_0", 257), ("beta2_0", 8), ("lr_only", 8),
                  ("lr_only", 257))

f32 = np.float32


def recursion(z0, z_tgt, n_iter, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, lam=0.02):
    """the latent after n_iter steps of Adam (torch's single-tensor form; m, v start at 0) on lam * mean((z - z_tgt)^2), in fp64; any shape [..., 24]"""
    z, zt = np.asarray(z0, np.float64).copy(), np.asarray(z_tgt, np.float64)
    m, v = np.zeros_like(z), np.zeros_like(z)
    for t in range(1, n_iter + 1):
        g = 2.0 * lam / 24.0 * (z - zt)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        z = z - lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    return z


def temporal_only(b, f, n_iter, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, lam=0.02):
    """the latent of frame f of batch b when it tracks nothing: only the pull towards z_tgt moves it (fp64)"""
    return recursion(b["z0"][f], b["z_tgt"][f], n_iter, lr, b1, b2, eps, lam)


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two floats is exact in double; the sum is rounded to double and then to float (a double rounding
    that differs from the fused result once in ~2^29 operations, by one ulp)"""
    return (a.astype(np.float64) * np.float64(b) + np.asarray(c, np.float64)).astype(f32)


def recursion_f32(z0, z_tgt, n_iter, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, lam=0.02):
    """`recursion` as the kernels compute it: see the module's docstring.  Returns float32."""
    lr_, b1_, b2_, eps_, lam_ = (f32(x) for x in (lr, b1, b2, eps, lam))  # dp_params' fields are floats
    ctmp = f32(f32(2.0) * lam_) / f32(24.0)
    one_m_b1, one_m_b2 = f32(1.0 - np.float64(b1_)), f32(1.0 - np.float64(b2_))
    z, zt = np.asarray(z0, f32).copy(), np.asarray(z_tgt, f32)
    m, v = np.zeros_like(z), np.zeros_like(z)
    b1t = b2t = 1.0
    for _ in range(n_iter):
        b1t *= float(b1_)
        b2t *= float(b2_)
        step, rbc2s = f32(float(lr_) / (1.0 - b1t)), f32(1.0 / np.sqrt(1.0 - b2t))
        g = ctmp * (z - zt)                       # (+ a tracker gradient of exactly 0)
        m = _fma(g - m, one_m_b1, m)              # m + (1 - b1) (g - m)
        v = _fma(v, b2_, one_m_b2 * (g * g))      # v b2 + (1 - b2) (g g)
        den = _fma(np.sqrt(v), rbc2s, eps_)       # sqrt(v) / sqrt(1 - b2^t) + eps
        z = _fma(m * (f32(1.0) / den), -step, z)  # z - step (m / den)
    return z


def smooth_targets(z0, n_total, lr, b1, seed):
    """z_tgt = z0 +- d, d drawn per component in [1, 2] x 1.5 n_total lr / (1 - b1): no component reaches its target within n_total steps"""
    rs = np.random.RandomState(seed)
    dmin = 1.5 * n_total * lr / (1.0 - b1)
    d = dmin * rs.uniform(1.0, 2.0, z0.shape) * rs.choice([-1.0, 1.0], z0.shape)
    zt = (z0.astype(np.float64) + d).astype(f32)
    assert np.abs(zt).max() < INPUT_LIMIT and np.abs(zt.astype(np.float64) - z0).min() >= dmin * (1 - 1e-6)
    return zt


def start_latents(seed=2024):
    """the eight frames' z0 (recipe S's scale)"""
    return (np.random.RandomState(seed).standard_normal((N_FRAMES, 24)) * 0.3).astype(f32)


@functools.lru_cache(maxsize=None)
def case(name, lam, n_iter, restarts=1):
    """One smooth case, computed once and left unchanged: z0, z_tgt, the expected latent (fp64), the twin's, the bar, and per knob that differs from
    its default the distance (in bars) of the fp64 result with that one knob put back.  `restarts` > 1: a whole-sequence launch of that many steps,
    Adam re-created per step -- the recursion restarted from the previous step's latent (expected / twin: [restarts, 8, 24])."""
    k = SETS[name]
    z0 = start_latents()
    zt = smooth_targets(z0, n_iter * restarts, k["lr"], k["b1"], seed=n_iter + 1000 * restarts)

    def run(fn, knobs):
        z, out = z0, []
        for _ in range(restarts):
            z = fn(z, zt, n_iter, lam=lam, **knobs)
            out.append(z)
        return np.stack(out) if restarts > 1 else out[0]

    want, twin = run(recursion, k), run(recursion_f32, k)
    bar = max(BAR_FACTOR * float(np.abs(twin - want).max()), BAR_FLOOR)
    margins = {}
    for knob in KNOBS:
        if k[knob] != DEFAULT[knob]:
            other = run(recursion, {**k, knob: DEFAULT[knob]})
            margins[knob] = float(np.abs(other - want).max(axis=-1).min() / bar)  # on the frame that tells them apart least
    out = dict(z0=z0, z_tgt=zt, want=want, twin=twin, bar=bar, margins=margins)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out

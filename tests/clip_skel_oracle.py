"""ORACLE of dp_optimize_clip_lm_skeleton and dp_optimize_lm_skeleton (include/dragposer_clip_skeleton.h): the clip solve and the per-frame LM
solver with one skeleton per sequence / per frame.  Nothing couples two sequences of a clip launch (two frames of an LM launch), so the oracle of
a mixed launch is, per sequence, the plain oracle -- tests/clip_lm_oracle.py or tests/clip_accel_oracle.py -- on an OracleModel copy whose
`offsets` rows 1..21 are that sequence's.  The plain oracle is run on the WHOLE launch once per distinct skeleton and the rows and
per-sequence results of that skeleton's sequences are taken from it (frame t of sequence s is row t * S + s): the same numbers as a run of
the sequence alone up to torch's batch-shape-dependent last bits, and exactly the plain oracle's when every sequence has the model's own
bones (clip_lm below says why).  The cases of tests/test_hip_clip_skeleton.py are listed here, so that tests/test_clip_skel_oracle.py pins their margins on the CPU."""
import copy
import functools

import numpy as np
import torch

import clip_accel_oracle as AO
import clip_lm_oracle as CO
import lm_oracle as LO
from oracle import ref_torch as R

LAM_TMP = 0.02
MARGIN = 1e-3  # tests/test_hip_lm.py's
LEGS, ARMS = tuple(range(1, 9)), tuple(range(14, 22))  # bones of the shipped tree: hips to toes, shoulders to hands

SHAPES = [(1, 1), (1, 3), (5, 7), (3, 33), (2, 65)]
SETTINGS = [(0.5, None), (0.0, 5.0), (0.5, 5.0)]  # (lambda_smooth, lambda_accel; None: the call without dp_clip_accel_params)
# three steps from mu0: (S, T, trackers, lambda_smooth, lambda_accel, seed).  Every seed is the first from 11 on at which no step of any
# sequence has an oracle margin below MARGIN and every sequence with a foreign skeleton moves (a sequence whose every trial is rejected
# returns its z0 on any bones): tests/test_clip_skel_oracle.py holds them to both.  Seed 11 leaves sequence 0 of (5, 7) at its z0 at
# lambda_smooth 0.5 without the acceleration term, so those two cases take 12.
SEVERAL = [(5, 7, 3, 0.5, None, 12), (5, 7, 3, 0.5, 5.0, 11), (3, 33, 3, 0.5, None, 11), (3, 33, 3, 0.5, 5.0, 11),
           (5, 7, 6, 0.5, None, 11), (5, 7, 6, 0.5, 5.0, 11), (3, 33, 6, 0.5, None, 11), (3, 33, 6, 0.5, 5.0, 11)]
ONE_STEP_SEED = {(5, 7): 12}  # one step at mu 1e-2, 3 trackers: the seed of a shape (11 where not listed)
T1 = (9, 3, 0.7, 11)          # T = 1: S, trackers, lambda_smooth, seed
BF16 = (3, 33, 3, 0.5, 5.0, 11)
E2E = (2, 9, 6, 0.5, 11)      # end to end: S, T, trackers, lambda_smooth, seed


def skeletons(base):
    """the context's own bones, 0.85 x, 1.12 x, and one non-uniform performer (legs x 1.1, arms x 0.9); [22,3] float32 each"""
    base = np.asarray(base, np.float32)
    mixed = base.copy()
    mixed[list(LEGS)] *= np.float32(1.1)
    mixed[list(ARMS)] *= np.float32(0.9)
    return [np.ascontiguousarray(o, dtype=np.float32) for o in (base, base * np.float32(0.85), base * np.float32(1.12), mixed)]


def k_of(S):
    """the skeleton of sequence s in the mixed cases: 1, 2, 3, 0, 1, ... -- a foreign one first, so that a single sequence has one"""
    return [(s + 1) % 4 for s in range(S)]


def with_offsets(model, off):
    """a copy of `model` with rows 1..21 of its offsets replaced by `off`'s (row 0 is never read and stays)"""
    m = copy.copy(model)
    m.offsets = model.offsets.clone()
    m.offsets[1:] = torch.as_tensor(np.asarray(off)[1:]).to(model.dtype)
    return m


@functools.lru_cache(maxsize=None)
def models(rounding="none"):
    return R.OracleModel(dtype=torch.float64, weight_rounding=rounding), R.OracleModel(dtype=torch.float32, weight_rounding=rounding)


def base_offsets():
    return np.asarray(np.load(R.DEFAULT_MODEL)["offsets"], np.float32)


def _take(b, rows):
    return {k: np.asarray(v)[rows] for k, v in b.items()}


def mixed_inputs(S, T, trackers, seed, ks=None, skels=None, model=None):
    """clip_lm_oracle.clip_inputs with every sequence's targets formed by ITS OWN model (lm_oracle.retarget): each problem is consistent, its
    z_src reproduces its targets exactly on its own bones"""
    m64 = model if model is not None else models()[0]
    skels = skels if skels is not None else skeletons(base_offsets())
    ks = ks if ks is not None else k_of(S)
    b = {k: np.array(v) for k, v in CO.clip_inputs(m64, S, T, trackers=trackers, seed=seed).items()}
    for s in range(S):
        if np.array_equal(skels[ks[s]][1:], base_offsets()[1:]):
            continue  # (the context's own bones: clip_inputs' targets are this model's already)
        rows = np.arange(s, S * T, S)
        sub = LO.retarget(with_offsets(m64, skels[ks[s]]), _take(b, rows))
        for k in ("tgt_pos", "tgt_rot"):
            b[k][rows] = sub[k]
    return b


def _by_skeleton(skels):
    """-> [(offsets, the indices that use them)], one entry per distinct skeleton"""
    groups = {}
    for i, s in enumerate(skels):
        groups.setdefault(np.asarray(s, np.float32).tobytes(), (s, []))[1].append(i)
    return list(groups.values())


def every_joint_mixed():
    """lm_oracle.every_joint_inputs' 28 warm frames -- between them every joint's rows of J -- with frame f on skeleton (f + 1) % 4 and its
    targets formed by its own model; -> (batch, the skeleton index of every frame)"""
    m64 = models()[0]
    skels = skeletons(base_offsets())
    b = {k: np.array(v) for k, v in LO.every_joint_inputs(m64, warm=True).items()}
    ks = [(f + 1) % 4 for f in range(len(b["z0"]))]
    for k in range(1, 4):
        rows = np.nonzero(np.asarray(ks) == k)[0]
        sub = LO.retarget(with_offsets(m64, skels[k]), _take(b, rows))
        for key in ("tgt_pos", "tgt_rot"):
            b[key][rows] = sub[key]
    return b, ks


def clip_lm(model, batch, S, skels_of_seq, n_steps, lam_smooth, lam_accel=None, lam_tmp=LAM_TMP, mu=None, **kw):
    """the launch's oracle: sequence s solved by clip_lm_oracle.clip_lm (lam_accel None) or clip_accel_oracle.clip_lm on with_offsets(model,
    skels_of_seq[s]); -> the plain oracle's dict with the launch's rows and sequences.  The plain oracle treats every sequence on its own, so
    sequence s's part of a run of the WHOLE launch on s's model is s solved alone; it is taken from such a run, one per distinct skeleton,
    rather than from a run of s's rows only, because torch's sums and products depend on the shape of the batch in their last bits -- this
    way a launch whose sequences all have the model's own bones gives the plain oracle's bits, which tests/test_clip_skel_oracle.py pins."""
    B = np.asarray(batch["z0"]).shape[0]
    T = B // S
    res = None
    for off, seqs in _by_skeleton(skels_of_seq):
        m = with_offsets(model, off)
        k = dict(kw, lam_tmp=lam_tmp, mu=mu)
        o = CO.clip_lm(m, batch, S, n_steps, lam_smooth, **k) if lam_accel is None else AO.clip_lm(m, batch, S, n_steps, lam_smooth, lam_accel, **k)
        if res is None:
            res = {key: ([np.array(d) for d in v] if key == "delta" else np.array(v)) for key, v in o.items()}
            continue
        rows = np.isin(np.arange(B) % S, seqs)
        for key, v in o.items():
            if key in ("z", "loss"):  # per frame
                res[key][rows] = v[rows]
            elif key == "delta":
                for i in range(n_steps):
                    res[key][i][rows] = v[i][rows]
            else:                     # per sequence
                res[key][seqs] = v[seqs]
    assert res["z"].shape == (T * S, 24)
    return res


def lm(model, batch, skels_of_frame, n_steps, lam_tmp=LAM_TMP, **kw):
    """dp_optimize_lm_skeleton's oracle: frame f solved by lm_oracle.lm on with_offsets(model, skels_of_frame[f]), taken from a run of the whole
    batch per distinct skeleton as in clip_lm; -> lm_oracle.lm's dict"""
    res = None
    for off, frames in _by_skeleton(skels_of_frame):
        o = LO.lm(with_offsets(model, off), batch, n_steps, lam_tmp=lam_tmp, **kw)
        if res is None:
            res = {key: np.array(v) for key, v in o.items()}
        else:
            for key, v in o.items():
                res[key][frames] = v[frames]
    return res


@functools.lru_cache(maxsize=None)
def case(S, T, trackers, steps, ls, la, mu, seed, rounding="none", foreign=True):
    """-> (batch, the skeletons of the sequences, fp64 oracle, fp32 oracle) of one mixed case, computed once and shared.  foreign=False: the
    same inputs solved on the context's own bones, what a kernel that ignored `skel` would compute."""
    m64, m32 = models(rounding)
    skels = skeletons(base_offsets())
    ks = k_of(S)
    b = mixed_inputs(S, T, trackers, seed, ks, skels, models()[0])
    of_seq = [skels[k if foreign else 0] for k in ks]
    kw = {} if mu is None else dict(mu=np.full(S, mu))
    return (b, [skels[k] for k in ks]) + tuple(clip_lm(m, b, S, of_seq, steps, ls, la, **kw) for m in (m64, m32))


def bar_of(ref, r32):
    """include/dragposer_clip_lm.h's comparison: max(4 x the fp32 oracle's deviation from the fp64 one, 1e-6 of the largest latent)"""
    return max(4.0 * np.abs(r32["z"] - ref["z"]).max(), 1e-6 * np.abs(ref["z"]).max())


def e2e_inputs():
    """the end-to-end case: (2, 9), every target formed by the 1.12 x performer; -> (batch, that performer's offsets)"""
    S, T, trackers, _, seed = E2E
    skels = skeletons(base_offsets())
    return mixed_inputs(S, T, trackers, seed, [2] * S, skels), skels[2]

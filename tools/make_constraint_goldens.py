#!/usr/bin/env python3
"""Goldens of the constrained optimise loop (include/dragposer_constraints.h) from the REAL reference.

Runs only in the build container (needs the reference checkout, like tools/make_goldens.py, whose harness it builds on).  The
reference's drag_pose.py is read, its `# Additional Losses` block (DragPose.loss, drag_pose.py:129-183) is un-commented IN MEMORY and
the module is executed from that text; nothing of it is written anywhere.  The block is checked first: it must be exactly the text
this tool was written against (SHA-256) and assign the four terms the C ABI implements -- anything else fails loudly.  Then, for every
frame, the real DragPose.run() runs: real Decoder, real loss() with the block active, real autograd and torch.optim.Adam.

Harness-side only, as in make_goldens.py: the temporal stub returns the stored z_tgt; set_initial_pose is bypassed (z0, cur_rot and
the random current_global_pos are stored inputs).  The block calls pymotion's quat.from_matrix, which the stand-in package does not
restate; it is supplied here (the standard trace-based conversion, w-first; q and -q rotate alike), and mul_vec takes the block's
integer forward axis in the quaternion's dtype.

  tests/golden/cons_s1.npz   256 frames, 6 trackers, 50 iterations at a fixed count
  tests/golden/cons_es.npz   128 frames, 6 trackers, the reference's early stop (eval_drag.py:210-214), at most 100 iterations
  tests/golden/cons_skel.npz     cons_s1's recipe and draws; frame b on make_goldens.skeleton_set(offsets, B)[b] (stored as `offsets`)
  tests/golden/cons_skel_es.npz  cons_es's recipe and draws, likewise

Names on the command line choose which files are written; none writes all four.
"""
import hashlib
import json
import os
import re
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as MG  # noqa: E402  (puts the reference and the pymotion stand-in on sys.path)

SRC = os.path.join(MG.REF, "src", "drag_pose.py")
HEAD = "        # Additional Losses ----------------------------------------------\n"
TAIL = "        additional_losses = 0\n"
BLOCK_SHA256 = "b7df2981f7e6fa7cc918875ad1793be68ec94f734fd1d80047dbb5a923254f8a"
TERMS = ("loss_feet_floor", "loss_head_hips_forward", "loss_head_hips_colinear", "loss_hips_feet_colinear")


def constrained_module():
    text = open(SRC).read()
    i = text.index(HEAD) + len(HEAD)
    k = text.index(TAIL, i)
    block = text[i:k]
    sha = hashlib.sha256(block.encode()).hexdigest()
    if sha != BLOCK_SHA256:
        raise RuntimeError(f"{SRC}: the # Additional Losses block is not the text this tool was written against (sha256 {sha})")
    lines = []
    for ln in block.split("\n"):
        if ln.strip():
            if not ln.startswith("        # "):
                raise RuntimeError(f"{SRC}: an active line inside the commented block: {ln!r}")
            ln = "        " + ln[len("        # "):]
        lines.append(ln)
    code = "\n".join(lines)
    assigned = set(re.findall(r"^\s+(loss_\w+)\s*=", code, flags=re.M))
    if assigned != set(TERMS):
        raise RuntimeError(f"the block assigns {sorted(assigned)}, expected the four terms {TERMS}")
    total = re.search(r"additional_losses = \((.*?)\)", code, flags=re.S).group(1).split("+")
    if [t.strip() for t in total] != ["loss_head_hips_forward", "loss_head_hips_colinear", "loss_feet_floor", "loss_hips_feet_colinear"]:
        raise RuntimeError(f"the block sums {total}")
    for needle in ("pos_qs[:, :, [4, 8], y_axis]", "rotmats_qs[0, 0, 13, :, :]", "rotmats_qs[0, 0, 0, :, :]", "torch.tensor([0, 0, 1]",
                   "fwd_head_norm > 0.5", "+ 0.2,", "pos_qs[0, 0, 13]", "pos_qs[0, 0, 0]", "pos_qs[0, 0, 3]", "pos_qs[0, 0, 7]",
                   "- 0.2 * 0.2", "floor_level = 0.0", "y_axis = 1"):
        if needle not in code:
            raise RuntimeError(f"the block lacks {needle!r}")
    mod = types.ModuleType("drag_pose_constrained")
    mod.__file__ = SRC
    exec(compile(text[:i] + code + "\n" + text[k + len(TAIL):], SRC + " (Additional Losses on)", "exec"), mod.__dict__)
    q = mod.quat
    mod.quat = types.SimpleNamespace(mul=q.mul, inverse=q.inverse, normalize=q.normalize, from_matrix=from_matrix,
                                     mul_vec=lambda a, v: q.mul_vec(a, v.to(a.dtype)))
    mod.fk_rotmat = MG._recording_fk
    return mod


def from_matrix(m):
    """rotation matrix [..., 3, 3] -> unit quaternion (w, x, y, z), Shepperd's branch on the largest of 1 + trace and the diagonal"""
    m = m.reshape(-1, 3, 3)
    out = []
    for r in m:
        t = r[0, 0] + r[1, 1] + r[2, 2]
        if t > max(r[0, 0], r[1, 1], r[2, 2]):
            s = torch.sqrt(1.0 + t) * 2.0
            q = torch.stack(((0.25 * s), (r[2, 1] - r[1, 2]) / s, (r[0, 2] - r[2, 0]) / s, (r[1, 0] - r[0, 1]) / s))
        elif r[0, 0] >= r[1, 1] and r[0, 0] >= r[2, 2]:
            s = torch.sqrt(1.0 + r[0, 0] - r[1, 1] - r[2, 2]) * 2.0
            q = torch.stack(((r[2, 1] - r[1, 2]) / s, 0.25 * s, (r[0, 1] + r[1, 0]) / s, (r[0, 2] + r[2, 0]) / s))
        elif r[1, 1] >= r[2, 2]:
            s = torch.sqrt(1.0 + r[1, 1] - r[0, 0] - r[2, 2]) * 2.0
            q = torch.stack(((r[0, 2] - r[2, 0]) / s, (r[0, 1] + r[1, 0]) / s, 0.25 * s, (r[1, 2] + r[2, 1]) / s))
        else:
            s = torch.sqrt(1.0 + r[2, 2] - r[0, 0] - r[1, 1]) * 2.0
            q = torch.stack(((r[1, 0] - r[0, 1]) / s, (r[0, 2] + r[2, 0]) / s, (r[1, 2] + r[2, 1]) / s, 0.25 * s))
        out.append(q)
    return torch.stack(out).reshape(4) if len(out) == 1 else torch.stack(out)


def build(mod, parents):
    gm, td, _, stub = MG.build_reference(parents)

    class Rec(mod.DragPose):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.rec = []

        def loss(self, *a, **k):
            out = super().loss(*a, **k)
            self.rec.append(dict(losses=[float(out[0]), float(out[1]), float(out[2])], extra=float(torch.as_tensor(out[3]).detach()),
                                 pos=out[7].detach().clone().reshape(MG.NJ, 3), rot=MG._FK_STASH["rot"].detach().clone().reshape(MG.NJ, 3, 3)))
            return out

    return td, Rec(gm, stub, torch.zeros(24), torch.ones(24), "cpu", "cpu"), stub


def run(name, B, n_iter, early_stop, mod, parents, offsets_t, offsets_frames=None):
    """offsets_frames [B,22,3]: frame b's skeleton -- its targets are the FK of that skeleton and DragPose.run gets it as `offsets`"""
    td, drag, stub = build(mod, parents)
    Zs, Z0, ZT, CR, _ = MG.draw_recipe(B, False)
    g = torch.Generator().manual_seed(4321)
    GP = torch.randn(B, 3, generator=g) * 0.1
    GP[:, 1] += 0.9  # (the recipe's feet sit about 0.9 m below the root: the floor term pulls both ways)
    track = MG.TRACK6
    wtab = torch.tensor([[10.0, 10.0], [5.0, 0.01], [5.0, 0.01], [5.0, 0.01], [5.0, 0.01], [5.0, 0.01]])
    idx = torch.tensor(track)
    out = dict(z0=Z0.numpy(), z_tgt=ZT.numpy(), cur_rot=CR.numpy(), global_pos=GP.numpy(), w=np.zeros((B, MG.NJ, 2), np.float32),
               tracked=np.zeros((B, MG.NJ), np.uint8), tgt_pos=np.zeros((B, MG.NJ, 3), np.float32), tgt_rot=np.zeros((B, MG.NJ, 9), np.float32),
               pos=np.zeros((B, MG.NJ, 3), np.float32), rot=np.zeros((B, MG.NJ, 9), np.float32), z_final=np.zeros((B, 24), np.float32),
               z_pre=np.zeros((B, 24), np.float32), iters=np.zeros(B, np.int32), loss_hist=np.full((B, n_iter, 3), np.nan, np.float32),
               extra_hist=np.full((B, n_iter), np.nan, np.float32))
    if offsets_frames is not None:
        out["offsets"] = offsets_frames.numpy()
    for b in range(B):
        off_b = offsets_t if offsets_frames is None else offsets_frames[b]
        pos_t, rot_t, _, _ = MG.forward_fk(drag, td, Zs[b], CR[b], off_b)
        tp, tR = pos_t[idx].clone(), rot_t[idx].clone()
        out["w"][b, track] = wtab.numpy()
        out["tracked"][b, track] = 1
        out["tgt_pos"][b, track] = tp.numpy()
        out["tgt_rot"][b, track] = tR.reshape(-1, 9).numpy()
        MG.reset_state(drag, Z0[b], CR[b])
        drag.current_global_pos = GP[b].reshape(1, 3, 1).clone()
        stub.z_tgt = ZT[b]
        if early_stop:
            kw = dict(stop_eps_pos=0.01 * 0.01, stop_eps_rot=0.01, max_iter=n_iter, min_loss_incr=0.00001)
        else:
            kw = dict(stop_eps_pos=0.0, stop_eps_rot=0.0, max_iter=n_iter, min_loss_incr=-float("inf"))
        drag.run(target_ee_pos=tp, target_ee_rot=tR, mask_joints=idx, weights_joints=wtab, offsets=off_b, learning_rate=1e-2,
                 lambda_rot=1, lambda_temporal=0.02, temporal_future_window=0, height_indices=[0, 4, 8, 13, 17, 21],
                 joint_adjustment_indices=None, joint_adjustment_weight=0.0, verbose=False, **kw)
        last = drag.rec[-1]
        out["iters"][b] = len(drag.rec)
        out["pos"][b], out["rot"][b] = last["pos"].numpy(), last["rot"].reshape(MG.NJ, 9).numpy()
        out["z_final"][b] = drag.latent.detach().reshape(24).numpy()
        out["z_pre"][b] = drag.current_latent.reshape(24).numpy()
        for i, r in enumerate(drag.rec):
            out["loss_hist"][b, i] = r["losses"]
            out["extra_hist"][b, i] = r["extra"]
        if b % 32 == 0:
            print(f"[{name}] frame {b}/{B} iters={len(drag.rec)} extra={last['extra']:.5f}", flush=True)
    meta = dict(name=name, B=B, n_iter=n_iter, lr=1e-2, lambda_rot=1.0, lambda_tmp=0.02, early_stop=bool(early_stop),
                stop_eps_pos=1e-4 if early_stop else 0.0, stop_eps_rot=1e-2 if early_stop else 0.0,
                min_loss_incr=1e-5 if early_stop else None, constraints="reference", weight_rounding="none", torch=torch.__version__)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    return out


def main():
    parents, offsets = MG.parse_bvh_skeleton(os.path.join(MG.REF, "data", "example", "eval", "example.bvh"))
    offsets_t = torch.tensor(offsets)
    mod = constrained_module()
    dst = os.path.join(MG.REPO, "tests", "golden")
    recipes = (("cons_s1", 256, 50, False, False), ("cons_es", 128, 100, True, False),
               ("cons_skel", 256, 50, False, True), ("cons_skel_es", 128, 100, True, True))
    unknown = set(sys.argv[1:]) - {r[0] for r in recipes}
    if unknown:
        raise SystemExit(f"unknown golden {sorted(unknown)}")
    for name, B, n_iter, es, skel in recipes:
        if sys.argv[1:] and name not in sys.argv[1:]:
            continue
        frames = MG.skeleton_set(offsets_t, B) if skel else None
        np.savez_compressed(os.path.join(dst, name + ".npz"), **run(name, B, n_iter, es, mod, parents, offsets_t, frames))


if __name__ == "__main__":
    main()

"""Differentiable decode + FK: the reference's forward pass as a torch autograd op on the HIP kernels.

`decode_fk(opt, z, cur_rot)` returns the outputs of ``LatentOptimizer.forward`` (drag_pose.py:84-113 with autoencoder.py:224-256,
utils.py:80-149) as tensors with a ``grad_fn``; their backward is ONE ``dp_forward_vjp`` launch (include/dragposer_grad.h) on
torch's current stream, which returns the gradients for both ``z`` and ``cur_rot``.  A user constraint is then a few lines of
PyTorch on those outputs, optimised the way the reference's DragPose.loss is (drag_pose.py:66-194, loss.backward(), Adam):

    z = z0.clone().requires_grad_()
    adam = torch.optim.Adam([z], lr=1e-2)
    for _ in range(n):
        o = decode_fk(opt, z, cur_rot)
        loss = tracker_loss(o["pos"], o["rot"]) + w * torch.relu(-o["pos"][:, feet, 1]).pow(2).sum()
        adam.zero_grad(); loss.backward(); adam.step()

`decode_fk(opt, z, cur_rot, offsets=...)` runs the same with the performer's bone offsets passed per call, as the reference's
fk_rotmat(..., offsets) takes them: [22,3] for every frame or [B,22,3] one per frame, the context's topology
(include/dragposer_skeleton.h).  The forward is then ``dp_forward_skeleton`` and the backward ONE ``dp_forward_vjp_skeleton`` launch,
which also returns the gradient of the offsets when they require it -- so a batch of mixed performers needs one context, and a
performer's bone lengths can be fitted to tracker data:

    s = torch.ones((), device=dev, requires_grad=True)
    adam = torch.optim.Adam([s], lr=1e-2)
    for _ in range(n):
        o = decode_fk(opt, z, cur_rot, outputs=("pos",), offsets=s * base)
        loss = ((o["pos"] - tgt_pos) ** 2).sum()
        adam.zero_grad(); loss.backward(); adam.step()

There is no CPU path: the forward and the backward are the library's kernels.  Second derivatives are not available (the backward
is a kernel, `once_differentiable`): asking for them raises.
"""
import torch
from torch.autograd.function import once_differentiable

from .model import NJ
from .optimizer import _GRAD_NAMES

OUTPUTS = _GRAD_NAMES


class _DecodeFK(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opt, names, z, cur_rot, offsets):
        z, cur_rot = z.detach().contiguous(), cur_rot.detach().contiguous()
        if offsets is not None:
            offsets = offsets.detach().contiguous()  # (an expanded view is materialised; autograd reduces its gradient)
        out = opt.forward(z, cur_rot, outputs=names, offsets=offsets)
        ctx.opt, ctx.names = opt, names
        ctx.save_for_backward(z, cur_rot, offsets)
        return tuple(out[n] for n in names)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        z, cur_rot, offsets = ctx.saved_tensors
        g = {n: gr.contiguous() for n, gr in zip(ctx.names, grads) if gr is not None}
        if offsets is None:
            r = ctx.opt.forward_vjp(z, cur_rot, g)
            doff = None
        else:
            want = ctx.needs_input_grad[4]
            r = ctx.opt.forward_vjp(z, cur_rot, g, offsets=offsets, doffsets=want)
            doff = (r["doffsets"] if offsets.dim() == 3 else r["doffsets"].sum(0)) if want else None
        return None, None, (r["dz"] if ctx.needs_input_grad[2] else None), (r["dcur_rot"] if ctx.needs_input_grad[3] else None), doff


def decode_fk(opt, z, cur_rot, outputs=OUTPUTS, offsets=None):
    """Decode + FK of z [B,24] under cur_rot [B,4] (fp32 device tensors on `opt`'s device, `opt` a LatentOptimizer) -> dict
    {name: tensor} of the requested `outputs` (pose [B,88], disp [B,3], world_disp [B,3], world_rot [B,4], pos [B,22,3],
    rot [B,22,9]), differentiable w.r.t. z and cur_rot.  `offsets`: the performer's bone offsets, an fp32 device tensor [22,3] (every
    frame) or [B,22,3] (one skeleton per frame; an expanded view is fine), row 0 ignored -- differentiable too."""
    names = tuple(outputs)
    for n in names:
        if n not in OUTPUTS:
            raise ValueError(f"decode_fk: unknown output {n!r} (one of {', '.join(OUTPUTS)})")
    if len(set(names)) != len(names) or not names:
        raise ValueError("decode_fk: outputs must be distinct and not empty")
    if offsets is not None:
        if not isinstance(offsets, torch.Tensor):
            raise TypeError("decode_fk: offsets must be a torch.Tensor, [22,3] or [B,22,3]")
        B = int(z.shape[0])
        if tuple(offsets.shape) not in ((NJ, 3), (B, NJ, 3)):
            raise ValueError(f"decode_fk: offsets must be [22,3] (one skeleton) or [{B},22,3] (one per frame), got {tuple(offsets.shape)}")
    return dict(zip(names, _DecodeFK.apply(opt, names, z, cur_rot, offsets)))

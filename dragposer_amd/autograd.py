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

There is no CPU path: the forward and the backward are the library's kernels.  Second derivatives are not available (the backward
is a kernel, `once_differentiable`): asking for them raises.
"""
import torch
from torch.autograd.function import once_differentiable

from .optimizer import _GRAD_NAMES

OUTPUTS = _GRAD_NAMES


class _DecodeFK(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opt, names, z, cur_rot):
        z, cur_rot = z.detach().contiguous(), cur_rot.detach().contiguous()
        out = opt.forward(z, cur_rot, outputs=names)
        ctx.opt, ctx.names = opt, names
        ctx.save_for_backward(z, cur_rot)
        return tuple(out[n] for n in names)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        z, cur_rot = ctx.saved_tensors
        g = {n: gr.contiguous() for n, gr in zip(ctx.names, grads) if gr is not None}
        r = ctx.opt.forward_vjp(z, cur_rot, g)
        return None, None, (r["dz"] if ctx.needs_input_grad[2] else None), (r["dcur_rot"] if ctx.needs_input_grad[3] else None)


def decode_fk(opt, z, cur_rot, outputs=OUTPUTS):
    """Decode + FK of z [B,24] under cur_rot [B,4] (fp32 device tensors on `opt`'s device, `opt` a LatentOptimizer) -> dict
    {name: tensor} of the requested `outputs` (pose [B,88], disp [B,3], world_disp [B,3], world_rot [B,4], pos [B,22,3],
    rot [B,22,9]), differentiable w.r.t. z and cur_rot."""
    names = tuple(outputs)
    for n in names:
        if n not in OUTPUTS:
            raise ValueError(f"decode_fk: unknown output {n!r} (one of {', '.join(OUTPUTS)})")
    if len(set(names)) != len(names) or not names:
        raise ValueError("decode_fk: outputs must be distinct and not empty")
    return dict(zip(names, _DecodeFK.apply(opt, names, z, cur_rot)))

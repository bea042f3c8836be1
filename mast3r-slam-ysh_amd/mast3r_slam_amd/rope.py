"""RoPE2D on the device kernel (mast3r_slam_backends.rope_2d), with the
interface of the reference's cuRoPE2D (croco models/curope/curope2d.py), and
``install`` to put it into a loaded MASt3R model:

    from mast3r_slam_amd import rope
    rope.install(model)

The reference's curope is a CUDA-only extension; without it croco's
models/pos_embed.py:106-159 falls back to a torch implementation that makes
about twenty small launches per call and reads ``positions.max()`` on the host
each time. This module is one launch per call and never synchronises.
"""
from __future__ import annotations

import torch

import mast3r_slam_backends as be


def _layout_ok(t):
    """Whether t.transpose(1, 2) of a [B, H, N, D] tensor is what rope_2d takes."""
    return t.stride(3) == 1 and (t.shape[1] == 1 or t.stride(1) == t.shape[3])


class _Rope2dFunction(torch.autograd.Function):
    """tokens [B, H, N, D], rotated in place; the backward is the inverse
    rotation (-F0) of the incoming gradient, in place as well."""

    @staticmethod
    def forward(ctx, tokens, positions, base, F0):
        ctx.save_for_backward(positions)
        ctx.base, ctx.F0 = base, F0
        be.rope_2d(tokens.transpose(1, 2), positions, base, F0)
        ctx.mark_dirty(tokens)
        return tokens

    @staticmethod
    def backward(ctx, grad):
        (positions,) = ctx.saved_tensors
        if not _layout_ok(grad):  # a gradient in some other layout: rotate a copy in the kernel's layout
            grad = grad.transpose(1, 2).contiguous().transpose(1, 2)
        be.rope_2d(grad.transpose(1, 2), positions, ctx.base, -ctx.F0)
        return grad, None, None, None


class RoPE2D(torch.nn.Module):
    """forward(tokens [B, H, N, D], positions [B, N, 2] int64 (y, x)) rotates
    ``tokens`` in place and returns it. ``tokens.transpose(1, 2)`` must have a
    contiguous head row and the heads of a token back to back, as the q and k
    slices of an attention's qkv buffer have."""

    def __init__(self, freq=100.0, F0=1.0):
        super().__init__()
        self.base = freq
        self.F0 = F0

    def forward(self, tokens, positions):
        return _Rope2dFunction.apply(tokens, positions, self.base, self.F0)

    def extra_repr(self):
        return f"base={self.base}, F0={self.F0}"


_REPLACED = ("RoPE2D", "cuRoPE2D")


def install(model) -> int:
    """Replace every submodule attribute named ``rope`` whose class is called
    RoPE2D or cuRoPE2D by a device RoPE2D with the old module's ``base`` and
    ``F0``. A module shared between blocks (croco builds one and hands it to
    every block) is replaced by one shared module. Returns the number of
    attributes replaced; modules already on the device kernel are left alone."""
    new_for = {}
    count = 0
    for module in list(model.modules()):
        old = module._modules.get("rope")
        if old is None or isinstance(old, RoPE2D) or type(old).__name__ not in _REPLACED:
            continue
        if id(old) not in new_for:
            new_for[id(old)] = RoPE2D(freq=old.base, F0=old.F0)
        module.rope = new_for[id(old)]
        count += 1
    return count

"""The attention core of MASt3R's blocks on the device kernel
(mast3r_slam_backends.attention_rope), and ``install`` to put it into a loaded
MASt3R model:

    from mast3r_slam_amd import attention
    attention.install(model)

croco's Attention and CrossAttention (models/blocks.py:94-112, 149-169) run,
between their ``Linear``s, two rope calls, a batched matmul that writes the
[B, H, N, N] score matrix, a multiply, a softmax, a second matmul and a
transpose-and-reshape copy. Here that is one launch: the module's own
``Linear``s run as before, views of their outputs go to the kernel, and its
[B, N, C] result goes to ``proj``; nothing is copied in between.

The kernel is fp32, head dimension 64, forward only. Whenever it does not apply
the module's original ``forward`` runs unchanged.
"""
from __future__ import annotations

import types

import torch

import mast3r_slam_backends as be

from . import rope as _rope

_SELF_ATTRS = ("qkv", "proj", "proj_drop", "attn_drop", "num_heads", "scale", "rope")
_CROSS_ATTRS = ("projq", "projk", "projv", "proj", "proj_drop", "attn_drop", "num_heads", "scale", "rope")
_ROPES = ("RoPE2D", "cuRoPE2D")  # the reference's two; the device RoPE2D is an instance check


def _rope_params(module):
    """(rotate, base, F0) of the module's rope as it is now, or None for a rope
    of an unknown class."""
    r = module.rope
    if r is None:
        return False, 100.0, 1.0
    if isinstance(r, _rope.RoPE2D) or type(r).__name__ in _ROPES:
        try:
            return True, float(r.base), float(r.F0)
        except (AttributeError, TypeError, ValueError):
            return None
    return None


def _applies(module, inputs, head_dim):
    """Whether the kernel computes what the original forward would: every input
    on a GPU and fp32, head dimension 64, nothing to differentiate, no dropout
    on the attention weights."""
    if head_dim != be.ATTN_HEAD_DIM:
        return False
    for t in inputs:
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.float32:
            return False
    if torch.is_autocast_enabled():
        return False
    if torch.is_grad_enabled() and (any(t.requires_grad for t in inputs)
                                    or any(p.requires_grad for p in module.parameters())):
        return False  # no backward
    if module.training and float(getattr(module.attn_drop, "p", 0.0)) > 0.0:
        return False
    return True


def fused_attention_forward(module, x, xpos):
    """Attention.forward (blocks.py:94-112) with its core on the device kernel."""
    original = vars(module).get("_m3s_original_forward") or type(module).forward.__get__(module)
    params = _rope_params(module)
    if params is None or not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[2] % module.num_heads \
            or not _applies(module, (x,), x.shape[2] // module.num_heads):
        return original(x, xpos)
    rotate, base, f0 = params
    B, N, C = x.shape
    H = module.num_heads
    qkv = module.qkv(x)
    if qkv.dtype != torch.float32:
        return original(x, xpos)
    qkv = qkv.view(B, N, 3, H, C // H)
    pos = xpos if rotate else None
    out = be.attention_rope(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], pos, pos, base, f0, float(module.scale))
    return module.proj_drop(module.proj(out))


def fused_cross_attention_forward(module, query, key, value, qpos, kpos):
    """CrossAttention.forward (blocks.py:149-169) with its core on the device kernel."""
    original = vars(module).get("_m3s_original_forward") or type(module).forward.__get__(module)
    params = _rope_params(module)
    ok = params is not None and all(isinstance(t, torch.Tensor) and t.dim() == 3 for t in (query, key, value))
    if ok:
        C = query.shape[2]
        ok = C % module.num_heads == 0 and key.shape[1] == value.shape[1] \
            and _applies(module, (query, key, value), C // module.num_heads)
    if not ok:
        return original(query, key, value, qpos, kpos)
    rotate, base, f0 = params
    B, Nq, C = query.shape
    Nk, H = key.shape[1], module.num_heads
    q, k, v = module.projq(query), module.projk(key), module.projv(value)
    if any(t.dtype != torch.float32 for t in (q, k, v)):
        return original(query, key, value, qpos, kpos)
    out = be.attention_rope(q.view(B, Nq, H, C // H), k.view(B, Nk, H, C // H), v.view(B, Nk, H, C // H),
                            qpos if rotate else None, kpos if rotate else None, base, f0, float(module.scale))
    return module.proj_drop(module.proj(out))


def _kind(module):
    name = type(module).__name__
    if name == "Attention" and all(hasattr(module, a) for a in _SELF_ATTRS):
        return fused_attention_forward
    if name == "CrossAttention" and all(hasattr(module, a) for a in _CROSS_ATTRS):
        return fused_cross_attention_forward
    return None


def install(model) -> int:
    """Put every submodule whose class is named ``Attention`` or
    ``CrossAttention`` and has the reference's attributes (``qkv`` or ``projq``
    / ``projk`` / ``projv``, ``proj``, ``proj_drop``, ``attn_drop``,
    ``num_heads``, ``scale``, ``rope``) on the fused path: ``forward`` is
    overridden on the instance, as ``head.install`` does. ``rope`` may be None,
    the reference's RoPE2D or cuRoPE2D, or the device RoPE2D; ``base`` and
    ``F0`` are read at call time, so the order of ``rope.install`` and this
    does not matter. The new forward calls the original one unchanged when the
    input is not on a GPU, not fp32 (or under autocast), the head dimension is
    not 64, something would need a gradient, the module trains with
    ``attn_drop.p > 0``, or the rope is of an unknown class. Returns the number
    of modules patched; modules already patched are left alone."""
    count = 0
    for module in list(model.modules()):
        fused = _kind(module)
        if fused is None or "_m3s_original_forward" in vars(module):
            continue
        module._m3s_original_forward = module.forward  # the bound original
        module.forward = types.MethodType(fused, module)
        count += 1
    return count

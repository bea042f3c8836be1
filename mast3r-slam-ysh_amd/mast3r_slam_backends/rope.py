"""include/m3s_rope.h: the 2-D rotary position embedding of MASt3R's attention."""
import ctypes

import torch

from ._abi import (_F32, _I64, _INT, _P, _VP, _call, _head_rows, _on_rocm, _p, _positions, _same_device, _stream,
                    _token_strides)

ROPE_F32, ROPE_F16, ROPE_BF16 = 0, 1, 2
_ROPE_DTYPES = {torch.float32: ROPE_F32, torch.float16: ROPE_F16, torch.bfloat16: ROPE_BF16}


class RopeArgs(ctypes.Structure):
    """Mirror of ``m3s_rope_args`` (include/m3s_rope.h)."""

    _fields_ = [
        ("tokens", _VP), ("pos", _VP), ("B", _I64), ("N", _I64), ("H", _I64), ("D", _I64), ("stride_b", _I64),
        ("stride_n", _I64), ("base", _F32), ("f0", _F32), ("dtype", _INT),
    ]


_SIGNATURES = {"m3s_rope_2d": (_INT, [_P(RopeArgs), _VP])}


def rope_2d(tokens, positions, base, f0):
    """2-D rotary position embedding, in place (new entry point; m3s_rope_2d;
    RoPE2D of croco's models/pos_embed.py:112-159, which the reference runs
    through its curope extension).

    tokens: the [B, N, H, D] view of q or k, float32, float16 or bfloat16, D a
    multiple of 4, a head row contiguous and the heads of a token back to back
    (stride(3) == 1, stride(2) == D); the token and batch strides are free, so
    ``qkv[:, :, i].transpose(1, 2)`` of an attention's [B, H, 3, N, D] view is
    taken as it is. positions [B, N, 2] int64, (y, x) per token. The angle of
    frequency i of an axis is position * f0 / base^(i / (D/4)), evaluated in
    fp32; the result is rounded once to the tokens' dtype. f0 -> -f0 undoes the
    rotation. One launch, no host synchronisation. Returns tokens."""
    if not isinstance(tokens, torch.Tensor) or not isinstance(positions, torch.Tensor):
        raise RuntimeError("rope_2d: tokens and positions must be tensors")
    # layout and dtype first, the device last, in the order of _check
    if tokens.dtype not in _ROPE_DTYPES:
        raise RuntimeError(f"tokens must be float32, float16 or bfloat16 (got {tokens.dtype})")
    if tokens.dim() != 4:
        raise RuntimeError(f"tokens must be [B, N, H, D] (got {tuple(tokens.shape)})")
    B, N, H, D = (int(x) for x in tokens.shape)
    if D % 4 != 0:
        raise RuntimeError(f"rope_2d: D = {D} is not a multiple of 4")
    _head_rows(tokens, "tokens", H, D)
    _positions(positions, "positions", B, N)
    _on_rocm(tokens, "tokens")
    _same_device("rope_2d", (("positions", positions),), "tokens", tokens.device)
    if tokens.numel() == 0:
        return tokens
    a = RopeArgs()
    a.tokens, a.pos = _p(tokens), _p(positions)
    a.B, a.N, a.H, a.D = B, N, H, D
    a.stride_b, a.stride_n = _token_strides(tokens, N, H * D)
    a.base, a.f0, a.dtype = float(base), float(f0), _ROPE_DTYPES[tokens.dtype]
    _call("m3s_rope_2d", ctypes.byref(a), _stream(tokens.device))
    return tokens

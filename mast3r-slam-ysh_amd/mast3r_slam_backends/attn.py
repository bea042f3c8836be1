"""include/m3s_attn.h: RoPE2D, scores, softmax and the product with v in one launch."""
import ctypes

import torch

from ._abi import _F32, _I64, _INT, _P, _VP, _call, _head_rows, _p, _positions, _same_device, _stream, _token_strides
from .rope import ROPE_F32

ATTN_HEAD_DIM = 64


class AttnArgs(ctypes.Structure):
    """Mirror of ``m3s_attn_args`` (include/m3s_attn.h)."""

    _fields_ = [
        ("q", _VP), ("k", _VP), ("v", _VP), ("out", _VP), ("qpos", _VP), ("kpos", _VP), ("B", _I64), ("Nq", _I64),
        ("Nk", _I64), ("H", _I64), ("D", _I64), ("q_sb", _I64), ("q_sn", _I64), ("k_sb", _I64), ("k_sn", _I64),
        ("v_sb", _I64), ("v_sn", _I64), ("o_sb", _I64), ("o_sn", _I64), ("base", _F32), ("f0", _F32), ("scale", _F32),
        ("dtype", _INT),
    ]


_SIGNATURES = {"m3s_attn_rope": (_INT, [_P(AttnArgs), _VP])}


def attention_rope(q, k, v, qpos, kpos, base, f0, scale, *, out=None):
    """The attention core of MASt3R's blocks in one launch (new entry point;
    m3s_attn_rope; croco models/blocks.py:94-112, 149-169): RoPE2D of q and k
    (the rotation of ``rope_2d``, bitwise), softmax(scale q' k'^T) v.

    q [B, Nq, H, 64], k and v [B, Nk, H, 64]: float32 views with a contiguous
    head row and the heads of a token back to back (stride(3) == 1, stride(2)
    == 64); the token and batch strides are free, so the three slices
    ``qkv[:, :, i]`` of an attention's [B, N, 3, H, D] buffer and the dense
    projections of a cross attention are taken as they are. They are only
    read. qpos [B, Nq, 2], kpos [B, Nk, 2] int64 (y, x), or both None for no
    rotation.

    -> out [B, Nq, H * 64] float32, the layout ``proj`` takes. out= writes into
    the caller's tensor: its rows must be contiguous, its token and batch
    strides are free. On the current stream; no allocation when out is given;
    no host synchronisation; two runs agree bitwise."""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"attention_rope: {name} must be a tensor")
    # layout and dtype first, the device last, in the order of rope_2d
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be {torch.float32} (got {t.dtype})")
        if t.dim() != 4:
            raise RuntimeError(f"{name} must be [B, N, H, D] (got {tuple(t.shape)})")
    B, Nq, H, D = (int(x) for x in q.shape)
    if D != ATTN_HEAD_DIM:
        raise RuntimeError(f"attention_rope: D = {D}, only the head dimension {ATTN_HEAD_DIM} is built")
    Nk = int(k.shape[1])
    if tuple(k.shape) != (B, Nk, H, D):
        raise RuntimeError(f"k must be [{B}, Nk, {H}, {D}] (got {tuple(k.shape)})")
    if tuple(v.shape) != (B, Nk, H, D):
        raise RuntimeError(f"v must be [{B}, {Nk}, {H}, {D}] (got {tuple(v.shape)})")
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        _head_rows(t, name, H, D)
    if (qpos is None) != (kpos is None):
        raise RuntimeError("attention_rope: qpos and kpos must both be given or both be None")
    for t, name, n in ((qpos, "qpos", Nq), (kpos, "kpos", Nk)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"attention_rope: {name} must be a tensor or None")
        _positions(t, name, B, n)
    row = H * D
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise RuntimeError("attention_rope: out must be a tensor")
        if out.dtype != torch.float32:
            raise RuntimeError(f"out must be {torch.float32} (got {out.dtype})")
        if tuple(out.shape) != (B, Nq, row):
            raise RuntimeError(f"out must be [{B}, {Nq}, {row}] (got {tuple(out.shape)})")
        if out.numel() and out.stride(2) != 1:
            raise RuntimeError("out: a row must be contiguous (stride(2) == 1)")
    if Nk == 0 and B * Nq * H:
        raise RuntimeError("attention_rope: Nk = 0, a softmax over no keys")
    _same_device("attention_rope", (("q", q), ("k", k), ("v", v), ("qpos", qpos), ("kpos", kpos), ("out", out)),
                 "q", q.device, rocm=True)
    if out is None:
        out = torch.empty((B, Nq, row), dtype=torch.float32, device=q.device)
    if B * Nq * H == 0:
        return out
    a = AttnArgs()
    a.q, a.k, a.v, a.out, a.qpos, a.kpos = _p(q), _p(k), _p(v), _p(out), _p(qpos), _p(kpos)
    a.B, a.Nq, a.Nk, a.H, a.D = B, Nq, Nk, H, D
    a.q_sb, a.q_sn = _token_strides(q, Nq, row)
    a.k_sb, a.k_sn = _token_strides(k, Nk, row)
    a.v_sb, a.v_sn = _token_strides(v, Nk, row)
    a.o_sb, a.o_sn = _token_strides(out, Nq, row)
    a.base, a.f0, a.scale, a.dtype = float(base), float(f0), float(scale), ROPE_F32
    _call("m3s_attn_rope", ctypes.byref(a), _stream(q.device))
    return out

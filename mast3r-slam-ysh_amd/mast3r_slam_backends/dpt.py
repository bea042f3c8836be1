"""include/m3s_dpt.h: the last four modules of MASt3R's DPT head in one launch."""
import ctypes

import torch

from ._abi import _I64, _INT, _P, _SIZE, _VP, _call, _p, _same_device, _stream, _sym

DPT_CH = 128  # Cin = Cmid
DPT_MAX_COUT = 4
DPT_TILE_H, DPT_TILE_W = 8, 32  # output pixels of one workgroup
DPT_MAX_SIDE = 1 << 20


class DptTailArgs(ctypes.Structure):
    """Mirror of ``m3s_dpt_tail_args`` (include/m3s_dpt.h)."""

    _fields_ = [
        ("x", _VP), ("packed", _VP), ("out", _VP), ("B", _I64), ("Hi", _I64), ("Wi", _I64), ("Cout", _I64),
        ("x_sb", _I64), ("out_sb", _I64), ("flags", _INT),
    ]


_SIGNATURES = {
    "m3s_dpt_tail_packed_size": (_SIZE, [_I64]),
    "m3s_dpt_tail_pack": (_INT, [_VP, _VP, _VP, _VP, _I64, _VP, _VP]),
    "m3s_dpt_tail": (_INT, [_P(DptTailArgs), _VP]),
}


def dpt_tail_packed_size(cout):
    """Bytes of the packed weights for ``cout`` outputs (m3s_dpt_tail_packed_size); 0 unless 1 <= cout <= 4."""
    return int(_sym("m3s_dpt_tail_packed_size")(int(cout)))


def dpt_tail_pack(w1, b1, w2, b2):
    """Pack the weights of the DPT tail once per model (m3s_dpt_tail_pack): w1
    [128,128,3,3], b1 [128], w2 [Cout,128] (or [Cout,128,1,1]), b2 [Cout], float32
    contiguous on one ROCm device, 1 <= Cout <= 4 -> a uint8 tensor of
    ``dpt_tail_packed_size(Cout)`` bytes for ``dpt_tail``. One launch on the
    current stream; the four tensors are only read."""
    items = (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2))
    for name, t in items:
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"dpt_tail_pack: {name} must be a tensor")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be {torch.float32} (got {t.dtype})")
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous")
    if tuple(w1.shape) != (DPT_CH, DPT_CH, 3, 3):
        raise RuntimeError(f"w1 must be [{DPT_CH}, {DPT_CH}, 3, 3] (got {tuple(w1.shape)})")
    if tuple(b1.shape) != (DPT_CH,):
        raise RuntimeError(f"b1 must be [{DPT_CH}] (got {tuple(b1.shape)})")
    if w2.dim() not in (2, 4) or tuple(w2.shape[1:]) not in ((DPT_CH,), (DPT_CH, 1, 1)):
        raise RuntimeError(f"w2 must be [Cout, {DPT_CH}] or [Cout, {DPT_CH}, 1, 1] (got {tuple(w2.shape)})")
    cout = int(w2.shape[0])
    if not 1 <= cout <= DPT_MAX_COUT:
        raise RuntimeError(f"dpt_tail_pack: Cout = {cout}, only 1..{DPT_MAX_COUT} are built")
    if tuple(b2.shape) != (cout,):
        raise RuntimeError(f"b2 must be [{cout}] (got {tuple(b2.shape)})")
    _same_device("dpt_tail_pack", items, "w1", w1.device, rocm=True)
    packed = torch.empty(dpt_tail_packed_size(cout), dtype=torch.uint8, device=w1.device)
    _call("m3s_dpt_tail_pack", _p(w1), _p(b1), _p(w2), _p(b2), cout, _p(packed), _stream(w1.device))
    return packed


def dpt_tail(x, packed, cout, *, out=None):
    """The last four modules of MASt3R's DPT head in one launch (new entry
    point; m3s_dpt_tail; croco models/dpt_block.py:318-324): bilinear x2
    upsampling with align_corners, Conv2d(128 -> 128, 3x3, padding 1), ReLU and
    Conv2d(128 -> cout, 1x1), float32.

    x [B,128,Hi,Wi] f32 whose images are contiguous (NCHW; the batch stride is
    free); packed: ``dpt_tail_pack``'s tensor for the same cout. Both are only
    read.

    -> out [B,cout,2Hi,2Wi] f32, the ``pts`` that ``head_postprocess`` reads.
    out= writes into the caller's tensor: each image must be contiguous, the
    batch stride is free. On the current stream; no allocation when out is
    given; no host synchronisation; two runs agree bitwise."""
    # layout and dtype first, the device last, in the order of head_postprocess
    for t, name in ((x, "x"), (packed, "packed")):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"dpt_tail: {name} must be a tensor")
    if x.dtype != torch.float32:
        raise RuntimeError(f"x must be {torch.float32} (got {x.dtype})")
    if packed.dtype != torch.uint8:
        raise RuntimeError(f"packed must be {torch.uint8} (got {packed.dtype}): dpt_tail_pack's tensor")
    cout = int(cout)
    if not 1 <= cout <= DPT_MAX_COUT:
        raise RuntimeError(f"dpt_tail: cout = {cout}, only 1..{DPT_MAX_COUT} are built")
    if x.dim() != 4 or x.shape[1] != DPT_CH:
        raise RuntimeError(f"x must be [B, {DPT_CH}, Hi, Wi] (got {tuple(x.shape)})")
    B, _, Hi, Wi = (int(v) for v in x.shape)
    if max(Hi, Wi) > DPT_MAX_SIDE:
        raise RuntimeError(f"x: Hi = {Hi} and Wi = {Wi} must be <= {DPT_MAX_SIDE}")
    if x.numel() and not x[0].is_contiguous():
        raise RuntimeError("x: every image must be contiguous (NCHW; only the batch stride is free)")
    need = dpt_tail_packed_size(cout)
    if packed.dim() != 1 or packed.numel() != need or not packed.is_contiguous():
        raise RuntimeError(f"packed must be dpt_tail_pack's tensor of {need} bytes (got {tuple(packed.shape)})")
    shape = (B, cout, 2 * Hi, 2 * Wi)
    x_sb, out_sb = DPT_CH * Hi * Wi, cout * 4 * Hi * Wi
    if B > 1:  # the stride of a dimension of size 1 is arbitrary: keep the dense value
        if x.stride(0) < x_sb:
            raise RuntimeError(f"x: the images overlap (batch stride {x.stride(0)} < {x_sb})")
        x_sb = x.stride(0)
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise RuntimeError("dpt_tail: out must be a tensor")
        if tuple(out.shape) != shape:
            raise RuntimeError(f"out must be {list(shape)} (got {tuple(out.shape)})")
        if out.dtype != torch.float32:
            raise RuntimeError(f"out must be {torch.float32} (got {out.dtype})")
        if out.numel() and not out[0].is_contiguous():
            raise RuntimeError("out: every image must be contiguous (only the batch stride is free)")
        if B > 1:
            if out.stride(0) < out_sb:
                raise RuntimeError(f"out: the images overlap (batch stride {out.stride(0)} < {out_sb})")
            out_sb = out.stride(0)
    if B * max(DPT_CH, cout * 4) * Hi * Wi > 2**31 - 1:
        raise RuntimeError(f"dpt_tail: {list(x.shape)} is too large (more than 2^31 - 1 elements in x or out)")
    _same_device("dpt_tail", (("x", x), ("packed", packed), ("out", out)), "x", x.device, rocm=True)
    if packed.data_ptr() % 16:
        raise RuntimeError("packed must be 16-byte aligned: dpt_tail_pack's tensor")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    if B * Hi * Wi == 0:
        return out
    a = DptTailArgs()
    a.x, a.packed, a.out = _p(x), _p(packed), _p(out)
    a.B, a.Hi, a.Wi, a.Cout = B, Hi, Wi, cout
    a.x_sb, a.out_sb, a.flags = x_sb, out_sb, 0
    _call("m3s_dpt_tail", ctypes.byref(a), _stream(x.device))
    return out

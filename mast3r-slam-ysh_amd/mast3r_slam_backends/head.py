"""include/m3s_head.h: the tail of MASt3R's catmlp+dpt head in one launch."""
import ctypes
import math

import torch

from ._abi import _F32, _I64, _INT, _VP, _call, _p, _same_device, _stream

HEAD_F32, HEAD_F16 = 0, 1
HEAD_GENERIC = 1  # flags
_HEAD_DTYPES = {torch.float32: HEAD_F32, torch.float16: HEAD_F16}
_HEAD_OUT = ("X", "C", "D", "Q")


class HeadArgs(ctypes.Structure):
    """Mirror of ``m3s_head_args`` (include/m3s_head.h)."""

    _fields_ = [
        ("pts", _VP), ("feat", _VP), ("X", _VP), ("C", _VP), ("D", _VP), ("Q", _VP), ("B", _I64), ("H", _I64),
        ("W", _I64), ("P", _I64), ("F", _I64), ("ds", _I64), ("sbX", _I64), ("sbC", _I64), ("sbD", _I64), ("sbQ", _I64),
        ("conf_vmin", _F32), ("conf_vmax", _F32), ("dconf_vmin", _F32), ("dconf_vmax", _F32), ("desc_dtype", _INT),
        ("flags", _INT),
    ]


_SIGNATURES = {"m3s_head_postprocess": (_INT, [ctypes.POINTER(HeadArgs), _VP])}


def _head_mode(mode, name):
    try:
        vmin, vmax = (float(v) for v in mode)
    except (TypeError, ValueError):
        raise RuntimeError(f"{name} must be (vmin, vmax)") from None
    if not math.isfinite(vmin) or not vmax >= vmin:
        raise RuntimeError(f"{name} must be a finite vmin and a vmax >= vmin (got {mode})")
    return vmin, vmax


def head_postprocess(pts, feat, patch_size, desc_dim, *, conf=(1.0, float("inf")), desc_conf=(0.0, float("inf")),
                     downsample=1, desc_dtype=torch.float32, out=None, generic=False):
    """The tail of MASt3R's catmlp+dpt head in one launch (new entry point;
    m3s_head_postprocess; catmlp_dpt_head.py:25-39, 82-96, dust3r
    heads/postprocess.py:22-58 and the stack / downsample / .half() of the SLAM
    side, mast3r_utils.py:43-52, 73-79).

    pts [B,4,H,W] f32 contiguous: the DPT output (x, y, z, raw confidence). feat
    [B,S,(F+1)*P*P] f32 contiguous: head_local_features' output, S =
    (H/P)*(W/P), P = patch_size, F = desc_dim. conf and desc_conf are the
    (vmin, vmax) of the two 'exp' confidence modes. downsample = k keeps the
    pixels [::k, ::k].

    -> (X [B,Ho,Wo,3] f32, C [B,Ho,Wo] f32, D [B,Ho,Wo,F] desc_dtype (float32 or
    float16, the fp32 value rounded once), Q [B,Ho,Wo] f32). out=(X, C, D, Q)
    writes into the caller's tensors instead: each image of each must be
    contiguous, the batch stride is free, so slot k of a stacked [4,B,Ho,Wo,.]
    buffer, or rows of a wider one, are taken as they are. generic=True takes
    the element-wise kernel whatever the shape (the same values, bitwise). On
    the current stream; no allocation when out is given; no host
    synchronisation."""
    a, out = _head_args(pts, feat, patch_size, desc_dim, conf, desc_conf, downsample, desc_dtype, out, generic)
    if a is not None:
        _call("m3s_head_postprocess", ctypes.byref(a), _stream(pts.device))
    return out


def _head_args(pts, feat, patch_size, desc_dim, conf, desc_conf, downsample, desc_dtype, out, generic):
    """Validate and fill an ``m3s_head_args``; -> (args or None when there is
    nothing to do, (X, C, D, Q))."""
    # layout and dtype first, the device last, in the order of rope_2d
    for t, name in ((pts, "pts"), (feat, "feat")):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{name} must be a tensor")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be {torch.float32} (got {t.dtype})")
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous")
    P, F, ds = int(patch_size), int(desc_dim), int(downsample)
    for v, name in ((P, "patch_size"), (F, "desc_dim"), (ds, "downsample")):
        if v < 1:
            raise RuntimeError(f"{name} must be >= 1 (got {v})")
    if pts.dim() != 4 or pts.shape[1] != 4:
        raise RuntimeError(f"pts must be [B, 4, H, W] (got {tuple(pts.shape)})")
    B, _, H, W = (int(x) for x in pts.shape)
    if H % P or W % P:
        raise RuntimeError(f"pts: H = {H} and W = {W} must be multiples of patch_size = {P}")
    want = (B, (H // P) * (W // P), (F + 1) * P * P)
    if tuple(feat.shape) != want:
        raise RuntimeError(f"feat must be {list(want)} (got {tuple(feat.shape)})")
    if desc_dtype not in _HEAD_DTYPES:
        raise RuntimeError(f"desc_dtype must be float32 or float16 (got {desc_dtype})")
    conf, desc_conf = _head_mode(conf, "conf"), _head_mode(desc_conf, "desc_conf")
    Ho, Wo = -(-H // ds), -(-W // ds)
    shapes = ((B, Ho, Wo, 3), (B, Ho, Wo), (B, Ho, Wo, F), (B, Ho, Wo))
    dtypes = (torch.float32, torch.float32, desc_dtype, torch.float32)
    strides = [math.prod(s[1:]) for s in shapes]
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 4:
            raise RuntimeError("out must be (X, C, D, Q)")
        for k, (t, name, shape, dtype) in enumerate(zip(out, _HEAD_OUT, shapes, dtypes)):
            if not isinstance(t, torch.Tensor):
                raise RuntimeError(f"out {name} must be a tensor")
            if tuple(t.shape) != shape:
                raise RuntimeError(f"out {name} must be {list(shape)} (got {tuple(t.shape)})")
            if t.dtype != dtype:
                raise RuntimeError(f"out {name} must be {dtype} (got {t.dtype})")
            if t.numel() and not t[0].is_contiguous():
                raise RuntimeError(f"out {name}: every image must be contiguous (only the batch stride is free)")
            # the stride of a dimension of size 1 is arbitrary: keep the dense value
            if B > 1:
                if t.stride(0) < strides[k]:
                    raise RuntimeError(f"out {name}: the images overlap (batch stride {t.stride(0)} < {strides[k]})")
                strides[k] = t.stride(0)
    _same_device("head_postprocess", (("pts", pts), ("feat", feat))
                 + tuple((f"out {n}", t) for t, n in zip(out or (), _HEAD_OUT)), "pts", pts.device, rocm=True)
    if out is None:
        out = tuple(torch.empty(s, dtype=d, device=pts.device) for s, d in zip(shapes, dtypes))
    if B * H * W == 0:
        return None, tuple(out)
    a = HeadArgs()
    a.pts, a.feat = _p(pts), _p(feat)
    a.X, a.C, a.D, a.Q = (_p(t) for t in out)
    a.B, a.H, a.W, a.P, a.F, a.ds = B, H, W, P, F, ds
    a.sbX, a.sbC, a.sbD, a.sbQ = strides
    (a.conf_vmin, a.conf_vmax), (a.dconf_vmin, a.dconf_vmax) = conf, desc_conf
    a.desc_dtype = _HEAD_DTYPES[desc_dtype]
    a.flags = HEAD_GENERIC if generic else 0
    return a, tuple(out)

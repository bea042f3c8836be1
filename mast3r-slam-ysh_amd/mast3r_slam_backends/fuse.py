"""include/m3s_fuse.h: keyframe pointmap fusion and the iter_proj inputs."""
import ctypes

import torch

from ._abi import _I64, _INT, _P, _VP, _call, _check, _p, _stream

FILTER_MODES = {"weighted_pointmap": 0, "indep_conf": 1, "recent": 2, "weighted_spherical": 3}


class FuseArgs(ctypes.Structure):
    """Mirror of ``m3s_fuse_args`` (include/m3s_fuse.h)."""

    _fields_ = [
        ("X_canon", _VP), ("C", _VP), ("X_new", _VP), ("C_new", _VP), ("T", _VP), ("HW", _I64), ("mode", _INT),
    ]


class PrepRaysArgs(ctypes.Structure):
    """Mirror of ``m3s_prep_rays_args`` (include/m3s_fuse.h)."""

    _fields_ = [
        ("X11", _VP), ("X21", _VP), ("B", _I64), ("H", _I64), ("W", _I64), ("rays_img", _VP), ("pts_norm", _VP),
    ]


# symbol -> (restype, argtypes): include/m3s_fuse.h
_SIGNATURES = {
    "m3s_fuse_pointmap": (_INT, [_P(FuseArgs), _VP]),
    "m3s_prep_rays": (_INT, [_P(PrepRaysArgs), _VP]),
}


def fuse_pointmap(X_canon, C, X_new, C_new, T=None, mode="weighted_pointmap"):
    """Keyframe pointmap fusion after tracking, in place (new entry point):
    X_canon/C <- filter(X_canon, C, T.act(X_new), C_new) — tracker.py:98-99 +
    Frame.update_pointmap (frame.py:41-100) for an initialised keyframe.
    X_canon, X_new [HW,3] f32; C, C_new [HW,1] (or [HW]) f32; T [8] or [1,8]."""
    for name, t in (("X_canon", X_canon), ("C", C), ("X_new", X_new), ("C_new", C_new)):
        _check(t, name, torch.float32)
    if mode not in FILTER_MODES:
        raise RuntimeError(f"fuse_pointmap: unsupported filtering mode {mode!r}")
    HW = int(X_canon.shape[0])
    if X_canon.numel() != 3 * HW or X_new.numel() != 3 * HW or C.numel() != HW or C_new.numel() != HW:
        raise RuntimeError("fuse_pointmap: expected X [HW,3] and C [HW,1]")
    if T is not None:
        T = T.contiguous()
        _check(T, "T", torch.float32)
    a = FuseArgs()
    a.X_canon, a.C, a.X_new, a.C_new, a.T = _p(X_canon), _p(C), _p(X_new), _p(C_new), _p(T)
    a.HW, a.mode = HW, FILTER_MODES[mode]
    _call("m3s_fuse_pointmap", ctypes.byref(a), _stream(X_canon.device))


def prep_rays(X11, X21):
    """iter_proj inputs in one pass (new entry point; prep_for_iter_proj,
    matching.py:25-49): X11 [B,H,W,3], X21 [B,H,W,3] (or [B,HW,3]) f32 ->
    (rays_with_grad [B,H,W,9], pts3d_norm [B,HW,3])."""
    _check(X11, "X11", torch.float32)
    _check(X21, "X21", torch.float32)
    B, H, W, _ = X11.shape
    if X21.numel() != B * H * W * 3:
        raise RuntimeError("prep_rays: X21 must hold B*H*W points")
    dev = X11.device
    rays = torch.empty(B, H, W, 9, dtype=torch.float32, device=dev)
    pts = torch.empty(B, H * W, 3, dtype=torch.float32, device=dev)
    a = PrepRaysArgs()
    a.X11, a.X21, a.B, a.H, a.W, a.rays_img, a.pts_norm = _p(X11), _p(X21), B, H, W, _p(rays), _p(pts)
    _call("m3s_prep_rays", ctypes.byref(a), _stream(dev))
    return rays, pts

"""include/m3s_match.h: the reference's two matching kernels, and ``match_dense``."""
import ctypes

import torch

from ._abi import _F32, _I64, _INT, _P, _SIZE, _VP, _call, _check, _p, _same_device, _stream, _sym, _workspace


class IterProjArgs(ctypes.Structure):
    """Mirror of ``m3s_iter_proj_args`` (include/m3s_match.h)."""

    _fields_ = [
        ("rays_img", _VP), ("pts_3d_norm", _VP), ("p_init", _VP), ("B", _I64), ("H", _I64), ("W", _I64), ("N", _I64),
        ("max_iter", _INT), ("lambda_init", _F32), ("cost_thresh", _F32), ("p_new", _VP), ("converged", _VP),
    ]


class RefineArgs(ctypes.Structure):
    """Mirror of ``m3s_refine_args`` (include/m3s_match.h)."""

    _fields_ = [
        ("D11", _VP), ("D21", _VP), ("p1", _VP), ("B", _I64), ("H", _I64), ("W", _I64), ("N", _I64), ("F", _I64),
        ("dtype", _INT), ("radius", _INT), ("dilation_max", _INT), ("p1_new", _VP),
    ]


class MatchDenseArgs(ctypes.Structure):
    """Mirror of ``m3s_match_dense_args`` (include/m3s_match.h)."""

    _fields_ = [
        ("X11", _VP), ("X21", _VP), ("D11", _VP), ("D21", _VP), ("Q11", _VP), ("Q21", _VP), ("idx_init", _VP),
        ("B", _I64), ("H", _I64), ("W", _I64), ("F", _I64), ("dtype", _INT), ("max_iter", _INT), ("lambda_init", _F32),
        ("cost_thresh", _F32), ("dist_thresh", _F32), ("radius", _INT), ("dilation_max", _INT), ("Q_conf", _F32),
        ("idx", _VP), ("valid", _VP), ("Q", _VP), ("idx_stride", _I64), ("valid_stride", _I64), ("Q_stride", _I64),
        ("n_valid", _VP), ("workspace", _VP), ("workspace_bytes", _SIZE),
    ]


# symbol -> (restype, argtypes): include/m3s_match.h
_SIGNATURES = {
    "m3s_iter_proj": (_INT, [_P(IterProjArgs), _VP]),
    "m3s_refine_matches": (_INT, [_P(RefineArgs), _VP]),
    "m3s_match_dense_workspace_size": (_SIZE, [_I64] * 3),
    "m3s_match_dense": (_INT, [_P(MatchDenseArgs), _VP]),
}


def iter_proj(rays_img_with_grad, pts_3d_norm, p_init, max_iter, lambda_init, cost_thresh):
    """gn.cpp:84-99 / matching_kernels.cu:119-296: per-pixel LM projection.

    rays_img_with_grad [B,H,W,9] f32, pts_3d_norm [B,N,3] f32, p_init [B,N,2]
    f32 -> [p_new [B,N,2] f32, converged [B,N] bool] (new tensors)."""
    for name, t in (("rays_img_with_grad", rays_img_with_grad), ("pts_3d_norm", pts_3d_norm),
                    ("p_init", p_init)):
        _check(t, name, torch.float32)
    B, H, W, C = rays_img_with_grad.shape
    Bn, N = int(p_init.shape[0]), int(p_init.shape[1])
    if C != 9 or Bn != B or tuple(pts_3d_norm.shape) != (B, N, 3) or tuple(p_init.shape) != (B, N, 2):
        raise RuntimeError("iter_proj: expected rays [B,H,W,9], pts_3d_norm [B,N,3], p_init [B,N,2]")
    dev = p_init.device
    p_new = torch.zeros(B, N, 2, dtype=torch.float32, device=dev)
    converged = torch.zeros(B, N, dtype=torch.bool, device=dev)
    a = IterProjArgs()
    a.rays_img, a.pts_3d_norm, a.p_init = _p(rays_img_with_grad), _p(pts_3d_norm), _p(p_init)
    a.B, a.H, a.W, a.N = B, H, W, N
    a.max_iter, a.lambda_init, a.cost_thresh = int(max_iter), float(lambda_init), float(cost_thresh)
    a.p_new, a.converged = _p(p_new), _p(converged)
    _call("m3s_iter_proj", ctypes.byref(a), _stream(dev))
    return [p_new, converged]


def refine_matches(D11, D21, p1, radius, dilation_max):
    """gn.cpp:101-114 / matching_kernels.cu:25-116: dilated local search.

    D11 [B,H,W,F] f16 (or f32), D21 [B,N,F] same dtype, p1 [B,N,2] int64 (u, v)
    -> [p1_new [B,N,2] int64] (new tensor)."""
    _check(D11, "D11")
    _check(D21, "D21", D11.dtype)
    _check(p1, "p1", torch.int64)
    dt = {torch.float16: 0, torch.float32: 1}.get(D11.dtype)
    if dt is None:
        raise RuntimeError(f"refine_matches: descriptors must be float16 or float32 (got {D11.dtype})")
    B, H, W, F = D11.shape
    N = int(p1.shape[1])
    if tuple(D21.shape) != (B, N, F) or tuple(p1.shape) != (B, N, 2):
        raise RuntimeError("refine_matches: expected D11 [B,H,W,F], D21 [B,N,F], p1 [B,N,2]")
    p1_new = torch.zeros(B, N, 2, dtype=torch.int64, device=p1.device)
    a = RefineArgs()
    a.D11, a.D21, a.p1 = _p(D11), _p(D21), _p(p1)
    a.B, a.H, a.W, a.N, a.F = B, H, W, N, F
    a.dtype, a.radius, a.dilation_max = dt, int(radius), int(dilation_max)
    a.p1_new = _p(p1_new)
    _call("m3s_refine_matches", ctypes.byref(a), _stream(p1.device))
    return [p1_new]


def _rows(t, name, dtype, B, HW):
    """Row stride (elements) of an output of match_dense: [B, HW(, 1)], the
    pixels of a row contiguous, the rows anywhere (every other row of an edge
    store is fine)."""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{name} must be a tensor on a ROCm device; no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype} (got {t.dtype})")
    if t.dim() == 3 and t.shape[2] == 1:
        t = t[:, :, 0]
    if t.dim() != 2 or t.shape[0] != B or t.shape[1] != HW:
        raise RuntimeError(f"{name} must be [{B}, {HW}(, 1)] (got {tuple(t.shape)})")
    if HW > 1 and t.stride(1) != 1:
        raise RuntimeError(f"{name}: the pixels of a row must be contiguous")
    stride = t.stride(0) if B > 1 else HW
    if stride < HW:
        raise RuntimeError(f"{name}: rows overlap (stride {stride} < {HW})")
    return stride


def match_dense_workspace_size(B, H, W):
    """Bytes of the match_dense workspace for B pairs of H x W views."""
    return int(_sym("m3s_match_dense_workspace_size")(int(B), int(H), int(W)))


def _match_dense(X11, X21, D11, D21, Q11, Q21, idx_init, max_iter, lambda_init, cost_thresh,
                 dist_thresh, radius, dilation_max, Q_conf, out):
    """m3s_match_dense on checked tensors; descriptors float16 or float32 as given."""
    _check(X11, "X11", torch.float32)
    _check(X21, "X21", torch.float32)
    _check(D11, "D11", (torch.float16, torch.float32))
    _check(D21, "D21", D11.dtype)
    _check(Q11, "Q11", torch.float32)
    _check(Q21, "Q21", torch.float32)
    if X11.dim() != 4 or X11.shape[3] != 3:
        raise RuntimeError("match_dense: X11 must be [B,H,W,3]")
    B, H, W, _ = (int(x) for x in X11.shape)
    HW = H * W
    F = int(D11.shape[-1])
    if X21.numel() != B * HW * 3 or X21.shape[0] != B or X21.shape[-1] != 3:
        raise RuntimeError("match_dense: X21 must be [B,H,W,3] or [B,HW,3]")
    if tuple(D11.shape) != (B, H, W, F) or D21.numel() != B * HW * F or D21.shape[0] != B or D21.shape[-1] != F:
        raise RuntimeError("match_dense: expected D11 [B,H,W,F] and D21 [B,HW,F]")
    for name, q in (("Q11", Q11), ("Q21", Q21)):
        if q.numel() != B * HW or q.shape[0] != B:
            raise RuntimeError(f"match_dense: {name} must be [B,HW] (or [B,H,W], [B,HW,1])")
    dev = X11.device
    _same_device("match_dense", (("X21", X21), ("D11", D11), ("D21", D21), ("Q11", Q11), ("Q21", Q21)), "X11", dev)
    if idx_init is not None:
        _check(idx_init, "idx_init", torch.int64)
        if tuple(idx_init.shape) != (B, HW) or idx_init.device != dev:
            raise RuntimeError("match_dense: idx_init must be [B,HW] int64 on the inputs' device")
    n_valid = None
    if out is None:
        idx = torch.empty(B, HW, dtype=torch.int32, device=dev)
        valid = torch.empty(B, HW, 1, dtype=torch.bool, device=dev)
        Q = torch.empty(B, HW, 1, dtype=torch.float32, device=dev)
    else:
        idx, valid, Q = out[:3]
        n_valid = out[3] if len(out) > 3 else None
    strides = [_rows(t, name, dt, B, HW) for t, name, dt in
               ((idx, "out idx", torch.int32), (valid, "out valid", torch.bool), (Q, "out Q", torch.float32))]
    if any(t.device != dev for t in (idx, valid, Q)):
        raise RuntimeError("match_dense: out tensors must be on the inputs' device")
    if n_valid is None:
        n_valid = torch.empty(B, dtype=torch.int32, device=dev)
    else:
        _check(n_valid, "out n_valid", torch.int32)
        if n_valid.numel() != B or n_valid.device != dev:
            raise RuntimeError("match_dense: out n_valid must be [B] int32 on the inputs' device")
    ws = _workspace(match_dense_workspace_size(B, H, W), dev)
    a = MatchDenseArgs()
    a.X11, a.X21, a.D11, a.D21, a.Q11, a.Q21 = _p(X11), _p(X21), _p(D11), _p(D21), _p(Q11), _p(Q21)
    a.idx_init = _p(idx_init)
    a.B, a.H, a.W, a.F = B, H, W, F
    a.dtype = 0 if D11.dtype == torch.float16 else 1
    a.max_iter, a.lambda_init, a.cost_thresh = int(max_iter), float(lambda_init), float(cost_thresh)
    a.dist_thresh, a.radius, a.dilation_max = float(dist_thresh), int(radius), int(dilation_max)
    a.Q_conf = float(Q_conf)
    a.idx, a.valid, a.Q = _p(idx), _p(valid), _p(Q)
    a.idx_stride, a.valid_stride, a.Q_stride = strides
    a.n_valid = _p(n_valid)
    a.workspace, a.workspace_bytes = _p(ws), ws.numel()
    _call("m3s_match_dense", ctypes.byref(a), _stream(dev))
    del ws  # stream-ordered by the caching allocator
    return idx, valid, Q, n_valid


def match_dense(X11, X21, D11, D21, Q11, Q21, idx_init=None, *, max_iter=10, lambda_init=1e-8,
                convergence_thresh=1e-6, dist_thresh=1e-1, radius=3, dilation_max=5, Q_conf=1.5,
                out=None):
    """Dense matching to GN-ready rows in three launches (new entry point;
    m3s_match_dense): matching.py:52-90, then Q = sqrt(Q11[b, idx] * Q21)
    (global_opt.py:53-57, tracker.py:41) and the per-pair count of
    valid & (Q > Q_conf) (global_opt.py:59-66).

    X11 [B,H,W,3], X21 [B,H,W,3] (or [B,HW,3]) f32; D11 [B,H,W,F], D21
    [B,H,W,F] (or [B,HW,F]), cast with .half() when not float16 like the
    reference's caller (matching.py:80); Q11, Q21 [B,HW] f32 (or [B,H,W],
    [B,HW,1]); idx_init [B,HW] int64 or None (the reference's
    idx_1_to_2_init). The keyword defaults are base.yaml's matching section
    and local_opt.Q_conf.

    -> (idx int32 [B,HW], valid bool [B,HW,1], Q f32 [B,HW,1], n_valid int32
    [B]). out=(idx, valid, Q[, n_valid]) writes into the caller's tensors
    instead: their rows may be strided views (rows r0:r1:2 of an EdgeStore),
    the pixels of a row contiguous. No host synchronisation."""
    D11 = D11 if D11.dtype == torch.float16 else D11.half()
    D21 = D21 if D21.dtype == torch.float16 else D21.half()
    return _match_dense(X11, X21, D11, D21, Q11, Q21, idx_init, max_iter, lambda_init,
                        convergence_thresh, dist_thresh, radius, dilation_max, Q_conf, out)

"""What the per-header modules share: the one way to the loaded library, the
return codes, pointer / stream helpers and the checks several entry points make."""
import ctypes
import sys

import torch

M3S_OK, M3S_EINVAL, M3S_ELAUNCH, M3S_ETOOLARGE = 0, 1, 2, 3
# the C types of the mirrors and the signature tables
_VP, _SIZE, _P = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER
_INT, _I32, _I64, _F32, _F64 = ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double


def _sym(symbol):
    """``symbol`` of the library the package holds now: ``be._lib = ...`` (the
    test build, a variant) redirects every wrapper from then on."""
    return getattr(sys.modules[__package__]._lib, symbol)


def _call(symbol, *args):
    """Call an entry point that returns an M3S_* code; raise unless M3S_OK."""
    _raise(_sym(symbol)(*args), symbol)


def _raise(rc, fn):
    if rc == M3S_OK:
        return
    msg = {M3S_EINVAL: "invalid argument", M3S_ELAUNCH: "HIP launch failed",
           M3S_ETOOLARGE: "problem size exceeds this build's limits"}.get(rc, f"error {rc}")
    raise RuntimeError(f"{fn}: {msg}")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------ checks --
def _on_rocm(t, name):
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} must be on a ROCm device (got {t.device}); no CPU path")


def _check(t: torch.Tensor, name: str, dtype=None):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    _on_rocm(t, name)
    if dtype is not None and t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
        raise RuntimeError(f"{name} must be {dtype} (got {t.dtype})")


def _same_device(fn, items, ref, dev, rocm=False):
    """Every tensor of ``items`` ((name, tensor or None), ...) is on ``dev``, the device
    of the input called ``ref``; rocm=True: and on a ROCm device, asked of each first."""
    for name, t in items:
        if rocm and t is not None:
            _on_rocm(t, name)
        if t is not None and t.device != dev:
            raise RuntimeError(f"{fn}: {name} is on {t.device}, {ref} on {dev}")


def _layout(symbol, sections, *dims):
    """{section: byte offset} as the layout entry point ``symbol`` reports it."""
    offs = (ctypes.c_size_t * len(sections))()
    _sym(symbol)(*(int(d) for d in dims), offs)
    return dict(zip(sections, list(offs)))


def _caller_workspace(workspace, need, dev, what):
    """A fresh workspace, or the caller's own (tests: reused / poisoned ones) once it is seen to hold ``need`` bytes."""
    if workspace is None:
        return _workspace(need, dev)
    _check(workspace, "workspace", torch.uint8)
    if workspace.device != dev or workspace.numel() < need:
        raise RuntimeError(f"{what} workspace must be a uint8 tensor of >= {need} bytes on {dev}")
    return workspace


def _head_rows(t, name, H, D):
    if t.numel() and (t.stride(3) != 1 or (H > 1 and t.stride(2) != D)):
        raise RuntimeError(f"{name}: a head row must be contiguous and the heads of a token back to back "
                           "(stride(3) == 1, stride(2) == D)")


def _positions(t, name, B, N):
    if t.dtype != torch.int64:
        raise RuntimeError(f"{name} must be {torch.int64} (got {t.dtype})")
    if tuple(t.shape) != (B, N, 2):
        raise RuntimeError(f"{name} must be [{B}, {N}, 2] (got {tuple(t.shape)})")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _token_strides(t, N, row):
    """(batch, token) element strides of a [B, N, H, D] view (or of [B, N, row]);
    the stride of a dimension of size 1 is arbitrary: give it the dense value."""
    sn = t.stride(1) if N > 1 else row
    sb = t.stride(0) if t.shape[0] > 1 else (N - 1) * sn + row
    return sb, sn

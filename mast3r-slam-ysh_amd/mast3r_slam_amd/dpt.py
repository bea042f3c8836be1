"""The last four modules of MASt3R's DPT head on the device kernel
(mast3r_slam_backends.dpt_tail), and ``install`` to put it into a loaded MASt3R
model:

    from mast3r_slam_amd import dpt
    dpt.install(model)

The DPT regression head ends in (croco models/dpt_block.py:318-324)

    Conv2d(256 -> 128, 3x3), Interpolate(2, 'bilinear', align_corners=True),
    Conv2d(128 -> 128, 3x3, padding 1), ReLU, Conv2d(128 -> 4, 1x1)

run as ``self.head(path_1)``. In torch the upsampled [B,128,H,W] tensor is
written and read, then the 3x3 convolution's output is written, read and
rewritten by the ReLU and read again by the 1x1 convolution. Here the first
convolution runs as before and the other four modules are one launch that
reads its [B,128,H/2,W/2] output and writes the [B,4,H,W] map
``head_postprocess`` takes.

The kernel is fp32, 128 channels, 1..4 outputs, forward only. Whenever it does
not apply the Sequential's original ``forward`` runs unchanged.
"""
from __future__ import annotations

import types

import torch

import mast3r_slam_backends as be

_ADAPTER_ATTRS = ("head", "scratch", "act_postprocess", "hooks")  # croco's DPTOutputAdapter


def _conv(m, cin, cout, k):
    """Whether ``m`` is a plain Conv2d(cin -> cout in `cout`, k x k, stride 1, padding k // 2) with a bias."""
    return (type(m).__name__ == "Conv2d" and isinstance(m, torch.nn.Conv2d) and m.in_channels == cin
            and m.out_channels in cout and tuple(m.kernel_size) == (k, k) and tuple(m.stride) == (1, 1)
            and tuple(m.padding) == (k // 2, k // 2) and tuple(m.dilation) == (1, 1) and m.groups == 1
            and m.bias is not None and m.padding_mode == "zeros")


def supported(seq) -> bool:
    """Whether ``seq`` is the regression head's Sequential in the shape the kernel computes:
    [Conv2d, Interpolate(scale_factor 2, 'bilinear', align_corners True), Conv2d(128 -> 128, 3x3,
    stride 1, padding 1, dilation 1, groups 1, bias), ReLU, Conv2d(128 -> 1..4, 1x1, bias)]."""
    if not isinstance(seq, torch.nn.Sequential) or len(seq) != 5:
        return False
    first, up, conv3, relu, conv1 = seq
    if type(first).__name__ != "Conv2d" or type(up).__name__ != "Interpolate" or type(relu).__name__ != "ReLU":
        return False
    try:
        scale = getattr(up, "scale_factor", None)
        if isinstance(scale, (tuple, list)):
            scale_ok = len(scale) == 2 and all(float(s) == 2.0 for s in scale)
        else:
            scale_ok = float(scale) == 2.0
    except (TypeError, ValueError):
        return False
    if not scale_ok or getattr(up, "mode", None) != "bilinear" or getattr(up, "align_corners", None) is not True:
        return False
    return (_conv(conv3, be.DPT_CH, (be.DPT_CH,), 3)
            and _conv(conv1, be.DPT_CH, range(1, be.DPT_MAX_COUT + 1), 1))


def _packed(seq):
    """The packed weights of ``seq``, cached on it; repacked when one of the four
    parameters was replaced or written (load_state_dict, an optimizer step)."""
    params = (seq[2].weight, seq[2].bias, seq[4].weight, seq[4].bias)
    key = tuple((p.data_ptr(), p._version) for p in params)
    cache = vars(seq).get("_m3s_dpt_packed")
    if cache is None or cache[0] != key:
        cache = (key, be.dpt_tail_pack(*(p.detach() for p in params)))
        seq._m3s_dpt_packed = cache
    return cache[1]


def _applies(seq, x):
    """Whether the kernel computes what the original forward would: the shape
    still the supported one, its input on a GPU, fp32 (no autocast), NCHW
    contiguous, nothing to differentiate."""
    if not supported(seq) or not isinstance(x, torch.Tensor) or x.dim() != 4:
        return False
    params = [p for m in (seq[0], seq[2], seq[4]) for p in (m.weight, m.bias)]
    if x.device.type != "cuda" or x.dtype != torch.float32 or torch.is_autocast_enabled():
        return False
    if any(p.dtype != torch.float32 or p.device != x.device or not p.is_contiguous() for p in params):
        return False
    if not x.is_contiguous():
        return False
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
        return False  # no backward
    return True


def fused_dpt_head_forward(seq, x):
    """The regression head's Sequential with its last four modules on the device kernel."""
    original = vars(seq).get("_m3s_original_forward") or type(seq).forward.__get__(seq)
    if not _applies(seq, x):
        return original(x)
    y = seq[0](x)
    if y.dtype != torch.float32 or not y.is_contiguous():
        return seq[4](seq[3](seq[2](seq[1](y))))
    return be.dpt_tail(y, _packed(seq), seq[4].out_channels)


def install(model) -> int:
    """Put the ``head`` of every submodule that has the DPT adapter's attributes
    (``head``, ``scratch``, ``act_postprocess``, ``hooks``) on the fused path,
    when it is an ``nn.Sequential`` of exactly the shape ``supported`` names:
    ``forward`` is overridden on the instance, as ``attention.install`` does,
    so ``self.head(path_1)`` reaches the kernel whoever calls the adapter
    (``head.install`` or the reference's own head forward; the two installs
    compose in either order). The new forward runs ``seq[0]`` as before and
    calls the original forward unchanged when the input is not on a GPU, not
    fp32 (or under autocast), not NCHW-contiguous, something would need a
    gradient, or the Sequential no longer has that shape. The packed weights
    are cached on the Sequential and follow its parameters. Returns the number
    of Sequentials patched; those already patched are left alone."""
    count = 0
    for module in list(model.modules()):
        if not all(hasattr(module, a) for a in _ADAPTER_ATTRS):
            continue
        seq = module.head
        if not supported(seq) or "_m3s_original_forward" in vars(seq):
            continue
        seq._m3s_original_forward = seq.forward  # the bound original
        seq.forward = types.MethodType(fused_dpt_head_forward, seq)
        count += 1
    return count

"""The tail of MASt3R's catmlp+dpt head on the device kernel
(mast3r_slam_backends.head_postprocess), and ``install`` to put it into a loaded
MASt3R model:

    from mast3r_slam_amd import head
    head.install(model)                              # res['desc'] stays float32
    head.install(model, desc_dtype=torch.float16)    # match_dense's dtype: no cast later

The network part of Cat_MLP_LocalFeatures_DPT_Pts3d.forward (the DPT and the
local-feature MLP) stays torch. What follows it in the reference
(catmlp_dpt_head.py:83-95: pixel_shuffle, cat, permute, then per output a handful
of element-wise ops over channel-strided views) is one launch here, and
``decode_pair_into`` writes a view straight into its slot of the stacked,
downsampled X / C / D / Q buffers the SLAM side builds with zip / stack /
downsample (mast3r_utils.py:73-79).
"""
from __future__ import annotations

import math
import types

import torch

import mast3r_slam_backends as be

_HEAD_ATTRS = ("dpt", "head_local_features", "patch_size", "local_feat_dim", "two_confs", "depth_mode",
               "conf_mode", "desc_conf_mode", "desc_mode")


def _exp_mode(mode):
    """(vmin, vmax) of an ('exp', vmin, vmax) confidence mode with a finite vmin, else None."""
    try:
        kind, vmin, vmax = mode
        vmin, vmax = float(vmin), float(vmax)
    except (TypeError, ValueError):
        return None
    return (vmin, vmax) if kind == "exp" and math.isfinite(vmin) and vmax >= vmin else None


def supported(head) -> bool:
    """Whether ``head`` is a catmlp+dpt head in the modes the kernel computes:
    depth ('exp', -inf, inf), 'exp' confidences, two_confs, desc 'norm', and a
    postprocess to replace."""
    if not all(hasattr(head, a) for a in _HEAD_ATTRS) or not getattr(head, "postprocess", None):
        return False
    try:
        depth_ok = tuple(head.depth_mode) == ("exp", -math.inf, math.inf)
    except TypeError:
        return False
    desc_conf_mode = head.desc_conf_mode if head.desc_conf_mode is not None else head.conf_mode
    return (depth_ok and bool(head.two_confs) and isinstance(head.desc_mode, str) and "norm" in head.desc_mode
            and _exp_mode(head.conf_mode) is not None and _exp_mode(desc_conf_mode) is not None)


def _raw(head, decout, img_shape):
    """The network part: (pts [B,4,H,W], feat [B,S,(F+1)*P*P]) as the kernel reads them."""
    H, W = int(img_shape[0]), int(img_shape[1])
    pts = head.dpt(decout, image_size=(H, W))
    feat = head.head_local_features(torch.cat([decout[0], decout[-1]], dim=-1))
    return pts.float().contiguous(), feat.float().contiguous()


def _modes(head):
    if not supported(head):
        raise RuntimeError("fused_head_forward: not a catmlp+dpt head in the 'exp' / two_confs / 'norm' modes")
    desc_conf_mode = head.desc_conf_mode if head.desc_conf_mode is not None else head.conf_mode
    return dict(conf=_exp_mode(head.conf_mode), desc_conf=_exp_mode(desc_conf_mode))


def fused_head_forward(head, decout, img_shape, **kw):
    """Cat_MLP_LocalFeatures_DPT_Pts3d.forward with its tail on the device
    kernel; -> the reference's dict: pts3d [B,H,W,3], conf [B,H,W], desc
    [B,H,W,F], desc_conf [B,H,W]. ``kw`` goes to be.head_postprocess
    (desc_dtype, downsample, out, generic)."""
    pts, feat = _raw(head, decout, img_shape)
    X, C, D, Q = be.head_postprocess(pts, feat, int(head.patch_size), int(head.local_feat_dim), **_modes(head), **kw)
    return dict(pts3d=X, conf=C, desc=D, desc_conf=Q)


def install(model, desc_dtype=torch.float32) -> int:
    """Put ``model.downstream_head1`` / ``downstream_head2`` on the fused path.
    The model's head1 / head2 are functools.partial objects that captured these
    very modules, so the modules themselves are switched: ``forward`` is
    overridden on the instance. A head whose modes the kernel does not compute,
    or without a postprocess, is left untouched. Returns the number of heads
    switched; a head already switched is not counted again (and keeps its
    desc_dtype). desc_dtype=torch.float16 is opt-in: it saves match_dense's cast
    but changes the dtype of res['desc']."""
    count = 0
    for name in ("downstream_head1", "downstream_head2"):
        head = getattr(model, name, None)
        if head is None or "_m3s_fused" in vars(head) or not supported(head):
            continue

        def forward(self, decout, img_shape, _dtype=desc_dtype):
            return fused_head_forward(self, decout, img_shape, desc_dtype=_dtype)

        head.forward = types.MethodType(forward, head)
        head._m3s_fused = True
        count += 1
    return count


def alloc_views(n_views, batch, img_shape, desc_dim, device, downsample=1, desc_dtype=torch.float16):
    """Stacked (X [n,b,h,w,3], C [n,b,h,w], D [n,b,h,w,F], Q [n,b,h,w]) buffers
    for ``decode_pair_into``: n is 2 for a tracked frame and 4 for a new edge."""
    h, w = -(-int(img_shape[0]) // downsample), -(-int(img_shape[1]) // downsample)
    lead = (int(n_views), int(batch), h, w)
    return (torch.empty(*lead, 3, dtype=torch.float32, device=device),
            torch.empty(lead, dtype=torch.float32, device=device),
            torch.empty(*lead, int(desc_dim), dtype=desc_dtype, device=device),
            torch.empty(lead, dtype=torch.float32, device=device))


def decode_pair_into(bufs, k, head, decout, img_shape, downsample=1):
    """One decoded view into slot ``k`` of the stacked (X, C, D, Q) buffers
    (``alloc_views``): what the reference does with zip / torch.stack / downsample
    (mast3r_utils.py:73-79), and, when D is float16, match_dense's cast as well.
    Returns the four slot views."""
    pts, feat = _raw(head, decout, img_shape)
    out = tuple(buf[k] for buf in bufs)
    return be.head_postprocess(pts, feat, int(head.patch_size), int(head.local_feat_dim), **_modes(head),
                               downsample=downsample, desc_dtype=out[2].dtype, out=out)

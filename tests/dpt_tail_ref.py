"""This project's own statement of the DPT tail that m3s_dpt_tail computes
(include/m3s_dpt.h), for the tests and the timing tool.

    u   = bilinear x2 upsampling of x, align_corners, with the header's fp32 lambdas
    mid = relu(conv3x3(u, w1, b1, zero padding 1))
    out = conv1x1(mid, w2, b2)

lambdas        the header's source indices and fp32 lambdas of one axis.
upsample_f32   u in torch fp32, op by op as the header writes it (every product
               and sum rounded): the kernel's u, bitwise.
dpt_tail_exact takes those fp32 lambdas and evaluates everything else in fp64.
dpt_tail_torch is the reference's four modules as torch runs them.
bound          is the derived per-element tolerance of an fp32 evaluation.
load_weights / load_fixture read tests/golden/dpt_tail_w.npz and
               dpt_tail_{a..e}.npz (make_dpt_tail_golden.py).
Interpolate, DPTOutputAdapter, make_head_seq are stand-ins with the reference's
class and attribute names (croco models/dpt_block.py), for dpt.install.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24  # unit roundoff of fp32
C = 128
K1 = 9 * C  # terms of the 3x3 convolution


def lambdas(n_in, device="cpu"):
    """(i0, i1 int64 [2 n_in], l0, l1 fp32 [2 n_in]) of one axis, as m3s_dpt.h states them."""
    n_out = 2 * n_in
    ratio = np.float32(n_in - 1) / np.float32(n_out - 1)  # one fp32 division
    r = ratio * np.arange(n_out, dtype=np.float32)  # one fp32 product
    i0 = r.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = r - i0.astype(np.float32)
    l0 = np.float32(1.0) - l1
    assert r.dtype == l0.dtype == l1.dtype == np.float32 and i1.max() <= n_in - 1
    return tuple(torch.from_numpy(t).to(device) for t in (i0, i1, l0, l1))


def _corners(x, dtype):
    """The four source values and the lambdas of every output pixel, in `dtype`."""
    Hi, Wi = x.shape[2], x.shape[3]
    y0, y1, lh0, lh1 = lambdas(Hi, x.device)
    x0, x1, lw0, lw1 = lambdas(Wi, x.device)
    x = x.to(dtype)
    top, bot = x[:, :, y0], x[:, :, y1]
    lam = tuple(t.to(dtype) for t in (lh0[:, None], lh1[:, None], lw0[None, :], lw1[None, :]))
    return (top[..., x0], top[..., x1], bot[..., x0], bot[..., x1]), lam


def upsample_f32(x):
    """u [B,C,2Hi,2Wi] in fp32, each of the header's 7 operations one rounded torch op."""
    assert x.dtype == torch.float32
    (v00, v01, v10, v11), (lh0, lh1, lw0, lw1) = _corners(x, torch.float32)
    a, b, c, d = lw0 * v00, lw1 * v01, lw0 * v10, lw1 * v11
    top, bot = a + b, c + d
    t, s = lh0 * top, lh1 * bot
    return t + s


def upsample_exact(x, absolute=False):
    """u in fp64 from the fp32 lambdas; absolute=True: the same sum over |x| (the lambdas are >= 0)."""
    (v00, v01, v10, v11), (lh0, lh1, lw0, lw1) = _corners(x.abs() if absolute else x, torch.float64)
    return lh0 * (lw0 * v00 + lw1 * v01) + lh1 * (lw0 * v10 + lw1 * v11)


def conv3x3(u, w, b):
    """F.conv2d(u, w, b, padding=1) as nine shifted channel products: plain matrix
    products in u's dtype on any device (fp64 included), no convolution library."""
    H, W = u.shape[2:]
    p = F.pad(u, (1, 1, 1, 1))
    out = sum(torch.einsum("oc,bchw->bohw", w[:, :, dy, dx], p[:, :, dy:dy + H, dx:dx + W])
              for dy in range(3) for dx in range(3))
    return out if b is None else out + b[None, :, None, None]


def conv1x1(m, w, b):
    out = torch.einsum("oc,bchw->bohw", w[:, :, 0, 0], m)
    return out if b is None else out + b[None, :, None, None]


def _w64(w1, b1, w2, b2):
    w2 = w2.reshape(w2.shape[0], C, 1, 1)
    return tuple(t.to(torch.float64) for t in (w1, b1, w2, b2))


def dpt_tail_exact(x, w1, b1, w2, b2):
    """The header's function with its fp32 lambdas, everything else in fp64; -> fp64 [B,Cout,2Hi,2Wi]."""
    w1, b1, w2, b2 = _w64(w1, b1, w2, b2)
    return conv1x1(F.relu(conv3x3(upsample_exact(x), w1, b1)), w2, b2)


def dpt_tail_torch(x, w1, b1, w2, b2):
    """The reference's four modules as torch runs them, in x's dtype."""
    u = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    return F.conv2d(F.relu(F.conv2d(u, w1, b1, padding=1)), w2.reshape(w2.shape[0], C, 1, 1), b2)


def bound(x, w1, b1, w2, b2):
    """Per-element tolerance |fp32 evaluation - dpt_tail_exact| of any evaluation
    that interpolates with the header's fp32 lambdas and rounds each of its 7
    operations, and forms each of the two convolutions as an fp32 sum of
    products in any order (rounded products or fmaf, MFMA included); fp64
    [B,Cout,2Hi,2Wi]. Derived, not measured; eps = 2^-24. First order in eps
    throughout; the second-order terms are covered by the final factor 1.01
    (every relative error here is below 1153 * 7 eps < 5e-4).

    1. interpolation. The lambdas are inputs here (the header's fp32 values, all
    >= 0), so u is a sum of four products lh lw v. Its evaluation makes 7
    roundings, each relative eps on a partial result that is bounded by U, the
    same expression over |v|: |du| <= 7 eps U. (Four of them lie on the path of
    any one term, so this is not tight; it is the count the operations give
    without looking at their nesting.)

    2. the 3x3 convolution. pre = b1 + sum of K1 = 1152 products w1 u^. Its
    terms move by |w1| |du|; a sum of n + 1 terms in any order makes at most n
    additions on the path of a term and one rounding per product (none for
    fmaf), each relative eps on a partial sum bounded by the absolute sum:
    |dpre| <= sum |w1| |du| + (K1 + 1) eps (|b1| + sum |w1| |u|), where |u| <= U.

    3. ReLU is 1-Lipschitz: |dmid| <= |dpre|.

    4. the 1x1 convolution, likewise with 128 + 1 terms:
    |dout| <= sum |w2| |dmid| + (128 + 1) eps (|b2| + sum |w2| mid)."""
    w1, b1, w2, b2 = _w64(w1, b1, w2, b2)
    U = upsample_exact(x, absolute=True)
    a1 = conv3x3(U, w1.abs(), b1.abs())  # |b1| + sum |w1| U
    dpre = 7.0 * EPS32 * (a1 - b1.abs()[None, :, None, None]) + (K1 + 1) * EPS32 * a1
    mid = F.relu(conv3x3(upsample_exact(x), w1, b1))
    dout = conv1x1(dpre, w2.abs(), None) + (C + 1) * EPS32 * conv1x1(mid, w2.abs(), b2.abs())
    return 1.01 * dout


def fraction(got, x, w1, b1, w2, b2):
    """max over the elements of |got - exact| / bound."""
    err = (got.to(torch.float64) - dpt_tail_exact(x, w1, b1, w2, b2)).abs()
    return float((err / bound(x, w1, b1, w2, b2)).max())


def load_weights(golden_dir, device="cpu"):
    """-> (w1 [128,128,3,3], b1 [128], w2 [4,128,1,1], b2 [4]) of every fixture."""
    z = np.load(os.path.join(golden_dir, "dpt_tail_w.npz"))
    return tuple(torch.from_numpy(z[n]).to(device) for n in ("w1", "b1", "w2", "b2"))


def load_fixture(golden_dir, name, device="cpu"):
    """-> dict(x, cout, out, w = (w1, b1, w2[:cout], b2[:cout]))."""
    z = np.load(os.path.join(golden_dir, f"dpt_tail_{name}.npz"))
    cout = int(z["cout"])
    w1, b1, w2, b2 = load_weights(golden_dir, device)
    return dict(x=torch.from_numpy(z["x"]).to(device), cout=cout, out=torch.from_numpy(z["out"]).to(device),
                w=(w1, b1, w2[:cout].contiguous(), b2[:cout].contiguous()))


FIXTURES = ("a", "b", "c", "d", "e")


# ---- stand-ins with the reference's class and attribute names
class Interpolate(torch.nn.Module):
    def __init__(self, scale_factor, mode, align_corners=False):
        super().__init__()
        self.interp = F.interpolate
        self.scale_factor, self.mode, self.align_corners = scale_factor, mode, align_corners

    def forward(self, x):
        return self.interp(x, scale_factor=self.scale_factor, mode=self.mode, align_corners=self.align_corners)


def make_head_seq(features=256, cout=4, kernel=3, scale=2, align_corners=True, mid=128, mode="bilinear"):
    """The regression head's Sequential (dpt_block.py:318-324), or a variant of it."""
    return torch.nn.Sequential(
        torch.nn.Conv2d(features, mid, kernel_size=3, stride=1, padding=1),
        Interpolate(scale_factor=scale, mode=mode, align_corners=align_corners),
        torch.nn.Conv2d(mid, mid, kernel_size=kernel, stride=1, padding=kernel // 2),
        torch.nn.ReLU(True),
        torch.nn.Conv2d(mid, cout, kernel_size=1, stride=1, padding=0))


class DPTOutputAdapter(torch.nn.Module):
    """The attributes dpt.install looks for; forward is `self.head(path_1)` alone."""

    def __init__(self, features=8, **kw):
        super().__init__()
        self.scratch, self.act_postprocess, self.hooks = torch.nn.Module(), torch.nn.ModuleList(), [0]
        self.head = make_head_seq(features=features, **kw)

    def forward(self, path_1):
        return self.head(path_1)

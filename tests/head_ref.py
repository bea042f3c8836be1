"""This project's own statement of the tail of MASt3R's catmlp+dpt head that
m3s_head_postprocess computes (include/m3s_head.h), for the tests and the timing
tool.

Inputs: pts [B,4,H,W] (the DPT map: x, y, z, raw confidence) and feat
[B,S,(F+1)*P*P] (the local-feature MLP's output, S = (H/P)*(W/P)). Per output
pixel (b, yo, xo), y = yo*ds, x = xo*ds:

    s = (y // P) * (W // P) + x // P,  i = y % P,  j = x % P
    lf(c) = feat[b, s, c*P*P + i*P + j],  c in [0, F]
    d = sqrt(px^2 + py^2 + pz^2)
    X = (px, py, pz) / max(d, 1e-8) * expm1(d)
    C = conf_vmin  + min(exp(pc),    conf_vmax  - conf_vmin)
    D = lf(0..F-1) / sqrt(sum lf(c)^2)
    Q = dconf_vmin + min(exp(lf(F)), dconf_vmax - dconf_vmin)

head_exact  evaluates that in fp64 with numpy on the fp32 inputs.
bounds      is the derived per-element tolerance of an fp32 evaluation.
compare     checks a result against both: NaN and inf by class and position,
            everything else within the tolerance.
head_torch  is the same statement in plain torch with the cost profile of what a
            ROCm user of the reference runs today (tools/head_time.py).
"""
import numpy as np

EPS32 = 2.0 ** -24    # unit roundoff of fp32
TINY32 = 2.0 ** -126  # smallest normal fp32: a result below it may be flushed to zero
EPS16 = 2.0 ** -11    # unit roundoff of fp16
TINY16 = 2.0 ** -25   # half the spacing of the fp16 subnormals


def unshuffle(feat, H, W, P, F):
    """feat [B,S,(F+1)*P*P] -> lf [B,H,W,F+1]: pixel_shuffle of the transposed MLP output."""
    B = feat.shape[0]
    lf = np.asarray(feat).reshape(B, H // P, W // P, F + 1, P, P)  # b, ty, tx, c, i, j
    return lf.transpose(0, 1, 4, 2, 5, 3).reshape(B, H, W, F + 1)  # b, (ty, i), (tx, j), c


def _terms(pts, feat, P, F, conf, desc_conf, ds):
    """The fp64 intermediates both head_exact and bounds need."""
    pts = np.asarray(pts, dtype=np.float64)
    B, four, H, W = pts.shape
    assert four == 4 and H % P == 0 and W % P == 0
    assert tuple(feat.shape) == (B, (H // P) * (W // P), (F + 1) * P * P)
    lf = unshuffle(np.asarray(feat, dtype=np.float64), H, W, P, F)[:, ::ds, ::ds]
    p = pts.transpose(0, 2, 3, 1)[:, ::ds, ::ds]
    with np.errstate(all="ignore"):
        d = np.sqrt((p[..., :3] ** 2).sum(-1))
        n = np.sqrt((lf[..., :F] ** 2).sum(-1))
        out = {"d": d, "xyz": p[..., :3], "n": n, "lf": lf[..., :F]}
        for key, raw, (vmin, vmax) in (("C", p[..., 3], conf), ("Q", lf[..., F], desc_conf)):
            # the bounds as the kernel receives them: fp32 values
            vmin, vmax = float(np.float32(vmin)), float(np.float32(vmax))
            cap = vmax - vmin
            out[key] = (vmin, cap, np.minimum(np.exp(raw), cap))  # np.minimum propagates NaN
    return out


def head_exact(pts, feat, P, F, conf=(1.0, np.inf), desc_conf=(0.0, np.inf), ds=1):
    """The function above in fp64; -> dict X [B,Ho,Wo,3], C [B,Ho,Wo], D [B,Ho,Wo,F], Q [B,Ho,Wo]."""
    t = _terms(pts, feat, P, F, conf, desc_conf, ds)
    with np.errstate(all="ignore"):
        X = t["xyz"] / np.where(t["d"] < 1e-8, 1e-8, t["d"])[..., None] * np.expm1(t["d"])[..., None]
        D = t["lf"] / t["n"][..., None]
    return {"X": X, "C": t["C"][0] + t["C"][2], "D": D, "Q": t["Q"][0] + t["Q"][2]}


def bounds(pts, feat, P, F, conf=(1.0, np.inf), desc_conf=(0.0, np.inf), ds=1, desc_half=False):
    """Per-element tolerance |fp32 evaluation - exact|, eps = 2^-24; same keys and
    shapes as head_exact. Derived, not measured; valid where no intermediate
    overflows and every square is a normal number (d = 0 or d >= 1e-18, and the
    same for the descriptor's norm). exp and expm1 are taken at OpenCL's limit
    of 3 ulp, 6 eps relative; sqrt, division, product and sum are correctly
    rounded, eps each.

    X. s = fl(fl(px^2 + py^2) + pz^2): three positive terms, each product eps,
    two sums: 3 eps relative in any order. d = sqrt(s): 1.5 eps + eps = 2.5 eps.
    q = fl(p / max(d, 1e-8)): the max is 1-Lipschitz, so 2.5 eps + eps = 3.5 eps.
    e = expm1(d): the error of d enters multiplied by the condition number
    kappa = d e^d / expm1(d) (1 at d -> 0, about d for large d), plus the
    function's own 6 eps: (2.5 kappa + 6) eps. X = fl(q e): + eps. Sum:
    (10.5 + 2.5 kappa) eps |X|, taken as (11 + 3 kappa) eps |X|.

    C, Q. t = min(exp(r), cap), cap = fl(vmax - vmin): exp contributes 6 eps
    exp(r), the rounding of a finite cap eps cap, and the min passes on at most
    the larger of the two where it takes either argument; vmin + t is rounded
    once more, eps |C|. Taken as (7 t + cap [if finite] + |C|) eps.

    D. s = the sum of F squares: eps per product and at most F - 1 sums of
    positive terms, F eps relative in any order. n = sqrt(s): F/2 eps + eps.
    D = fl(lf / n): + eps. Sum (F/2 + 2) eps |D|, taken as (F/2 + 3) eps |D|.
    An fp16 D is that fp32 value rounded once more: + 2^-11 (|D| + bound) and
    2^-25 where it is an fp16 subnormal.

    Every bound gets 2^-126 on top: an fp32 result below the smallest normal may
    be flushed to zero (exp(-100) is one)."""
    t = _terms(pts, feat, P, F, conf, desc_conf, ds)
    exact = head_exact(pts, feat, P, F, conf, desc_conf, ds)
    with np.errstate(all="ignore"):
        d = t["d"]
        kappa = np.where(d > 0, d * np.exp(d) / np.where(d > 0, np.expm1(d), 1.0), 1.0)
        out = {"X": (11.0 + 3.0 * kappa)[..., None] * EPS32 * np.abs(exact["X"]) + TINY32}
        for key in ("C", "Q"):
            vmin, cap, tt = t[key]
            out[key] = (7.0 * tt + (cap if np.isfinite(cap) else 0.0) + np.abs(exact[key])) * EPS32 + TINY32
        bD = (F / 2.0 + 3.0) * EPS32 * np.abs(exact["D"]) + TINY32
        if desc_half:
            bD = bD + EPS16 * (np.abs(exact["D"]) + bD) + TINY16
        out["D"] = bD
    return out


def compare(got, exact, tol):
    """-> (ok, worst): ok when `got` is NaN exactly where `exact` is, infinite
    with the same sign exactly where `exact` rounded to fp32 is, and elsewhere
    within `tol`; worst is the largest |got - exact| / tol over those."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        want32 = exact.astype(np.float32)
    nan, inf = np.isnan(exact), np.isinf(want32) & ~np.isnan(exact)
    ok = np.array_equal(np.isnan(got), nan) and np.array_equal(np.isinf(got), inf)
    ok = ok and np.array_equal(np.sign(got[inf]), np.sign(want32[inf]))
    fin = ~nan & ~inf
    with np.errstate(all="ignore"):
        ratio = np.abs(got[fin] - exact[fin]) / tol[fin]
    worst = float(ratio.max()) if ratio.size else 0.0
    return bool(ok and not np.isnan(worst) and worst <= 1.0), worst


def head_torch(pts, feat, H, W, P, F, conf=(1.0, float("inf")), desc_conf=(0.0, float("inf"))):
    """The statement above in plain torch, fp32, with the ops and the copies a
    user of the reference pays for today (pixel_shuffle, cat, permute, then
    element-wise ops on channel-strided views); -> (pts3d [B,H,W,3], conf
    [B,H,W], desc [B,H,W,F], desc_conf [B,H,W])."""
    import torch

    B = feat.shape[0]
    lf = feat.transpose(-1, -2).view(B, -1, H // P, W // P)
    lf = torch.nn.functional.pixel_shuffle(lf, P)
    fmap = torch.cat([pts, lf], dim=1).permute(0, 2, 3, 1)
    xyz = fmap[..., 0:3]
    d = xyz.norm(dim=-1, keepdim=True)
    X = xyz / d.clip(min=1e-8) * torch.expm1(d)
    C = conf[0] + fmap[..., 3].exp().clip(max=conf[1] - conf[0])
    desc = fmap[..., 4:4 + F]
    D = desc / desc.norm(dim=-1, keepdim=True)
    Q = desc_conf[0] + fmap[..., 4 + F].exp().clip(max=desc_conf[1] - desc_conf[0])
    return X, C, D, Q

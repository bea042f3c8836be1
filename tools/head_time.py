"""The fused head tail (mast3r_slam_backends.head_postprocess, m3s_head_postprocess)
against the plain-torch tail a ROCm user of the reference runs today
(tests/head_ref.head_torch, then the SLAM side's stack and match_dense's .half()),
at MASt3R's shapes -- GPU box:

    python tools/head_time.py [--out profiles/head/head_time.json]

512 x 384 and 512 x 512 images, patch 16, 24 descriptor channels, the raw maps
[1,4,H,W] and [1,S,25*256] already on the device (the network is not timed),
under torch.inference_mode, img_downsample 1.

(a) torch   view: pixel_shuffle, cat, permute, the element-wise ops, D.half().
            frame: two views, torch.stack of X, C, D, Q, D.half().
(b) fp32    view: one head_postprocess call, fresh outputs, then D.half() as
            match_dense does. frame: two views, the four stacks, D.half().
(c) slots   view: one head_postprocess call with fp16 descriptors, written
            into its slot of preallocated stacked buffers. frame: two calls.

Wall clock per unit, the device idle before and after, the three paths
interleaved round by round; the figure is the median round, the spread its
min..max. Before anything is timed, (b) is checked against the fp64 statement
within head_ref.bounds, (a) likewise, and (c)'s D is bitwise (b)'s D.half().

kernel: the patch kernel alone, eight views per launch so that the launch is
long against the host's issue rate, device events around `reps` launches; its
algorithmic bytes (one read of both inputs, one write of the four outputs) per
second next to the streaming-copy rate bench.py --full measures
(bench.copy_leg, run here on the same device). The test build's direct-store
variant (every lane stores its own pixel) is timed the same way beside it.
Prints one JSON line; --out also writes it to a file."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam-ysh_amd"), os.path.join(ROOT, "tools"),
                os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import head_ref  # noqa: E402
import mast3r_slam_backends as be  # noqa: E402
from quantize_time import figures, rounds_of  # noqa: E402

SHAPES = ((384, 512), (512, 512))
P, F = 16, 24
HEAD_DIRECT = 2  # flags, test build only (csrc/m3s_head.hip)


def inputs(B, H, W, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    pts = torch.randn(B, 4, H, W, generator=gen)
    feat = torch.randn(B, (H // P) * (W // P), (F + 1) * P * P, generator=gen)
    return pts.to(dev), feat.to(dev)


def stacked(n, H, W, dev, dtype):
    lead = (n, 1, H, W)
    return (torch.empty(*lead, 3, device=dev), torch.empty(lead, device=dev),
            torch.empty(*lead, F, dtype=dtype, device=dev), torch.empty(lead, device=dev))


def check(pts, feat, H, W, bufs):
    args = (pts.cpu().numpy(), feat.cpu().numpy(), P, F)
    exact, tol = head_ref.head_exact(*args), head_ref.bounds(*args)
    fused = be.head_postprocess(pts, feat, P, F)
    plain = head_ref.head_torch(pts, feat, H, W, P, F)
    worst = {}
    for name, got in (("device", fused), ("torch", plain)):
        for key, g in zip(("X", "C", "D", "Q"), got):
            ok, w = head_ref.compare(g.cpu().numpy(), exact[key], tol[key])
            assert ok, f"{name} {key} outside the bound ({w:.3f})"
            worst[f"{name}_{key}"] = round(w, 3)
    slot = be.head_postprocess(pts, feat, P, F, desc_dtype=torch.float16, out=tuple(b[1] for b in bufs))
    assert torch.equal(slot[2], fused[2].half()) and all(torch.equal(slot[i], fused[i]) for i in (0, 1, 3))
    return worst


def measure(H, W, dev, rounds, reps):
    views = [inputs(1, H, W, dev, 40 + k) for k in range(2)]
    bufs = stacked(2, H, W, dev, torch.float16)
    out = {"H": H, "W": W, "worst_error_over_bound": check(*views[0], H, W, bufs)}

    def torch_view(k=0):
        X, C, D, Q = head_ref.head_torch(*views[k], H, W, P, F)
        return X, C, D.half(), Q

    def stack_frame(res):
        X, C, D, Q = (torch.stack([r[i][0] for r in res]) for i in range(4))
        return X, C, D.half(), Q

    def fp32_view(k=0):
        X, C, D, Q = be.head_postprocess(*views[k], P, F)
        return X, C, D.half(), Q

    def slot_view(k=0):
        return be.head_postprocess(*views[k], P, F, desc_dtype=torch.float16, out=tuple(b[k] for b in bufs))

    unit = {
        "view": {"torch": torch_view, "fp32": fp32_view, "slots": slot_view},
        "frame": {"torch": lambda: stack_frame([head_ref.head_torch(*v, H, W, P, F) for v in views]),
                  "fp32": lambda: stack_frame([be.head_postprocess(*v, P, F) for v in views]),
                  "slots": lambda: [slot_view(k) for k in range(2)]},
    }
    for name, fns in unit.items():
        fig = figures(rounds_of(fns, rounds, reps))
        fig["fp32_over_torch"] = round(fig["ms_fp32"] / fig["ms_torch"], 3)
        fig["slots_over_torch"] = round(fig["ms_slots"] / fig["ms_torch"], 3)
        out[name] = fig
    return out


def kernel_rate(H, W, dev, reps, test_lib):
    """GB/s of the patch kernel and of the test build's direct-store variant, B = 8 views per launch."""
    B = 8
    pts, feat = inputs(B, H, W, dev, 50)
    out = {"H": H, "W": W, "views_per_launch": B}
    for dt, dtype in (("f32", torch.float32), ("f16", torch.float16)):
        res = tuple(torch.empty(B, H, W, *tail, dtype=d, device=dev)
                    for tail, d in (((3,), torch.float32), ((), torch.float32), ((F,), dtype), ((), torch.float32)))
        nbytes = pts.numel() * 4 + feat.numel() * 4 + sum(r.numel() * r.element_size() for r in res)
        a, _ = be._head_args(pts, feat, P, F, (1.0, float("inf")), (0.0, float("inf")), 1, dtype, res, False)
        stream = be._stream(dev)
        ref = None
        for name, lib, flags in (("lds", be._lib, 0), ("direct", test_lib, HEAD_DIRECT)):
            a.flags = flags
            times = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                assert lib.m3s_head_postprocess(ctypes.byref(a), stream) == 0  # warm
                torch.cuda.synchronize()
                e0.record()
                for _ in range(reps):
                    lib.m3s_head_postprocess(ctypes.byref(a), stream)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) / reps)
            if ref is None:
                ref = [r.clone() for r in res]
            else:  # the variant computes the same values
                assert all(torch.equal(r.view(torch.uint8), q.view(torch.uint8)) for r, q in zip(res, ref)), name
            ms = float(np.median(times))
            out[f"{name}_{dt}"] = {"ms_per_launch": round(ms, 4), "ms_min_max": [round(min(times), 4), round(max(times), 4)],
                                  "bytes": nbytes, "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.rounds < 7:
        sys.exit("head_time: at least 7 rounds")
    if not torch.cuda.is_available():
        sys.exit("head_time: no GPU; this tool only measures on the device")
    from bench import copy_leg

    dev = torch.device("cuda:0")
    test_lib = be.load_test_library()
    with torch.inference_mode():
        timed = [measure(H, W, dev, a.rounds, a.reps) for H, W in SHAPES]
        kernels = [kernel_rate(H, W, dev, a.reps, test_lib) for H, W in SHAPES]
        copy = copy_leg(be, dev)
    for k in kernels:
        for key in [x for x in k if isinstance(k[x], dict)]:
            k[key]["frac_of_measured_copy"] = round(k[key]["GB_per_s"] / copy["GB_per_s"], 3)
    res = {"workload": "tail of the catmlp+dpt head, patch %d, %d descriptor channels, one view per call" % (P, F),
           "clock": "wall clock, device idle before and after; median of the rounds, paths interleaved",
           "rounds": a.rounds, "reps_per_round": a.reps, "paths": timed,
           "kernel_clock": "device events around reps launches, median of 5", "kernel": kernels,
           "hbm_copy": copy, "device": torch.cuda.get_device_name(0), "lib": be.version()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""The fused attention core (mast3r_slam_backends.attention_rope, m3s_attn_rope)
against what runs between an attention's Linears today, at MASt3R's shapes, by
the method of tools/rope_time.py -- GPU box:

    python tools/attn_time.py [--out profiles/attn/attn_time.json]

(a) torch   the reference's statement (croco blocks.py:94-112, 149-169) with the
            device rope_2d, which is what rope.install gives: two rope
            launches, matmul, scale, softmax, matmul, transpose-reshape copy.
(b) sdpa    rope_2d twice, then torch.nn.functional.scaled_dot_product_attention
            and the transpose-reshape copy.
(c) fused   attention_rope: one launch, no copy.

Per call at (B, H, Nq, Nk) = (1,16,768,768), (1,12,768,768), (2,12,768,768) and
(1,16,1024,1024), fp32, both "self" (q, k, v are the slices of one [B,N,3,H,D]
qkv buffer) and "cross" (three dense projections), under torch.inference_mode;
and the 72 attentions of one tracked frame as one unit (24 encoder self at H =
16, then 12 decoder blocks x 2 views x (self + cross) at H = 12, B = 1, N = 768).
All paths run in this process, interleaved round by round; wall clock with the
device idle before and after; the figure is the median round, the spread its
min..max. Before anything is timed every path is checked against the fp64
attn_ref.attn_exact within attn_ref.bound on the same input (on copies: rope_2d
rotates in place, so in the timed rounds q and k keep turning, at the same
norms and the same cost).

"kernel" is the fused launch alone: device events around `--burst` back-to-back
launches (enough to outrun the host's issue rate), per launch, against the
fp32 MFMA floor 4 B H Nq Nk D / 157 TFLOP/s. Prints one JSON line; --out also
writes it to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam-ysh_amd"), os.path.join(ROOT, "tools"),
                os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import attn_ref  # noqa: E402
import mast3r_slam_backends as be  # noqa: E402
from quantize_time import figures, rounds_of  # noqa: E402

D = 64
BASE, F0, SCALE = 100.0, 1.0, D ** -0.5
SHAPES = ((1, 16, 768, 768), (1, 12, 768, 768), (2, 12, 768, 768), (1, 16, 1024, 1024))
GRIDS = {768: (24, 32), 1024: (32, 32)}  # patches of a 384 x 512 and of a 512 x 512 image
FRAME = ((16, "self", 24), (12, "self", 24), (12, "cross", 24))  # (heads, kind, calls), B = 1, N = 768
F32_MFMA_TFLOPS = 157.0


def grid_positions(B, N, dev):
    pos = torch.cartesian_prod(torch.arange(GRIDS[N][0]), torch.arange(GRIDS[N][1]))
    return pos.expand(B, N, 2).contiguous().to(dev)


def inputs(B, H, Nq, Nk, kind, dev, seed=5):
    """-> q, k, v [B, N, H, D] views (qkv slices or dense projections), qpos, kpos."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "self":
        assert Nq == Nk
        qkv = (2.0 * torch.randn(B, Nq, 3 * H * D, generator=gen)).to(dev).view(B, Nq, 3, H, D)
        q, k, v = (qkv[:, :, i] for i in range(3))
    else:
        q, k, v = ((2.0 * torch.randn(B, n, H * D, generator=gen)).to(dev).view(B, n, H, D) for n in (Nq, Nk, Nk))
    return q, k, v, grid_positions(B, Nq, dev), grid_positions(B, Nk, dev)


def rotate(t, pos):
    """rope_2d, in place, on a [B, N, H, D] view; -> its [B, H, N, D] view."""
    return be.rope_2d(t, pos, BASE, F0).transpose(1, 2)


def path_torch(q, k, v, qpos, kpos):
    B, Nq, H, _ = q.shape
    q, k = rotate(q, qpos), rotate(k, kpos)
    attn = (q @ k.transpose(-2, -1)) * SCALE
    attn = attn.softmax(dim=-1)
    return (attn @ v.transpose(1, 2)).transpose(1, 2).reshape(B, Nq, H * D)


def path_sdpa(q, k, v, qpos, kpos):
    B, Nq, H, _ = q.shape
    x = torch.nn.functional.scaled_dot_product_attention(rotate(q, qpos), rotate(k, kpos), v.transpose(1, 2),
                                                         scale=SCALE)
    return x.transpose(1, 2).reshape(B, Nq, H * D)


def path_fused(q, k, v, qpos, kpos):
    return be.attention_rope(q, k, v, qpos, kpos, BASE, F0, SCALE)


PATHS = {"torch": path_torch, "sdpa": path_sdpa, "fused": path_fused}


def check(args):
    """Every path on copies of the same input (two of them rotate in place)
    against the fp64 statement; raises when one is outside the bound."""
    q, k, v, qpos, kpos = args
    exact = attn_ref.attn_exact(q, k, v, qpos, kpos, BASE, F0, SCALE)
    tol = attn_ref.bound(q, k, v, qpos, kpos, BASE, F0, SCALE)
    out = {}
    for name, fn in PATHS.items():
        err = (fn(q.clone(), k.clone(), v, qpos, kpos).to(torch.float64) - exact).abs()
        out["max_abs_err_" + name] = float(err.max())
        out["err_over_bound_" + name] = round(float((err / tol).max()), 4)
        assert bool((err <= tol).all()), f"{name} outside the bound"
    return out


def kernel_alone(args, burst, rounds):
    """ms per fused launch by device events over `burst` back-to-back launches."""
    out = torch.empty(args[0].shape[0], args[0].shape[1], args[0].shape[2] * D, device=args[0].device)
    call = lambda: be.attention_rope(*args, BASE, F0, SCALE, out=out)  # noqa: E731
    for _ in range(10):
        call()
    times = []
    for _ in range(rounds):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(burst):
            call()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) / burst)
    return times


def measure_call(B, H, Nq, Nk, kind, dev, rounds, reps, burst):
    args = inputs(B, H, Nq, Nk, kind, dev)
    out = {"B": B, "heads": H, "Nq": Nq, "Nk": Nk, "kind": kind, **check(args)}
    out.update(figures(rounds_of({name: (lambda fn=fn: fn(*args)) for name, fn in PATHS.items()}, rounds, reps)))
    k = kernel_alone(args, burst, rounds)
    floor_ms = 4.0 * B * H * Nq * Nk * D / (F32_MFMA_TFLOPS * 1e12) * 1e3
    out["ms_kernel"] = round(statistics.median(k), 4)
    out["ms_kernel_min_max"] = [round(min(k), 4), round(max(k), 4)]
    out["ms_mfma_floor"] = round(floor_ms, 4)
    out["kernel_fraction_of_floor"] = round(floor_ms / out["ms_kernel"], 3)
    out["torch_over_fused"] = round(out["ms_torch"] / out["ms_fused"], 2)
    out["sdpa_over_fused"] = round(out["ms_sdpa"] / out["ms_fused"], 2)
    return out


def measure_frame(dev, rounds):
    sets = [(inputs(1, H, 768, 768, kind, dev), calls) for H, kind, calls in FRAME]

    def frame(fn):
        for args, calls in sets:
            for _ in range(calls):
                fn(*args)

    t = rounds_of({name: (lambda fn=fn: frame(fn)) for name, fn in PATHS.items()}, rounds, 1)
    out = {"B": 1, "N": 768, "attentions": sum(c for _, _, c in FRAME), **figures(t)}
    out["torch_over_fused"] = round(out["ms_torch"] / out["ms_fused"], 2)
    out["sdpa_over_fused"] = round(out["ms_sdpa"] / out["ms_fused"], 2)
    lo, hi = out["ms_fused_min_max"]
    out["fused_faster_than_torch"] = hi < out["ms_torch_min_max"][0]  # the ranges do not overlap
    out["sdpa_faster_than_fused"] = out["ms_sdpa_min_max"][1] < lo
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--burst", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.rounds < 7:
        sys.exit("attn_time: at least 7 rounds")
    if not torch.cuda.is_available():
        sys.exit("attn_time: no GPU; this tool only measures on the device")
    dev = torch.device("cuda:0")
    with torch.inference_mode():
        calls = [measure_call(*shape, kind, dev, a.rounds, a.reps, a.burst)
                 for shape in SHAPES for kind in ("self", "cross")]
        frame = measure_frame(dev, a.rounds)
    res = {"workload": "attention core between the Linears, fp32, D=64, RoPE2D base %g, positions of a patch grid" % BASE,
           "clock": "wall clock, device idle before and after; median of the rounds, paths interleaved; "
                    "kernel: device events over a burst of launches",
           "paths": {"torch": "rope_2d x 2 + matmul, scale, softmax, matmul, reshape copy",
                     "sdpa": "rope_2d x 2 + scaled_dot_product_attention + reshape copy",
                     "fused": "attention_rope"},
           "rounds": a.rounds, "reps_per_round": a.reps, "burst": a.burst, "call": calls,
           "frame_72_attentions": frame, "device": torch.cuda.get_device_name(0), "lib": be.version()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

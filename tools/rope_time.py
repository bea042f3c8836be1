"""The device RoPE2D (mast3r_slam_amd.rope, m3s_rope_2d) against the plain-torch
implementation a ROCm user of the reference runs today (tests/rope_ref.
rope2d_torch: cos / sin tables sized by int(positions.max()), `embedding`
lookups, rotate-half), at MASt3R's shapes -- GPU box:

    python tools/rope_time.py [--out profiles/rope/rope_time.json]

N = 768 tokens (a 24 x 32 grid of patches), (heads, D) = (16, 64) for the
encoder and (12, 64) for the decoders, B = 1 and 2, fp32 and fp16; q and k are
slices of a [B, H, 3, N, D] view of one qkv buffer, as Attention.forward makes
them, under torch.inference_mode.

(a) call      one RoPE on q: wall clock per call over `reps` back-to-back calls,
              the device idle before and after.
(b) frame     the 144 calls of one tracked frame as one unit, q and k in turn:
              48 at (16, 64), then 96 at (12, 64); wall clock of the whole
              sequence, the device idle before and after. Nothing else is
              enqueued in between, so this is the cost of the calls alone; in a
              forward pass the torch version's host read per call also drains
              whatever was enqueued before it.

Both paths run in this process, interleaved round by round (device, torch,
device, ...); the figure is the median round, the spread its min..max. Before
anything is timed the two are checked against each other on the same input:
in fp32 both within rope_ref.bound of the fp64 rope_ref.rope2d_exact; in fp16
the device within 1 ulp + bound of exact, and the torch version, which rounds
the angle to fp16 before cos / sin (up to 2^-7 rad at these positions), within
2^-6 (|u| + |v|) + 2 ulp of the device. Prints one JSON line; --out also writes
it to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam-ysh_amd"), os.path.join(ROOT, "tools"),
                os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import mast3r_slam_backends as be  # noqa: E402
import rope_ref  # noqa: E402
from mast3r_slam_amd.rope import RoPE2D  # noqa: E402
from quantize_time import figures, rounds_of  # noqa: E402
from retrieval_time import wall  # noqa: E402

GRID = (24, 32)  # patches of a 384 x 512 image
N = GRID[0] * GRID[1]
HEADS = ((16, 64), (12, 64))  # ViT-L encoder; the two decoders
FRAME = ((16, 64, 48), (12, 64, 96))  # (heads, D, calls) of one tracked frame
BASE, F0 = 100.0, 1.0


def inputs(B, H, D, dtype, dev, seed=3):
    """-> (q, k) [B, H, N, D] slices of one qkv buffer, positions [B, N, 2]."""
    gen = torch.Generator().manual_seed(seed)
    buf = torch.randn(B, N, 3 * H * D, generator=gen).to(dev, dtype)
    qkv = buf.reshape(B, N, 3, H, D).transpose(1, 3)
    pos = torch.cartesian_prod(torch.arange(GRID[0]), torch.arange(GRID[1]))
    return qkv[:, :, 0], qkv[:, :, 1], pos.expand(B, N, 2).contiguous().to(dev)


def check(q, pos, device_rope):
    """The two paths on the same q (copies of it); raises when they disagree."""
    pmax = max(GRID) - 1
    exact = rope_ref.rope2d_exact(q, pos, BASE, F0)
    tol = rope_ref.bound(q, pmax, F0)
    got_t = rope_ref.rope2d_torch(q, pos, BASE, F0).to(torch.float64)
    got_d = device_rope(q.transpose(1, 2).contiguous().transpose(1, 2), pos).to(torch.float64)
    if q.dtype == torch.float32:
        assert bool(((got_d - exact).abs() <= tol).all()), "device fp32 outside the bound"
        assert bool(((got_t - exact).abs() <= tol).all()), "torch fp32 outside the bound"
    else:
        ulp = rope_ref.ulp(exact, q.dtype)
        assert bool(((got_d - exact).abs() <= ulp + tol).all()), "device fp16 outside 1 ulp + bound"
        loose = 2.0 ** -6 * rope_ref.pair_sum(q) + 2 * ulp
        assert bool(((got_t - got_d).abs() <= loose).all()), "torch fp16 far from the device"
    return {"max_abs_err_device": float((got_d - exact).abs().max()),
            "max_abs_err_torch": float((got_t - exact).abs().max())}


def measure_call(B, H, D, dtype, dev, device_rope, rounds, reps):
    q, _, pos = inputs(B, H, D, dtype, dev)
    out = {"B": B, "heads": H, "D": D, "dtype": str(dtype).replace("torch.", ""), **check(q, pos, device_rope)}
    t = rounds_of({"device": lambda: device_rope(q, pos),
                   "torch": lambda: rope_ref.rope2d_torch(q, pos, BASE, F0)}, rounds, reps)
    out.update(figures(t))
    out["torch_over_device"] = round(out["ms_torch"] / out["ms_device"], 2)
    return out


def measure_frame(B, dtype, dev, device_rope, rounds):
    sets = [(inputs(B, H, D, dtype, dev), calls) for H, D, calls in FRAME]

    def frame(fn):
        for (q, k, pos), calls in sets:
            for c in range(calls):
                fn(q if c % 2 == 0 else k, pos)

    t = rounds_of({"device": lambda: frame(device_rope),
                   "torch": lambda: frame(lambda x, pos: rope_ref.rope2d_torch(x, pos, BASE, F0))}, rounds, 1)
    out = {"B": B, "dtype": str(dtype).replace("torch.", ""), "calls": sum(c for _, _, c in FRAME), **figures(t)}
    out["torch_over_device"] = round(out["ms_torch"] / out["ms_device"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.rounds < 7:
        sys.exit("rope_time: at least 7 rounds")
    if not torch.cuda.is_available():
        sys.exit("rope_time: no GPU; this tool only measures on the device")
    dev = torch.device("cuda:0")
    device_rope = RoPE2D(BASE, F0)
    calls, frames = [], []
    with torch.inference_mode():
        for dtype in (torch.float32, torch.float16):
            for B in (1, 2):
                for H, D in HEADS:
                    calls.append(measure_call(B, H, D, dtype, dev, device_rope, a.rounds, a.reps))
                frames.append(measure_frame(B, dtype, dev, device_rope, a.rounds))
    res = {"workload": "RoPE2D on q / k slices of a qkv buffer, N=%d tokens (%d x %d), base %g" % (N, *GRID, BASE),
           "clock": "wall clock, device idle before and after; median of the rounds, paths interleaved",
           "rounds": a.rounds, "reps_per_round": a.reps, "call": calls, "frame_144_calls": frames,
           "device": torch.cuda.get_device_name(0), "lib": be.version()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

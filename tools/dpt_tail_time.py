"""The fused DPT tail (mast3r_slam_backends.dpt_tail, m3s_dpt_tail) against the
four torch modules that run today, at MASt3R's shapes, by the method of
tools/attn_time.py -- GPU box:

    python tools/dpt_tail_time.py [--out profiles/dpt_tail/dpt_tail_time.json]

(a)  torch        the Sequential's last four modules as they run today
                  (Interpolate, Conv2d 3x3, ReLU in place, Conv2d 1x1), with
                  torch.backends.cudnn.benchmark off: the library's default
                  convolution.
(a') torch_find   the same with cudnn.benchmark on, after warm-up: the best
                  convolution the library's search finds.
(c)  fused        dpt_tail: one launch.

Per call at x = (1,128,192,256), the 512 x 384 view, and (1,128,256,256), fp32,
Cout = 4, under torch.inference_mode; per frame = 2 views. All paths run in
this process, interleaved round by round; wall clock with the device idle
before and after; the figure is the median round, the spread its min..max.
Before anything is timed every path is checked against the fp64
dpt_tail_ref.dpt_tail_exact within dpt_tail_ref.bound on the same input.

"kernel" is the fused launch alone: device events around `--burst` back-to-back
launches, per launch, against the fp32 MFMA floor 2 B Ho Wo 128 (1152 + Cout) /
157.3 TFLOP/s. Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam-ysh_amd"), os.path.join(ROOT, "tools"),
                os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import dpt_tail_ref as ref  # noqa: E402
import mast3r_slam_backends as be  # noqa: E402
from quantize_time import figures, rounds_of  # noqa: E402

SHAPES = ((1, 128, 192, 256), (1, 128, 256, 256))
COUT = 4
VIEWS_PER_FRAME = 2
F32_MFMA_TFLOPS = 157.3


def modules(dev, seed=7):
    """seq[1:] of the regression head with seeded weights of the trained scale."""
    torch.manual_seed(seed)
    seq = ref.make_head_seq(features=8, cout=COUT).to(dev).eval()
    return seq[1:], tuple(p.detach() for p in (seq[2].weight, seq[2].bias, seq[4].weight, seq[4].bias))


def torch_path(tail, benchmark):
    def run(x):
        torch.backends.cudnn.benchmark = benchmark
        return tail(x)

    return run


def kernel_alone(x, packed, burst, rounds):
    """ms per fused launch by device events over `burst` back-to-back launches."""
    out = torch.empty(x.shape[0], COUT, 2 * x.shape[2], 2 * x.shape[3], device=x.device)
    call = lambda: be.dpt_tail(x, packed, COUT, out=out)  # noqa: E731
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


def measure(shape, dev, rounds, reps, burst):
    tail, w = modules(dev)
    packed = be.dpt_tail_pack(*w)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(8)).to(dev)
    paths = {"torch": torch_path(tail, False), "torch_find": torch_path(tail, True),
             "fused": lambda x: be.dpt_tail(x, packed, COUT)}
    B, _, Hi, Wi = shape
    out = {"x": list(shape), "cout": COUT}
    exact, tol = ref.dpt_tail_exact(x, *w), ref.bound(x, *w)
    for name, fn in paths.items():
        err = (fn(x).to(torch.float64) - exact).abs()
        out["err_over_bound_" + name] = round(float((err / tol).max()), 6)
        assert bool((err <= tol).all()), f"{name} outside the bound"
    del exact, tol
    for _ in range(3):  # the search of (a') happens here, not in a timed round
        paths["torch_find"](x)
    torch.cuda.synchronize()
    out.update(figures(rounds_of({name: (lambda fn=fn: fn(x)) for name, fn in paths.items()}, rounds, reps)))
    torch.backends.cudnn.benchmark = False
    for name in paths:
        out[f"ms_frame_{name}"] = round(VIEWS_PER_FRAME * out["ms_" + name], 4)
        out[f"ms_frame_{name}_min_max"] = [round(VIEWS_PER_FRAME * v, 4) for v in out[f"ms_{name}_min_max"]]
    k = kernel_alone(x, packed, burst, rounds)
    floor_ms = 2.0 * B * 4 * Hi * Wi * 128 * (1152 + COUT) / (F32_MFMA_TFLOPS * 1e12) * 1e3
    out["ms_kernel"] = round(statistics.median(k), 4)
    out["ms_kernel_min_max"] = [round(min(k), 4), round(max(k), 4)]
    out["ms_mfma_floor"] = round(floor_ms, 4)
    out["kernel_fraction_of_floor"] = round(floor_ms / out["ms_kernel"], 3)
    out["torch_over_fused"] = round(out["ms_torch"] / out["ms_fused"], 2)
    out["torch_find_over_fused"] = round(out["ms_torch_find"] / out["ms_fused"], 2)
    hi = out["ms_fused_min_max"][1]
    # the rule of the ranges: fused wholly below both torch paths
    out["fused_below_both"] = hi < out["ms_torch_min_max"][0] and hi < out["ms_torch_find_min_max"][0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.rounds < 7:
        sys.exit("dpt_tail_time: at least 7 rounds")
    if not torch.cuda.is_available():
        sys.exit("dpt_tail_time: no GPU; this tool only measures on the device")
    dev = torch.device("cuda:0")
    with torch.inference_mode():
        calls = [measure(shape, dev, a.rounds, a.reps, a.burst) for shape in SHAPES]
    res = {"workload": "last four modules of the DPT head, fp32, 128 channels, Cout = 4; frame = 2 views",
           "clock": "wall clock, device idle before and after; median of the rounds, paths interleaved; "
                    "kernel: device events over a burst of launches",
           "paths": {"torch": "Interpolate, Conv2d 3x3, ReLU, Conv2d 1x1; cudnn.benchmark off",
                     "torch_find": "the same, cudnn.benchmark on, searched before timing",
                     "fused": "dpt_tail"},
           "rounds": a.rounds, "reps_per_round": a.reps, "burst": a.burst, "call": calls,
           "device": torch.cuda.get_device_name(0), "lib": be.version()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

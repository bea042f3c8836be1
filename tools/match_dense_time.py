"""match_dense against the composed path it replaces, end to end, on one
symmetric 512x512 pair (B = 2, F = 24, float16 descriptors, base.yaml's
matching config, Q_conf = 1.5) -- GPU box:

    python tools/match_dense_time.py [--out FILE] [--rounds 7] [--reps 50]

composed   matching.match (prep_rays, iter_proj, refine_matches and the torch
           glue between them), then what FactorGraph.add_factors and its caller
           add before the edge store: sqrt(Q11[b, idx] * Q21) (global_opt.py:
           53-57), valid & (Q > Q_conf), the match fraction per direction, and
           the int64 -> int32 copy of idx into an edge-store row
           (EdgeStore.append). Entry points this tool's subject leaves untouched.
fused      mast3r_slam_backends.match_dense writing the same rows.

Both run in this process, interleaved round by round (composed, fused,
composed, ...), every round `reps` calls between two device events after a
warm-up of each; the figure is the median round, the spread its min..max.
Launch counts come from torch's profiler (kernel and memcpy/memset records of
one call each). The outputs of the two paths are compared before anything is
timed. Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam-ysh_amd")]
import torch  # noqa: E402

import mast3r_slam_backends as be  # noqa: E402
from mast3r_slam_amd import matching, synthetic  # noqa: E402

Q_CONF = 1.5


def inputs(H, W, dev, B=2):
    ms = [synthetic.make_match_inputs(H, W, seed=1005 + 17 * k, device=dev) for k in range(B)]
    gen = torch.Generator().manual_seed(1006)
    Q11 = (1.0 + 2.0 * torch.rand(B, H * W, generator=gen)).to(dev)
    Q21 = (1.0 + 2.0 * torch.rand(B, H * W, generator=gen)).to(dev)
    cat = lambda name: torch.cat([getattr(m, name) for m in ms]).contiguous()
    return cat("X11"), cat("X21"), cat("D11"), cat("D21"), Q11, Q21


def composed(X11, X21, D11, D21, Q11, Q21, rows):
    idx, valid = matching.match(X11, X21, D11, D21)
    B, HW = idx.shape
    bi = torch.arange(B, device=idx.device)[:, None].repeat(1, HW)
    Q = torch.sqrt(Q11.reshape(B, HW, 1)[bi, idx] * Q21.reshape(B, HW, 1))
    frac = (valid & (Q > Q_CONF)).reshape(B, -1).float().mean(1)
    rows[0][:], rows[1][:], rows[2][:] = idx, valid, Q
    return frac


def fused(X11, X21, D11, D21, Q11, Q21, rows):
    return be.match_dense(X11, X21, D11, D21, Q11, Q21, Q_conf=Q_CONF, out=rows)[3]


def launches(fn):
    """Device records (kernels, copies, fills) of one call, or None where the
    profiler has no device tracing."""
    from torch.profiler import ProfilerActivity, profile

    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as exc:  # noqa: BLE001
        print("profiler unavailable: %r" % (exc,), file=sys.stderr)
        return None
    return n or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=(512, 512))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("match_dense_time: no GPU; this tool only measures on the device")
    dev = torch.device("cuda:0")
    H, W = a.size
    ins = inputs(H, W, dev)
    B, HW = 2, H * W

    def rows():
        return (torch.empty(B, HW, dtype=torch.int32, device=dev),
                torch.empty(B, HW, 1, dtype=torch.bool, device=dev),
                torch.empty(B, HW, 1, dtype=torch.float32, device=dev))

    rc, rf = rows(), rows()
    paths = {"composed": lambda: composed(*ins, rc), "fused": lambda: fused(*ins, rf)}
    frac, n = paths["composed"](), paths["fused"]()
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(rc, rf)) and torch.equal(
        (frac * HW).round().long(), n.long())
    times = {k: [] for k in paths}
    for fn in paths.values():  # warm-up: code objects, the allocator's blocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.reps)
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"workload": "one symmetric %dx%d pair: B=2, F=%d float16 descriptors, base.yaml matching config, "
                       "Q_conf=%.1f" % (H, W, ins[2].shape[-1], Q_CONF),
           "rounds": a.rounds, "reps_per_round": a.reps, "outputs_identical": bool(same),
           "ms_composed": round(med["composed"], 4), "ms_fused": round(med["fused"], 4),
           "ms_composed_min_max": [round(min(times["composed"]), 4), round(max(times["composed"]), 4)],
           "ms_fused_min_max": [round(min(times["fused"]), 4), round(max(times["fused"]), 4)],
           "composed_over_fused": round(med["composed"] / med["fused"], 3),
           "launches_composed": launches(paths["composed"]), "launches_fused": launches(paths["fused"]),
           "device": torch.cuda.get_device_name(0), "lib": be.version()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

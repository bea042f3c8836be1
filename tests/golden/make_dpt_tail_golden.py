"""Writes tests/golden/dpt_tail_{a..e}.npz and dpt_tail_w.npz from the reference's
own DPT modules.

    python tests/golden/make_dpt_tail_golden.py <reference checkout>

It needs the reference's source tree and runs only where that is present; the
tests read the fixtures it leaves. One file is loaded from its path:
<reference>/thirdparty/mast3r/dust3r/croco/models/dpt_block.py (it imports only
torch and einops). The last four modules of its regression head
(dpt_block.py:318-324) are built from its `Interpolate` class,

    nn.Sequential(Interpolate(2, 'bilinear', True), Conv2d(128, 128, 3, padding=1),
                  ReLU(True), Conv2d(128, Cout, 1))

with seeded weights, and run on the CPU in fp32 under no_grad.

dpt_tail_w.npz holds `w1` [128,128,3,3], `b1` [128], `w2` [4,128,1,1], `b2` [4],
shared by every case (a case with Cout < 4 takes the first Cout rows of w2 and
b2). w1 is normal / sqrt(1152) times a factor spread log-uniformly over three
decades per element, so the 1152-term sums cancel heavily and `mid` has many
negatives. Every case file stores `x` [B,128,Hi,Wi] f32, `cout` and the
reference's `out` [B,cout,2Hi,2Wi] f32.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LARGEST_FIXTURE = 662425  # bytes: the largest fixture committed before these

#        B  Hi  Wi  Cout spread
CASES = {
    "a": (2, 5, 7, 4, False),
    "b": (1, 1, 1, 4, False),
    "c": (1, 1, 5, 4, False),
    "d": (1, 3, 2, 3, False),
    "e": (1, 12, 9, 4, True),  # |x| from 1e-3 to 1e3
}


def weights(rng):
    w1 = rng.standard_normal((128, 128, 3, 3)) / np.sqrt(1152.0)
    w1 *= np.exp(rng.uniform(np.log(0.03), np.log(30.0), w1.shape))
    b1 = 0.5 * rng.standard_normal(128)
    w2 = rng.standard_normal((4, 128, 1, 1)) / np.sqrt(128.0)
    w2 *= np.exp(rng.uniform(np.log(0.03), np.log(30.0), w2.shape))
    b2 = rng.standard_normal(4)
    return tuple(t.astype(np.float32) for t in (w1, b1, w2, b2))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    path = os.path.join(sys.argv[1], "thirdparty", "mast3r", "dust3r", "croco", "models", "dpt_block.py")
    spec = importlib.util.spec_from_file_location("reference_dpt_block", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    w1, b1, w2, b2 = weights(np.random.RandomState(300))
    wpath = os.path.join(HERE, "dpt_tail_w.npz")
    np.savez_compressed(wpath, w1=w1, b1=b1, w2=w2, b2=b2)
    assert os.path.getsize(wpath) <= LARGEST_FIXTURE, os.path.getsize(wpath)
    print(f"{wpath}: {os.path.getsize(wpath)} bytes")
    for k, (name, (B, Hi, Wi, cout, spread)) in enumerate(sorted(CASES.items())):
        rng = np.random.RandomState(301 + k)
        x = rng.standard_normal((B, 128, Hi, Wi))
        if spread:
            x *= np.exp(rng.uniform(np.log(1e-3), np.log(1e3), x.shape))
        x = x.astype(np.float32)
        seq = torch.nn.Sequential(ref.Interpolate(scale_factor=2, mode="bilinear", align_corners=True),
                                  torch.nn.Conv2d(128, 128, kernel_size=3, stride=1, padding=1), torch.nn.ReLU(True),
                                  torch.nn.Conv2d(128, cout, kernel_size=1, stride=1, padding=0))
        with torch.no_grad():
            seq[1].weight.copy_(torch.from_numpy(w1)), seq[1].bias.copy_(torch.from_numpy(b1))
            seq[3].weight.copy_(torch.from_numpy(w2[:cout])), seq[3].bias.copy_(torch.from_numpy(b2[:cout]))
            out = seq(torch.from_numpy(x))
            mid = seq[:3](torch.from_numpy(x))
        assert tuple(out.shape) == (B, cout, 2 * Hi, 2 * Wi) and out.dtype == torch.float32
        cpath = os.path.join(HERE, f"dpt_tail_{name}.npz")
        np.savez_compressed(cpath, x=x, cout=np.int64(cout), out=out.numpy())
        print(f"{cpath}: B={B} Hi={Hi} Wi={Wi} Cout={cout}, mid == 0 on {float((mid == 0).float().mean()):.2f} "
              f"of its elements, max {float(mid.max()):.3g} ({os.path.getsize(cpath)} bytes)")


if __name__ == "__main__":
    main()

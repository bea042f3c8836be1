"""Writes tests/golden/rope_{a..f}.npz from the reference's own RoPE2D.

    python tests/golden/make_rope_golden.py <reference checkout>

It needs the reference's source tree and runs only where that is present; the
tests read the fixtures it leaves. <reference>/thirdparty/mast3r/dust3r/croco/
models/pos_embed.py is loaded from its file; its `models.curope` import fails
(the compiled extension is absent), so the RoPE2D it defines is its PyTorch
implementation. That module runs on the CPU in fp32 with base = 100, F0 = 1 on
seeded inputs; every fixture stores `tokens` [B, H, N, D] f32, `pos` [B, N, 2]
int64 (y, x), `out` [B, H, N, D] f32 and `base`, `F0`, `pmax`. Each fixture has
its maximum position on both axes and one token at (0, 0).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
BASE, F0 = 100.0, 1.0

#        B   H   N   D  max position
SHAPES = {
    "a": (2, 3, 37, 64, 31),   # 16-byte vectors; tails in the heads and in the tokens
    "b": (1, 19, 5, 64, 47),   # several head passes and a tail, for 4 and for 8 lanes per head
    "c": (1, 2, 5, 8, 63),     # Q = 2: element by element
    "d": (1, 1, 3, 4, 100),    # Q = 1
    "e": (1, 2, 7, 40, 31),    # Q = 10: no vector width divides it, and i/Q is inexact
    "f": (2, 5, 9, 96, 31),    # Q = 24
}


def load_reference(ref_root):
    path = os.path.join(ref_root, "thirdparty", "mast3r", "dust3r", "croco", "models", "pos_embed.py")
    spec = importlib.util.spec_from_file_location("reference_pos_embed", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.RoPE2D.__module__ == "reference_pos_embed", "expected the PyTorch RoPE2D, not the compiled one"
    return mod.RoPE2D


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rope = load_reference(sys.argv[1])(freq=BASE, F0=F0)
    for k, (name, (B, H, N, D, pmax)) in enumerate(sorted(SHAPES.items())):
        rng = np.random.RandomState(100 + k)
        tokens = rng.standard_normal((B, H, N, D)).astype(np.float32)
        pos = rng.randint(0, pmax + 1, size=(B, N, 2)).astype(np.int64)
        pos[0, 0] = (pmax, pmax)
        pos[0, 1] = (0, 0)
        pos[-1, -1] = (pmax, 0)
        with torch.no_grad():
            out = rope(torch.from_numpy(tokens), torch.from_numpy(pos))
        assert out.dtype == torch.float32 and tuple(out.shape) == tokens.shape
        path = os.path.join(HERE, f"rope_{name}.npz")
        np.savez(path, tokens=tokens, pos=pos, out=out.numpy(), base=np.float64(BASE), F0=np.float64(F0),
                 pmax=np.int64(pmax))
        print(f"{path}: B={B} H={H} N={N} D={D} pmax={pmax} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()

"""Writes tests/golden/attn_{a..d}.npz from the reference's own Attention and
CrossAttention.

    python tests/golden/make_attn_golden.py <reference checkout>

It needs the reference's source tree and runs only where that is present; the
tests read the fixtures it leaves. <reference>/thirdparty/mast3r/dust3r/croco/
models/pos_embed.py and blocks.py are loaded from their files (blocks.py needs
only torch; pos_embed.py's `models.curope` import fails, so its RoPE2D is the
PyTorch implementation). The reference's module is built with RoPE2D(100, 1)
and `proj = nn.Identity()`, runs on the CPU in fp32 on seeded inputs, and
forward hooks capture what its Linears return. Every fixture stores, all fp32:

    self   qkv [B, N, 3 H D] (the qkv Linear's output), pos [B, N, 2] int64
    cross  q [B, Nq, H D], k, v [B, Nk, H D] (projq / projk / projv), qpos, kpos
    both   out [B, Nq, H D] (the module's output), H, scale, base, F0, pmax, kind

Positions run up to 31 on both axes; each fixture holds (31, 31) and (0, 0). The
weights of fixtures b and c are scaled up so that max |score| >= 10 (the default
initialisation gives about 1.5, which barely exercises the softmax).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
BASE, F0, PMAX, D = 100.0, 1.0, 31, 64

#        kind     B  H  Nq  Nk   weight gain
SHAPES = {
    "a": ("self", 2, 2, 37, 37, 1.0),
    "b": ("self", 1, 3, 65, 65, 4.0),
    "c": ("cross", 1, 2, 33, 70, 4.0),
    "d": ("cross", 2, 1, 1, 100, 1.0),
}


def load(ref_root, name):
    path = os.path.join(ref_root, "thirdparty", "mast3r", "dust3r", "croco", "models", name + ".py")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def positions(rng, B, N):
    pos = rng.randint(0, PMAX + 1, size=(B, N, 2)).astype(np.int64)
    pos[0, 0] = (PMAX, PMAX)
    pos[-1, -1] = (0, 0)
    if N > 2:
        pos[0, 1] = (PMAX, 0)
    return pos


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    pos_embed, blocks = load(sys.argv[1], "pos_embed"), load(sys.argv[1], "blocks")
    assert pos_embed.RoPE2D.__module__ == "reference_pos_embed", "expected the PyTorch RoPE2D, not the compiled one"
    for n, (name, (kind, B, H, Nq, Nk, gain)) in enumerate(sorted(SHAPES.items())):
        torch.manual_seed(300 + n)
        rng = np.random.RandomState(300 + n)
        C = H * D
        rope = pos_embed.RoPE2D(freq=BASE, F0=F0)
        cls = blocks.Attention if kind == "self" else blocks.CrossAttention
        module = cls(C, rope=rope, num_heads=H, qkv_bias=True).eval()
        module.proj = torch.nn.Identity()
        linears = ("qkv",) if kind == "self" else ("projq", "projk", "projv")
        captured = {}
        for lin in linears:
            with torch.no_grad():
                getattr(module, lin).weight.mul_(gain)
            getattr(module, lin).register_forward_hook(
                lambda mod, inp, out, lin=lin: captured.__setitem__(lin, out.detach().clone()))
        qpos = positions(rng, B, Nq)
        with torch.no_grad():
            if kind == "self":
                x = torch.from_numpy(rng.standard_normal((B, Nq, C)).astype(np.float32))
                out = module(x, torch.from_numpy(qpos))
                data = dict(qkv=captured["qkv"].numpy(), pos=qpos)
                q, k = captured["qkv"].reshape(B, Nq, 3, H, D)[:, :, 0], captured["qkv"].reshape(B, Nq, 3, H, D)[:, :, 1]
            else:
                kpos = positions(rng, B, Nk)
                xq = torch.from_numpy(rng.standard_normal((B, Nq, C)).astype(np.float32))
                xk = torch.from_numpy(rng.standard_normal((B, Nk, C)).astype(np.float32))
                xv = torch.from_numpy(rng.standard_normal((B, Nk, C)).astype(np.float32))
                out = module(xq, xk, xv, torch.from_numpy(qpos), torch.from_numpy(kpos))
                data = dict(q=captured["projq"].numpy(), k=captured["projk"].numpy(), v=captured["projv"].numpy(),
                            qpos=qpos, kpos=kpos)
                q, k = captured["projq"].reshape(B, Nq, H, D), captured["projk"].reshape(B, Nk, H, D)
        assert out.dtype == torch.float32 and tuple(out.shape) == (B, Nq, C)
        # rotations keep norms: |score| <= scale |q| |k|, and the unrotated products show the order
        smax = float((torch.einsum("bihd,bjhd->bhij", q, k) * module.scale).abs().max())
        if gain != 1.0:
            assert smax >= 10.0, (name, smax)
        path = os.path.join(HERE, f"attn_{name}.npz")
        np.savez(path, out=out.numpy(), H=np.int64(H), scale=np.float64(module.scale), base=np.float64(BASE),
                 F0=np.float64(F0), pmax=np.int64(PMAX), kind=np.array(kind), **data)
        print(f"{path}: {kind} B={B} H={H} Nq={Nq} Nk={Nk} max |q.k| scale = {smax:.1f} "
              f"({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()

"""tests/rope_ref.py against the reference's own RoPE2D (no GPU needed): for every
fixture of tests/golden/make_rope_golden.py the reference's fp32 output lies
within rope_ref.bound of rope_ref.rope2d_exact, which pins the restatement's
layout, axis order and frequency law to the reference's code; and a wrong layout
(interleaved pairs, or X before Y) is off by O(1), so the bound can tell."""
import os

import numpy as np
import pytest
import torch

import rope_ref

FIXTURES = ("a", "b", "c", "d", "e", "f")


def load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, f"rope_{name}.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].ndim else z[k].item()) for k in z.files}


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_shape_and_positions(golden_dir, name):
    fx = load(golden_dir, name)
    B, H, N, D = fx["tokens"].shape
    assert D % 4 == 0 and tuple(fx["pos"].shape) == (B, N, 2) and fx["pos"].dtype == torch.int64
    assert fx["out"].shape == fx["tokens"].shape and fx["out"].dtype == torch.float32
    assert int(fx["pos"][..., 0].max()) == fx["pmax"] == int(fx["pos"][..., 1].max())
    assert int(fx["pos"].min()) == 0 and bool((fx["pos"] == 0).all(-1).any())
    assert (fx["base"], fx["F0"]) == (100.0, 1.0)


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_within_bound_of_exact(golden_dir, name):
    fx = load(golden_dir, name)
    exact = rope_ref.rope2d_exact(fx["tokens"], fx["pos"], fx["base"], fx["F0"])
    tol = rope_ref.bound(fx["tokens"], fx["pmax"], fx["F0"])
    err = (fx["out"].to(torch.float64) - exact).abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"rope_{name}: max |reference - exact| / bound = {worst:.3f}")
    assert bool((err <= tol).all()), worst


def test_wrong_layouts_are_far_outside_the_bound(golden_dir):
    fx = load(golden_dir, "a")
    tokens, pos = fx["tokens"], fx["pos"]
    B, H, N, D = tokens.shape
    tol = rope_ref.bound(tokens, fx["pmax"], fx["F0"])
    ref = fx["out"].to(torch.float64)
    # X before Y
    swapped = rope_ref.rope2d_exact(tokens, pos.flip(-1), fx["base"], fx["F0"])
    # interleaved pairs (u0 v0 u1 v1 ...) within each axis half
    Q = D // 4
    to_inter = tokens.reshape(B, H, N, 2, Q, 2).transpose(-1, -2).reshape(B, H, N, D)
    inter = rope_ref.rope2d_exact(to_inter, pos, fx["base"], fx["F0"])
    inter = inter.reshape(B, H, N, 2, 2, Q).transpose(-1, -2).reshape(B, H, N, D)
    for name, wrong in (("X before Y", swapped), ("interleaved", inter)):
        err = (wrong - ref).abs()
        assert float(err.max()) > 1.0, name
        assert float((err > tol).double().mean()) > 0.5, name


def test_inverse_and_norm_of_exact(golden_dir):
    fx = load(golden_dir, "e")
    exact = rope_ref.rope2d_exact(fx["tokens"], fx["pos"], fx["base"], fx["F0"])
    back = rope_ref.rope2d_exact(exact, fx["pos"], fx["base"], -fx["F0"])
    assert float((back - fx["tokens"].to(torch.float64)).abs().max()) < 1e-13
    zero = (fx["pos"] == 0).all(-1)  # a token at (0, 0) is not rotated
    assert torch.equal(exact.transpose(1, 2)[zero], fx["tokens"].to(torch.float64).transpose(1, 2)[zero])


def test_torch_version_agrees_in_fp32(golden_dir):
    fx = load(golden_dir, "f")
    got = rope_ref.rope2d_torch(fx["tokens"], fx["pos"], fx["base"], fx["F0"])
    exact = rope_ref.rope2d_exact(fx["tokens"], fx["pos"], fx["base"], fx["F0"])
    assert bool(((got.to(torch.float64) - exact).abs() <= rope_ref.bound(fx["tokens"], fx["pmax"], fx["F0"])).all())

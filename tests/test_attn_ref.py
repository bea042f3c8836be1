"""CPU: ties tests/attn_ref.py (the fp64 statement of m3s_attn_rope's function
and the derived fp32 tolerance) to the reference's own Attention and
CrossAttention, through the fixtures of tests/golden/make_attn_golden.py. The
GPU tests then need only attn_ref."""
import os

import pytest
import torch

import attn_ref
import rope_ref

FIXTURES = {"a": ("self", 2, 2, 37, 37), "b": ("self", 1, 3, 65, 65), "c": ("cross", 1, 2, 33, 70),
            "d": ("cross", 2, 1, 1, 100)}
D = 64


load, call_args = attn_ref.load_fixture, attn_ref.call_args


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture_is_what_the_generator_describes(golden_dir, name):
    kind, B, H, Nq, Nk = FIXTURES[name]
    c = load(golden_dir, name)
    assert c["kind"] == kind and c["H"] == H and (c["base"], c["F0"], c["pmax"]) == (100.0, 1.0, 31)
    assert c["scale"] == D ** -0.5
    assert tuple(c["q"].shape) == (B, Nq, H, D) and tuple(c["k"].shape) == tuple(c["v"].shape) == (B, Nk, H, D)
    assert tuple(c["out"].shape) == (B, Nq, H * D) and c["out"].dtype == torch.float32
    for pos, n in ((c["qpos"], Nq), (c["kpos"], Nk)):
        assert pos.dtype == torch.int64 and tuple(pos.shape) == (B, n, 2)
        assert int(pos.min()) == 0 and int(pos.max()) == 31
        assert bool((pos == 31).all(-1).any()) and bool((pos == 0).all(-1).any())
    if kind == "self":
        assert c["q"].stride() == (3 * Nq * H * D, 3 * H * D, D, 1)
    assert os.path.getsize(os.path.join(golden_dir, f"attn_{name}.npz")) \
        < os.path.getsize(os.path.join(golden_dir, "head_a.npz"))
    smax = float(attn_ref.attn_parts(*call_args(c))[3].abs().max())
    print(f"attn_{name}: max |score| = {smax:.2f}")
    if name in ("b", "c"):
        assert smax >= 10.0


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_reference_output_within_bound_of_exact(golden_dir, name):
    c = load(golden_dir, name)
    exact = attn_ref.attn_exact(*call_args(c))
    tol = attn_ref.bound(*call_args(c))
    err = (c["out"].to(torch.float64) - exact).abs()
    print(f"attn_{name}: max |reference - exact| = {float(err.max()):.3e} at output scale "
          f"{float(exact.abs().max()):.2f}; max of error / bound = {float((err / tol).max()):.3f}")
    assert bool((tol > 0).all()) and bool((err <= tol).all())
    # the bound is a tolerance, not a licence: worst case over every rounding, it still
    # stays below 1 % of the output even at |score| > 20 (fixtures b and c)
    assert float(tol.max()) < 1e-2 * float(exact.abs().max())
    # and rope_bound is rope_ref.bound without its last relaxation: never above it
    tok = c["k"].permute(0, 2, 1, 3)
    assert bool((attn_ref.rope_bound(tok, c["kpos"], c["base"], c["F0"])
                 <= rope_ref.bound(tok, c["pmax"], c["F0"])).all())


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_attn_torch_is_the_same_function(golden_dir, name):
    c = load(golden_dir, name)
    rope = lambda t, pos: rope_ref.rope2d_exact(t, pos, c["base"], c["F0"])  # noqa: E731
    q, k, v = (t.to(torch.float64) for t in (c["q"], c["k"], c["v"]))
    got = attn_ref.attn_torch(q, k, v, c["qpos"], c["kpos"], c["scale"], rope)
    exact = attn_ref.attn_exact(*call_args(c))
    assert float((got - exact).abs().max()) < 1e-13 * max(1.0, float(exact.abs().max()))

"""m3s_rope_2d on the device (include/m3s_rope.h) against tests/rope_ref.py: the
fp64 statement of the function and the derived tolerance of an fp32 evaluation.
The fixtures of tests/golden/make_rope_golden.py supply shapes, tokens and
positions (tests/test_rope_ref.py ties rope_ref to the reference's own output
on them); nothing here reads the reference."""
import os

import numpy as np
import pytest
import torch

import rope_ref

pytestmark = pytest.mark.gpu

FIXTURES = ("a", "b", "c", "d", "e", "f")
HALF = {"f16": torch.float16, "bf16": torch.bfloat16}
DTYPES = {"f32": torch.float32, **HALF}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


@pytest.fixture(scope="module")
def cases(golden_dir, dev):
    """{name: tokens [B,H,N,D] f32, pos, base, F0, pmax} on the device, and per
    fixture the fp64 exact result and the fp32 bound; computed once, not written to."""
    out = {}
    for name in FIXTURES:
        z = np.load(os.path.join(golden_dir, f"rope_{name}.npz"))
        c = {"tokens": torch.from_numpy(z["tokens"]).to(dev), "pos": torch.from_numpy(z["pos"]).to(dev),
             "base": float(z["base"]), "F0": float(z["F0"]), "pmax": int(z["pmax"])}
        c["exact"] = rope_ref.rope2d_exact(c["tokens"], c["pos"], c["base"], c["F0"])
        c["bound"] = rope_ref.bound(c["tokens"], c["pmax"], c["F0"])
        out[name] = c
    return out


def rotate(be, tokens_bhnd, pos, base, F0):
    """A fresh [B,N,H,D]-contiguous copy of the tokens through the kernel; -> [B,H,N,D]."""
    x = tokens_bhnd.transpose(1, 2).contiguous()
    assert be.rope_2d(x, pos, base, F0) is x
    return x.transpose(1, 2)


def worst(err, tol):
    return float((err / tol.clamp_min(1e-300)).max())


@pytest.mark.parametrize("name", FIXTURES)
def test_fp32_within_bound_of_exact(cases, be, name):
    c = cases[name]
    got = rotate(be, c["tokens"], c["pos"], c["base"], c["F0"])
    err = (got.to(torch.float64) - c["exact"]).abs()
    print(f"rope_{name} f32: max |device - exact| / bound = {worst(err, c['bound']):.3f}")
    assert bool((err <= c["bound"]).all())
    zero = (c["pos"] == 0).all(-1)  # a token at (0, 0) is left bitwise as it was
    assert torch.equal(got.transpose(1, 2)[zero], c["tokens"].transpose(1, 2)[zero])


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", ("a", "e"))
def test_qkv_slices_equal_contiguous_and_touch_nothing_else(cases, be, dev, name, dt):
    c, dtype = cases[name], DTYPES[dt]
    B, H, N, D = c["tokens"].shape
    guard = 64  # elements: 16-byte alignment of the buffer is kept for every dtype
    gen = torch.Generator().manual_seed(5)
    flat = torch.randn(2 * guard + B * N * 3 * H * D, generator=gen).to(dev, dtype)
    before = flat.clone()
    qkv = flat[guard:guard + B * N * 3 * H * D].view(B, N, 3, H, D)
    q, k = qkv[:, :, 0], qkv[:, :, 1]  # [B, N, H, D], strides (3NHD, 3HD, D, 1)
    assert q.stride() == (3 * N * H * D, 3 * H * D, D, 1)
    want_q = rotate(be, q.transpose(1, 2), c["pos"], c["base"], c["F0"])
    want_k = rotate(be, k.transpose(1, 2), c["pos"], c["base"], -c["F0"])
    be.rope_2d(q, c["pos"], c["base"], c["F0"])
    be.rope_2d(k, c["pos"], c["base"], -c["F0"])
    after = flat[guard:guard + B * N * 3 * H * D].view(B, N, 3, H, D)
    assert torch.equal(after[:, :, 0], want_q.transpose(1, 2))
    assert torch.equal(after[:, :, 1], want_k.transpose(1, 2))
    assert not torch.equal(after[:, :, 0], before[guard:-guard].view(B, N, 3, H, D)[:, :, 0])
    assert torch.equal(after[:, :, 2], before[guard:-guard].view(B, N, 3, H, D)[:, :, 2])
    assert torch.equal(flat[:guard], before[:guard]) and torch.equal(flat[-guard:], before[-guard:])


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("name", ("a", "b", "f"))
def test_misaligned_view_equals_aligned_bitwise(cases, be, dev, name, dt):
    c, dtype = cases[name], DTYPES[dt]
    tokens = c["tokens"].to(dtype)
    B, H, N, D = tokens.shape
    want = rotate(be, tokens, c["pos"], c["base"], c["F0"])  # base 16-byte aligned: vectors
    again = rotate(be, tokens, c["pos"], c["base"], c["F0"])
    assert torch.equal(want, again)
    flat = torch.zeros(B * N * H * D + 8, dtype=dtype, device=dev)
    assert flat.data_ptr() % 16 == 0
    for offset in (1, 3):  # elements: never a multiple of 16 bytes
        x = flat[offset:offset + B * N * H * D].view(B, N, H, D)
        assert x.data_ptr() % 16 != 0
        x.copy_(tokens.transpose(1, 2))
        be.rope_2d(x, c["pos"], c["base"], c["F0"])
        assert torch.equal(x.transpose(1, 2), want), offset


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_padded_rows_with_odd_strides(cases, be, dev, dt):
    """Token rows one element apart from dense: the base is aligned, the token
    and batch strides are not multiples of 16 bytes, and the padding stays."""
    c, dtype = cases["a"], DTYPES[dt]
    tokens = c["tokens"].to(dtype)
    B, H, N, D = tokens.shape
    want = rotate(be, tokens, c["pos"], c["base"], c["F0"])
    buf = torch.full((B, N, H * D + 1), 7.0, dtype=dtype, device=dev)
    x = buf[:, :, :H * D].view(B, N, H, D)
    assert x.stride() == (N * (H * D + 1), H * D + 1, D, 1) and x.data_ptr() % 16 == 0
    x.copy_(tokens.transpose(1, 2))
    be.rope_2d(x, c["pos"], c["base"], c["F0"])
    assert torch.equal(x.transpose(1, 2), want)
    assert bool((buf[:, :, H * D] == 7.0).all())


@pytest.mark.parametrize("dt", sorted(HALF))
@pytest.mark.parametrize("name", ("a", "b"))
def test_half_within_one_ulp_plus_bound(cases, be, name, dt):
    """An fp32 result rounded once is within 1/2 ulp of the fp32 result, which
    is within `bound` of the exact one; the ulp is taken at the exact value's
    binade, which can be the smaller neighbour of the fp32 result's, so 1 ulp."""
    c, dtype = cases[name], HALF[dt]
    tokens = c["tokens"].to(dtype)
    exact = rope_ref.rope2d_exact(tokens, c["pos"], c["base"], c["F0"])
    tol = rope_ref.ulp(exact, dtype) + rope_ref.bound(tokens, c["pmax"], c["F0"])
    got = rotate(be, tokens, c["pos"], c["base"], c["F0"])
    assert got.dtype == dtype
    err = (got.to(torch.float64) - exact).abs()
    print(f"rope_{name} {dt}: max |device - exact| / (ulp + bound) = {worst(err, tol):.3f}")
    assert bool((err <= tol).all())


@pytest.mark.parametrize("name", ("a", "e"))
def test_inverse_restores_the_input(cases, be, name):
    c = cases[name]
    fwd = rotate(be, c["tokens"], c["pos"], c["base"], c["F0"])
    back = rotate(be, fwd, c["pos"], c["base"], -c["F0"])
    err = (back.to(torch.float64) - c["tokens"].to(torch.float64)).abs()
    print(f"rope_{name}: max |inverse(forward) - input| / (2 bound) = {worst(err, 2 * c['bound']):.3f}")
    assert bool((err <= 2 * c["bound"]).all())
    assert not torch.equal(fwd, c["tokens"])


def test_autograd_through_qkv_views(be, dev):
    """x -> Linear -> q, k, v views of one qkv buffer -> RoPE2D on q and k ->
    sum(q gq + k gk + v gv). The loss is linear in q, k, v, so x.grad does not
    depend on the forward values: it is W^T applied to (R^-1 gq | R^-1 gk | gv).
    Tolerance: the fp32 inverse rotation of g is within bound(g) of exact, which
    the Linear's backward carries as |W|^T bound; that product itself, 3C terms
    in fp32, is within (3C + 2) eps |W|^T |d| of exact."""
    from mast3r_slam_amd.rope import RoPE2D

    B, N, C, H, D, pmax = 2, 37, 128, 2, 64, 11
    gen = torch.Generator().manual_seed(9)
    lin = torch.nn.Linear(C, 3 * C).to(dev)
    x = torch.randn(B, N, C, generator=gen).to(dev).requires_grad_()
    pos = torch.randint(0, pmax + 1, (B, N, 2), generator=gen).to(dev)
    gq = torch.randn(B, N, H, D, generator=gen).to(dev).transpose(1, 2)  # a gradient in the kernel's layout
    gk, gv = (torch.randn(B, H, N, D, generator=gen).to(dev) for _ in range(2))  # and two that are not
    rope = RoPE2D(100.0, 1.0)

    buf = lin(x)
    qkv = buf.reshape(B, N, 3, H, D).transpose(1, 3)
    q, k, v = (qkv[:, :, i] for i in range(3))
    q_in = q.detach().clone()
    q2, k2 = rope(q, pos), rope(k, pos)
    assert q2.data_ptr() == q.data_ptr() and k2.data_ptr() == k.data_ptr()  # in place,
    assert q2.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()  # in the qkv buffer
    fwd_exact = rope_ref.rope2d_exact(q_in, pos, 100.0, 1.0)
    assert bool(((q2.detach().to(torch.float64) - fwd_exact).abs() <= rope_ref.bound(q_in, pmax, 1.0)).all())
    ((q2 * gq).sum() + (k2 * gk).sum() + (v * gv).sum()).backward()

    W = lin.weight.detach().to(torch.float64)  # [3C, C]
    x64 = x.detach().to(torch.float64).requires_grad_()
    qkv64 = (x64 @ W.T + lin.bias.detach().to(torch.float64)).reshape(B, N, 3, H, D).transpose(1, 3)
    q64, k64 = (rope_ref.rope2d_exact(qkv64[:, :, i], pos, 100.0, 1.0) for i in range(2))
    ((q64 * gq).sum() + (k64 * gk).sum() + (qkv64[:, :, 2] * gv).sum()).backward()

    # per qkv channel: the exact upstream gradient and the bound on its fp32 evaluation, as [B, N, 3C]
    d_exact = torch.stack((rope_ref.rope2d_exact(gq, pos, 100.0, -1.0), rope_ref.rope2d_exact(gk, pos, 100.0, -1.0),
                           gv.to(torch.float64)), dim=2)  # [B, H, 3, N, D]
    d_bound = torch.stack((rope_ref.bound(gq, pmax, 1.0), rope_ref.bound(gk, pmax, 1.0),
                           torch.zeros_like(gv, dtype=torch.float64)), dim=2)
    flat = lambda t: t.transpose(1, 3).reshape(B, N, 3 * C)  # noqa: E731
    tol = flat(d_bound) @ W.abs() + (3 * C + 2) * rope_ref.EPS32 * (flat(d_exact).abs() @ W.abs())
    err = (x.grad.to(torch.float64) - x64.grad).abs()
    print(f"autograd: max |x.grad - exact| / tolerance = {worst(err, tol):.3f}")
    assert bool((err <= tol).all())
    # without the inverse rotation the gradient is far outside
    wrong = torch.stack((gq.to(torch.float64), gk.to(torch.float64), gv.to(torch.float64)), dim=2)
    assert float(((flat(wrong) @ W) - x64.grad).abs().max()) > 1e2 * float(tol.max())


def test_inference_mode_no_allocation_no_copy(cases, be, dev):
    from torch.profiler import ProfilerActivity, profile

    from mast3r_slam_amd.rope import RoPE2D

    c = cases["a"]
    rope = RoPE2D(c["base"], c["F0"])
    tokens = c["tokens"].transpose(1, 2).contiguous().transpose(1, 2).half()  # [B,H,N,D] over [B,N,H,D] storage
    with torch.inference_mode():
        assert rope(tokens, c["pos"]) is tokens  # also the warm-up: the code object
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        rope(tokens, c["pos"])
        assert torch.cuda.memory_allocated() == held
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(10):
                rope(tokens, c["pos"])
            torch.cuda.synchronize()
    device_type = torch.autograd.DeviceType
    on_device = [e.name for e in prof.events() if e.device_type == device_type.CUDA]
    host = [e.name for e in prof.events() if e.device_type == device_type.CPU]
    # the runtime's own view, for where the profiler has no device tracing
    copies_api = [n for n in host if n.startswith("hipMemcpy")]
    launches_api = [n for n in host if "LaunchKernel" in n]
    print("device records:", on_device, "runtime launches:", len(launches_api), "runtime copies:", copies_api)
    assert on_device or launches_api, "the profiler recorded neither device activity nor runtime calls"
    if on_device:
        assert len([n for n in on_device if "rope_vec_kernel" in n]) == 10, on_device
        assert not [n for n in on_device if "memcpy" in n.lower() or "memset" in n.lower()], on_device
    if launches_api:
        assert len(launches_api) == 10, launches_api
    assert not copies_api, copies_api


class RoPE2D(torch.nn.Module):
    """The stand-in install looks for (by class name): rope_ref.rope2d_exact
    rounded once to the tokens' dtype, out of place."""

    def __init__(self, freq=100.0, F0=1.0):
        super().__init__()
        self.base, self.F0 = freq, F0

    def forward(self, tokens, positions):
        return rope_ref.rope2d_exact(tokens, positions, self.base, self.F0).to(tokens.dtype)


class Attention(torch.nn.Module):
    """Self-attention with the reference's tensor plumbing: one qkv Linear, q, k
    and v as slices of its [B, H, 3, N, D] view, rope on q and k."""

    def __init__(self, dim, heads, rope):
        super().__init__()
        self.heads = heads
        self.qkv = torch.nn.Linear(dim, 3 * dim)
        self.proj = torch.nn.Linear(dim, dim)
        self.rope = rope

    def forward(self, x, pos):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.heads, C // self.heads).transpose(1, 3)
        q, k, v = (qkv[:, :, i] for i in range(3))
        if self.rope is not None:
            q, k = self.rope(q, pos), self.rope(k, pos)
        attn = (q @ k.transpose(-2, -1) * (C // self.heads) ** -0.5).softmax(dim=-1)
        return x + self.proj((attn @ v).transpose(1, 2).reshape(B, N, C))


def test_install_on_an_attention_stack(be, dev):
    """Two blocks, embed 128, 2 heads of D = 64, N = 37 tokens of a 6 x 7 grid,
    fp32. Both runs do the same torch ops on the same weights; they differ only
    in q and k, by at most bound = (12 * 6 + 7) eps (|u| + |v|) ~ 5e-6 relative
    per block. Logits are bilinear in (q, k) and softmax, the weighted sum and
    the Linears are Lipschitz with constants of order one at these scales, so
    the outputs differ by a small multiple of 2 blocks x 2 operands x 5e-6;
    tolerance 1e-4 of the largest output. The stack without any rope differs
    from the exact one by more than a thousand times that."""
    from mast3r_slam_amd import rope

    torch.manual_seed(13)
    shared = RoPE2D(100.0, 1.0)
    blocks = torch.nn.ModuleList([Attention(128, 2, shared), Attention(128, 2, shared)]).to(dev)
    with torch.no_grad():
        for blk in blocks:
            blk.qkv.weight.mul_(3.0)  # logits of order one: the rotation matters to the output
    gen = torch.Generator().manual_seed(14)
    x = torch.randn(1, 37, 128, generator=gen).to(dev)
    grid = torch.cartesian_prod(torch.arange(6), torch.arange(7))[:37]
    pos = grid.reshape(1, 37, 2).to(dev)

    def run():
        with torch.inference_mode():
            y = x
            for blk in blocks:
                y = blk(y, pos)
        return y

    want = run()
    assert rope.install(blocks) == 2
    assert type(blocks[0].rope) is rope.RoPE2D and blocks[0].rope is blocks[1].rope
    got = run()
    tol = 1e-4 * float(want.abs().max())
    err = float((got - want).abs().max())
    for blk in blocks:
        blk.rope = None
    bare = float((run() - want).abs().max())
    print(f"install: max |device stack - exact stack| = {err:.3e}, tolerance {tol:.3e}, without rope {bare:.3e}")
    assert err <= tol
    assert bare > 1e3 * tol

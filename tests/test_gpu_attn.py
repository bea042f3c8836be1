"""m3s_attn_rope on the device (include/m3s_attn.h) against tests/attn_ref.py:
the fp64 statement of the function and the derived tolerance of an fp32
evaluation. The fixtures of tests/golden/make_attn_golden.py supply the
reference's own Linear outputs (tests/test_attn_ref.py ties attn_ref to the
reference's output on them); nothing here reads the reference."""
import copy

import numpy as np
import pytest
import torch

import attn_ref

pytestmark = pytest.mark.gpu

FIXTURES = ("a", "b", "c", "d")
D = 64
BASE, F0 = 100.0, 1.0
KERNEL = "attn_rope_kernel"


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
    """The four fixtures on the device, each with its fp64 exact result and its
    fp32 bound; computed once, not written to."""
    out = {}
    for name in FIXTURES:
        c = attn_ref.load_fixture(golden_dir, name, dev)
        c["exact"] = attn_ref.attn_exact(*attn_ref.call_args(c))
        c["bound"] = attn_ref.bound(*attn_ref.call_args(c))
        out[name] = c
    return out


def worst(err, tol):
    return float((err / tol.clamp_min(1e-300)).max())


def randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def positions(gen, B, N, pmax=31):
    """[B, N, 2] int64, different per batch, with (pmax, pmax) and (0, 0)."""
    pos = torch.randint(0, pmax + 1, (B, N, 2), generator=gen)
    pos[0, 0] = pmax
    pos[-1, -1] = 0
    return pos


def check(be, q, k, v, qpos, kpos, scale, what, base=BASE, f0=F0):
    """One call against the exact function and the bound; -> the device result."""
    got = be.attention_rope(q, k, v, qpos, kpos, base, f0, scale)
    exact = attn_ref.attn_exact(q, k, v, qpos, kpos, base, f0, scale)
    tol = attn_ref.bound(q, k, v, qpos, kpos, base, f0, scale)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(exact.shape)
    assert bool(torch.isfinite(got).all()), what
    err = (got.to(torch.float64) - exact).abs()
    print(f"{what}: max |device - exact| = {float(err.max()):.3e}, max of error / bound = {worst(err, tol):.3f}")
    assert bool((err <= tol).all()), what
    return got


# ------------------------------------------------------------- 1. fixtures --
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_within_bound_of_exact(cases, be, name):
    c = cases[name]
    if c["kind"] == "self":  # the real qkv-slice views
        assert c["q"].stride() == (c["qkv"][0].numel(), 3 * c["H"] * D, D, 1) and not c["q"].is_contiguous()
    got = be.attention_rope(*attn_ref.call_args(c))
    err = (got.to(torch.float64) - c["exact"]).abs()
    ref = (c["out"].to(torch.float64) - c["exact"]).abs()
    print(f"attn_{name}: max |device - exact| = {float(err.max()):.3e} (the reference's own fp32: "
          f"{float(ref.max()):.3e}), max of error / bound = {worst(err, c['bound']):.3f}")
    assert bool((err <= c["bound"]).all())


# --------------------------------------------------------- 2. exact layout --
def test_one_hot_softmax_returns_rows_of_v_bitwise(be, dev):
    """q_i = 64 k_pi(i) on distinct +-1 keys: the matching score is 512, every
    other at most 240, every other weight exp(<= -272) = 0 in fp32, so out[i] is
    v[pi(i)] to the bit. A row / column swap or the natural k order in the second
    product returns other rows or mixtures of them."""
    Nq, Nk, H = 70, 100, 2
    keys = np.random.RandomState(0).choice([-1, 1], (Nk, D)).astype(np.float32)
    gram = keys @ keys.T
    assert float(np.abs(gram - np.diag(np.diag(gram))).max()) == 30.0 and bool((np.diag(gram) == 64).all())
    rng = np.random.RandomState(1)
    pis = [rng.permutation(Nk)[:Nq] for _ in range(H)]
    assert all((pi != np.arange(Nq)).any() for pi in pis) and (pis[0] != pis[1]).any()
    v = rng.standard_normal((1, Nk, H, D)).astype(np.float32)
    v[v == 0] = 1.0
    k = np.broadcast_to(keys[None, :, None, :], (1, Nk, H, D)).copy()
    q = np.stack([64.0 * keys[pi] for pi in pis], axis=1)[None]  # [1, Nq, H, D]
    want = np.stack([v[0, pi, h] for h, pi in enumerate(pis)], axis=1).reshape(1, Nq, H * D)
    got = be.attention_rope(*(torch.from_numpy(t).to(dev) for t in (q, k, v)), None, None, BASE, F0, 0.125)
    assert torch.equal(got.cpu(), torch.from_numpy(want))


# ---------------------------------------------------------------- 3. tails --
SIZES = (1, 31, 32, 33, 64, 65, 100)
PAIRS = [(SIZES[i], SIZES[(i + s) % 7]) for s in (0, 2, 5) for i in range(7)]  # every size on both axes
# with B H = 6 workgroups the kernel splits the kv tiles of 32 four ways: from 129 keys on a part
# walks more than one tile (two at 129 and 256, with an empty part at 129; three at 300: the
# prefetch two tiles ahead)
LONG = [(33, 129), (64, 256), (65, 300)]


def test_pairs_keep_every_size_on_both_axes():
    assert {a for a, _ in PAIRS} == {b for _, b in PAIRS} == set(SIZES)


@pytest.mark.parametrize("Nq,Nk", PAIRS + LONG)
def test_tails_within_bound(be, dev, Nq, Nk):
    B, H = 2, 3
    gen = torch.Generator().manual_seed(1000 * Nq + Nk)
    q, k, v = (randn(gen, B, n, H, D).to(dev) for n in (Nq, Nk, Nk))
    qpos, kpos = positions(gen, B, Nq).to(dev), positions(gen, B, Nk).to(dev)
    assert Nq == 1 or not torch.equal(qpos[0], qpos[1])
    check(be, 2.0 * q, k, v, qpos, kpos, 0.125, f"tails Nq={Nq} Nk={Nk}")


@pytest.mark.parametrize("H,Nk", ((256, 300), (257, 300), (257, 33)))
def test_both_workgroup_shapes(be, dev, H, Nk):
    """Up to 256 workgroups (one per compute unit; here one per head) the kernel
    splits the kv range four ways over eight waves, beyond that two ways over
    four: the threshold from both sides, with five tiles per part on the far side."""
    gen = torch.Generator().manual_seed(H + Nk)
    B, Nq = 1, 33
    q, k, v = (randn(gen, B, n, H, D).to(dev) for n in (Nq, Nk, Nk))
    qpos, kpos = positions(gen, B, Nq).to(dev), positions(gen, B, Nk).to(dev)
    check(be, 2.0 * q, k, v, qpos, kpos, 0.125, f"H={H} Nk={Nk}")


# ------------------------------------------------------ 4. running maximum --
def ramp_case(dev, order):
    """Scores that are exactly monotone along j: q_i = c_i e and k_j = a_j e for
    one unit-norm direction e, no rotation; |score| up to 80. 300 keys: every
    part of the kernel's four-way kv split walks three tiles (two in the last)."""
    Nq, Nk, H = 33, 300, 2
    gen = torch.Generator().manual_seed(41)
    e = randn(gen, D)
    e = e / e.norm()
    a = torch.linspace(-80.0, 80.0, Nk)
    if order == "decreasing":
        a = a.flip(0)
    c = 0.25 + 0.75 * torch.rand(Nq, generator=gen)
    c[0] = 1.0
    q = (c[:, None] * e)[None, :, None, :].expand(1, Nq, H, D).contiguous()
    k = (a[:, None] * e)[None, :, None, :].expand(1, Nk, H, D).contiguous()
    return q.to(dev), k.to(dev), randn(gen, 1, Nk, H, D).to(dev)


@pytest.mark.parametrize("order", ("increasing", "decreasing"))
def test_maximum_in_the_last_or_first_tile(be, dev, order):
    q, k, v = ramp_case(dev, order)
    s = attn_ref.attn_parts(q, k, v, None, None, BASE, F0, 1.0)[3]
    d = s[..., 1:] - s[..., :-1]
    assert bool((d > 0).all() if order == "increasing" else (d < 0).all()) and float(s.abs().max()) > 75.0
    check(be, q, k, v, None, None, 1.0, f"scores {order}")


def test_scores_up_to_80(be, dev):
    gen = torch.Generator().manual_seed(42)
    B, Nq, Nk, H = 1, 40, 300, 2
    q, k, v = (randn(gen, B, n, H, D).to(dev) for n in (Nq, Nk, Nk))
    qpos, kpos = positions(gen, B, Nq).to(dev), positions(gen, B, Nk).to(dev)
    s = attn_ref.attn_parts(q, k, v, qpos, kpos, BASE, F0, 1.0)[3]
    scale = 80.0 / float(s.abs().max())
    check(be, q, k, v, qpos, kpos, scale, "random scores, |s| up to 80")


def test_zero_q_gives_the_mean_of_v(be, dev):
    gen = torch.Generator().manual_seed(43)
    B, Nq, Nk, H = 2, 33, 70, 2
    k, v = randn(gen, B, Nk, H, D).to(dev), randn(gen, B, Nk, H, D).to(dev)  # random V: zeros would hide a softmax bug
    q = torch.zeros(B, Nq, H, D, device=dev)
    qpos, kpos = positions(gen, B, Nq).to(dev), positions(gen, B, Nk).to(dev)
    got = check(be, q, k, v, qpos, kpos, 0.125, "zero q")
    mean = v.to(torch.float64).mean(dim=1).reshape(B, 1, H * D)
    tol = attn_ref.bound(q, k, v, qpos, kpos, BASE, F0, 0.125)
    assert bool(((got.to(torch.float64) - mean).abs() <= tol + 1e-15).all())


# ---------------------------------------------------- 5. views and guards --
def test_qkv_slices_equal_contiguous_and_inputs_stay(cases, be):
    c = cases["a"]
    before = c["qkv"].clone()
    got = be.attention_rope(*attn_ref.call_args(c))
    dense = be.attention_rope(c["q"].contiguous(), c["k"].contiguous(), c["v"].contiguous(),
                              *attn_ref.call_args(c)[3:])
    assert torch.equal(got, dense)
    assert torch.equal(c["qkv"], before)  # q, k and v are read only


def test_nan_rows_around_k_and_v_are_never_read(cases, be, dev):
    c = cases["c"]
    B, Nk, H, _ = c["k"].shape
    want = be.attention_rope(*attn_ref.call_args(c))
    for guard in (1, 40):
        big = [torch.full((B, Nk + 2 * guard, H, D), float("nan"), device=dev) for _ in range(2)]
        views = [b[:, guard:guard + Nk] for b in big]
        views[0].copy_(c["k"])
        views[1].copy_(c["v"])
        got = be.attention_rope(c["q"], views[0], views[1], *attn_ref.call_args(c)[3:])
        assert torch.equal(got, want), guard
    # B = 2: the batch stride spans the NaN rows as well
    c = cases["d"]
    B, Nk, H, _ = c["k"].shape
    want = be.attention_rope(*attn_ref.call_args(c))
    big = [torch.full((B, Nk + 9, H, D), float("nan"), device=dev) for _ in range(2)]
    views = [b[:, 4:4 + Nk] for b in big]
    views[0].copy_(c["k"])
    views[1].copy_(c["v"])
    assert torch.equal(be.attention_rope(c["q"], views[0], views[1], *attn_ref.call_args(c)[3:]), want)


@pytest.mark.parametrize("lead,pad", ((4, 8), (1, 3)))  # 16-byte vectors; element by element
def test_out_slot_of_a_padded_buffer(cases, be, dev, lead, pad):
    c = cases["a"]
    B, Nq, H, _ = c["q"].shape
    want = be.attention_rope(*attn_ref.call_args(c))
    big = torch.full((B, Nq + 2, H * D + pad), 7.5, device=dev)
    slot = big[:, 1:1 + Nq, lead:lead + H * D]
    assert (slot.data_ptr() % 16 == 0 and slot.stride(1) % 4 == 0) == (lead == 4)
    assert be.attention_rope(*attn_ref.call_args(c), out=slot) is slot
    assert torch.equal(slot, want)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[:, 1:1 + Nq, lead:lead + H * D] = False
    assert bool((big[mask] == 7.5).all())


def test_misaligned_inputs_equal_aligned_bitwise(cases, be, dev):
    c = cases["c"]
    want = be.attention_rope(*attn_ref.call_args(c))
    moved = []
    for t in (c["q"], c["k"], c["v"]):
        flat = torch.zeros(t.numel() + 4, device=dev)
        x = flat[1:1 + t.numel()].view(t.shape)
        assert x.data_ptr() % 16 != 0
        x.copy_(t)
        moved.append(x)
    assert torch.equal(be.attention_rope(*moved, *attn_ref.call_args(c)[3:]), want)


# ------------------------------------------------ 6. agreement with rope_2d --
@pytest.mark.parametrize("name", ("a", "c"))
def test_fused_rotation_is_rope_2d_bitwise(cases, be, name):
    c = cases[name]
    fused = be.attention_rope(*attn_ref.call_args(c))
    q, k = (c[n].clone(memory_format=torch.contiguous_format) for n in ("q", "k"))  # rope_2d rotates in place
    be.rope_2d(q, c["qpos"], c["base"], c["F0"])
    be.rope_2d(k, c["kpos"], c["base"], c["F0"])
    assert not torch.equal(q, c["q"])
    assert torch.equal(be.attention_rope(q, k, c["v"], None, None, c["base"], c["F0"], c["scale"]), fused)


def test_positions_beyond_the_cos_sin_table(be, dev):
    """The kernel keeps (cos, sin) of the positions 0 .. 63 in a table and
    evaluates every other position directly: 63, 64, negative and large ones in
    one call, bitwise against rope_2d and within the bound of the exact function."""
    gen = torch.Generator().manual_seed(61)
    B, Nq, Nk, H = 2, 33, 70, 2
    q, k, v = (randn(gen, B, n, H, D).to(dev) for n in (Nq, Nk, Nk))
    qpos = torch.randint(-9, 200, (B, Nq, 2), generator=gen)
    kpos = torch.randint(-9, 200, (B, Nk, 2), generator=gen)
    qpos[0, :4] = torch.tensor([[63, 64], [64, 63], [-1, 0], [0, -1]])
    kpos[1, :4] = torch.tensor([[63, 64], [64, 63], [-1, 199], [1000, -1000]])
    qpos, kpos = qpos.to(dev), kpos.to(dev)
    fused = check(be, q, k, v, qpos, kpos, 0.125, "positions in and out of the table")
    qr, kr = q.clone(), k.clone()
    be.rope_2d(qr, qpos, BASE, F0)
    be.rope_2d(kr, kpos, BASE, F0)
    assert torch.equal(be.attention_rope(qr, kr, v, None, None, BASE, F0, 0.125), fused)


def test_null_positions_equal_zero_positions_bitwise(cases, be):
    c = cases["b"]
    none = be.attention_rope(c["q"], c["k"], c["v"], None, None, c["base"], c["F0"], c["scale"])
    zero = torch.zeros_like(c["qpos"])
    assert torch.equal(be.attention_rope(c["q"], c["k"], c["v"], zero, zero, c["base"], c["F0"], c["scale"]), none)
    assert not torch.equal(be.attention_rope(*attn_ref.call_args(c)), none)


# ------------------------------------------------------------- 7. plumbing --
def test_two_runs_agree_bitwise_and_side_stream(cases, be, dev):
    c = cases["b"]
    first = be.attention_rope(*attn_ref.call_args(c))
    assert torch.equal(be.attention_rope(*attn_ref.call_args(c)), first)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = be.attention_rope(*attn_ref.call_args(c))
    side.synchronize()
    assert torch.equal(got, first)


def test_inference_mode_no_allocation_one_launch_no_copy(cases, be, dev):
    from torch.profiler import ProfilerActivity, profile

    c = cases["a"]
    args = attn_ref.call_args(c)
    with torch.inference_mode():
        out = be.attention_rope(*args)  # also the warm-up: the code object
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        assert be.attention_rope(*args, out=out) is out
        assert torch.cuda.memory_allocated() == held
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                be.attention_rope(*args, out=out)
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
        assert len([n for n in on_device if KERNEL in n]) == 5, on_device
        assert not [n for n in on_device if "rope_vec_kernel" in n or "rope_elem_kernel" in n], on_device
        assert not [n for n in on_device if "memcpy" in n.lower() or "memset" in n.lower()], on_device
    if launches_api:
        assert len(launches_api) == 5, launches_api
    assert not copies_api, copies_api


# ------------------------------------------------------- 8. stand-in model --
class Stack(torch.nn.Module):
    """One self and one cross block in the reference's attribute names."""

    def __init__(self, dim=128, heads=2):
        super().__init__()
        rope = attn_ref.RoPE2D(BASE, F0)
        self.attn = attn_ref.Attention(dim, rope, heads)
        self.cross_attn = attn_ref.CrossAttention(dim, rope, heads)

    def forward(self, x, mem, pos, mpos):
        y = x + self.attn(x, pos)
        return y + self.cross_attn(y, mem, mem, pos, mpos)


def test_install_on_a_stand_in_stack(be, dev):
    """Embed 128, 2 heads of D = 64, 37 query and 70 memory tokens, fp32.

    Every attention is checked where it happens: the tensors the patched forward
    hands to the kernel are the module's own Linear outputs (views, no copy), and
    the kernel's result is within attn_ref.bound of attn_exact on exactly those.

    End to end the patched stack is compared with the same stack on fp64
    arithmetic. A worst-case bound carried through five Linears and two
    attentions (lin_bound and bound with input errors) multiplies by the
    absolute row sums of every stage and ends above the output itself, so it
    says nothing; the tolerance here is the reasoning of
    test_gpu_rope.test_install_on_an_attention_stack instead: per stage the fp32
    error is a few eps sqrt(K) ~ 1e-6 relative for K = 128 (Linear) and of the
    same order for the attention (test_attn_ref prints 3e-7 for the reference's
    own), softmax, the weighted sum and the Linears are Lipschitz with constants
    of order one at these scales, seven stages: 1e-4 of the largest output. The
    stack without rope differs from the exact one by far more than that."""
    from mast3r_slam_amd import attention

    torch.manual_seed(17)
    stack = Stack().to(dev).eval()
    with torch.no_grad():
        stack.attn.qkv.weight.mul_(3.0)  # logits of order one: rope and softmax matter to the output
        stack.cross_attn.projq.weight.mul_(3.0)
        stack.cross_attn.projk.weight.mul_(3.0)
    gen = torch.Generator().manual_seed(18)
    B, N, M = 2, 37, 70
    x, mem = randn(gen, B, N, 128).to(dev), randn(gen, B, M, 128).to(dev)
    pos, mpos = positions(gen, B, N, 7).to(dev), positions(gen, B, M, 7).to(dev)
    plain = copy.deepcopy(stack)
    with torch.no_grad():
        exact = copy.deepcopy(stack).double()(x.double(), mem.double(), pos, mpos)
    tol = 1e-4 * float(exact.abs().max())

    assert attention.install(stack) == 2 and attention.install(stack) == 0
    calls = []
    real = be.attention_rope

    def spy(*a, **kw):
        out = real(*a, **kw)
        calls.append((a, out))
        return out

    be.attention_rope = spy
    try:
        with torch.inference_mode():
            got = stack(x, mem, pos, mpos)
            want32 = plain(x, mem, pos, mpos)
            assert len(calls) == 2  # both attentions went through the kernel
            (a_self, o_self), (a_cross, o_cross) = calls
            # self: the three slices of the qkv Linear's buffer; cross: the dense projections
            assert a_self[0].stride() == (N * 3 * 128, 3 * 128, D, 1)
            assert a_self[1].data_ptr() - a_self[0].data_ptr() == 128 * 4 == a_self[2].data_ptr() - a_self[1].data_ptr()
            assert a_cross[0].is_contiguous() and tuple(a_cross[1].shape) == (B, M, 2, D)
            assert a_self[3] is pos and a_self[4] is pos and a_cross[3] is pos and a_cross[4] is mpos
            for what, (a, out) in zip(("self", "cross"), calls):
                assert a[5:] == (BASE, F0, stack.attn.scale)
                err = (out.to(torch.float64) - attn_ref.attn_exact(*a)).abs()
                print(f"stack, {what} attention: max of error / bound = {worst(err, attn_ref.bound(*a)):.3f}")
                assert bool((err <= attn_ref.bound(*a)).all())
        err = float((got.to(torch.float64) - exact).abs().max())
        ref = float((want32.to(torch.float64) - exact).abs().max())
        for m in (plain.attn, plain.cross_attn):
            m.rope = None
        with torch.inference_mode():
            bare = float((plain(x, mem, pos, mpos).to(torch.float64) - exact).abs().max())
        for m in (plain.attn, plain.cross_attn):
            m.rope = stack.attn.rope
        print(f"stack: max |patched - exact| = {err:.3e} (plain torch fp32: {ref:.3e}), tolerance {tol:.3e}, "
              f"without rope {bare:.3e}")
        assert err <= tol
        assert bare > 1e3 * tol
        # fall-backs: bitwise the unpatched module, and no launch
        del calls[:]
        with torch.no_grad():
            with torch.autocast("cuda", dtype=torch.float16):
                assert torch.equal(stack(x, mem, pos, mpos), plain(x, mem, pos, mpos))
        half, plain_half = copy.deepcopy(stack).half(), copy.deepcopy(plain).half()
        assert "forward" in vars(half.attn)  # the copy is still patched
        with torch.no_grad():
            assert torch.equal(half(x.half(), mem.half(), pos, mpos), plain_half(x.half(), mem.half(), pos, mpos))
        y = stack(x, mem, pos, mpos)  # gradients enabled, parameters require them
        assert y.requires_grad and torch.equal(y.detach(), plain(x, mem, pos, mpos).detach())
        assert not calls
    finally:
        be.attention_rope = real

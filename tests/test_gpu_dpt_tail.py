"""m3s_dpt_tail on the device (include/m3s_dpt.h) against tests/dpt_tail_ref.py:
the fp64 statement of the function with the header's fp32 lambdas and the
derived tolerance of an fp32 evaluation. The fixtures of
tests/golden/make_dpt_tail_golden.py supply inputs and weights
(tests/test_dpt_tail_ref.py ties dpt_tail_ref to the reference's own output on
them, at fractions of 1e-4 to 3e-4 of the bound); nothing here reads the
reference. The geometry and routing tests are bitwise: with one-hot weights
every sum has one non-zero term, so the output is the header's u itself."""
import copy

import pytest
import torch

import dpt_tail_ref as ref

pytestmark = pytest.mark.gpu

KERNEL = "dpt_tail_kernel"
C = 128


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
def cases(golden_dir, dev, be):
    """{name: x and packed weights on the device, cout, the fp64 exact result
    and the fp32 bound (CPU)}; computed once, not written to."""
    out = {}
    for name in ref.FIXTURES:
        c = ref.load_fixture(golden_dir, name)
        c["exact"], c["bound"] = ref.dpt_tail_exact(c["x"], *c["w"]), ref.bound(c["x"], *c["w"])
        c["ref_fraction"] = float(((c["out"].double() - c["exact"]).abs() / c["bound"]).max())
        c["xd"] = c["x"].to(dev)
        c["packed"] = be.dpt_tail_pack(*(t.to(dev) for t in c["w"]))
        out[name] = c
    return out


def frac(got, c, sel=slice(None)):
    return float(((got.double().cpu() - c["exact"][:, sel]).abs() / c["bound"][:, sel]).max())


def bitwise(a, b):
    """Equal bit for bit, NaN included."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


# ------------------------------------------------------------ 1. fixtures --
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_fixture_within_bound_of_exact(cases, be, name):
    c = cases[name]
    got = be.dpt_tail(c["xd"], c["packed"], c["cout"])
    B, _, Hi, Wi = c["x"].shape
    assert tuple(got.shape) == (B, c["cout"], 2 * Hi, 2 * Wi) and got.dtype == torch.float32 and got.is_contiguous()
    f = frac(got, c)
    print(f"dpt_tail_{name}: max |device - exact| / bound = {f:.3g} (the reference's own: {c['ref_fraction']:.3g})")
    assert f <= 1.0


# ------------------------------------------------- 2. geometry, bitwise --
def tile_shape(be):
    """Outputs that end past a tile border in both directions and span 3 x 3
    workgroup tiles. The output sizes are even and so are the tile sizes, so the
    closest an image can end behind a border is two pixels, not one."""
    return be.DPT_TILE_H + 1, be.DPT_TILE_W + 1


def one_hot_weights(dev, tap, chans, src=None, sign=1.0):
    """w1[c, src(c), tap] = sign, b1 = 0, row o of w2 one-hot on chans[o], b2 = 0."""
    src = torch.arange(C) if src is None else src
    w1 = torch.zeros(C, C, 3, 3)
    w1[torch.arange(C), src, tap // 3, tap % 3] = sign
    w2 = torch.zeros(len(chans), C)
    w2[torch.arange(len(chans)), torch.tensor(chans)] = 1.0
    return tuple(t.to(dev) for t in (w1, torch.zeros(C), w2, torch.zeros(len(chans))))


def shifted(u, tap):
    """u [B,C,Ho,Wo] seen through tap (dy, dx) of a zero-padded 3x3 window."""
    dy, dx = tap // 3, tap % 3
    Ho, Wo = u.shape[2:]
    return torch.nn.functional.pad(u, (1, 1, 1, 1))[:, :, dy:dy + Ho, dx:dx + Wo]


def geometry_shapes(be):
    return [(5, 7), (1, 1), (1, 5), (3, 2), tile_shape(be)]


@pytest.fixture(scope="module")
def positive(be, dev):
    """{(Hi, Wi): (x > 0 [2,128,Hi,Wi], the header's u in torch fp32 op by op)}."""
    gen = torch.Generator().manual_seed(41)
    out = {}
    for Hi, Wi in geometry_shapes(be):
        x = (torch.rand(2, C, Hi, Wi, generator=gen) + 0.25).to(dev)
        out[Hi, Wi] = (x, ref.upsample_f32(x))
    return out


@pytest.mark.parametrize("tap", range(9))
def test_each_tap_returns_shifted_u_bitwise(be, dev, positive, tap):
    chans = [0, 37, 64 + 5, 127]
    packed = be.dpt_tail_pack(*one_hot_weights(dev, tap, chans))
    for (Hi, Wi), (x, u) in positive.items():
        got = be.dpt_tail(x, packed, 4)
        want = shifted(u, tap)[:, chans]
        assert bitwise(got, want), (tap, Hi, Wi, int((got != want).sum()))
        if Hi > 1 and tap == 0:
            assert bool((got[:, :, 0] == 0).all()) and bool((got[:, :, :, 0] == 0).all())  # the padding row and column
            assert bool((got[:, :, 1:, 1:] > 0).all())


def test_relu_gives_exact_zeros(be, dev, positive):
    packed = be.dpt_tail_pack(*one_hot_weights(dev, 4, [3, 70, 101], sign=-1.0))
    for x, _ in positive.values():
        got = be.dpt_tail(x, packed, 3)
        assert bitwise(got, torch.zeros_like(got))


# ------------------------------------------------------ 3. channel routing --
@pytest.mark.parametrize("cout", [1, 3, 4])
def test_channel_routing_bitwise(be, dev, positive, cout):
    """w1[c, pi(c), centre] = 1 for a fixed permutation pi, every row of w2 one-hot on
    another channel: out[o] = u[pi(c_o)]. All 128 mid channels are visited, cout at a time."""
    pi = torch.randperm(C, generator=torch.Generator().manual_seed(43))
    x, u = positive[tile_shape(be)]
    xs, us = positive[5, 7]
    order = torch.randperm(C, generator=torch.Generator().manual_seed(44)).tolist()
    groups = [order[i:i + cout] for i in range(0, C - cout + 1, cout)]
    for k, chans in enumerate(groups):
        packed = be.dpt_tail_pack(*one_hot_weights(dev, 4, chans, src=pi))
        xx, uu = (x, u) if k % 8 == 0 else (xs, us)  # the tiled shape now and then, the small one otherwise
        got = be.dpt_tail(xx, packed, cout)
        assert bitwise(got, uu[:, pi[chans]]), (cout, chans)


# ------------------------------------------- 4. strides, slots, plumbing --
def test_padded_batch_strides_on_x_and_out(cases, be, dev):
    c = cases["a"]
    B, _, Hi, Wi = c["x"].shape
    n_in, n_out = C * Hi * Wi, 4 * 4 * Hi * Wi
    xbuf = torch.full((B, n_in + 24), float("nan"), device=dev)
    xbuf[:, :n_in] = c["xd"].reshape(B, -1)
    x = xbuf[:, :n_in].view(B, C, Hi, Wi)
    obuf = torch.full((B, n_out + 40), float("nan"), device=dev)
    out = obuf[:, :n_out].view(B, 4, 2 * Hi, 2 * Wi)
    assert x.stride(0) == n_in + 24 and out.stride(0) == n_out + 40
    assert be.dpt_tail(x, c["packed"], 4, out=out) is out
    assert bitwise(out, be.dpt_tail(c["xd"], c["packed"], 4))
    assert bool(obuf[:, n_out:].isnan().all())


def test_out_slot_of_a_nan_buffer_and_inputs_stay(cases, be, dev):
    c = cases["e"]
    B, _, Hi, Wi = c["x"].shape
    x0, p0 = c["xd"].clone(), c["packed"].clone()
    buf = torch.full((3, B, 4, 2 * Hi, 2 * Wi), float("nan"), device=dev)
    assert be.dpt_tail(c["xd"], c["packed"], 4, out=buf[1]) is not None
    assert frac(buf[1], c) <= 1.0
    assert bool(buf[0].isnan().all()) and bool(buf[2].isnan().all())  # the guard bands
    assert bitwise(c["xd"], x0) and bitwise(c["packed"], p0)


def test_fewer_outputs_from_weights_packed_for_fewer(cases, be, dev):
    """Cout = 1 and 3 from the fixture's first rows of w2 and b2: within the bound of those rows of the exact result."""
    c = cases["a"]
    w1, b1, w2, b2 = (t.to(dev) for t in c["w"])
    for cout in (1, 3):
        packed = be.dpt_tail_pack(w1, b1, w2[:cout].contiguous(), b2[:cout].contiguous())
        got = be.dpt_tail(c["xd"], packed, cout)
        assert got.shape[1] == cout and frac(got, c, slice(0, cout)) <= 1.0
        assert bitwise(got, be.dpt_tail(c["xd"], c["packed"], 4)[:, :cout])  # the order of the sums does not depend on Cout


def test_two_runs_agree_bitwise_and_side_stream(cases, be, dev):
    c = cases["e"]
    first = be.dpt_tail(c["xd"], c["packed"], 4)
    assert bitwise(be.dpt_tail(c["xd"], c["packed"], 4), first)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = be.dpt_tail(c["xd"], c["packed"], 4)
    side.synchronize()
    assert bitwise(got, first)


def test_inference_mode_no_allocation_one_launch_no_copy(cases, be, dev):
    from torch.profiler import ProfilerActivity, profile

    c = cases["a"]
    with torch.inference_mode():
        out = be.dpt_tail(c["xd"], c["packed"], 4)  # also the warm-up: the code object
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        assert be.dpt_tail(c["xd"], c["packed"], 4, out=out) is out
        assert torch.cuda.memory_allocated() == held
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                be.dpt_tail(c["xd"], c["packed"], 4, out=out)
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
        assert len(on_device) == 5, on_device  # nothing else: no MIOpen kernel, no copy, no fill
        assert not [n for n in on_device if "memcpy" in n.lower() or "memset" in n.lower() or "miopen" in n.lower()]
    if launches_api:
        assert len(launches_api) == 5, launches_api
    assert not copies_api, copies_api


# ------------------------------------------------------- 5. stand-in model --
def spy_on(be, calls):
    real = be.dpt_tail

    def spy(x, packed, cout, **kw):
        out = real(x, packed, cout, **kw)
        calls.append((x, out))
        return out

    be.dpt_tail = spy
    return real


def test_install_on_a_stand_in_stack(be, dev):
    """An adapter whose head is [Conv2d(8 -> 128, 3x3) real, then the four fused
    modules]. The kernel's result is checked where it happens: within
    dpt_tail_ref.bound of dpt_tail_exact on exactly the tensor it was handed
    (seq[0]'s output) and the Sequential's own weights."""
    from mast3r_slam_amd import dpt

    torch.manual_seed(51)
    adapter = ref.DPTOutputAdapter().to(dev).eval()
    plain = copy.deepcopy(adapter)
    seq = adapter.head
    assert dpt.install(adapter) == 1 and dpt.install(adapter) == 0
    x = torch.randn(2, 8, 6, 9, device=dev)
    calls = []
    real = spy_on(be, calls)
    try:
        with torch.no_grad():
            got = adapter(x)
            assert len(calls) == 1 and got is calls[0][1]
            handed = calls[0][0]
            assert bitwise(handed, plain.head[0](x)) and tuple(got.shape) == (2, 4, 12, 18)
            w = [t.detach().cpu() for t in (seq[2].weight, seq[2].bias, seq[4].weight, seq[4].bias)]
            f = ref.fraction(got.cpu(), handed.cpu(), *w)
            fp = ref.fraction(plain(x).cpu(), handed.cpu(), *w)
            print(f"install: max |device - exact| / bound = {f:.3g} (torch's own four modules: {fp:.3g})")
            assert f <= 1.0

            # channels_last: the original forward, no kernel call
            xc = x.to(memory_format=torch.channels_last)
            assert not xc.is_contiguous()
            y = adapter(xc)
            assert len(calls) == 1
            # both are torch's own modules on the same weights; its convolution may pick another
            # algorithm from one call to the next, so they are held to the derived bound, not bitwise
            handed_c = plain.head[0](xc).contiguous().cpu()
            assert ref.fraction(y.cpu(), handed_c, *w) <= 1.0 and ref.fraction(plain(xc).cpu(), handed_c, *w) <= 1.0
            # autocast and a needed gradient likewise
            with torch.autocast("cuda", dtype=torch.float16):
                adapter(x)
            assert len(calls) == 1
        adapter(x.clone().requires_grad_()).sum().backward()
        assert len(calls) == 1

        # load_state_dict after install repacks: the cache follows the parameters
        with torch.no_grad():
            packed0 = vars(seq)["_m3s_dpt_packed"][1]
            adapter(x)
            assert vars(seq)["_m3s_dpt_packed"][1] is packed0  # cached between calls
            other = ref.DPTOutputAdapter().to(dev)
            adapter.load_state_dict(other.state_dict())
            got2 = adapter(x)
            assert len(calls) == 3 and vars(seq)["_m3s_dpt_packed"][1] is not packed0
            w = [t.detach().cpu() for t in (other.head[2].weight, other.head[2].bias, other.head[4].weight,
                                            other.head[4].bias)]
            assert ref.fraction(got2.cpu(), calls[2][0].cpu(), *w) <= 1.0
            assert not torch.equal(got2, got)
    finally:
        be.dpt_tail = real


class Head(torch.nn.Module):
    """A catmlp+dpt head stand-in for head.install whose `dpt` is the adapter stand-in:
    patch size 2, so the decoder tokens are the adapter's [B,8,H/2,W/2] input."""

    def __init__(self, feat=5):
        super().__init__()
        self.dpt = ref.DPTOutputAdapter()
        self.head_local_features = torch.nn.Linear(6 + 8, (feat + 1) * 4)
        self.patch_size, self.local_feat_dim, self.two_confs = 2, feat, True
        self.depth_mode, self.conf_mode = ("exp", -float("inf"), float("inf")), ("exp", 1.0, float("inf"))
        self.desc_conf_mode, self.desc_mode = ("exp", 0.0, float("inf")), "norm"
        self.postprocess = True
        real = self.dpt.forward

        def dpt_forward(decout, image_size=None):  # tokens [B,S,8] -> path_1 [B,8,H/2,W/2]
            H, W = image_size
            return real(decout[-1].transpose(1, 2).reshape(-1, 8, H // 2, W // 2).contiguous())

        self.dpt.forward = dpt_forward


class Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.downstream_head1 = Head()


@pytest.mark.parametrize("order", ["dpt first", "head first"])
def test_composes_with_head_install(be, dev, order):
    from mast3r_slam_amd import dpt, head

    torch.manual_seed(52)
    model = Model().to(dev).eval()
    h = model.downstream_head1
    H, W = 8, 12
    decout = [torch.randn(1, 24, 6, device=dev), torch.randn(1, 24, 8, device=dev)]
    with torch.no_grad():
        pts = h.dpt.head[0](decout[-1].transpose(1, 2).reshape(1, 8, H // 2, W // 2).contiguous())
        w = [t.detach() for t in (h.dpt.head[2].weight, h.dpt.head[2].bias, h.dpt.head[4].weight, h.dpt.head[4].bias)]
        want_pts = be.dpt_tail(pts, be.dpt_tail_pack(*w), 4)
        feat = h.head_local_features(torch.cat([decout[0], decout[-1]], dim=-1))
        want = be.head_postprocess(want_pts, feat.contiguous(), 2, 5)
    installs = (dpt.install, head.install) if order == "dpt first" else (head.install, dpt.install)
    assert [f(model) for f in installs] == [1, 1]
    calls = []
    real = spy_on(be, calls)
    try:
        with torch.no_grad():
            res = h(decout, (H, W))
    finally:
        be.dpt_tail = real
    assert len(calls) == 1 and bitwise(calls[0][1], want_pts)
    for key, t in zip(("pts3d", "conf", "desc", "desc_conf"), want):
        assert bitwise(res[key], t), key

"""m3s_head_postprocess on the device (include/m3s_head.h) against
tests/head_ref.py: the fp64 statement of the function and the derived tolerance
of an fp32 evaluation. The fixtures of tests/golden/make_head_golden.py supply
the raw inputs (tests/test_head_ref.py ties head_ref to the reference's own
output on them); nothing here reads the reference."""
import math
import os

import numpy as np
import pytest
import torch

import head_ref

pytestmark = pytest.mark.gpu

FIXTURES = ("a", "b", "c", "d", "e")
PATCH = ("a", "b", "e")  # P = 16, F = 24: the patch kernel takes them
KEYS = ("X", "C", "D", "Q")
INF = float("inf")


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
    """{name: pts, feat on the device, P, F, conf, desc_conf, and the fp64
    exact result and fp32 bounds}; computed once, not written to."""
    out = {}
    for name in FIXTURES:
        z = np.load(os.path.join(golden_dir, f"head_{name}.npz"))
        c = {"P": int(z["P"]), "F": int(z["F"]), "conf": tuple(float(v) for v in z["conf"]),
             "desc_conf": tuple(float(v) for v in z["desc_conf"])}
        args = (z["pts"], z["feat"], c["P"], c["F"], c["conf"], c["desc_conf"])
        c["exact"], c["bounds"] = head_ref.head_exact(*args), head_ref.bounds(*args)
        c["pts"], c["feat"] = torch.from_numpy(z["pts"]).to(dev), torch.from_numpy(z["feat"]).to(dev)
        out[name] = c
    return out


def run(be, c, **kw):
    kw.setdefault("conf", c["conf"])
    kw.setdefault("desc_conf", c["desc_conf"])
    return be.head_postprocess(c["pts"], c["feat"], c["P"], c["F"], **kw)


def bitwise(a, b):
    """Equal bit for bit, NaN included."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def within(got, exact, tol, label):
    for key, g in zip(KEYS, got):
        ok, worst = head_ref.compare(g.float().cpu().numpy(), exact[key], tol[key])
        print(f"{label} {key}: max |device - exact| / bound = {worst:.3f}")
        assert ok, (label, key, worst)


@pytest.mark.parametrize("name,generic", [(n, False) for n in PATCH] + [(n, True) for n in FIXTURES])
def test_fp32_within_bound_of_exact(cases, be, name, generic):
    c = cases[name]
    got = run(be, c, generic=generic)
    H, W = c["pts"].shape[2:]
    assert [tuple(g.shape[1:]) for g in got] == [(H, W, 3), (H, W), (H, W, c["F"]), (H, W)]
    assert all(g.dtype == torch.float32 and g.is_contiguous() for g in got)
    within(got, c["exact"], c["bounds"], f"head_{name} {'generic' if generic else 'patch'}")


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("name", PATCH)
def test_generic_equals_patch_kernel_bitwise(cases, be, name, dt):
    dtype = {"f32": torch.float32, "f16": torch.float16}[dt]
    fast = run(be, cases[name], desc_dtype=dtype)
    slow = run(be, cases[name], desc_dtype=dtype, generic=True)
    for key, a, b in zip(KEYS, fast, slow):
        assert bitwise(a, b), key


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("name", ("a", "c", "e"))
def test_fp16_descriptors_are_the_fp32_ones_rounded_once(cases, be, name, generic):
    c = cases[name]
    X32, C32, D32, Q32 = run(be, c, generic=generic)
    X16, C16, D16, Q16 = run(be, c, generic=generic, desc_dtype=torch.float16)
    assert D16.dtype == torch.float16 and bitwise(D16, D32.half())
    assert bitwise(X16, X32) and bitwise(C16, C32) and bitwise(Q16, Q32)
    tol = head_ref.bounds(c["pts"].cpu().numpy(), c["feat"].cpu().numpy(), c["P"], c["F"], c["conf"], c["desc_conf"],
                          desc_half=True)
    ok, worst = head_ref.compare(D16.float().cpu().numpy(), c["exact"]["D"], tol["D"])
    print(f"head_{name} f16 D: max |device - exact| / bound = {worst:.3f}")
    assert ok, worst


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("ds", [2, 3])
def test_downsample_is_the_strided_full_result_bitwise(cases, be, ds, dt):
    c = cases["a"]  # 32 x 48: 16 x 24 at ds = 2, 11 x 16 at ds = 3
    dtype = {"f32": torch.float32, "f16": torch.float16}[dt]
    full = run(be, c, desc_dtype=dtype)
    sub = run(be, c, desc_dtype=dtype, downsample=ds)
    assert tuple(sub[1].shape) == (2, -(-32 // ds), -(-48 // ds))
    for key, f, s in zip(KEYS, full, sub):
        assert s.is_contiguous() and bitwise(s, f[:, ::ds, ::ds].contiguous()), key


SENTINEL = -7.0


def stacked(dev, n, B, h, w, F, dtype, guard=64):
    """Stacked [n,B,h,w,.] X, C, D, Q buffers, each cut out of a flat
    sentinel-filled allocation with `guard` elements on either side."""
    flats, bufs = [], []
    for tail, dt in (((3,), torch.float32), ((), torch.float32), ((F,), dtype), ((), torch.float32)):
        shape = (n, B, h, w) + tail
        flat = torch.full((2 * guard + math.prod(shape),), SENTINEL, dtype=dt, device=dev)
        flats.append(flat)
        bufs.append(flat[guard:flat.numel() - guard].view(shape))
    return flats, bufs


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("name,ds", [("a", 1), ("a", 2), ("c", 1)])
def test_out_slots_of_a_stacked_buffer(cases, be, dev, name, ds, dt):
    c, dtype = cases[name], {"f32": torch.float32, "f16": torch.float16}[dt]
    B, _, H, W = c["pts"].shape
    want = run(be, c, desc_dtype=dtype, downsample=ds)
    flats, bufs = stacked(dev, 4, B, -(-H // ds), -(-W // ds), c["F"], dtype)
    for k in (2, 0):
        got = run(be, c, desc_dtype=dtype, downsample=ds, out=tuple(buf[k] for buf in bufs))
        assert all(g.data_ptr() == buf[k].data_ptr() for g, buf in zip(got, bufs))
    for key, buf, flat, w_ in zip(KEYS, bufs, flats, want):
        assert bitwise(buf[2], w_) and bitwise(buf[0], w_), key
        assert bool((buf[1] == SENTINEL).all()) and bool((buf[3] == SENTINEL).all()), key
        assert bool((flat[:64] == SENTINEL).all()) and bool((flat[-64:] == SENTINEL).all()), key


@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("which", ["X", "D", "both"])
def test_misaligned_out_takes_the_generic_path_and_stays_correct(cases, be, dev, which, dt):
    c, dtype = cases["a"], {"f32": torch.float32, "f16": torch.float16}[dt]
    B, _, H, W = c["pts"].shape
    want = run(be, c, desc_dtype=dtype)
    shapes = ((B, H, W, 3), (B, H, W), (B, H, W, c["F"]), (B, H, W))
    off = {"X": (1, 0, 0, 0), "D": (0, 0, 3, 0), "both": (3, 1, 1, 1)}[which]  # elements: never 16 bytes
    flats = [torch.full((math.prod(s) + 8,), SENTINEL, dtype=w_.dtype, device=dev) for s, w_ in zip(shapes, want)]
    out = tuple(f[o:o + math.prod(s)].view(s) for f, o, s in zip(flats, off, shapes))
    assert all(f.data_ptr() % 16 == 0 for f in flats) and (out[0].data_ptr() % 16 or out[2].data_ptr() % 16)
    run(be, c, desc_dtype=dtype, out=out)
    for key, o, f, of, w_ in zip(KEYS, out, flats, off, want):
        assert bitwise(o, w_), key
        assert bool((f[:of] == SENTINEL).all()) and bool((f[of + o.numel():] == SENTINEL).all()), key


def test_padded_batch_stride(cases, be, dev):
    """Rows of a wider buffer: every image contiguous, the batch stride one
    element more than an image (not a multiple of 16 bytes), the padding stays."""
    c = cases["a"]
    B, _, H, W = c["pts"].shape
    want = run(be, c)
    wide = [torch.full((B, w_[0].numel() + 1), SENTINEL, device=dev) for w_ in want]
    out = tuple(b[:, :-1].view(w_.shape) for b, w_ in zip(wide, want))
    assert out[2].stride(0) == H * W * c["F"] + 1
    run(be, c, out=out)
    for key, o, b, w_ in zip(KEYS, out, wide, want):
        assert bitwise(o, w_) and bool((b[:, -1] == SENTINEL).all()), key


@pytest.mark.parametrize("generic", [False, True])
def test_special_values_by_class_and_position(cases, be, generic):
    c = dict(cases["a"])
    B, _, H, W = c["pts"].shape
    P, F = c["P"], c["F"]
    pts, feat = c["pts"].clone(), c["feat"].clone()

    def lf(b, y, x):
        """The feat elements of pixel (b, y, x): [F + 1] flat indices into feat[b, s]."""
        return b, (y // P) * (W // P) + x // P, torch.arange(F + 1) * P * P + (y % P) * P + x % P

    pts[0, :3, 5, 7] = 0.0                                   # zero point
    pts[1, 3, 17, 40], pts[1, 3, 31, 47] = 100.0, -100.0      # raw confidence
    b, s, idx = lf(1, 20, 33)
    feat[b, s, idx[:F]] = 0.0                                 # zero descriptor
    b, s, idx = lf(0, 31, 0)
    feat[b, s, idx[F]] = 100.0                                # raw descriptor confidence
    b, s, idx = lf(0, 16, 16)
    feat[b, s, idx[F]] = -100.0
    b, s, idx = lf(1, 0, 47)
    feat[b, s, idx[3]] = float("nan")                         # one NaN channel poisons its pixel's descriptor only
    c["pts"], c["feat"] = pts, feat
    X, C, D, Q = run(be, c, generic=generic)
    assert bool((X[0, 5, 7] == 0).all()) and int((X == 0).sum()) == 3
    assert bool(D[1, 20, 33].isnan().all()) and bool(D[1, 0, 47].isnan().all()) and int(D.isnan().sum()) == 2 * F
    assert not bool(X.isnan().any() | C.isnan().any() | Q.isnan().any())
    assert float(C[1, 17, 40]) == INF and int(C.isinf().sum()) == 1 and float(C[1, 31, 47]) == 1.0
    assert float(Q[0, 31, 0]) == INF and int(Q.isinf().sum()) == 1 and 0.0 <= float(Q[0, 16, 16]) <= 2.0 ** -126
    args = (pts.cpu().numpy(), feat.cpu().numpy(), P, F, c["conf"], c["desc_conf"])
    within((X, C, D, Q), head_ref.head_exact(*args), head_ref.bounds(*args), f"special generic={generic}")
    # a NaN raw confidence stays NaN through the min
    pts[0, 3, 2, 2] = float("nan")
    C2 = run(be, c, generic=generic, conf=(1.0, 5.0))[1]
    assert bool(C2[0, 2, 2].isnan()) and int(C2.isnan().sum()) == 1


@pytest.mark.parametrize("name,generic", [("b", False), ("b", True), ("c", True)])
def test_a_finite_vmax_clips(cases, be, name, generic):
    c = cases[name]
    modes = dict(conf=(1.0, 2.5), desc_conf=(0.25, 1.0))
    X, C, D, Q = got = run(be, c, generic=generic, **modes)
    assert float(C.max()) == 2.5 and float(Q.max()) == 1.0 and float(C.min()) > 1.0 and float(Q.min()) > 0.25
    assert 0.1 < float((C == 2.5).float().mean()) < 0.9 and 0.1 < float((Q == 1.0).float().mean()) < 0.9
    args = (c["pts"].cpu().numpy(), c["feat"].cpu().numpy(), c["P"], c["F"], modes["conf"], modes["desc_conf"])
    within(got, head_ref.head_exact(*args), head_ref.bounds(*args), f"head_{name} clipped")


def test_side_stream_no_allocation_one_launch(cases, be, dev):
    from torch.profiler import ProfilerActivity, profile

    c = cases["a"]
    want = run(be, c, desc_dtype=torch.float16)
    out = tuple(torch.zeros_like(w_) for w_ in want)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run(be, c, desc_dtype=torch.float16, out=out)  # also the warm-up
        side.synchronize()
        held = torch.cuda.memory_allocated()
        run(be, c, desc_dtype=torch.float16, out=out)
        assert torch.cuda.memory_allocated() == held
        side.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                run(be, c, desc_dtype=torch.float16, out=out)
            side.synchronize()
    for key, o, w_ in zip(KEYS, out, want):
        assert bitwise(o, w_), key
    device_type = torch.autograd.DeviceType
    on_device = [e.name for e in prof.events() if e.device_type == device_type.CUDA]
    host = [e.name for e in prof.events() if e.device_type == device_type.CPU]
    copies_api = [n for n in host if n.startswith("hipMemcpy")]
    launches_api = [n for n in host if "LaunchKernel" in n]
    print("device records:", on_device, "runtime launches:", len(launches_api), "runtime copies:", copies_api)
    assert on_device or launches_api, "the profiler recorded neither device activity nor runtime calls"
    if on_device:  # the patch kernel, once per call, and nothing else
        assert len([n for n in on_device if "head_patch_kernel" in n]) == 5, on_device
        assert not [n for n in on_device if "memcpy" in n.lower() or "memset" in n.lower()], on_device
    if launches_api:
        assert len(launches_api) == 5, launches_api
    assert not copies_api, copies_api


@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_install_on_a_stand_in_model(be, dev, dt):
    """head1(decout, true_shape) of the switched model against the statement,
    evaluated on the very maps the model's dpt and MLP produced in that call
    (forward hooks record them), and against the plain-torch tail on them."""
    from mast3r_slam_amd import head as fused
    from test_head_abi import Model

    dtype = {"f32": torch.float32, "f16": torch.float16}[dt]
    torch.manual_seed(31)
    P, F, B, H, W = 16, 24, 2, 32, 48
    model = Model(common=dict(patch=P, feat=F)).to(dev)
    assert fused.install(model, desc_dtype=dtype) == 2
    gen = torch.Generator().manual_seed(32)
    S = (H // P) * (W // P)
    decout = [torch.randn(B, S, 6, generator=gen).to(dev), torch.randn(B, S, 10, generator=gen).to(dev)]
    true_shape = torch.tensor([[H, W]] * B)
    seen = {}
    head = model.downstream_head1
    hooks = [head.dpt.register_forward_hook(lambda m, i, o: seen.__setitem__("pts", o.detach().clone())),
             head.head_local_features.register_forward_hook(lambda m, i, o: seen.__setitem__("feat", o.detach().clone()))]
    with torch.inference_mode():
        res = model.head1(decout, true_shape)
    for h in hooks:
        h.remove()
    assert set(res) == {"pts3d", "conf", "desc", "desc_conf"}
    got = (res["pts3d"], res["conf"], res["desc"], res["desc_conf"])
    assert [tuple(g.shape) for g in got] == [(B, H, W, 3), (B, H, W), (B, H, W, F), (B, H, W)]
    assert res["desc"].dtype == dtype and res["pts3d"].dtype == torch.float32
    args = (seen["pts"].cpu().numpy(), seen["feat"].cpu().numpy(), P, F, (1.0, INF), (0.0, INF))
    exact, tol = head_ref.head_exact(*args), head_ref.bounds(*args, desc_half=dtype == torch.float16)
    within(got, exact, tol, f"install {dt}")
    plain = head_ref.head_torch(seen["pts"], seen["feat"], H, W, P, F)
    within(plain, exact, head_ref.bounds(*args), "plain torch tail")
    for key, g, p in zip(KEYS, got, plain):  # two fp32 evaluations, each within the bound of the exact value
        assert bool(((g.double() - p.double()).abs().cpu() <= 2 * torch.from_numpy(tol[key])).all()), key


def test_decode_pair_into_stacked_slots(cases, be, dev):
    """Two views into slots 1 and 0 of stacked, downsampled buffers; the head is
    any object with the attributes (here its dpt and MLP hand back fixed maps)."""
    import types

    from mast3r_slam_amd import head as fused

    c = cases["a"]
    B, _, H, W = c["pts"].shape
    P, F, ds = c["P"], c["F"], 2
    S = (H // P) * (W // P)
    decout = [torch.zeros(B, S, 2, device=dev), torch.zeros(B, S, 3, device=dev)]
    bufs = fused.alloc_views(2, B, (H, W), F, dev, downsample=ds)
    assert [tuple(b.shape) for b in bufs] == [(2, B, 16, 24, 3), (2, B, 16, 24), (2, B, 16, 24, F), (2, B, 16, 24)]
    assert bufs[2].dtype == torch.float16
    for k, scale in ((1, 1.0), (0, 0.5)):
        pts, feat = c["pts"] * scale, c["feat"] * scale
        head = types.SimpleNamespace(
            dpt=lambda decout, image_size, _p=pts: _p, head_local_features=lambda x, _f=feat: _f, patch_size=P,
            local_feat_dim=F, two_confs=True, depth_mode=("exp", -INF, INF), conf_mode=("exp", 1.0, INF),
            desc_conf_mode=("exp", 0.0, INF), desc_mode="norm", postprocess=True)
        slot = fused.decode_pair_into(bufs, k, head, decout, (H, W), downsample=ds)
        res = fused.fused_head_forward(head, decout, (H, W), desc_dtype=torch.float16)
        full = (res["pts3d"], res["conf"], res["desc"], res["desc_conf"])
        for key, s_, buf, f in zip(KEYS, slot, bufs, full):
            assert s_.data_ptr() == buf[k].data_ptr() and bitwise(buf[k], f[:, ::ds, ::ds].contiguous()), (k, key)
    assert not bitwise(bufs[0][0], bufs[0][1])

"""CPU-side checks of the head-tail C ABI (no GPU needed), by the method of
tests/test_rope_abi.py: the ctypes mirror of m3s_head_args has exactly the C
layout (a gcc-compiled probe prints sizeof / offsetof from the header), the
header's symbols are be.HEAD_EXPORTS and in the library, every documented
M3S_EINVAL condition is refused with a null stream and no device, the Python
wrapper refuses what it cannot take and names it, and head.install switches the
right heads of a stand-in model."""
import ctypes
import functools
import math

import abi_probe
import pytest
import torch

FIELDS = ("pts", "feat", "X", "C", "D", "Q", "B", "H", "W", "P", "F", "ds", "sbX", "sbC", "sbD", "sbQ",
          "conf_vmin", "conf_vmax", "dconf_vmin", "dconf_vmax", "desc_dtype", "flags")


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


def test_ctypes_mirror_matches_header(be):
    assert tuple(n for n, _ in be.HeadArgs._fields_) == FIELDS
    got = abi_probe.probe(["m3s_head.h"], {"m3s_head_args": be.HeadArgs},
                          ["M3S_HEAD_F32", "M3S_HEAD_F16", "M3S_HEAD_GENERIC"])
    assert (got["M3S_HEAD_F32"], got["M3S_HEAD_F16"], got["M3S_HEAD_GENERIC"]) == (be.HEAD_F32, be.HEAD_F16, be.HEAD_GENERIC)


def test_header_symbols_are_head_exports(be):
    declared = abi_probe.declared_symbols("m3s_head.h")
    assert declared == set(be.HEAD_EXPORTS) == {"m3s_head_postprocess"}
    for sym in be.HEAD_EXPORTS:
        assert hasattr(be._lib, sym), sym
    assert not set(be.HEAD_EXPORTS) & (set(be.EXPORTS) | set(be.RETRIEVAL_EXPORTS) | set(be.ROPE_EXPORTS))


def good_args(be, keep):
    """A record that passes every check: one 512 x 384 view into dense outputs
    (the pointers are never followed: every call below is refused before a
    launch)."""
    buf = (ctypes.c_char * 64)()
    keep.append(buf)
    a = be.HeadArgs()
    a.pts = a.feat = a.X = a.C = a.D = a.Q = ctypes.addressof(buf)
    a.B, a.H, a.W, a.P, a.F, a.ds = 1, 384, 512, 16, 24, 1
    hw = 384 * 512
    a.sbX, a.sbC, a.sbD, a.sbQ = 3 * hw, hw, 24 * hw, hw
    a.conf_vmin, a.conf_vmax, a.dconf_vmin, a.dconf_vmax = 1.0, math.inf, 0.0, math.inf
    a.desc_dtype, a.flags = be.HEAD_F16, 0
    return a


HW2 = 192 * 256  # one image at ds = 2
EINVAL_CASES = {
    **{f"null {p}": {p: None} for p in ("pts", "feat", "X", "C", "D", "Q")},
    **{f"{n} = 0": {n: 0} for n in ("B", "H", "W", "P", "F", "ds")},
    **{f"{n} < 0": {n: -1} for n in ("B", "H", "W", "P", "F", "ds")},
    "H % P": dict(H=392), "W % P": dict(W=520), "P = 5": dict(P=5),
    "sbX one short": dict(sbX=3 * 384 * 512 - 1), "sbC one short": dict(sbC=384 * 512 - 1),
    "sbD one short": dict(sbD=24 * 384 * 512 - 1), "sbQ one short": dict(sbQ=384 * 512 - 1),
    "sbX = 0": dict(sbX=0), "sbD < 0": dict(sbD=-24 * 384 * 512),
    "ds = 2, sbD one short": dict(ds=2, sbX=3 * HW2, sbC=HW2, sbD=24 * HW2 - 1, sbQ=HW2),
    "ds = 3, sbC one short": dict(ds=3, sbC=128 * 171 - 1),  # Ho = 128, Wo = ceil(512 / 3) = 171
    "B H W = 2^31": dict(B=1 << 13, H=512, W=512, sbX=1 << 40, sbC=1 << 40, sbD=1 << 40, sbQ=1 << 40),
    "B H W overflows int64": dict(B=1 << 62, H=1 << 62, W=1 << 62, P=2),
    "F + 1 overflows": dict(F=(1 << 63) - 1), "(F + 1) P^2 = 2^31": dict(F=(1 << 23) - 1, sbD=1 << 60),
    "conf_vmin -inf": dict(conf_vmin=-math.inf), "conf_vmin nan": dict(conf_vmin=math.nan),
    "dconf_vmin inf": dict(dconf_vmin=math.inf), "dconf_vmin nan": dict(dconf_vmin=math.nan),
    "conf_vmax < vmin": dict(conf_vmax=0.5), "conf_vmax nan": dict(conf_vmax=math.nan),
    "dconf_vmax < vmin": dict(dconf_vmax=-1.0), "dconf_vmax nan": dict(dconf_vmax=math.nan),
    "desc_dtype 2": dict(desc_dtype=2), "desc_dtype -1": dict(desc_dtype=-1),
    "flags 2": dict(flags=2), "flags 1 | 4": dict(flags=5), "flags < 0": dict(flags=-1),
}


@pytest.mark.parametrize("what", sorted(EINVAL_CASES))
def test_head_refuses_before_any_launch(be, what):
    keep = []
    a = good_args(be, keep)
    for k, v in EINVAL_CASES[what].items():
        setattr(a, k, v)
    assert be._lib.m3s_head_postprocess(ctypes.byref(a), None) == be.M3S_EINVAL


def test_null_record_refused(be):
    assert be._lib.m3s_head_postprocess(None, None) == be.M3S_EINVAL


def test_wrapper_refusals(be):
    P, F, B, H, W = 4, 5, 2, 8, 12
    pts = torch.zeros(B, 4, H, W)
    feat = torch.zeros(B, 6, (F + 1) * P * P)
    hp = functools.partial(be.head_postprocess, patch_size=P, desc_dim=F)
    with pytest.raises(RuntimeError, match="pts must be on a ROCm device"):
        hp(pts, feat)
    with pytest.raises(RuntimeError, match="pts must be a tensor"):
        hp(None, feat)
    with pytest.raises(RuntimeError, match="feat must be torch.float32"):
        hp(pts, feat.half())
    with pytest.raises(RuntimeError, match="pts must be contiguous"):
        hp(torch.zeros(B, 4, W, H).transpose(2, 3), feat)
    with pytest.raises(RuntimeError, match=r"pts must be \[B, 4, H, W\]"):
        hp(torch.zeros(B, 3, H, W), feat)
    with pytest.raises(RuntimeError, match="multiples of patch_size"):
        hp(torch.zeros(B, 4, H + 2, W), feat)
    with pytest.raises(RuntimeError, match=r"feat must be \[2, 6, 96\]"):
        hp(pts, feat[:, :5].contiguous())
    with pytest.raises(RuntimeError, match=r"feat must be \[2, 6, 112\]"):
        be.head_postprocess(pts, feat, P, F + 1)
    for name in ("patch_size", "desc_dim", "downsample"):
        kw = dict(patch_size=P, desc_dim=F, downsample=1)
        kw[name] = 0
        with pytest.raises(RuntimeError, match=f"{name} must be >= 1"):
            be.head_postprocess(pts, feat, **kw)
    with pytest.raises(RuntimeError, match="desc_dtype must be float32 or float16"):
        hp(pts, feat, desc_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="desc_conf must be"):
        hp(pts, feat, desc_conf=(0.0, -1.0))
    with pytest.raises(RuntimeError, match="conf must be"):
        hp(pts, feat, conf=(-math.inf, math.inf))
    with pytest.raises(RuntimeError, match="conf must be"):
        hp(pts, feat, conf=(1.0, math.nan))
    with pytest.raises(RuntimeError, match="conf must be"):
        hp(pts, feat, conf=("exp", 1.0, math.inf))

    def outs(ds=1, dtype=torch.float32):
        h, w = -(-H // ds), -(-W // ds)
        return [torch.zeros(B, h, w, 3), torch.zeros(B, h, w), torch.zeros(B, h, w, F, dtype=dtype), torch.zeros(B, h, w)]

    with pytest.raises(RuntimeError, match=r"out must be \(X, C, D, Q\)"):
        hp(pts, feat, out=outs()[:3])
    with pytest.raises(RuntimeError, match="out Q must be a tensor"):
        hp(pts, feat, out=outs()[:3] + [None])
    with pytest.raises(RuntimeError, match=r"out X must be \[2, 4, 6, 3\]"):  # the downsampled shape is asked for
        hp(pts, feat, downsample=2, out=outs())
    with pytest.raises(RuntimeError, match=r"out C must be \[2, 3, 4\]"):
        hp(pts, feat, downsample=3, out=[outs(3)[0]] + outs(2)[1:])
    with pytest.raises(RuntimeError, match="out D must be torch.float16"):
        hp(pts, feat, desc_dtype=torch.float16, out=outs())
    with pytest.raises(RuntimeError, match="out D must be torch.float32"):
        hp(pts, feat, out=outs(dtype=torch.float16))
    o = outs()
    o[0] = torch.zeros(B, H, W, 6)[..., ::2]
    with pytest.raises(RuntimeError, match="out X: every image must be contiguous"):
        hp(pts, feat, out=o)
    o = outs()
    o[1] = torch.zeros(1, H, W).expand(B, H, W)
    with pytest.raises(RuntimeError, match="out C: the images overlap"):
        hp(pts, feat, out=o)
    with pytest.raises(RuntimeError, match="pts must be on a ROCm device"):  # all else in order: the device is what is left
        hp(pts, feat, out=outs())


# ------------------------------------------------------------ install ---
class Dpt(torch.nn.Module):
    """[B,S,C] tokens -> [B,4,H,W]: a tiny stand-in for the DPT."""

    def __init__(self, dim, patch):
        super().__init__()
        self.patch = patch
        self.proj = torch.nn.Linear(dim, 4 * patch * patch)

    def forward(self, decout, image_size):
        H, W = image_size
        B = decout[-1].shape[0]
        x = self.proj(decout[-1]).transpose(-1, -2).reshape(B, -1, H // self.patch, W // self.patch)
        return torch.nn.functional.pixel_shuffle(x, self.patch)


class Head(torch.nn.Module):
    """The attributes install looks for; its own forward is not the fused one."""

    def __init__(self, enc=6, dec=10, patch=4, feat=5, conf_mode=("exp", 1.0, math.inf), postprocess=True):
        super().__init__()
        self.dpt = Dpt(dec, patch)
        self.head_local_features = torch.nn.Linear(enc + dec, (feat + 1) * patch * patch)
        self.patch_size, self.local_feat_dim, self.two_confs = patch, feat, True
        self.depth_mode, self.conf_mode = ("exp", -math.inf, math.inf), conf_mode
        self.desc_conf_mode, self.desc_mode = ("exp", 0.0, math.inf), "norm"
        self.postprocess = postprocess

    def forward(self, decout, img_shape):
        return "plain"


def call_head(head, decout, true_shape):
    H, W = true_shape[0].tolist()
    return head(decout, (H, W))


class Model(torch.nn.Module):
    """downstream_head1 / 2 and the partials that captured them; `common` goes
    to both heads, `head2` to the second only."""

    def __init__(self, common=None, head2=None):
        super().__init__()
        self.downstream_head1 = Head(**(common or {}))
        self.downstream_head2 = Head(**{**(common or {}), **(head2 or {})})
        self.head1 = functools.partial(call_head, self.downstream_head1)
        self.head2 = functools.partial(call_head, self.downstream_head2)


def test_install_switches_the_captured_heads():
    from mast3r_slam_amd import head as fused

    model = Model()
    h1, h2, f1 = model.downstream_head1, model.downstream_head2, model.head1
    assert fused.install(model) == 2
    assert model.downstream_head1 is h1 and model.head1 is f1 and f1.args[0] is h1  # the captured object itself
    decout = [torch.zeros(1, 6, 6), torch.zeros(1, 6, 10)]
    shape = torch.tensor([[8, 12]])
    for head_fn in (model.head1, model.head2):  # the partial now reaches the kernel wrapper, which has no CPU path
        with pytest.raises(RuntimeError, match="pts must be on a ROCm device"):
            head_fn(decout, shape)
    assert fused.install(model) == 0  # nothing left to switch
    assert fused.install(model, desc_dtype=torch.float16) == 0


@pytest.mark.parametrize("what", ["sigmoid conf", "no postprocess", "one conf", "linear depth", "missing attribute"])
def test_install_leaves_other_heads_alone(what):
    from mast3r_slam_amd import head as fused

    model = Model(head2={"sigmoid conf": dict(conf_mode=("sigmoid", 0, 1)), "no postprocess": dict(postprocess=None)}.get(what))
    h2 = model.downstream_head2
    if what == "one conf":
        h2.two_confs = False
    elif what == "linear depth":
        h2.depth_mode = ("linear", -math.inf, math.inf)
    elif what == "missing attribute":
        del h2.local_feat_dim
    assert fused.install(model) == 1
    decout = [torch.zeros(1, 6, 6), torch.zeros(1, 6, 10)]
    assert model.head2(decout, torch.tensor([[8, 12]])) == "plain"
    assert "forward" not in vars(h2)
    with pytest.raises(RuntimeError, match="ROCm device"):
        model.head1(decout, torch.tensor([[8, 12]]))


def test_fused_forward_refuses_an_unsupported_head():
    from mast3r_slam_amd import head as fused

    with pytest.raises(RuntimeError, match="not a catmlp\\+dpt head"):
        fused.fused_head_forward(Head(conf_mode=("sigmoid", 0, 1)), [torch.zeros(1, 6, 6), torch.zeros(1, 6, 10)], (8, 12))

"""CPU-side checks of the DPT-tail C ABI (no GPU needed), by the method of
tests/test_head_abi.py: the ctypes mirror of m3s_dpt_tail_args has exactly the C
layout (a gcc-compiled probe prints sizeof / offsetof from the header), the
header's symbols are be.DPT_EXPORTS, in the library with their signatures and
in no other export list, every documented M3S_EINVAL condition is refused with
a null stream and no device, the Python wrappers refuse what they cannot take
and name it, and dpt.install patches the right Sequential of a stand-in model."""
import copy
import ctypes

import abi_probe
import pytest
import torch

import dpt_tail_ref as ref

FIELDS = ("x", "packed", "out", "B", "Hi", "Wi", "Cout", "x_sb", "out_sb", "flags")
SYMBOLS = {"m3s_dpt_tail_packed_size", "m3s_dpt_tail_pack", "m3s_dpt_tail"}
PACKED_BYTES = 4 * (9 * 128 * 128 + 128 + 4 * 128 + 4)  # w1, b1, w2 and b2 padded to 4 rows


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


def test_ctypes_mirror_matches_header(be):
    assert tuple(n for n, _ in be.DptTailArgs._fields_) == FIELDS
    macros = ["M3S_DPT_CH", "M3S_DPT_MAX_COUT", "M3S_DPT_TILE_H", "M3S_DPT_TILE_W", "M3S_DPT_MAX_SIDE"]
    got = abi_probe.probe(["m3s_dpt.h"], {"m3s_dpt_tail_args": be.DptTailArgs}, macros)
    assert [got[m] for m in macros] == [be.DPT_CH, be.DPT_MAX_COUT, be.DPT_TILE_H, be.DPT_TILE_W, be.DPT_MAX_SIDE]


def test_header_symbols_are_dpt_exports(be):
    declared = abi_probe.declared_symbols("m3s_dpt.h")
    assert declared == set(be.DPT_EXPORTS) == SYMBOLS
    others = (set(be.EXPORTS) | set(be.RETRIEVAL_EXPORTS) | set(be.ROPE_EXPORTS) | set(be.ATTN_EXPORTS)
              | set(be.HEAD_EXPORTS))
    assert not set(be.DPT_EXPORTS) & others
    lib = be._load()  # a fresh handle: the table's signatures are applied on load
    for sym in be.DPT_EXPORTS:
        assert hasattr(be._lib, sym), sym
        restype, argtypes = be.dpt._SIGNATURES[sym]
        fn = getattr(lib, sym)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), sym


def test_packed_size(be):
    assert [be.dpt_tail_packed_size(c) for c in (1, 2, 3, 4)] == [PACKED_BYTES] * 4
    assert [be.dpt_tail_packed_size(c) for c in (0, -1, 5, 1 << 40)] == [0] * 4
    assert PACKED_BYTES % 16 == 0


def aligned(keep, n=64):
    buf = (ctypes.c_char * (n + 16))()
    keep.append(buf)
    return (ctypes.addressof(buf) + 15) & ~15


def good_args(be, keep):
    """A record that passes every check: one 512 x 384 view (the pointers are
    never followed: every call below is refused before a launch)."""
    a = be.DptTailArgs()
    a.x = a.packed = a.out = aligned(keep)
    a.B, a.Hi, a.Wi, a.Cout = 1, 192, 256, 4
    a.x_sb, a.out_sb, a.flags = 128 * 192 * 256, 4 * 384 * 512, 0
    return a


BIG = 1 << 40
EINVAL_CASES = {
    **{f"null {p}": {p: None} for p in ("x", "packed", "out")},
    **{f"{n} = 0": {n: 0} for n in ("B", "Hi", "Wi", "Cout")},
    **{f"{n} < 0": {n: -1} for n in ("B", "Hi", "Wi", "Cout")},
    "Cout = 5": dict(Cout=5, out_sb=BIG),
    "Hi past the largest side": dict(Hi=(1 << 20) + 1, Wi=1, x_sb=BIG, out_sb=BIG),
    "Wi past the largest side": dict(Hi=1, Wi=(1 << 20) + 1, x_sb=BIG, out_sb=BIG),
    "x_sb one short": dict(x_sb=128 * 192 * 256 - 1), "out_sb one short": dict(out_sb=4 * 384 * 512 - 1),
    "out_sb of Cout = 3": dict(out_sb=3 * 384 * 512), "x_sb = 0": dict(x_sb=0), "out_sb < 0": dict(out_sb=-4 * 384 * 512),
    "B 128 Hi Wi = 2^31": dict(B=256, Hi=256, Wi=256, x_sb=BIG, out_sb=BIG),
    "B Hi Wi overflows int64": dict(B=1 << 62, Hi=1 << 20, Wi=1 << 20, x_sb=BIG, out_sb=BIG),
    "packed misaligned": dict(packed="+4"),
    "flags 1": dict(flags=1), "flags 2": dict(flags=2), "flags < 0": dict(flags=-1),
}


@pytest.mark.parametrize("what", sorted(EINVAL_CASES))
def test_dpt_tail_refuses_before_any_launch(be, what):
    keep = []
    a = good_args(be, keep)
    for k, v in EINVAL_CASES[what].items():
        setattr(a, k, a.packed + 4 if v == "+4" else v)
    assert be._lib.m3s_dpt_tail(ctypes.byref(a), None) == be.M3S_EINVAL


def test_largest_accepted_sizes_are_not_refused_by_the_size_checks(be):
    """The other side of the 2^31 limit: one element fewer passes every size check
    (and is then refused for a reason that is checked later: a flag)."""
    keep = []
    a = good_args(be, keep)
    a.B, a.Hi, a.Wi, a.x_sb, a.out_sb = 255, 256, 256, BIG, BIG
    a.flags = 1
    assert be._lib.m3s_dpt_tail(ctypes.byref(a), None) == be.M3S_EINVAL  # nothing is launched on a null stream here


def test_null_record_refused(be):
    assert be._lib.m3s_dpt_tail(None, None) == be.M3S_EINVAL


def test_pack_refuses_before_any_launch(be):
    keep = []
    p = aligned(keep)
    pack = be._lib.m3s_dpt_tail_pack
    for k in range(4):
        args = [p, p, p, p]
        args[k] = None
        assert pack(*args, 4, p, None) == be.M3S_EINVAL
    assert pack(p, p, p, p, 4, None, None) == be.M3S_EINVAL
    for cout in (0, -1, 5):
        assert pack(p, p, p, p, cout, p, None) == be.M3S_EINVAL
    assert pack(p, p, p, p, 4, p + 4, None) == be.M3S_EINVAL


def test_wrapper_refusals(be):
    B, Hi, Wi = 2, 3, 5
    x = torch.zeros(B, 128, Hi, Wi)
    packed = torch.zeros(PACKED_BYTES, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="x must be on a ROCm device"):
        be.dpt_tail(x, packed, 4)
    with pytest.raises(RuntimeError, match="x must be a tensor"):
        be.dpt_tail(None, packed, 4)
    with pytest.raises(RuntimeError, match="packed must be a tensor"):
        be.dpt_tail(x, None, 4)
    with pytest.raises(RuntimeError, match="x must be torch.float32"):
        be.dpt_tail(x.half(), packed, 4)
    with pytest.raises(RuntimeError, match="packed must be torch.uint8"):
        be.dpt_tail(x, packed.float(), 4)
    for cout in (0, 5):
        with pytest.raises(RuntimeError, match=f"cout = {cout}, only 1..4 are built"):
            be.dpt_tail(x, packed, cout)
    with pytest.raises(RuntimeError, match=r"x must be \[B, 128, Hi, Wi\]"):
        be.dpt_tail(torch.zeros(B, 64, Hi, Wi), packed, 4)
    with pytest.raises(RuntimeError, match=r"x must be \[B, 128, Hi, Wi\]"):
        be.dpt_tail(torch.zeros(128, Hi, Wi), packed, 4)
    with pytest.raises(RuntimeError, match="x: every image must be contiguous"):
        be.dpt_tail(x.to(memory_format=torch.channels_last), packed, 4)
    with pytest.raises(RuntimeError, match="x: the images overlap"):
        be.dpt_tail(torch.zeros(1, 128, Hi, Wi).expand(B, 128, Hi, Wi), packed, 4)
    with pytest.raises(RuntimeError, match=f"packed must be dpt_tail_pack's tensor of {PACKED_BYTES} bytes"):
        be.dpt_tail(x, packed[:-16], 4)
    with pytest.raises(RuntimeError, match="out must be a tensor"):
        be.dpt_tail(x, packed, 4, out=[1])
    with pytest.raises(RuntimeError, match=r"out must be \[2, 3, 6, 10\]"):
        be.dpt_tail(x, packed, 3, out=torch.zeros(B, 4, 6, 10))
    with pytest.raises(RuntimeError, match="out must be torch.float32"):
        be.dpt_tail(x, packed, 4, out=torch.zeros(B, 4, 6, 10, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="out: every image must be contiguous"):
        be.dpt_tail(x, packed, 4, out=torch.zeros(B, 4, 6, 20)[..., ::2])
    with pytest.raises(RuntimeError, match="out: the images overlap"):
        be.dpt_tail(x, packed, 4, out=torch.zeros(1, 4, 6, 10).expand(B, 4, 6, 10))
    with pytest.raises(RuntimeError, match="x must be on a ROCm device"):  # all else in order: the device is what is left
        be.dpt_tail(x, packed, 4, out=torch.zeros(B, 4, 6, 10))


def test_pack_wrapper_refusals(be):
    w1, b1, w2, b2 = torch.zeros(128, 128, 3, 3), torch.zeros(128), torch.zeros(4, 128, 1, 1), torch.zeros(4)
    with pytest.raises(RuntimeError, match="w1 must be on a ROCm device"):
        be.dpt_tail_pack(w1, b1, w2, b2)
    with pytest.raises(RuntimeError, match="b1 must be a tensor"):
        be.dpt_tail_pack(w1, None, w2, b2)
    with pytest.raises(RuntimeError, match="w2 must be torch.float32"):
        be.dpt_tail_pack(w1, b1, w2.double(), b2)
    with pytest.raises(RuntimeError, match="w1 must be contiguous"):
        be.dpt_tail_pack(w1.transpose(0, 1), b1, w2, b2)
    with pytest.raises(RuntimeError, match=r"w1 must be \[128, 128, 3, 3\]"):
        be.dpt_tail_pack(torch.zeros(128, 128, 5, 5), b1, w2, b2)
    with pytest.raises(RuntimeError, match=r"b1 must be \[128\]"):
        be.dpt_tail_pack(w1, torch.zeros(64), w2, b2)
    with pytest.raises(RuntimeError, match=r"w2 must be \[Cout, 128\]"):
        be.dpt_tail_pack(w1, b1, torch.zeros(4, 64), b2)
    with pytest.raises(RuntimeError, match="Cout = 5, only 1..4 are built"):
        be.dpt_tail_pack(w1, b1, torch.zeros(5, 128), torch.zeros(5))
    with pytest.raises(RuntimeError, match=r"b2 must be \[4\]"):
        be.dpt_tail_pack(w1, b1, w2, torch.zeros(3))


# ------------------------------------------------------------ install ---
class Model(torch.nn.Module):
    """Two heads, each with a DPT adapter stand-in; `kw2` shapes the second adapter's head."""

    def __init__(self, **kw2):
        super().__init__()
        self.downstream_head1, self.downstream_head2 = torch.nn.Module(), torch.nn.Module()
        self.downstream_head1.dpt = ref.DPTOutputAdapter()
        self.downstream_head2.dpt = ref.DPTOutputAdapter(**kw2)


def test_install_patches_the_head_sequentials_and_falls_back_on_the_cpu():
    from mast3r_slam_amd import dpt

    torch.manual_seed(3)
    model = Model().eval()
    plain = copy.deepcopy(model)
    seqs = [model.downstream_head1.dpt.head, model.downstream_head2.dpt.head]
    assert all(dpt.supported(s) for s in seqs)
    assert dpt.install(model) == 2
    assert model.downstream_head1.dpt.head is seqs[0]  # the Sequential itself, patched on the instance
    assert all("forward" in vars(s) and "_m3s_original_forward" in vars(s) for s in seqs)
    assert dpt.install(model) == 0  # idempotent
    x = torch.randn(1, 8, 3, 5)
    with torch.no_grad():  # a CPU input: the original forward, the identical result
        for a, b in ((model.downstream_head1.dpt, plain.downstream_head1.dpt),
                     (model.downstream_head2.dpt, plain.downstream_head2.dpt)):
            assert torch.equal(a(x), b(x))
    assert "_m3s_dpt_packed" not in vars(seqs[0])  # nothing was packed for it
    y = model.downstream_head1.dpt(x.requires_grad_())  # and with a gradient
    assert y.requires_grad and torch.equal(y.detach(), plain.downstream_head1.dpt(x).detach())


VARIANTS = {"5x5 conv": dict(kernel=5), "scale 4": dict(scale=4), "align_corners False": dict(align_corners=False),
            "64 channels": dict(mid=64), "Cout 5": dict(cout=5), "nearest": dict(mode="nearest")}


@pytest.mark.parametrize("what", sorted(VARIANTS))
def test_install_leaves_other_shapes_alone(what):
    from mast3r_slam_amd import dpt

    model = Model(**VARIANTS[what])
    other = model.downstream_head2.dpt.head
    assert not dpt.supported(other)
    assert dpt.install(model) == 1
    assert "forward" not in vars(other) and "forward" in vars(model.downstream_head1.dpt.head)


def test_install_wants_the_adapter_and_the_exact_sequential():
    from mast3r_slam_amd import dpt

    holder = torch.nn.Module()
    holder.head = ref.make_head_seq(features=8)  # a supported Sequential, but not in a DPT adapter
    assert dpt.supported(holder.head) and dpt.install(holder) == 0
    adapter = ref.DPTOutputAdapter()
    adapter.head = torch.nn.Sequential(*list(adapter.head)[1:])  # without the first convolution
    assert dpt.install(adapter) == 0
    adapter = ref.DPTOutputAdapter()
    adapter.head[2] = torch.nn.Conv2d(128, 128, 3, padding=1, bias=False)
    assert dpt.install(adapter) == 0
    adapter = ref.DPTOutputAdapter()
    adapter.head[2] = torch.nn.Conv2d(128, 128, 3, padding=1, stride=2)
    assert dpt.install(adapter) == 0
    assert dpt.install(ref.DPTOutputAdapter()) == 1


def test_a_sequential_changed_after_install_runs_its_original_forward():
    from mast3r_slam_amd import dpt

    adapter = ref.DPTOutputAdapter().eval()
    assert dpt.install(adapter) == 1
    adapter.head[1].align_corners = False
    x = torch.randn(1, 8, 2, 2)
    with torch.no_grad():
        want = adapter.head[4](adapter.head[3](adapter.head[2](adapter.head[1](adapter.head[0](x)))))
        assert torch.equal(adapter(x), want)

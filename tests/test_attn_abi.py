"""CPU-side checks of the attention C ABI (no GPU needed), by the method of
tests/test_rope_abi.py: the ctypes mirror of m3s_attn_args has exactly the C
layout (a gcc-compiled probe prints sizeof / offsetof from the header), the
header's symbols are be.ATTN_EXPORTS and in the library, every documented
M3S_EINVAL condition is refused with a null stream and no device, the Python
wrapper refuses what it cannot take, and attention.install patches the right
modules, whose forward then falls back, bitwise, wherever the kernel does not
apply (as everywhere on the CPU)."""
import ctypes
import math

import abi_probe
import pytest
import torch

FIELDS = ("q", "k", "v", "out", "qpos", "kpos", "B", "Nq", "Nk", "H", "D",
          "q_sb", "q_sn", "k_sb", "k_sn", "v_sb", "v_sn", "o_sb", "o_sn", "base", "f0", "scale", "dtype")


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


def test_ctypes_mirror_matches_header(be):
    assert tuple(n for n, _ in be.AttnArgs._fields_) == FIELDS
    got = abi_probe.probe(["m3s_attn.h"], {"m3s_attn_args": be.AttnArgs}, ["M3S_ROPE_F32"])
    assert got["M3S_ROPE_F32"] == be.ROPE_F32


def test_header_symbols_are_attn_exports(be):
    declared = abi_probe.declared_symbols("m3s_attn.h")
    assert declared == set(be.ATTN_EXPORTS) == {"m3s_attn_rope"}
    for sym in be.ATTN_EXPORTS:
        assert hasattr(be._lib, sym), sym
    others = set(be.EXPORTS) | set(be.RETRIEVAL_EXPORTS) | set(be.ROPE_EXPORTS) | set(be.HEAD_EXPORTS)
    assert not set(be.ATTN_EXPORTS) & others


N, H, D = 768, 16, 64
ROW = H * D


def good_args(be, keep):
    """A record that passes every check: the three slices of a [B, N, 3, H, D]
    qkv buffer at MASt3R's encoder shape and a dense out (the pointers are never
    followed: every call below is refused before a launch)."""
    buf = (ctypes.c_char * 64)()
    keep.append(buf)
    a = be.AttnArgs()
    a.q = a.k = a.v = a.out = a.qpos = a.kpos = ctypes.addressof(buf)
    a.B, a.Nq, a.Nk, a.H, a.D = 2, N, N, H, D
    a.q_sn = a.k_sn = a.v_sn = 3 * ROW
    a.q_sb = a.k_sb = a.v_sb = N * 3 * ROW
    a.o_sn, a.o_sb = ROW, N * ROW
    a.base, a.f0, a.scale, a.dtype = 100.0, 1.0, 0.125, be.ROPE_F32
    return a


EINVAL_CASES = {
    "null q": dict(q=None), "null k": dict(k=None), "null v": dict(v=None), "null out": dict(out=None),
    "only qpos null": dict(qpos=None), "only kpos null": dict(kpos=None),
    "B = 0": dict(B=0), "B < 0": dict(B=-1), "Nq = 0": dict(Nq=0), "Nq < 0": dict(Nq=-5),
    "Nk = 0": dict(Nk=0), "Nk < 0": dict(Nk=-5), "H = 0": dict(H=0), "H < 0": dict(H=-2),
    "D = 0": dict(D=0), "D < 0": dict(D=-64), "D = 32": dict(D=32), "D = 128": dict(D=128, H=8), "D = 60": dict(D=60),
    "dtype f16": dict(dtype=1), "dtype bf16": dict(dtype=2), "dtype 3": dict(dtype=3), "dtype -1": dict(dtype=-1),
    "q_sn one short": dict(q_sn=ROW - 1), "k_sn one short": dict(k_sn=ROW - 1),
    "v_sn one short": dict(v_sn=ROW - 1), "o_sn one short": dict(o_sn=ROW - 1),
    "q_sn = 0": dict(q_sn=0), "k_sn < 0": dict(k_sn=-3 * ROW), "o_sn = 0": dict(o_sn=0),
    "q_sb one short": dict(q_sb=(N - 1) * 3 * ROW + ROW - 1),
    "k_sb one short": dict(k_sb=(N - 1) * 3 * ROW + ROW - 1),
    "v_sb one short": dict(v_sb=(N - 1) * 3 * ROW + ROW - 1),
    "o_sb one short": dict(o_sb=N * ROW - 1), "v_sb = 0": dict(v_sb=0),
    "k_sb short for a longer Nk": dict(Nk=N + 1),
    "B * H * Nq = 2^31": dict(B=1 << 10, H=1 << 10, Nq=1 << 11, Nk=1, q_sn=1 << 16, q_sb=1 << 27, o_sn=1 << 16,
                              o_sb=1 << 27, k_sn=1 << 16, k_sb=1 << 16, v_sn=1 << 16, v_sb=1 << 16),
    "B * Nk = 2^31": dict(B=1 << 16, H=1, Nq=1, Nk=1 << 15, q_sn=64, q_sb=64, o_sn=64, o_sb=64, k_sn=64,
                          k_sb=64 << 15, v_sn=64, v_sb=64 << 15),
    "base = 0": dict(base=0.0), "base < 0": dict(base=-100.0),
    "base inf": dict(base=math.inf), "base nan": dict(base=math.nan),
    "f0 inf": dict(f0=-math.inf), "f0 nan": dict(f0=math.nan),
    "scale inf": dict(scale=math.inf), "scale nan": dict(scale=math.nan),
}


@pytest.mark.parametrize("what", sorted(EINVAL_CASES))
def test_attn_refuses_before_any_launch(be, what):
    keep = []
    a = good_args(be, keep)
    for k, v in EINVAL_CASES[what].items():
        setattr(a, k, v)
    assert be._lib.m3s_attn_rope(ctypes.byref(a), None) == be.M3S_EINVAL


def test_size_cases_are_refused_for_their_size_alone(be):
    """The records of the two 2^31 cases have strides that fit their sizes and
    exactly 2^31 as their product, so the product is what is refused above."""
    for what in ("B * H * Nq = 2^31", "B * Nk = 2^31"):
        keep = []
        a = good_args(be, keep)
        for k, v in EINVAL_CASES[what].items():
            setattr(a, k, v)
        row = a.H * a.D
        for sb, sn, n in ((a.q_sb, a.q_sn, a.Nq), (a.k_sb, a.k_sn, a.Nk), (a.v_sb, a.v_sn, a.Nk), (a.o_sb, a.o_sn, a.Nq)):
            assert sn >= row and sb >= (n - 1) * sn + row, what  # the strides are not the reason
        assert max(a.B * a.H * a.Nq, a.B * a.Nk) == 1 << 31


def test_null_record_refused(be):
    assert be._lib.m3s_attn_rope(None, None) == be.M3S_EINVAL


def test_wrapper_refusals(be):
    q = torch.zeros(2, 5, 3, 64)
    k = v = torch.zeros(2, 7, 3, 64)
    qpos, kpos = torch.zeros(2, 5, 2, dtype=torch.int64), torch.zeros(2, 7, 2, dtype=torch.int64)
    call = lambda *a, **kw: be.attention_rope(*a, 100.0, 1.0, 0.125, **kw)  # noqa: E731
    with pytest.raises(RuntimeError, match="ROCm device"):
        call(q, k, v, qpos, kpos)
    with pytest.raises(RuntimeError, match="ROCm device"):
        call(q, k, v, None, None)
    with pytest.raises(RuntimeError, match="must be a tensor"):
        call(q, None, v, qpos, kpos)
    with pytest.raises(RuntimeError, match="q must be torch.float32"):
        call(q.half(), k, v, qpos, kpos)
    with pytest.raises(RuntimeError, match="v must be torch.float32"):
        call(q, k, v.double(), qpos, kpos)
    with pytest.raises(RuntimeError, match=r"k must be \[B, N, H, D\]"):
        call(q, k[0], v, qpos, kpos)
    with pytest.raises(RuntimeError, match="only the head dimension 64"):
        call(torch.zeros(2, 5, 3, 32), torch.zeros(2, 7, 3, 32), torch.zeros(2, 7, 3, 32), qpos, kpos)
    with pytest.raises(RuntimeError, match=r"k must be \[2, Nk, 3, 64\]"):
        call(q, torch.zeros(2, 7, 4, 64), v, qpos, kpos)
    with pytest.raises(RuntimeError, match=r"v must be \[2, 7, 3, 64\]"):
        call(q, k, torch.zeros(2, 8, 3, 64), qpos, kpos)
    with pytest.raises(RuntimeError, match="q: a head row must be contiguous"):  # stride(3) == 2
        call(torch.zeros(2, 5, 3, 128)[..., ::2], k, v, qpos, kpos)
    with pytest.raises(RuntimeError, match="k: a head row must be contiguous"):  # [B, H, N, D] contiguous, transposed
        call(q, torch.zeros(2, 3, 7, 64).transpose(1, 2), v, qpos, kpos)
    with pytest.raises(RuntimeError, match="both be given or both be None"):
        call(q, k, v, qpos, None)
    with pytest.raises(RuntimeError, match="kpos must be torch.int64"):
        call(q, k, v, qpos, kpos.int())
    with pytest.raises(RuntimeError, match=r"qpos must be \[2, 5, 2\]"):
        call(q, k, v, qpos[:, :4], kpos)
    with pytest.raises(RuntimeError, match="kpos must be contiguous"):
        call(q, k, v, qpos, torch.zeros(2, 2, 7, dtype=torch.int64).transpose(1, 2))
    with pytest.raises(RuntimeError, match=r"out must be \[2, 5, 192\]"):
        call(q, k, v, qpos, kpos, out=torch.zeros(2, 5, 3, 64))
    with pytest.raises(RuntimeError, match="out must be torch.float32"):
        call(q, k, v, qpos, kpos, out=torch.zeros(2, 5, 192, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="out: a row must be contiguous"):
        call(q, k, v, qpos, kpos, out=torch.zeros(2, 5, 384)[..., ::2])
    with pytest.raises(RuntimeError, match="softmax over no keys"):
        call(q, k[:, :0], v[:, :0], qpos, kpos[:, :0])


import attn_ref  # noqa: E402
from attn_ref import Attention, CrossAttention, RoPE2D  # noqa: E402  (install goes by these class names)


class Block(torch.nn.Module):
    def __init__(self, rope):
        super().__init__()
        self.attn = Attention(128, rope)
        self.cross_attn = CrossAttention(128, rope)


def test_install_patches_the_right_instances():
    from mast3r_slam_amd import attention

    torch.manual_seed(2)
    rope = RoPE2D()
    tree = torch.nn.Sequential(Block(rope), Block(None), torch.nn.Linear(8, 8))
    lacking = Attention(128, rope)
    del lacking.proj_drop  # the class name alone is not enough
    tree.add_module("lacking", lacking)

    class Other(torch.nn.Module):  # every attribute, another class name
        def __init__(self):
            super().__init__()
            self.inner = Attention(128, None)
            for a in ("qkv", "proj", "proj_drop", "attn_drop", "num_heads", "scale", "rope"):
                setattr(self, a, getattr(self.inner, a))

    tree.add_module("other", Other())
    x = torch.randn(2, 9, 128)
    mem = torch.randn(2, 11, 128)
    pos = torch.randint(0, 8, (2, 9, 2))
    mpos = torch.randint(0, 8, (2, 11, 2))
    with torch.no_grad():
        want = [(b.attn(x, pos), b.cross_attn(x, mem, mem, pos, mpos)) for b in (tree[0], tree[1])]
    assert attention.install(tree) == 5  # 2 + 2 and other.inner
    for b in (tree[0], tree[1]):
        assert "forward" in vars(b.attn) and "forward" in vars(b.cross_attn)
    assert "forward" in vars(tree.other.inner)
    assert "forward" not in vars(tree.lacking) and "forward" not in vars(tree.other)
    assert attention.install(tree) == 0  # idempotent
    # on the CPU the patched forward is the original, bitwise; so is a call that needs a gradient
    with torch.no_grad():
        got = [(b.attn(x, pos), b.cross_attn(x, mem, mem, pos, mpos)) for b in (tree[0], tree[1])]
    for (ws, wc), (gs, gc) in zip(want, got):
        assert torch.equal(ws, gs) and torch.equal(wc, gc)
    y = tree[0].attn(x, pos)
    assert y.requires_grad and torch.equal(y.detach(), want[0][0])
    # the state dict is untouched: nothing was registered
    assert not [k for k in tree.state_dict() if "m3s" in k]

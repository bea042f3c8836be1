"""CPU-side checks of the RoPE C ABI (no GPU needed), by the method of
tests/test_quantize_abi.py: the ctypes mirror of m3s_rope_args has exactly the C
layout (a gcc-compiled probe prints sizeof / offsetof from the header), the
header's symbols are be.ROPE_EXPORTS and in the library, every documented
M3S_EINVAL condition is refused with a null stream and no device, the Python
wrapper refuses what it cannot take, and rope.install swaps the right modules."""
import ctypes
import math

import abi_probe
import pytest
import torch

FIELDS = ("tokens", "pos", "B", "N", "H", "D", "stride_b", "stride_n", "base", "f0", "dtype")


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


def test_ctypes_mirror_matches_header(be):
    assert tuple(n for n, _ in be.RopeArgs._fields_) == FIELDS
    got = abi_probe.probe(["m3s_rope.h"], {"m3s_rope_args": be.RopeArgs}, ["M3S_ROPE_F32", "M3S_ROPE_F16", "M3S_ROPE_BF16"])
    assert (got["M3S_ROPE_F32"], got["M3S_ROPE_F16"], got["M3S_ROPE_BF16"]) == (be.ROPE_F32, be.ROPE_F16, be.ROPE_BF16)


def test_header_symbols_are_rope_exports(be):
    declared = abi_probe.declared_symbols("m3s_rope.h")
    assert declared == set(be.ROPE_EXPORTS) == {"m3s_rope_2d"}
    for sym in be.ROPE_EXPORTS:
        assert hasattr(be._lib, sym), sym
    assert not set(be.ROPE_EXPORTS) & (set(be.EXPORTS) | set(be.RETRIEVAL_EXPORTS))


def good_args(be, keep):
    """A record that passes every check: the q slice of a [B, N, 3, H, D] qkv
    buffer at MASt3R's shape (the pointers are never followed: every call below
    is refused before a launch)."""
    buf = (ctypes.c_char * 64)()
    keep.append(buf)
    a = be.RopeArgs()
    a.tokens = a.pos = ctypes.addressof(buf)
    a.B, a.N, a.H, a.D = 2, 768, 16, 64
    a.stride_n, a.stride_b = 3 * 16 * 64, 768 * 3 * 16 * 64
    a.base, a.f0, a.dtype = 100.0, 1.0, be.ROPE_F16
    return a


EINVAL_CASES = {
    "null tokens": dict(tokens=None), "null pos": dict(pos=None),
    "B = 0": dict(B=0), "B < 0": dict(B=-1), "N = 0": dict(N=0), "N < 0": dict(N=-5),
    "H = 0": dict(H=0), "H < 0": dict(H=-2), "D = 0": dict(D=0), "D < 0": dict(D=-64),
    "D % 4 = 2": dict(D=62, stride_n=3 * 16 * 64), "D % 4 = 1": dict(D=33),
    "stride_n one short": dict(stride_n=16 * 64 - 1),
    "stride_n = 0": dict(stride_n=0), "stride_n < 0": dict(stride_n=-3072),
    "stride_b one short": dict(stride_b=767 * 3072 + 1024 - 1),
    "stride_b = 0": dict(stride_b=0),
    "B * N = 2^31": dict(B=1 << 16, N=1 << 15, H=1, D=4, stride_n=4, stride_b=4 << 15),
    "base = 0": dict(base=0.0), "base < 0": dict(base=-100.0),
    "base inf": dict(base=math.inf), "base nan": dict(base=math.nan),
    "f0 inf": dict(f0=-math.inf), "f0 nan": dict(f0=math.nan),
    "dtype 3": dict(dtype=3), "dtype -1": dict(dtype=-1),
}


@pytest.mark.parametrize("what", sorted(EINVAL_CASES))
def test_rope_refuses_before_any_launch(be, what):
    keep = []
    a = good_args(be, keep)
    for k, v in EINVAL_CASES[what].items():
        setattr(a, k, v)
    assert be._lib.m3s_rope_2d(ctypes.byref(a), None) == be.M3S_EINVAL


def test_null_record_refused(be):
    assert be._lib.m3s_rope_2d(None, None) == be.M3S_EINVAL


def test_wrapper_refusals(be):
    tokens = torch.zeros(2, 5, 3, 8)
    pos = torch.zeros(2, 5, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm device"):
        be.rope_2d(tokens, pos, 100.0, 1.0)
    with pytest.raises(RuntimeError, match="contiguous"):  # stride(3) == 2
        be.rope_2d(torch.zeros(2, 5, 3, 16)[..., ::2], pos, 100.0, 1.0)
    with pytest.raises(RuntimeError, match="contiguous"):  # [B, H, N, D] contiguous, transposed: stride(2) == N * D
        be.rope_2d(torch.zeros(2, 3, 5, 8).transpose(1, 2), pos, 100.0, 1.0)
    with pytest.raises(RuntimeError, match="float32, float16 or bfloat16"):
        be.rope_2d(tokens.double(), pos, 100.0, 1.0)
    with pytest.raises(RuntimeError, match="int64"):
        be.rope_2d(tokens, pos.int(), 100.0, 1.0)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        be.rope_2d(torch.zeros(2, 5, 3, 6), pos, 100.0, 1.0)
    with pytest.raises(RuntimeError, match=r"positions must be \[2, 5, 2\]"):
        be.rope_2d(tokens, pos[:, :4], 100.0, 1.0)
    from mast3r_slam_amd import rope

    with pytest.raises(RuntimeError, match="ROCm device"):  # the module ([B, H, N, D]) goes the same way
        rope.RoPE2D()(tokens.transpose(1, 2), pos)


class RoPE2D(torch.nn.Module):
    """A stand-in with the name and the attributes install looks for."""

    def __init__(self, freq, F0):
        super().__init__()
        self.base, self.F0 = freq, F0

    def forward(self, tokens, positions):
        return tokens


class Block(torch.nn.Module):
    def __init__(self, rope):
        super().__init__()
        self.proj = torch.nn.Linear(8, 8)
        self.rope = rope


def test_install_replaces_the_shared_module():
    from mast3r_slam_amd import rope

    shared = RoPE2D(50.0, -2.0)
    tree = torch.nn.Sequential(Block(shared), Block(shared), Block(None), torch.nn.Linear(8, 8))
    other = torch.nn.Identity()
    tree.add_module("odd", torch.nn.Sequential())
    tree.odd.rope = other  # named rope, but not a RoPE2D: stays
    assert rope.install(tree) == 2
    assert type(tree[0].rope) is rope.RoPE2D and tree[0].rope is tree[1].rope
    assert (tree[0].rope.base, tree[0].rope.F0) == (50.0, -2.0)
    assert tree[2].rope is None and tree.odd.rope is other
    assert rope.install(tree) == 0  # nothing left to replace

"""CPU-side checks of the quantize part of the retrieval C ABI (no GPU needed),
by the method of tests/test_retrieval_abi.py: the ctypes mirror of
m3s_asmk_quantize_args has exactly the C layout (a gcc-compiled probe prints
sizeof / offsetof from the header), the three new symbols are in
be.RETRIEVAL_EXPORTS and in the library, the workspace size is monotone, every
documented M3S_EINVAL condition is refused with a null stream and no device,
and the Python layers refuse CPU tensors and unknown quantizers."""
import ctypes

import abi_probe
import pytest
import torch

FIELDS = ("des", "centroids", "norms", "n", "Kc", "D", "ma", "assign", "dist", "workspace", "workspace_bytes")
NEW_SYMBOLS = ("m3s_asmk_quantize_workspace_size", "m3s_asmk_centroid_norms", "m3s_asmk_quantize")


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


def test_ctypes_mirror_matches_header(be):
    assert tuple(n for n, _ in be.AsmkQuantizeArgs._fields_) == FIELDS
    got = abi_probe.probe(["m3s_retrieval.h"], {"m3s_asmk_quantize_args": be.AsmkQuantizeArgs},
                          ["M3S_ASMK_QUANTIZE_MAX_MA"])
    assert got["M3S_ASMK_QUANTIZE_MAX_MA"] == be.ASMK_QUANTIZE_MAX_MA == 8


def test_new_symbols_listed_and_exported(be):
    for sym in NEW_SYMBOLS:
        assert sym in be.RETRIEVAL_EXPORTS, sym
        assert hasattr(be._lib, sym), sym


def test_workspace_size_monotone(be):
    ws = be.asmk_quantize_workspace_size
    base = ws(300, 20000, 5)
    assert base >= 300 * (20000 // 128) * 5 * 8  # one (value, word) pair per feature, tile and rank
    assert base < 300 * 20000 * 4 // 8  # and nothing [n, Kc]-shaped
    assert base < ws(600, 20000, 5) and base < ws(300, 40000, 5) and base < ws(300, 20000, 8)
    assert ws(299, 20000, 5) <= base and ws(300, 19999, 5) <= base and ws(300, 20000, 4) < base
    for n, kc, ma in ((1, 1, 1), (37, 97, 5), (300, 512, 8)):
        assert 0 < ws(n, kc, ma) <= ws(n + 1, kc, ma) <= ws(n + 1, kc + 1, ma)
        if ma < 8:
            assert ws(n, kc, ma) <= ws(n, kc, ma + 1)


def good_args(be, keep):
    """An argument record that passes every check (the pointers are never
    followed: every call below is refused before a launch). `keep` holds what
    the pointers refer to."""
    buf = (ctypes.c_char * 64)()
    keep.append(buf)
    p = ctypes.addressof(buf)
    a = be.AsmkQuantizeArgs()
    a.des = a.centroids = a.norms = a.assign = a.dist = a.workspace = p
    a.n, a.Kc, a.D, a.ma = 300, 20000, 1024, 5
    a.workspace_bytes = be.asmk_quantize_workspace_size(300, 20000, 5)
    return a


EINVAL_CASES = {
    "null des": dict(des=None), "null centroids": dict(centroids=None), "null norms": dict(norms=None),
    "null assign": dict(assign=None), "null workspace": dict(workspace=None),
    "n = 0": dict(n=0), "n < 0": dict(n=-3),
    "n * ma > MAX_PAIRS": dict(n=820, workspace_bytes=1 << 40),  # 4100 pairs
    "ma = 0": dict(ma=0), "ma < 0": dict(ma=-1), "ma > MAX_MA": dict(ma=9, n=10),
    "ma > Kc": dict(Kc=4), "Kc = 0": dict(Kc=0),
    "Kc = 2^20": dict(Kc=1 << 20, workspace_bytes=1 << 40),
    "D = 0": dict(D=0), "D < 0": dict(D=-8),
    "workspace one byte short": dict(workspace_bytes=-1),
}


@pytest.mark.parametrize("what", sorted(EINVAL_CASES))
def test_quantize_refuses_before_any_launch(be, what):
    keep = []
    a = good_args(be, keep)
    for k, v in EINVAL_CASES[what].items():
        if k == "workspace_bytes" and v == -1:
            v = a.workspace_bytes - 1
        setattr(a, k, v)
    assert be._lib.m3s_asmk_quantize(ctypes.byref(a), None) == be.M3S_EINVAL


def test_null_record_and_norms_arguments_refused(be):
    assert be._lib.m3s_asmk_quantize(None, None) == be.M3S_EINVAL
    buf = (ctypes.c_char * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    norms = be._lib.m3s_asmk_centroid_norms
    assert norms(None, 97, 64, p, None) == be.M3S_EINVAL
    assert norms(p, 97, 64, None, None) == be.M3S_EINVAL
    assert norms(p, 0, 64, p, None) == be.M3S_EINVAL
    assert norms(p, 1 << 20, 64, p, None) == be.M3S_EINVAL
    assert norms(p, 97, 0, p, None) == be.M3S_EINVAL


def test_wrappers_refuse_cpu_tensors(be):
    feat, cent, norms = torch.zeros(37, 64), torch.zeros(97, 64), torch.zeros(97)
    ws = torch.zeros(be.asmk_quantize_workspace_size(37, 97, 5), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="ROCm device"):
        be.asmk_quantize(feat, cent, norms, 5, ws)
    with pytest.raises(RuntimeError, match="ROCm device"):
        be.asmk_centroid_norms(cent)
    with pytest.raises(RuntimeError, match="contiguous"):
        be.asmk_centroid_norms(torch.zeros(64, 97).t())


def test_unknown_quantizer_refused_before_the_device():
    from mast3r_slam_amd.retrieval import RetrievalDatabase

    cent = torch.zeros(97, 64)  # a CPU tensor: any touch of the device would fail differently
    with pytest.raises(ValueError, match="quantizer"):
        RetrievalDatabase(cent, quantizer="nope")
    with pytest.raises(ValueError, match="quantizer"):
        RetrievalDatabase(cent, max_features=100, query_ma=9, quantizer="device")  # above MAX_MA
    with pytest.raises(RuntimeError, match="ROCm device"):
        RetrievalDatabase(cent, quantizer="device")

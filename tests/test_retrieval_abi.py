"""CPU-side checks of the retrieval C ABI (no GPU needed), by the method of
tests/test_abi.py: the ctypes mirrors of the m3s_asmk_* structs have exactly
the C layout (a gcc-compiled probe prints sizeof / offsetof from the header),
the symbols include/m3s_retrieval.h declares are be.RETRIEVAL_EXPORTS and the
library exports them, the size functions are monotone, unsupported settings
and CPU tensors are refused before the device is touched, and backend_edges
restates main.py:103-125."""
import ctypes

import abi_probe
import pytest
import torch

STRUCTS = {
    "m3s_asmk_out": ("AsmkOut", ("count", "n_images", "info", "n_query_words", "idx", "score")),
    "m3s_asmk_db": ("AsmkDb", ("store", "store_bytes", "workspace", "workspace_bytes", "cap_images",
                               "cap_entries", "Kc", "D")),
    "m3s_asmk_aggregate_args": ("AsmkAggregateArgs", ("db", "des", "centroids", "assign", "n", "ma", "query_ma",
                                                      "build_ma")),
    "m3s_asmk_search_args": ("AsmkSearchArgs", ("db", "n_images", "k", "alpha", "similarity_threshold",
                                                "min_thresh")),
}


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


def test_ctypes_struct_layout_matches_header(be):
    for name, fields in STRUCTS.values():
        assert tuple(n for n, _ in getattr(be, name)._fields_) == fields
    got = abi_probe.probe(["m3s_retrieval.h"], {t: getattr(be, name) for t, (name, _) in STRUCTS.items()},
                          ["M3S_ASMK_MAX_PAIRS", "M3S_ASMK_MAX_K", "M3S_ASMK_INFO_BAD_WORD", "M3S_ASMK_INFO_FULL",
                           "M3S_ASMK_STORE_SECTIONS", "M3S_ASMK_WS_SECTIONS"])
    assert got["M3S_ASMK_MAX_PAIRS"] == be.ASMK_MAX_PAIRS == 4096
    assert got["M3S_ASMK_MAX_K"] == be.ASMK_MAX_K
    assert got["M3S_ASMK_INFO_BAD_WORD"] == be.ASMK_INFO_BAD_WORD
    assert got["M3S_ASMK_INFO_FULL"] == be.ASMK_INFO_FULL
    assert got["M3S_ASMK_STORE_SECTIONS"] == len(be.ASMK_STORE_SECTIONS)
    assert got["M3S_ASMK_WS_SECTIONS"] == len(be.ASMK_WS_SECTIONS)


def test_library_exports_every_header_symbol(be):
    declared = abi_probe.declared_symbols("m3s_retrieval.h")
    assert declared == set(be.RETRIEVAL_EXPORTS)
    assert not declared & set(be.EXPORTS)
    for sym in declared:
        assert hasattr(be._lib, sym), sym


def test_size_functions_monotone_and_layouts_ordered(be):
    ss, ws = be.asmk_store_size, be.asmk_workspace_size
    base = ss(512, 512 * 300, 1024)
    assert base >= 512 * 300 * (128 + 4)  # codes and words
    assert base <= ss(513, 512 * 300, 1024) and base < ss(1024, 512 * 300, 1024)  # sections are 256-B aligned
    assert base < ss(512, 512 * 301, 1024) and base < ss(512, 512 * 300, 1056)
    assert ss(64, 64 * 300, 1024) < base
    wbase = ws(20000, 1024, 512)
    assert wbase >= 4 * 20000 + 2 * 4096 * 128 + 8 * 512
    assert wbase < ws(40000, 1024, 512) and wbase < ws(20000, 2048, 512) and wbase < ws(20000, 1024, 4096)
    so = be.asmk_store_layout(512, 512 * 300, 1024)
    assert [so[k] for k in be.ASMK_STORE_SECTIONS] == sorted(so.values()) and so["total"] == base
    wo = be.asmk_workspace_layout(20000, 1024, 512)
    assert [wo[k] for k in be.ASMK_WS_SECTIONS] == sorted(wo.values()) and wo["total"] == wbase
    assert wo["total"] - wo["out"] >= ctypes.sizeof(be.AsmkOut)
    assert all(v % 16 == 0 for v in list(so.values()) + list(wo.values()))


def test_unsupported_settings_refused_before_the_device(be):
    from mast3r_slam_amd.retrieval import RetrievalDatabase

    cent = torch.zeros(97, 64)  # a CPU tensor: any touch of the device would fail differently
    with pytest.raises(ValueError, match="use_idf"):
        RetrievalDatabase(cent, use_idf=True)
    with pytest.raises(ValueError, match="binary"):
        RetrievalDatabase(cent, binary=False)
    with pytest.raises(ValueError, match="4096"):
        RetrievalDatabase(cent, max_features=820, query_ma=5)  # n * MA = 4100
    with pytest.raises(RuntimeError, match="ROCm device"):
        RetrievalDatabase(cent)
    with pytest.raises(RuntimeError, match="ROCm device"):
        be.AsmkHandle(torch.zeros(1 << 16, dtype=torch.uint8), torch.zeros(1 << 16, dtype=torch.uint8), 4, 16, 97, 64)
    # the C entry points refuse the same without a launch: null buffers, too many pairs
    db = be.AsmkDb()
    assert be._lib.m3s_asmk_reset(ctypes.byref(db), None) == be.M3S_EINVAL
    assert be._lib.m3s_asmk_append(ctypes.byref(db), None) == be.M3S_EINVAL
    a = be.AsmkAggregateArgs()
    assert be._lib.m3s_asmk_aggregate(ctypes.byref(a), None) == be.M3S_EINVAL
    s = be.AsmkSearchArgs()
    assert be._lib.m3s_asmk_search(ctypes.byref(s), None) == be.M3S_EINVAL


def test_backend_edges_restates_main():
    from mast3r_slam_amd.retrieval import backend_edges

    assert backend_edges(0, []) == ([], [])  # idx = 0: no previous keyframe
    assert backend_edges(0, [0]) == ([], [])
    ii, jj = backend_edges(5, [4, 1])  # a hit equal to idx - 1: once
    assert sorted(ii) == [1, 4] and jj == [5, 5]
    ii, jj = backend_edges(5, [5, 2])  # a hit equal to idx: dropped
    assert sorted(ii) == [2, 4] and jj == [5, 5]
    ii, jj = backend_edges(3, [], n_consec=5)
    assert sorted(ii) == [0, 1, 2] and jj == [3, 3, 3]
    ii, jj = backend_edges(1, [0, 0])
    assert ii == [0] and jj == [1]

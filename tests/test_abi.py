"""CPU-side checks of the C ABI boundary (no GPU needed):

* libm3s_gn.so loads and exports every symbol include/m3s_gn.h declares;
* the ctypes mirrors of m3s_gn_args / m3s_track_args have exactly the C
  layout (tests/abi_probe.py: sizeof and every offsetof, from the header);
* workspace sizing is monotone and covers the documented sections;
* the drop-in module exposes the reference's five entry points (gn.cpp:116-122)
  and rejects CPU tensors / non-contiguous inputs before touching the device.
"""
import os

import abi_probe
import pytest
import torch

HEADERS = ["m3s_gn.h", "m3s_match.h", "m3s_fuse.h"]


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


def test_library_exports_every_header_symbol(be):
    declared = set().union(*(abi_probe.declared_symbols(h) for h in HEADERS))
    assert declared == set(be.EXPORTS)
    for sym in declared:
        assert hasattr(be._lib, sym), sym
    assert "gfx950" in be.version()


def test_reference_entry_points_present(be):
    for f in ("gauss_newton_points", "gauss_newton_rays", "gauss_newton_calib", "iter_proj",
              "refine_matches"):
        assert callable(getattr(be, f))
    with pytest.raises(RuntimeError):  # CPU tensors: no CPU path
        be.iter_proj(torch.zeros(1, 4, 4, 9), torch.zeros(1, 16, 3), torch.zeros(1, 16, 2), 10, 1e-8,
                     1e-6)
    with pytest.raises(RuntimeError):
        be.refine_matches(torch.zeros(1, 4, 4, 8, dtype=torch.float16),
                          torch.zeros(1, 16, 8, dtype=torch.float16),
                          torch.zeros(1, 16, 2, dtype=torch.int64), 3, 5)


def test_ctypes_struct_layout_matches_header(be):
    # every field of every mirror, by its _fields_
    abi_probe.probe(HEADERS, {"m3s_gn_args": be.GnArgs, "m3s_track_args": be.TrackArgs,
                              "m3s_iter_proj_args": be.IterProjArgs, "m3s_refine_args": be.RefineArgs,
                              "m3s_fuse_args": be.FuseArgs, "m3s_prep_rays_args": be.PrepRaysArgs})


def test_workspace_size_monotone(be):
    s1 = be._lib.m3s_gn_workspace_size(32, 262144, 96)
    s2 = be._lib.m3s_gn_workspace_size(48, 262144, 96)
    s3 = be._lib.m3s_gn_workspace_size(32, 262144, 200)
    assert 0 < s1 < s2 and s1 < s3
    # dense (N-1)*7 fp64 system dominates for large N
    assert be._lib.m3s_gn_workspace_size(256, 262144, 1024) >= 8 * (7 * 255) ** 2
    assert be._lib.m3s_track_workspace_size(262144) > 0


def test_cpu_tensors_rejected(be):
    N, HW, E = 3, 16, 2
    Twc = torch.zeros(N, 8)
    with pytest.raises(RuntimeError, match="ROCm device"):
        be.gauss_newton_rays(Twc, torch.zeros(N, HW, 3), torch.zeros(N, HW, 1),
                             torch.zeros(E, dtype=torch.long), torch.zeros(E, dtype=torch.long),
                             torch.zeros(E, HW, dtype=torch.long),
                             torch.zeros(E, HW, 1, dtype=torch.bool), torch.zeros(E, HW, 1),
                             0.003, 10.0, 0.0, 1.5, 10, 1e-8)
    with pytest.raises(RuntimeError, match="contiguous"):
        be.gauss_newton_rays(Twc.t(), torch.zeros(N, HW, 3), torch.zeros(N, HW, 1),
                             torch.zeros(E, dtype=torch.long), torch.zeros(E, dtype=torch.long),
                             torch.zeros(E, HW, dtype=torch.long),
                             torch.zeros(E, HW, 1, dtype=torch.bool), torch.zeros(E, HW, 1),
                             0.003, 10.0, 0.0, 1.5, 10, 1e-8)


def test_build_inputs_cover_every_source_file():
    # a file under csrc/ that build() does not know leaves a stale library in place
    import __graft_entry__ as ge

    found = {"h": set(), "src": set()}
    for d, _, files in os.walk(ge.CSRC):
        for f in files:
            if f.endswith(".h"):
                found["h"].add(os.path.join(d, f))
            elif f.endswith((".hip", ".cpp")):
                found["src"].add(os.path.join(d, f))
    assert found["h"] and found["h"] <= set(ge.HEADERS)
    assert found["src"] and found["src"] <= set(ge.SOURCES)

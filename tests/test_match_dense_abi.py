"""CPU-side checks of the match_dense C ABI (no GPU needed), by the method of
tests/test_abi.py: the ctypes mirror of m3s_match_dense_args has exactly the C
layout (a gcc-compiled probe prints sizeof / offsetof from the header), the
workspace size grows with B, H and W, and the wrapper turns away CPU tensors
before it touches the device."""

import abi_probe
import pytest
import torch

FIELDS = ("X11", "X21", "D11", "D21", "Q11", "Q21", "idx_init", "B", "H", "W", "F", "dtype", "max_iter",
          "lambda_init", "cost_thresh", "dist_thresh", "radius", "dilation_max", "Q_conf", "idx", "valid", "Q",
          "idx_stride", "valid_stride", "Q_stride", "n_valid", "workspace", "workspace_bytes")


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


def test_ctypes_struct_layout_matches_header(be):
    assert tuple(n for n, _ in be.MatchDenseArgs._fields_) == FIELDS
    abi_probe.probe(["m3s_match.h"], {"m3s_match_dense_args": be.MatchDenseArgs})


def test_workspace_size_monotone(be):
    size = be.match_dense_workspace_size
    base = size(2, 48, 64)
    # ray image (9 floats), unit rays (3), integer pixel pair, flag: 57 B per pixel
    assert base >= 2 * 48 * 64 * 57
    assert base < size(3, 48, 64) and base < size(2, 49, 64) and base < size(2, 48, 65)
    assert size(2, 512, 512) < size(4, 512, 512)
    assert size(0, 48, 64) == 0 or size(0, 48, 64) < base


def test_entry_points_present_and_cpu_tensors_rejected(be):
    from mast3r_slam_amd import factor_graph, matching

    assert callable(be.match_dense) and callable(matching.match_dense)
    assert callable(factor_graph.FactorGraph.add_factors_dense)
    H, W, F = 4, 5, 8
    X = torch.zeros(1, H, W, 3)
    D = torch.zeros(1, H, W, F, dtype=torch.float16)
    Q = torch.ones(1, H * W)
    with pytest.raises(RuntimeError, match="ROCm device"):  # no CPU path
        be.match_dense(X, X, D, D, Q, Q)
    with pytest.raises(RuntimeError, match="contiguous"):
        be.match_dense(X.transpose(1, 2), X, D, D, Q, Q)

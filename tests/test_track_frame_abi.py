"""CPU-side checks of the track_frame C ABI (no GPU needed), by the method of
tests/test_match_dense_abi.py: the ctypes mirror of m3s_track_frame_args has
exactly the C layout (a gcc-compiled probe prints sizeof / offsetof from the
header), the symbols are exported, the workspace size grows with HW and covers
its own sections, argument errors come back as M3S_EINVAL before anything is
launched, and the wrapper turns away CPU tensors before it touches the device
(wrong dtypes and shapes on device tensors: tests/test_gpu_track_frame.py)."""
import ctypes

import abi_probe
import pytest
import torch

FIELDS = ("Xf_canon", "Cf_sum", "Xk_canon", "Ck_sum", "idx_f2k", "valid_match", "Qk", "T_WCf", "T_WCk", "K",
          "HW", "Nf", "Nk", "height", "width", "C_conf", "Q_conf", "pixel_border", "z_eps", "sigma_a", "sigma_b",
          "huber_k", "max_iters", "rel_error", "delta_norm", "sync_every", "T_WCf_out", "T_CkCf_out", "info",
          "stats", "Xf_out", "Xk_out", "valid_opt_out", "workspace", "workspace_bytes")


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


def test_ctypes_struct_layout_matches_header(be):
    assert tuple(n for n, _ in be.TrackFrameArgs._fields_) == FIELDS
    abi_probe.probe(["m3s_gn.h"], {"m3s_track_frame_args": be.TrackFrameArgs})


def test_symbols_exported(be):
    for sym in ("m3s_track_frame", "m3s_track_frame_workspace_size"):
        assert sym in be.EXPORTS
        assert hasattr(be._lib, sym), sym
    assert callable(be.track_frame) and callable(be.track_frame_workspace_size)
    assert (be.STAT_N_OPT, be.STAT_N_KF, be.STAT_N_UNIQUE) == (0, 1, 2)


def test_workspace_size_monotone_and_covers_its_sections(be):
    size = be.track_frame_workspace_size
    sizes = [size(hw) for hw in (1, 63, 64, 768, 1023, 3072, 512 * 384, 512 * 512)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[3] < sizes[-1]
    for hw in (1, 63, 1023, 3072, 512 * 512):
        # the tracker's workspace, the byte map of the frame's pixels, two
        # prepared [HW,3] float rows and the valid_opt bytes
        assert size(hw) >= be.track_workspace_size(hw) + hw + 2 * 12 * hw + hw


def _args(be, HW, H, W, ws_bytes):
    """m3s_track_frame_args whose pointers are non-NULL but never valid: the
    calls below must return before reading or launching anything."""
    a = be.TrackFrameArgs()
    fake = ctypes.c_void_p(0x1000)
    for name in ("Xf_canon", "Cf_sum", "Xk_canon", "Ck_sum", "idx_f2k", "valid_match", "Qk", "T_WCf", "T_WCk",
                 "T_WCf_out", "T_CkCf_out", "info", "stats", "workspace"):
        setattr(a, name, fake)
    a.HW, a.Nf, a.Nk, a.height, a.width = HW, 1, 1, H, W
    a.max_iters = 1
    a.sigma_a = a.sigma_b = 1.0
    a.workspace_bytes = ws_bytes
    return a


def test_argument_errors_return_einval_without_a_launch(be):
    HW, H, W = 3072, 48, 64
    need = be.track_frame_workspace_size(HW)
    call = lambda a: be._lib.m3s_track_frame(ctypes.byref(a), None)  # noqa: E731
    assert be._lib.m3s_track_frame(None, None) == be.M3S_EINVAL
    assert call(_args(be, HW, H, W, need - 1)) == be.M3S_EINVAL  # workspace too small
    assert call(_args(be, HW, H, W + 1, need)) == be.M3S_EINVAL  # HW != H * W
    assert call(_args(be, 0, 0, 0, need)) == be.M3S_EINVAL
    for name in ("Xf_canon", "Cf_sum", "Xk_canon", "Ck_sum", "idx_f2k", "valid_match", "Qk", "T_WCf", "T_WCk",
                 "T_WCf_out", "T_CkCf_out", "info", "stats", "workspace"):
        a = _args(be, HW, H, W, need)
        setattr(a, name, None)
        assert call(a) == be.M3S_EINVAL, name
    a = _args(be, HW, H, W, need)
    a.Nf = 0  # an empty pointmap has no average confidence
    assert call(a) == be.M3S_EINVAL


def _cpu_inputs(H=4, W=5):
    HW = H * W
    X = torch.zeros(HW, 3)
    C = torch.ones(HW, 1)
    idx = torch.zeros(HW, dtype=torch.int32)
    valid = torch.ones(HW, 1, dtype=torch.bool)
    T = torch.tensor([[0.0, 0, 0, 0, 0, 0, 1, 1]])
    return [X, C, 1, X, C, 1, idx, valid, C, T, T, None, (H, W), 0.0, 1.5, 0.003, 10.0, 1.345, 5, 1e-3, 1e-3]


def test_cpu_tensors_rejected(be):
    from mast3r_slam_amd import tracker

    assert callable(tracker.FrameTracker)
    for k in ("C_conf", "Q_conf", "min_match_frac", "match_frac_thresh"):
        assert k in tracker.TRACKING_CFG
    with pytest.raises(RuntimeError, match="ROCm device"):  # no CPU path
        be.track_frame(*_cpu_inputs())
    bad = _cpu_inputs()
    bad[0] = torch.zeros(3, 20).t()
    with pytest.raises(RuntimeError, match="contiguous"):
        be.track_frame(*bad)

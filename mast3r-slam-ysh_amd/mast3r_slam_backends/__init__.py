"""``mast3r_slam_backends`` — drop-in for the reference's CUDA extension module,
backed by the MI355X HIP library ``libm3s_gn.so`` through its C ABI
(``include/m3s_gn.h``, ``include/m3s_match.h``).

Reference interface (``/root/reference/mast3r_slam/backend/src/gn.cpp:116-122``):
same module name, same function names, same positional arguments, same
in-place update of ``Twc`` and the same return value ``[dx]`` (the last GN step,
``[N-1, 7]`` float32). Callers: ``global_opt.py:140-155`` (rays) and
``global_opt.py:190-210`` (calib).

Error behaviour: like ``TORCH_CHECK(x.is_contiguous())`` (``gn.cpp:14-21``) a
non-contiguous input raises ``RuntimeError("<name> must be contiguous")``. In
addition, tensors that are not on a ROCm device, or have the wrong dtype,
raise ``RuntimeError`` — there is no CPU fallback: without the HIP library this
module fails at import.

New entry points (the reference tracker has no backend call, tracker.py:173-266):
``track_rays_sim3`` and ``track_calib_sim3``, and ``track_frame``: the rest of
FrameTracker.track between the matching and the fusion (gathers, the calib ray
constraint, valid_opt, the three counts of the skip / new-keyframe decisions)
in three launches in front of the same tracker launches.

``iter_proj`` / ``refine_matches`` (gn.cpp:84-114, matching_kernels.cu) run
the HIP matching kernels with the reference's signatures and return values.
``match_dense`` (new) is the whole of matching.py:52-90 plus the caller's
quality combine and match count, from the network's outputs to the rows the
GN entry points, the edge store and the trackers consume, in three launches.

``asmk_*`` (new; include/m3s_retrieval.h) are the ASMK retrieval steps the
reference runs on the host after its torch quantize: aggregate (residual sums,
binarise, pack), search (Hamming similarity, scores, top-k) and append, on an
``AsmkHandle``; ``mast3r_slam_amd.retrieval.RetrievalDatabase`` is built on them.
``asmk_centroid_norms`` and ``asmk_quantize`` are that quantize itself as a
fused distance and top-MA kernel (no distance matrix), for callers without torch
and for ``RetrievalDatabase(quantizer="device")``.

``rope_2d`` (new; include/m3s_rope.h) is the 2-D rotary position embedding of
MASt3R's attention, in place on the q or k slice of a qkv buffer, one launch;
``mast3r_slam_amd.rope`` puts it into a loaded model.

``attention_rope`` (new; include/m3s_attn.h) is the attention core between an
attention's ``Linear``s: RoPE2D of q and k, scores, softmax and the product
with v in one launch, fp32, head dimension 64, written in the [B, N, C] layout
``proj`` takes; ``mast3r_slam_amd.attention`` puts it into a loaded model.

``head_postprocess`` (new; include/m3s_head.h) is the tail of MASt3R's
catmlp+dpt head: from the DPT map and the local-feature MLP's output to X, C, D
and Q in the slots and dtypes ``match_dense``, ``track_frame`` and the factor
graph take, one launch; ``mast3r_slam_amd.head`` puts it into a loaded model.
"""
from __future__ import annotations

import ctypes
import math
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libm3s_gn.so"
LIB_PATH = os.environ.get("M3S_LIB") or os.path.join(_HERE, LIB_NAME)  # override: experiments only
# the same sources built with -DM3S_TEST_PATHS: the A/B reference solver paths
# and test hooks, for the tests that compare against them (never the product)
TEST_LIB_PATH = os.path.join(_HERE, "libm3s_gn_test.so")

M3S_OK, M3S_EINVAL, M3S_ELAUNCH, M3S_ETOOLARGE = 0, 1, 2, 3
MODE_POINTS, MODE_RAYS, MODE_CALIB = 0, 1, 2
INFO_ITERS, INFO_SOLVE_FAIL, INFO_BAD_EDGE, INFO_CONVERGED, INFO_N_UNIQUE = 0, 1, 2, 3, 4
EDGE_SUM_STRIDE = 36

_VP = ctypes.c_void_p


class GnArgs(ctypes.Structure):
    """Mirror of ``m3s_gn_args`` (include/m3s_gn.h)."""

    _fields_ = [
        ("Twc", _VP), ("Xs", _VP), ("Cs", _VP), ("ii", _VP), ("jj", _VP),
        ("idx_ii2jj", _VP), ("valid_match", _VP), ("Q", _VP), ("K", _VP),
        ("N", ctypes.c_int64), ("HW", ctypes.c_int64), ("E", ctypes.c_int64),
        ("mode", ctypes.c_int),
        ("sigma_a", ctypes.c_float), ("sigma_b", ctypes.c_float),
        ("C_thresh", ctypes.c_float), ("Q_thresh", ctypes.c_float),
        ("height", ctypes.c_int), ("width", ctypes.c_int), ("pixel_border", ctypes.c_int),
        ("z_eps", ctypes.c_float),
        ("max_iter", ctypes.c_int), ("delta_thresh", ctypes.c_float),
        ("dx_out", _VP), ("info", _VP),
        ("workspace", _VP), ("workspace_bytes", ctypes.c_size_t),
        ("idx_i32", ctypes.c_int),
    ]


class IterProjArgs(ctypes.Structure):
    """Mirror of ``m3s_iter_proj_args`` (include/m3s_match.h)."""

    _fields_ = [
        ("rays_img", _VP), ("pts_3d_norm", _VP), ("p_init", _VP),
        ("B", ctypes.c_int64), ("H", ctypes.c_int64), ("W", ctypes.c_int64), ("N", ctypes.c_int64),
        ("max_iter", ctypes.c_int), ("lambda_init", ctypes.c_float), ("cost_thresh", ctypes.c_float),
        ("p_new", _VP), ("converged", _VP),
    ]


class RefineArgs(ctypes.Structure):
    """Mirror of ``m3s_refine_args`` (include/m3s_match.h)."""

    _fields_ = [
        ("D11", _VP), ("D21", _VP), ("p1", _VP),
        ("B", ctypes.c_int64), ("H", ctypes.c_int64), ("W", ctypes.c_int64), ("N", ctypes.c_int64),
        ("F", ctypes.c_int64), ("dtype", ctypes.c_int), ("radius", ctypes.c_int),
        ("dilation_max", ctypes.c_int), ("p1_new", _VP),
    ]


class MatchDenseArgs(ctypes.Structure):
    """Mirror of ``m3s_match_dense_args`` (include/m3s_match.h)."""

    _fields_ = [
        ("X11", _VP), ("X21", _VP), ("D11", _VP), ("D21", _VP), ("Q11", _VP), ("Q21", _VP),
        ("idx_init", _VP),
        ("B", ctypes.c_int64), ("H", ctypes.c_int64), ("W", ctypes.c_int64), ("F", ctypes.c_int64),
        ("dtype", ctypes.c_int), ("max_iter", ctypes.c_int), ("lambda_init", ctypes.c_float),
        ("cost_thresh", ctypes.c_float), ("dist_thresh", ctypes.c_float), ("radius", ctypes.c_int),
        ("dilation_max", ctypes.c_int), ("Q_conf", ctypes.c_float),
        ("idx", _VP), ("valid", _VP), ("Q", _VP),
        ("idx_stride", ctypes.c_int64), ("valid_stride", ctypes.c_int64), ("Q_stride", ctypes.c_int64),
        ("n_valid", _VP), ("workspace", _VP), ("workspace_bytes", ctypes.c_size_t),
    ]


class FuseArgs(ctypes.Structure):
    """Mirror of ``m3s_fuse_args`` (include/m3s_fuse.h)."""

    _fields_ = [
        ("X_canon", _VP), ("C", _VP), ("X_new", _VP), ("C_new", _VP), ("T", _VP),
        ("HW", ctypes.c_int64), ("mode", ctypes.c_int),
    ]


class PrepRaysArgs(ctypes.Structure):
    """Mirror of ``m3s_prep_rays_args`` (include/m3s_fuse.h)."""

    _fields_ = [
        ("X11", _VP), ("X21", _VP), ("B", ctypes.c_int64), ("H", ctypes.c_int64),
        ("W", ctypes.c_int64), ("rays_img", _VP), ("pts_norm", _VP),
    ]


class TrackArgs(ctypes.Structure):
    """Mirror of ``m3s_track_args`` (include/m3s_gn.h)."""

    _fields_ = [
        ("Xf", _VP), ("Xk", _VP), ("Qk", _VP), ("valid", _VP), ("T_WCf", _VP), ("T_WCk", _VP),
        ("K", _VP), ("HW", ctypes.c_int64),
        ("height", ctypes.c_int), ("width", ctypes.c_int), ("pixel_border", ctypes.c_int),
        ("z_eps", ctypes.c_float), ("sigma_a", ctypes.c_float), ("sigma_b", ctypes.c_float),
        ("huber_k", ctypes.c_float), ("max_iters", ctypes.c_int),
        ("rel_error", ctypes.c_float), ("delta_norm", ctypes.c_float),
        ("sync_every", ctypes.c_int),
        ("T_WCf_out", _VP), ("T_CkCf_out", _VP), ("info", _VP),
        ("workspace", _VP), ("workspace_bytes", ctypes.c_size_t),
    ]


class TrackFrameArgs(ctypes.Structure):
    """Mirror of ``m3s_track_frame_args`` (include/m3s_gn.h)."""

    _fields_ = [
        ("Xf_canon", _VP), ("Cf_sum", _VP), ("Xk_canon", _VP), ("Ck_sum", _VP),
        ("idx_f2k", _VP), ("valid_match", _VP), ("Qk", _VP), ("T_WCf", _VP), ("T_WCk", _VP), ("K", _VP),
        ("HW", ctypes.c_int64), ("Nf", ctypes.c_int32), ("Nk", ctypes.c_int32),
        ("height", ctypes.c_int), ("width", ctypes.c_int),
        ("C_conf", ctypes.c_float), ("Q_conf", ctypes.c_float),
        ("pixel_border", ctypes.c_int), ("z_eps", ctypes.c_float),
        ("sigma_a", ctypes.c_float), ("sigma_b", ctypes.c_float), ("huber_k", ctypes.c_float),
        ("max_iters", ctypes.c_int), ("rel_error", ctypes.c_float), ("delta_norm", ctypes.c_float),
        ("sync_every", ctypes.c_int),
        ("T_WCf_out", _VP), ("T_CkCf_out", _VP), ("info", _VP), ("stats", _VP),
        ("Xf_out", _VP), ("Xk_out", _VP), ("valid_opt_out", _VP),
        ("workspace", _VP), ("workspace_bytes", ctypes.c_size_t),
    ]


STAT_N_OPT, STAT_N_KF, STAT_N_UNIQUE = 0, 1, 2

# every symbol include/m3s_gn.h declares
EXPORTS = (
    "m3s_gn_workspace_size", "m3s_gauss_newton_points", "m3s_gauss_newton_rays",
    "m3s_gauss_newton_calib", "m3s_gn_prepare", "m3s_gn_linearize", "m3s_gn_solve", "m3s_gn_release",
    "m3s_track_workspace_size", "m3s_track_rays_sim3", "m3s_track_calib_sim3", "m3s_version",
    "m3s_sparse_plan_debug", "m3s_gn_layout_debug", "m3s_iter_proj", "m3s_refine_matches",
    "m3s_fuse_pointmap", "m3s_prep_rays", "m3s_debug_stamps", "m3s_debug_sim3",
    "m3s_debug_copy", "m3s_set_knob", "m3s_debug_call_timing", "m3s_debug_call_times",
    "m3s_match_dense_workspace_size", "m3s_match_dense",
    "m3s_track_frame_workspace_size", "m3s_track_frame",
)
FILTER_MODES = {"weighted_pointmap": 0, "indep_conf": 1, "recent": 2, "weighted_spherical": 3}

# every symbol include/m3s_retrieval.h declares
RETRIEVAL_EXPORTS = (
    "m3s_asmk_store_size", "m3s_asmk_workspace_size", "m3s_asmk_store_layout", "m3s_asmk_workspace_layout",
    "m3s_asmk_reset", "m3s_asmk_aggregate", "m3s_asmk_search", "m3s_asmk_append",
    "m3s_asmk_quantize_workspace_size", "m3s_asmk_centroid_norms", "m3s_asmk_quantize",
)
ASMK_MAX_PAIRS, ASMK_MAX_K = 4096, 64
ASMK_QUANTIZE_MAX_MA = 8
ASMK_INFO_BAD_WORD, ASMK_INFO_FULL = 1, 2
ASMK_STORE_SECTIONS = ("header", "img_ptr", "word", "codes", "total")
ASMK_WS_SECTIONS = ("counts", "slot", "words", "start", "members", "codes", "scores", "out", "total")


class AsmkOut(ctypes.Structure):
    """Mirror of ``m3s_asmk_out`` (include/m3s_retrieval.h)."""

    _fields_ = [
        ("count", ctypes.c_int32), ("n_images", ctypes.c_int32), ("info", ctypes.c_int32),
        ("n_query_words", ctypes.c_int32), ("idx", ctypes.c_int32 * ASMK_MAX_K),
        ("score", ctypes.c_double * ASMK_MAX_K),
    ]


class AsmkDb(ctypes.Structure):
    """Mirror of ``m3s_asmk_db`` (include/m3s_retrieval.h)."""

    _fields_ = [
        ("store", _VP), ("store_bytes", ctypes.c_size_t), ("workspace", _VP), ("workspace_bytes", ctypes.c_size_t),
        ("cap_images", ctypes.c_int64), ("cap_entries", ctypes.c_int64), ("Kc", ctypes.c_int64),
        ("D", ctypes.c_int64),
    ]


class AsmkAggregateArgs(ctypes.Structure):
    """Mirror of ``m3s_asmk_aggregate_args`` (include/m3s_retrieval.h)."""

    _fields_ = [
        ("db", AsmkDb), ("des", _VP), ("centroids", _VP), ("assign", _VP),
        ("n", ctypes.c_int64), ("ma", ctypes.c_int64), ("query_ma", ctypes.c_int), ("build_ma", ctypes.c_int),
    ]


class AsmkSearchArgs(ctypes.Structure):
    """Mirror of ``m3s_asmk_search_args`` (include/m3s_retrieval.h)."""

    _fields_ = [
        ("db", AsmkDb), ("n_images", ctypes.c_int64), ("k", ctypes.c_int), ("alpha", ctypes.c_float),
        ("similarity_threshold", ctypes.c_float), ("min_thresh", ctypes.c_double),
    ]


class AsmkQuantizeArgs(ctypes.Structure):
    """Mirror of ``m3s_asmk_quantize_args`` (include/m3s_retrieval.h)."""

    _fields_ = [
        ("des", _VP), ("centroids", _VP), ("norms", _VP),
        ("n", ctypes.c_int64), ("Kc", ctypes.c_int64), ("D", ctypes.c_int64), ("ma", ctypes.c_int),
        ("assign", _VP), ("dist", _VP), ("workspace", _VP), ("workspace_bytes", ctypes.c_size_t),
    ]


# every symbol include/m3s_rope.h declares
ROPE_EXPORTS = ("m3s_rope_2d",)
ROPE_F32, ROPE_F16, ROPE_BF16 = 0, 1, 2


class RopeArgs(ctypes.Structure):
    """Mirror of ``m3s_rope_args`` (include/m3s_rope.h)."""

    _fields_ = [
        ("tokens", _VP), ("pos", _VP),
        ("B", ctypes.c_int64), ("N", ctypes.c_int64), ("H", ctypes.c_int64), ("D", ctypes.c_int64),
        ("stride_b", ctypes.c_int64), ("stride_n", ctypes.c_int64),
        ("base", ctypes.c_float), ("f0", ctypes.c_float), ("dtype", ctypes.c_int),
    ]


# every symbol include/m3s_attn.h declares
ATTN_EXPORTS = ("m3s_attn_rope",)
ATTN_HEAD_DIM = 64


class AttnArgs(ctypes.Structure):
    """Mirror of ``m3s_attn_args`` (include/m3s_attn.h)."""

    _fields_ = [
        ("q", _VP), ("k", _VP), ("v", _VP), ("out", _VP), ("qpos", _VP), ("kpos", _VP),
        ("B", ctypes.c_int64), ("Nq", ctypes.c_int64), ("Nk", ctypes.c_int64), ("H", ctypes.c_int64),
        ("D", ctypes.c_int64),
        ("q_sb", ctypes.c_int64), ("q_sn", ctypes.c_int64), ("k_sb", ctypes.c_int64), ("k_sn", ctypes.c_int64),
        ("v_sb", ctypes.c_int64), ("v_sn", ctypes.c_int64), ("o_sb", ctypes.c_int64), ("o_sn", ctypes.c_int64),
        ("base", ctypes.c_float), ("f0", ctypes.c_float), ("scale", ctypes.c_float), ("dtype", ctypes.c_int),
    ]


# every symbol include/m3s_head.h declares
HEAD_EXPORTS = ("m3s_head_postprocess",)
HEAD_F32, HEAD_F16 = 0, 1
HEAD_GENERIC = 1  # flags


class HeadArgs(ctypes.Structure):
    """Mirror of ``m3s_head_args`` (include/m3s_head.h)."""

    _fields_ = [
        ("pts", _VP), ("feat", _VP), ("X", _VP), ("C", _VP), ("D", _VP), ("Q", _VP),
        ("B", ctypes.c_int64), ("H", ctypes.c_int64), ("W", ctypes.c_int64), ("P", ctypes.c_int64),
        ("F", ctypes.c_int64), ("ds", ctypes.c_int64),
        ("sbX", ctypes.c_int64), ("sbC", ctypes.c_int64), ("sbD", ctypes.c_int64), ("sbQ", ctypes.c_int64),
        ("conf_vmin", ctypes.c_float), ("conf_vmax", ctypes.c_float),
        ("dconf_vmin", ctypes.c_float), ("dconf_vmax", ctypes.c_float),
        ("desc_dtype", ctypes.c_int), ("flags", ctypes.c_int),
    ]


def _load(path=LIB_PATH):
    if not os.path.exists(path):
        raise ImportError(
            f"mast3r_slam_backends: {path} is missing; build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)"
        )
    lib = ctypes.CDLL(path)
    P = ctypes.POINTER
    lib.m3s_gn_workspace_size.restype = ctypes.c_size_t
    lib.m3s_gn_workspace_size.argtypes = [ctypes.c_int64] * 3
    for f in ("m3s_gauss_newton_points", "m3s_gauss_newton_rays", "m3s_gauss_newton_calib",
              "m3s_gn_prepare"):
        getattr(lib, f).restype = ctypes.c_int
        getattr(lib, f).argtypes = [P(GnArgs), _VP]
    lib.m3s_gn_linearize.restype = ctypes.c_int
    lib.m3s_gn_linearize.argtypes = [P(GnArgs), ctypes.c_int64, ctypes.c_int64, _VP, _VP]
    lib.m3s_gn_solve.restype = ctypes.c_int
    lib.m3s_gn_solve.argtypes = [P(GnArgs), _VP, _VP]
    lib.m3s_gn_release.restype = ctypes.c_int
    lib.m3s_gn_release.argtypes = [P(GnArgs), _VP]
    lib.m3s_track_workspace_size.restype = ctypes.c_size_t
    lib.m3s_track_workspace_size.argtypes = [ctypes.c_int64]
    for f in ("m3s_track_rays_sim3", "m3s_track_calib_sim3"):
        getattr(lib, f).restype = ctypes.c_int
        getattr(lib, f).argtypes = [P(TrackArgs), _VP]
    lib.m3s_track_frame_workspace_size.restype = ctypes.c_size_t
    lib.m3s_track_frame_workspace_size.argtypes = [ctypes.c_int64]
    lib.m3s_track_frame.restype = ctypes.c_int
    lib.m3s_track_frame.argtypes = [P(TrackFrameArgs), _VP]
    lib.m3s_version.restype = ctypes.c_char_p
    lib.m3s_version.argtypes = []
    lib.m3s_sparse_plan_debug.restype = ctypes.c_int64
    lib.m3s_sparse_plan_debug.argtypes = [ctypes.c_int32, ctypes.c_int64, _VP, _VP, ctypes.c_int32, ctypes.c_int32, _VP,
                                          ctypes.c_int64, _VP]
    lib.m3s_fuse_pointmap.restype = ctypes.c_int
    lib.m3s_fuse_pointmap.argtypes = [P(FuseArgs), _VP]
    lib.m3s_prep_rays.restype = ctypes.c_int
    lib.m3s_prep_rays.argtypes = [P(PrepRaysArgs), _VP]
    lib.m3s_iter_proj.restype = ctypes.c_int
    lib.m3s_iter_proj.argtypes = [P(IterProjArgs), _VP]
    lib.m3s_refine_matches.restype = ctypes.c_int
    lib.m3s_refine_matches.argtypes = [P(RefineArgs), _VP]
    lib.m3s_match_dense_workspace_size.restype = ctypes.c_size_t
    lib.m3s_match_dense_workspace_size.argtypes = [ctypes.c_int64] * 3
    lib.m3s_match_dense.restype = ctypes.c_int
    lib.m3s_match_dense.argtypes = [P(MatchDenseArgs), _VP]
    lib.m3s_debug_stamps.restype = ctypes.c_int
    lib.m3s_debug_stamps.argtypes = [ctypes.c_int, _VP]
    lib.m3s_debug_sim3.restype = ctypes.c_int
    lib.m3s_debug_sim3.argtypes = [ctypes.c_int, _VP, _VP, _VP, ctypes.c_int64, _VP]
    lib.m3s_set_knob.restype = ctypes.c_int
    lib.m3s_set_knob.argtypes = [ctypes.c_char_p, ctypes.c_int]
    lib.m3s_debug_copy.restype = ctypes.c_int
    lib.m3s_debug_copy.argtypes = [_VP, _VP, ctypes.c_int64, ctypes.c_int, _VP]
    lib.m3s_debug_call_timing.restype = ctypes.c_int
    lib.m3s_debug_call_timing.argtypes = [ctypes.c_int]
    lib.m3s_debug_call_times.restype = ctypes.c_int
    lib.m3s_debug_call_times.argtypes = [_VP, _VP, ctypes.c_int]
    lib.m3s_gn_layout_debug.restype = ctypes.c_size_t
    lib.m3s_gn_layout_debug.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _VP]
    for f in RETRIEVAL_EXPORTS:  # include/m3s_retrieval.h
        fn = getattr(lib, f)
        if f == "m3s_asmk_quantize_workspace_size":
            fn.restype = ctypes.c_size_t
            fn.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
        elif f == "m3s_asmk_centroid_norms":
            fn.restype = ctypes.c_int
            fn.argtypes = [_VP, ctypes.c_int64, ctypes.c_int64, _VP, _VP]
        elif f.endswith("_size") or f.endswith("_layout"):
            fn.restype = ctypes.c_size_t
            fn.argtypes = [ctypes.c_int64] * 3 + ([P(ctypes.c_size_t)] if f.endswith("_layout") else [])
        else:
            fn.restype = ctypes.c_int
            fn.argtypes = [P({"m3s_asmk_aggregate": AsmkAggregateArgs,
                              "m3s_asmk_search": AsmkSearchArgs,
                              "m3s_asmk_quantize": AsmkQuantizeArgs}.get(f, AsmkDb)), _VP]
    lib.m3s_rope_2d.restype = ctypes.c_int  # include/m3s_rope.h
    lib.m3s_rope_2d.argtypes = [P(RopeArgs), _VP]
    lib.m3s_attn_rope.restype = ctypes.c_int  # include/m3s_attn.h
    lib.m3s_attn_rope.argtypes = [P(AttnArgs), _VP]
    lib.m3s_head_postprocess.restype = ctypes.c_int  # include/m3s_head.h
    lib.m3s_head_postprocess.argtypes = [P(HeadArgs), _VP]
    return lib


_lib = _load()


def load_test_library():
    """The test build of the library (A/B reference paths, test hooks)."""
    return _load(TEST_LIB_PATH)


def version() -> str:
    return _lib.m3s_version().decode()


PLAN_SECTIONS = ("perm", "col_ptr", "col_row", "col_slot", "lev_ptr", "lev_col", "dtr_ptr",
                 "dtr_slot", "dtr_p", "task_lev_ptr", "task_dst", "task_col", "task_tr_ptr", "tr_a",
                 "tr_b", "asm_ptr", "asm_edge", "g_ptr", "g_edge", "ctask_ptr", "items", "wave_ptr", "witems",
                 "part_q0", "part_q1", "part_tgt", "dpart_ptr", "opart_ptr", "clq", "corder", "ctask0")


LAYOUT_SECTIONS = ("flags", "rank_i", "rank_j", "first", "partials", "edge_sums", "A", "fin",
                   "plan", "Lblk", "Dinv", "tail", "eorder", "planes", "total")


SIM3_OPS = {"exp": (0, 7, None, 8), "retract": (1, 7, 8, 8), "compose": (2, 8, 8, 8), "inverse": (3, 8, None, 8),
            "relative": (4, 8, 8, 8), "act": (5, 8, 3, 3), "act_matrix": (6, 8, 3, 3), "adjT_inv": (7, 8, None, 49),
            "retract_f32": (8, 7, 8, 8)}


def debug_sim3(op: str, a: torch.Tensor, b: torch.Tensor = None) -> torch.Tensor:
    """The device Sim(3) helpers of the hot path on [n, ...] float32 device
    tensors (m3s_debug_sim3; diagnostics/tests). op in SIM3_OPS."""
    code, wa, wb, wo = SIM3_OPS[op]
    a = a.contiguous()
    _check(a, "a", torch.float32)
    n = a.numel() // wa
    if a.numel() != n * wa:
        raise RuntimeError(f"debug_sim3({op}): a must be [n, {wa}]")
    if wb is not None:
        if b is None:
            raise RuntimeError(f"debug_sim3({op}) needs b")
        b = b.contiguous()
        _check(b, "b", torch.float32)
        if b.numel() != n * wb:
            raise RuntimeError(f"debug_sim3({op}): b must be [n, {wb}]")
    out = torch.empty(n, wo, dtype=torch.float32, device=a.device)
    _raise(_lib.m3s_debug_sim3(code, _p(a), _p(b), _p(out), n, _stream(a.device)), "m3s_debug_sim3")
    return out


def set_knob(name: str, value: int) -> int:
    """Set a solver knob for the calls that follow (include/m3s_gn.h
    m3s_set_knob); returns the previous value."""
    old = _lib.m3s_set_knob(name.encode(), int(value))
    if old == -(1 << 30):
        raise RuntimeError(f"unknown knob {name!r}")
    return old


class knob:
    """``with knob("df", 0): ...`` — a knob set for the block, restored after."""

    def __init__(self, name: str, value: int):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = set_knob(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_knob(self.name, self.old)


def debug_call_timing(enable: bool) -> None:
    """Turn in-call launch timing on or off (m3s_debug_call_timing); the
    record of the calls that follow is read by debug_call_times()."""
    _raise(_lib.m3s_debug_call_timing(1 if enable else 0), "m3s_debug_call_timing")


def debug_call_times(cap: int = 4096):
    """[(kind, ms)] of the timed calls since debug_call_timing(True), in launch
    order; kind 0 = first-iteration (gathering) linearize, 1 = packed
    linearize, 2 = solve launches of one iteration."""
    import numpy as np

    ms = np.zeros(cap, np.float32)
    kinds = np.zeros(cap, np.int32)
    n = _lib.m3s_debug_call_times(ms.ctypes.data, kinds.ctypes.data, cap)
    if n < 0:
        _raise(n, "m3s_debug_call_times")
    n = min(n, cap)
    return [(int(kinds[k]), float(ms[k])) for k in range(n)]


def debug_copy(src: torch.Tensor, dst: torch.Tensor, blocks: int = 4096):
    """dst <- src by the 16-B streaming copy kernel (m3s_debug_copy)."""
    _check(src, "src")
    _check(dst, "dst")
    nb = src.numel() * src.element_size()
    if dst.numel() * dst.element_size() < nb:
        raise RuntimeError("debug_copy: dst too small")
    _raise(_lib.m3s_debug_copy(_p(src), _p(dst), nb, int(blocks), _stream(src.device)), "m3s_debug_copy")


def workspace_layout(N, HW, E):
    """Byte offsets of the GN workspace sections (diagnostics/tests)."""
    offs = (ctypes.c_size_t * len(LAYOUT_SECTIONS))()
    _lib.m3s_gn_layout_debug(int(N), int(HW), int(E), offs)
    return dict(zip(LAYOUT_SECTIONS, list(offs)))


def sparse_plan(N, ri, rj, split=0, max_parts=0):
    """Host symbolic plan of the block-sparse LLT (diagnostics/tests; CPU only).
    split > 0: long update lists cut into PART items (global-factor solves).
    The dense tail (clq) follows M3S_DENSE_TAIL_MIN like the solver."""
    import numpy as np

    ri = np.ascontiguousarray(ri, dtype=np.int32)
    rj = np.ascontiguousarray(rj, dtype=np.int32)
    meta = np.zeros(4 + len(PLAN_SECTIONS), np.int32)
    P = ctypes.c_void_p
    args = (int(N), ri.size, P(ri.ctypes.data), P(rj.ctypes.data), int(split), int(max_parts))
    n = _lib.m3s_sparse_plan_debug(*args, None, 0, P(meta.ctypes.data))
    out = np.zeros(max(n, 1), np.int32)
    _lib.m3s_sparse_plan_debug(*args, P(out.ctypes.data), n, P(meta.ctypes.data))
    offs = list(meta[3:3 + len(PLAN_SECTIONS)]) + [n]
    plan = {"m": int(meta[0]), "S": int(meta[1]), "levels": int(meta[2]),
            "n_parts": int(meta[3 + len(PLAN_SECTIONS)])}
    for k, name in enumerate(PLAN_SECTIONS):
        plan[name] = out[offs[k]:]
    m, S, L, NP = plan["m"], plan["S"], plan["levels"], plan["n_parts"]
    T = int(plan["task_lev_ptr"][L])
    sp = NP > 0 or split > 0
    nc = int(plan["clq"][0])  # dense-tail columns: not dataflow items
    plan["nc"] = nc
    n_items = (m - nc) + (T - nc * (nc - 1) // 2) + NP
    lens = {"perm": m, "col_ptr": m + 1, "lev_ptr": L + 1, "lev_col": m, "dtr_ptr": m + 1,
            "task_lev_ptr": L + 1, "task_dst": T, "task_col": T, "task_tr_ptr": T + 1,
            "asm_ptr": S + 1, "g_ptr": m + 1, "ctask_ptr": m + 1, "clq": 2 + nc + nc * nc,
            "items": n_items, "wave_ptr": 2, "witems": n_items,
            "part_q0": NP, "part_q1": NP, "part_tgt": NP,
            "dpart_ptr": m + 1 if sp else 0, "opart_ptr": T + 1 if sp else 0,
            "corder": m - nc, "ctask0": m}
    for name, ln in lens.items():
        plan[name] = plan[name][:ln]
    nnz = int(plan["col_ptr"][m])
    plan["col_row"], plan["col_slot"] = plan["col_row"][:nnz], plan["col_slot"][:nnz]
    nd = int(plan["dtr_ptr"][m])
    plan["dtr_slot"], plan["dtr_p"] = plan["dtr_slot"][:nd], plan["dtr_p"][:nd]
    nt = int(plan["task_tr_ptr"][T])
    plan["tr_a"], plan["tr_b"] = plan["tr_a"][:nt], plan["tr_b"][:nt]
    plan["asm_edge"] = plan["asm_edge"][:int(plan["asm_ptr"][S])]
    plan["g_edge"] = plan["g_edge"][:int(plan["g_ptr"][m])]
    return plan


# ------------------------------------------------------------------ checks --
def _check(t: torch.Tensor, name: str, dtype=None):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} must be on a ROCm device (got {t.device}); no CPU path")
    if dtype is not None and t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
        raise RuntimeError(f"{name} must be {dtype} (got {t.dtype})")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _raise(rc, fn):
    if rc == M3S_OK:
        return
    msg = {M3S_EINVAL: "invalid argument", M3S_ELAUNCH: "HIP launch failed",
           M3S_ETOOLARGE: "problem size exceeds this build's limits"}.get(rc, f"error {rc}")
    raise RuntimeError(f"{fn}: {msg}")


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def make_gn_args(mode, Twc, Xs, Cs, ii, jj, idx_ii2jj, valid_match, Q, K=None, *, sigma_a=0.0,
                 sigma_b=0.0, C_thresh=0.0, Q_thresh=0.0, height=0, width=0, pixel_border=0,
                 z_eps=0.0, max_iter=0, delta_thresh=0.0, dx=None, info=None, workspace=None):
    """Validate reference-layout tensors and fill an ``m3s_gn_args``. Returns
    (args, keepalive) — keepalive holds every tensor the struct points to."""
    _check(Twc, "Twc", torch.float32)
    _check(Xs, "Xs", torch.float32)
    _check(Cs, "Cs", torch.float32)
    if K is not None:
        _check(K, "K", torch.float32)
    _check(ii, "ii", torch.int64)
    _check(jj, "jj", torch.int64)
    # int64 as the reference passes it; int32 from the device edge store
    _check(idx_ii2jj, "idx_ii2jj", (torch.int64, torch.int32))
    _check(valid_match, "valid_match", torch.bool)
    _check(Q, "Q", torch.float32)
    N, HW = int(Xs.shape[0]), int(Xs.shape[1])
    E = int(ii.shape[0])
    if Xs.dim() != 3 or Xs.shape[2] != 3:
        raise RuntimeError("Xs must be [N, HW, 3]")
    if Twc.numel() != 8 * N:
        raise RuntimeError(f"Twc must be [N, 8] with N = Xs.size(0) = {N}")
    if Cs.numel() != N * HW:
        raise RuntimeError("Cs must be [N, HW, 1]")
    if jj.numel() != E or idx_ii2jj.numel() != E * HW or valid_match.numel() != E * HW or Q.numel() != E * HW:
        raise RuntimeError("edge tensors must be [E, HW(,1)] with E = ii.size(0)")
    dev = Xs.device
    # no fill launches: m3s_gn_prepare zeroes dx and uploads info on the stream
    if dx is None:
        dx = torch.empty(max(N - 1, 0), 7, dtype=torch.float32, device=dev)
    if info is None:
        info = torch.empty(8, dtype=torch.int32, device=dev)
    ws_bytes = int(_lib.m3s_gn_workspace_size(N, HW, E))
    if workspace is None or workspace.numel() < ws_bytes:
        workspace = _workspace(ws_bytes, dev)
    a = GnArgs()
    a.Twc, a.Xs, a.Cs, a.ii, a.jj = _p(Twc), _p(Xs), _p(Cs), _p(ii), _p(jj)
    a.idx_ii2jj, a.valid_match, a.Q, a.K = _p(idx_ii2jj), _p(valid_match), _p(Q), _p(K)
    a.idx_i32 = 1 if idx_ii2jj.dtype == torch.int32 else 0
    a.N, a.HW, a.E, a.mode = N, HW, E, mode
    a.sigma_a, a.sigma_b = float(sigma_a), float(sigma_b)
    a.C_thresh, a.Q_thresh = float(C_thresh), float(Q_thresh)
    a.height, a.width, a.pixel_border = int(height), int(width), int(pixel_border)
    a.z_eps = float(z_eps)
    a.max_iter, a.delta_thresh = int(max_iter), float(delta_thresh)
    a.dx_out, a.info = _p(dx), _p(info)
    a.workspace, a.workspace_bytes = _p(workspace), workspace.numel()
    keep = dict(Twc=Twc, Xs=Xs, Cs=Cs, ii=ii, jj=jj, idx=idx_ii2jj, valid=valid_match, Q=Q, K=K,
                dx=dx, info=info, workspace=workspace)
    return a, keep


def _run_gn(fn_name, a, keep):
    st = _stream(keep["Xs"].device)
    rc = getattr(_lib, fn_name)(ctypes.byref(a), st)
    # the per-call workspace goes back to the caching allocator: drop its host
    # state too (m3s_gn_release: no stream sync; the call returns as soon as
    # its launches are queued)
    rc_rel = _lib.m3s_gn_release(ctypes.byref(a), st)
    _raise(rc, fn_name)
    _raise(rc_rel, "m3s_gn_release")
    return [keep["dx"]]


# ------------------------------------------------- reference entry points --
def gauss_newton_points(Twc, Xs, Cs, ii, jj, idx_ii2jj, valid_match, Q, sigma_point, C_thresh,
                        Q_thresh, max_iter, delta_thresh, *, info=None):
    """gn.cpp:3-27 / gn_kernels.cu:725-811."""
    a, keep = make_gn_args(MODE_POINTS, Twc, Xs, Cs, ii, jj, idx_ii2jj, valid_match, Q,
                           sigma_a=sigma_point, C_thresh=C_thresh, Q_thresh=Q_thresh,
                           max_iter=max_iter, delta_thresh=delta_thresh, info=info)
    return _run_gn("m3s_gauss_newton_points", a, keep)


def gauss_newton_rays(Twc, Xs, Cs, ii, jj, idx_ii2jj, valid_match, Q, sigma_ray, sigma_dist,
                      C_thresh, Q_thresh, max_iter, delta_thresh, *, info=None):
    """gn.cpp:29-54 / gn_kernels.cu:1140-1228."""
    a, keep = make_gn_args(MODE_RAYS, Twc, Xs, Cs, ii, jj, idx_ii2jj, valid_match, Q,
                           sigma_a=sigma_ray, sigma_b=sigma_dist, C_thresh=C_thresh,
                           Q_thresh=Q_thresh, max_iter=max_iter, delta_thresh=delta_thresh,
                           info=info)
    return _run_gn("m3s_gauss_newton_rays", a, keep)


def gauss_newton_calib(Twc, Xs, Cs, K, ii, jj, idx_ii2jj, valid_match, Q, height, width,
                       pixel_border, z_eps, sigma_pixel, sigma_depth, C_thresh, Q_thresh, max_iter,
                       delta_thresh, *, info=None):
    """gn.cpp:56-85 / gn_kernels.cu:1546-1638."""
    a, keep = make_gn_args(MODE_CALIB, Twc, Xs, Cs, ii, jj, idx_ii2jj, valid_match, Q, K,
                           sigma_a=sigma_pixel, sigma_b=sigma_depth, C_thresh=C_thresh,
                           Q_thresh=Q_thresh, height=height, width=width,
                           pixel_border=pixel_border, z_eps=z_eps, max_iter=max_iter,
                           delta_thresh=delta_thresh, info=info)
    return _run_gn("m3s_gauss_newton_calib", a, keep)


def iter_proj(rays_img_with_grad, pts_3d_norm, p_init, max_iter, lambda_init, cost_thresh):
    """gn.cpp:84-99 / matching_kernels.cu:119-296: per-pixel LM projection.

    rays_img_with_grad [B,H,W,9] f32, pts_3d_norm [B,N,3] f32, p_init [B,N,2]
    f32 -> [p_new [B,N,2] f32, converged [B,N] bool] (new tensors)."""
    for name, t in (("rays_img_with_grad", rays_img_with_grad), ("pts_3d_norm", pts_3d_norm),
                    ("p_init", p_init)):
        _check(t, name, torch.float32)
    B, H, W, C = rays_img_with_grad.shape
    Bn, N = int(p_init.shape[0]), int(p_init.shape[1])
    if C != 9 or Bn != B or tuple(pts_3d_norm.shape) != (B, N, 3) or tuple(p_init.shape) != (B, N, 2):
        raise RuntimeError("iter_proj: expected rays [B,H,W,9], pts_3d_norm [B,N,3], p_init [B,N,2]")
    dev = p_init.device
    p_new = torch.zeros(B, N, 2, dtype=torch.float32, device=dev)
    converged = torch.zeros(B, N, dtype=torch.bool, device=dev)
    a = IterProjArgs()
    a.rays_img, a.pts_3d_norm, a.p_init = _p(rays_img_with_grad), _p(pts_3d_norm), _p(p_init)
    a.B, a.H, a.W, a.N = B, H, W, N
    a.max_iter, a.lambda_init, a.cost_thresh = int(max_iter), float(lambda_init), float(cost_thresh)
    a.p_new, a.converged = _p(p_new), _p(converged)
    _raise(_lib.m3s_iter_proj(ctypes.byref(a), _stream(dev)), "m3s_iter_proj")
    return [p_new, converged]


def refine_matches(D11, D21, p1, radius, dilation_max):
    """gn.cpp:101-114 / matching_kernels.cu:25-116: dilated local search.

    D11 [B,H,W,F] f16 (or f32), D21 [B,N,F] same dtype, p1 [B,N,2] int64 (u, v)
    -> [p1_new [B,N,2] int64] (new tensor)."""
    _check(D11, "D11")
    _check(D21, "D21", D11.dtype)
    _check(p1, "p1", torch.int64)
    dt = {torch.float16: 0, torch.float32: 1}.get(D11.dtype)
    if dt is None:
        raise RuntimeError(f"refine_matches: descriptors must be float16 or float32 (got {D11.dtype})")
    B, H, W, F = D11.shape
    N = int(p1.shape[1])
    if tuple(D21.shape) != (B, N, F) or tuple(p1.shape) != (B, N, 2):
        raise RuntimeError("refine_matches: expected D11 [B,H,W,F], D21 [B,N,F], p1 [B,N,2]")
    p1_new = torch.zeros(B, N, 2, dtype=torch.int64, device=p1.device)
    a = RefineArgs()
    a.D11, a.D21, a.p1 = _p(D11), _p(D21), _p(p1)
    a.B, a.H, a.W, a.N, a.F = B, H, W, N, F
    a.dtype, a.radius, a.dilation_max = dt, int(radius), int(dilation_max)
    a.p1_new = _p(p1_new)
    _raise(_lib.m3s_refine_matches(ctypes.byref(a), _stream(p1.device)), "m3s_refine_matches")
    return [p1_new]


def _rows(t, name, dtype, B, HW):
    """Row stride (elements) of an output of match_dense: [B, HW(, 1)], the
    pixels of a row contiguous, the rows anywhere (every other row of an edge
    store is fine)."""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{name} must be a tensor on a ROCm device; no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype} (got {t.dtype})")
    if t.dim() == 3 and t.shape[2] == 1:
        t = t[:, :, 0]
    if t.dim() != 2 or t.shape[0] != B or t.shape[1] != HW:
        raise RuntimeError(f"{name} must be [{B}, {HW}(, 1)] (got {tuple(t.shape)})")
    if HW > 1 and t.stride(1) != 1:
        raise RuntimeError(f"{name}: the pixels of a row must be contiguous")
    stride = t.stride(0) if B > 1 else HW
    if stride < HW:
        raise RuntimeError(f"{name}: rows overlap (stride {stride} < {HW})")
    return stride


def match_dense_workspace_size(B, H, W):
    """Bytes of the match_dense workspace for B pairs of H x W views."""
    return int(_lib.m3s_match_dense_workspace_size(int(B), int(H), int(W)))


def _match_dense(X11, X21, D11, D21, Q11, Q21, idx_init, max_iter, lambda_init, cost_thresh,
                 dist_thresh, radius, dilation_max, Q_conf, out):
    """m3s_match_dense on checked tensors; descriptors float16 or float32 as given."""
    _check(X11, "X11", torch.float32)
    _check(X21, "X21", torch.float32)
    _check(D11, "D11", (torch.float16, torch.float32))
    _check(D21, "D21", D11.dtype)
    _check(Q11, "Q11", torch.float32)
    _check(Q21, "Q21", torch.float32)
    if X11.dim() != 4 or X11.shape[3] != 3:
        raise RuntimeError("match_dense: X11 must be [B,H,W,3]")
    B, H, W, _ = (int(x) for x in X11.shape)
    HW = H * W
    F = int(D11.shape[-1])
    if X21.numel() != B * HW * 3 or X21.shape[0] != B or X21.shape[-1] != 3:
        raise RuntimeError("match_dense: X21 must be [B,H,W,3] or [B,HW,3]")
    if tuple(D11.shape) != (B, H, W, F) or D21.numel() != B * HW * F or D21.shape[0] != B or D21.shape[-1] != F:
        raise RuntimeError("match_dense: expected D11 [B,H,W,F] and D21 [B,HW,F]")
    for name, q in (("Q11", Q11), ("Q21", Q21)):
        if q.numel() != B * HW or q.shape[0] != B:
            raise RuntimeError(f"match_dense: {name} must be [B,HW] (or [B,H,W], [B,HW,1])")
    dev = X11.device
    for name, t in (("X21", X21), ("D11", D11), ("D21", D21), ("Q11", Q11), ("Q21", Q21)):
        if t.device != dev:
            raise RuntimeError(f"match_dense: {name} is on {t.device}, X11 on {dev}")
    if idx_init is not None:
        _check(idx_init, "idx_init", torch.int64)
        if tuple(idx_init.shape) != (B, HW) or idx_init.device != dev:
            raise RuntimeError("match_dense: idx_init must be [B,HW] int64 on the inputs' device")
    n_valid = None
    if out is None:
        idx = torch.empty(B, HW, dtype=torch.int32, device=dev)
        valid = torch.empty(B, HW, 1, dtype=torch.bool, device=dev)
        Q = torch.empty(B, HW, 1, dtype=torch.float32, device=dev)
    else:
        idx, valid, Q = out[:3]
        n_valid = out[3] if len(out) > 3 else None
    strides = [_rows(t, name, dt, B, HW) for t, name, dt in
               ((idx, "out idx", torch.int32), (valid, "out valid", torch.bool), (Q, "out Q", torch.float32))]
    if any(t.device != dev for t in (idx, valid, Q)):
        raise RuntimeError("match_dense: out tensors must be on the inputs' device")
    if n_valid is None:
        n_valid = torch.empty(B, dtype=torch.int32, device=dev)
    else:
        _check(n_valid, "out n_valid", torch.int32)
        if n_valid.numel() != B or n_valid.device != dev:
            raise RuntimeError("match_dense: out n_valid must be [B] int32 on the inputs' device")
    need = match_dense_workspace_size(B, H, W)
    ws = _workspace(need, dev)
    a = MatchDenseArgs()
    a.X11, a.X21, a.D11, a.D21, a.Q11, a.Q21 = _p(X11), _p(X21), _p(D11), _p(D21), _p(Q11), _p(Q21)
    a.idx_init = _p(idx_init)
    a.B, a.H, a.W, a.F = B, H, W, F
    a.dtype = 0 if D11.dtype == torch.float16 else 1
    a.max_iter, a.lambda_init, a.cost_thresh = int(max_iter), float(lambda_init), float(cost_thresh)
    a.dist_thresh, a.radius, a.dilation_max = float(dist_thresh), int(radius), int(dilation_max)
    a.Q_conf = float(Q_conf)
    a.idx, a.valid, a.Q = _p(idx), _p(valid), _p(Q)
    a.idx_stride, a.valid_stride, a.Q_stride = strides
    a.n_valid = _p(n_valid)
    a.workspace, a.workspace_bytes = _p(ws), ws.numel()
    _raise(_lib.m3s_match_dense(ctypes.byref(a), _stream(dev)), "m3s_match_dense")
    del ws  # stream-ordered by the caching allocator
    return idx, valid, Q, n_valid


def match_dense(X11, X21, D11, D21, Q11, Q21, idx_init=None, *, max_iter=10, lambda_init=1e-8,
                convergence_thresh=1e-6, dist_thresh=1e-1, radius=3, dilation_max=5, Q_conf=1.5,
                out=None):
    """Dense matching to GN-ready rows in three launches (new entry point;
    m3s_match_dense): matching.py:52-90, then Q = sqrt(Q11[b, idx] * Q21)
    (global_opt.py:53-57, tracker.py:41) and the per-pair count of
    valid & (Q > Q_conf) (global_opt.py:59-66).

    X11 [B,H,W,3], X21 [B,H,W,3] (or [B,HW,3]) f32; D11 [B,H,W,F], D21
    [B,H,W,F] (or [B,HW,F]), cast with .half() when not float16 like the
    reference's caller (matching.py:80); Q11, Q21 [B,HW] f32 (or [B,H,W],
    [B,HW,1]); idx_init [B,HW] int64 or None (the reference's
    idx_1_to_2_init). The keyword defaults are base.yaml's matching section
    and local_opt.Q_conf.

    -> (idx int32 [B,HW], valid bool [B,HW,1], Q f32 [B,HW,1], n_valid int32
    [B]). out=(idx, valid, Q[, n_valid]) writes into the caller's tensors
    instead: their rows may be strided views (rows r0:r1:2 of an EdgeStore),
    the pixels of a row contiguous. No host synchronisation."""
    D11 = D11 if D11.dtype == torch.float16 else D11.half()
    D21 = D21 if D21.dtype == torch.float16 else D21.half()
    return _match_dense(X11, X21, D11, D21, Q11, Q21, idx_init, max_iter, lambda_init,
                        convergence_thresh, dist_thresh, radius, dilation_max, Q_conf, out)


def fuse_pointmap(X_canon, C, X_new, C_new, T=None, mode="weighted_pointmap"):
    """Keyframe pointmap fusion after tracking, in place (new entry point):
    X_canon/C <- filter(X_canon, C, T.act(X_new), C_new) — tracker.py:98-99 +
    Frame.update_pointmap (frame.py:41-100) for an initialised keyframe.
    X_canon, X_new [HW,3] f32; C, C_new [HW,1] (or [HW]) f32; T [8] or [1,8]."""
    _check(X_canon, "X_canon", torch.float32)
    _check(C, "C", torch.float32)
    _check(X_new, "X_new", torch.float32)
    _check(C_new, "C_new", torch.float32)
    if mode not in FILTER_MODES:
        raise RuntimeError(f"fuse_pointmap: unsupported filtering mode {mode!r}")
    HW = int(X_canon.shape[0])
    if X_canon.numel() != 3 * HW or X_new.numel() != 3 * HW or C.numel() != HW or C_new.numel() != HW:
        raise RuntimeError("fuse_pointmap: expected X [HW,3] and C [HW,1]")
    if T is not None:
        T = T.contiguous()
        _check(T, "T", torch.float32)
    a = FuseArgs()
    a.X_canon, a.C, a.X_new, a.C_new, a.T = _p(X_canon), _p(C), _p(X_new), _p(C_new), _p(T)
    a.HW, a.mode = HW, FILTER_MODES[mode]
    _raise(_lib.m3s_fuse_pointmap(ctypes.byref(a), _stream(X_canon.device)), "m3s_fuse_pointmap")


def prep_rays(X11, X21):
    """iter_proj inputs in one pass (new entry point; prep_for_iter_proj,
    matching.py:25-49): X11 [B,H,W,3], X21 [B,H,W,3] (or [B,HW,3]) f32 ->
    (rays_with_grad [B,H,W,9], pts3d_norm [B,HW,3])."""
    _check(X11, "X11", torch.float32)
    _check(X21, "X21", torch.float32)
    B, H, W, _ = X11.shape
    if X21.numel() != B * H * W * 3:
        raise RuntimeError("prep_rays: X21 must hold B*H*W points")
    dev = X11.device
    rays = torch.empty(B, H, W, 9, dtype=torch.float32, device=dev)
    pts = torch.empty(B, H * W, 3, dtype=torch.float32, device=dev)
    a = PrepRaysArgs()
    a.X11, a.X21, a.B, a.H, a.W, a.rays_img, a.pts_norm = _p(X11), _p(X21), B, H, W, _p(rays), _p(pts)
    _raise(_lib.m3s_prep_rays(ctypes.byref(a), _stream(dev)), "m3s_prep_rays")
    return rays, pts


# --------------------------------------------------------------- rope ---
_ROPE_DTYPES = {torch.float32: ROPE_F32, torch.float16: ROPE_F16, torch.bfloat16: ROPE_BF16}


def rope_2d(tokens, positions, base, f0):
    """2-D rotary position embedding, in place (new entry point; m3s_rope_2d;
    RoPE2D of croco's models/pos_embed.py:112-159, which the reference runs
    through its curope extension).

    tokens: the [B, N, H, D] view of q or k, float32, float16 or bfloat16, D a
    multiple of 4, a head row contiguous and the heads of a token back to back
    (stride(3) == 1, stride(2) == D); the token and batch strides are free, so
    ``qkv[:, :, i].transpose(1, 2)`` of an attention's [B, H, 3, N, D] view is
    taken as it is. positions [B, N, 2] int64, (y, x) per token. The angle of
    frequency i of an axis is position * f0 / base^(i / (D/4)), evaluated in
    fp32; the result is rounded once to the tokens' dtype. f0 -> -f0 undoes the
    rotation. One launch, no host synchronisation. Returns tokens."""
    if not isinstance(tokens, torch.Tensor) or not isinstance(positions, torch.Tensor):
        raise RuntimeError("rope_2d: tokens and positions must be tensors")
    # layout and dtype first, the device last, in the order of _check
    if tokens.dtype not in _ROPE_DTYPES:
        raise RuntimeError(f"tokens must be float32, float16 or bfloat16 (got {tokens.dtype})")
    if tokens.dim() != 4:
        raise RuntimeError(f"tokens must be [B, N, H, D] (got {tuple(tokens.shape)})")
    B, N, H, D = (int(x) for x in tokens.shape)
    if D % 4 != 0:
        raise RuntimeError(f"rope_2d: D = {D} is not a multiple of 4")
    if tokens.numel() and (tokens.stride(3) != 1 or (H > 1 and tokens.stride(2) != D)):
        raise RuntimeError("tokens: a head row must be contiguous and the heads of a token back to back "
                           "(stride(3) == 1, stride(2) == D)")
    if positions.dtype != torch.int64:
        raise RuntimeError(f"positions must be {torch.int64} (got {positions.dtype})")
    if tuple(positions.shape) != (B, N, 2):
        raise RuntimeError(f"positions must be [{B}, {N}, 2] (got {tuple(positions.shape)})")
    if not positions.is_contiguous():
        raise RuntimeError("positions must be contiguous")
    if tokens.device.type != "cuda":
        raise RuntimeError(f"tokens must be on a ROCm device (got {tokens.device}); no CPU path")
    if positions.device != tokens.device:
        raise RuntimeError(f"rope_2d: positions is on {positions.device}, tokens on {tokens.device}")
    if tokens.numel() == 0:
        return tokens
    row = H * D
    a = RopeArgs()
    a.tokens, a.pos = _p(tokens), _p(positions)
    a.B, a.N, a.H, a.D = B, N, H, D
    # the stride of a dimension of size 1 is arbitrary: give it the dense value
    a.stride_n = tokens.stride(1) if N > 1 else row
    a.stride_b = tokens.stride(0) if B > 1 else (N - 1) * a.stride_n + row
    a.base, a.f0, a.dtype = float(base), float(f0), _ROPE_DTYPES[tokens.dtype]
    _raise(_lib.m3s_rope_2d(ctypes.byref(a), _stream(tokens.device)), "m3s_rope_2d")
    return tokens


# ---------------------------------------------------------- attention ---
def _attn_strides(t, N, row):
    """(batch, token) element strides of a [B, N, H, D] view; the stride of a
    dimension of size 1 is arbitrary: give it the dense value."""
    sn = t.stride(1) if N > 1 else row
    sb = t.stride(0) if t.shape[0] > 1 else (N - 1) * sn + row
    return sb, sn


def attention_rope(q, k, v, qpos, kpos, base, f0, scale, *, out=None):
    """The attention core of MASt3R's blocks in one launch (new entry point;
    m3s_attn_rope; croco models/blocks.py:94-112, 149-169): RoPE2D of q and k
    (the rotation of ``rope_2d``, bitwise), softmax(scale q' k'^T) v.

    q [B, Nq, H, 64], k and v [B, Nk, H, 64]: float32 views with a contiguous
    head row and the heads of a token back to back (stride(3) == 1, stride(2)
    == 64); the token and batch strides are free, so the three slices
    ``qkv[:, :, i]`` of an attention's [B, N, 3, H, D] buffer and the dense
    projections of a cross attention are taken as they are. They are only
    read. qpos [B, Nq, 2], kpos [B, Nk, 2] int64 (y, x), or both None for no
    rotation.

    -> out [B, Nq, H * 64] float32, the layout ``proj`` takes. out= writes into
    the caller's tensor: its rows must be contiguous, its token and batch
    strides are free. On the current stream; no allocation when out is given;
    no host synchronisation; two runs agree bitwise."""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"attention_rope: {name} must be a tensor")
    # layout and dtype first, the device last, in the order of rope_2d
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be {torch.float32} (got {t.dtype})")
        if t.dim() != 4:
            raise RuntimeError(f"{name} must be [B, N, H, D] (got {tuple(t.shape)})")
    B, Nq, H, D = (int(x) for x in q.shape)
    if D != ATTN_HEAD_DIM:
        raise RuntimeError(f"attention_rope: D = {D}, only the head dimension {ATTN_HEAD_DIM} is built")
    Nk = int(k.shape[1])
    if tuple(k.shape) != (B, Nk, H, D):
        raise RuntimeError(f"k must be [{B}, Nk, {H}, {D}] (got {tuple(k.shape)})")
    if tuple(v.shape) != (B, Nk, H, D):
        raise RuntimeError(f"v must be [{B}, {Nk}, {H}, {D}] (got {tuple(v.shape)})")
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if t.numel() and (t.stride(3) != 1 or (H > 1 and t.stride(2) != D)):
            raise RuntimeError(f"{name}: a head row must be contiguous and the heads of a token back to back "
                               "(stride(3) == 1, stride(2) == D)")
    if (qpos is None) != (kpos is None):
        raise RuntimeError("attention_rope: qpos and kpos must both be given or both be None")
    for t, name, n in ((qpos, "qpos", Nq), (kpos, "kpos", Nk)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"attention_rope: {name} must be a tensor or None")
        if t.dtype != torch.int64:
            raise RuntimeError(f"{name} must be {torch.int64} (got {t.dtype})")
        if tuple(t.shape) != (B, n, 2):
            raise RuntimeError(f"{name} must be [{B}, {n}, 2] (got {tuple(t.shape)})")
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous")
    row = H * D
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise RuntimeError("attention_rope: out must be a tensor")
        if out.dtype != torch.float32:
            raise RuntimeError(f"out must be {torch.float32} (got {out.dtype})")
        if tuple(out.shape) != (B, Nq, row):
            raise RuntimeError(f"out must be [{B}, {Nq}, {row}] (got {tuple(out.shape)})")
        if out.numel() and out.stride(2) != 1:
            raise RuntimeError("out: a row must be contiguous (stride(2) == 1)")
    if Nk == 0 and B * Nq * H:
        raise RuntimeError("attention_rope: Nk = 0, a softmax over no keys")
    for t, name in ((q, "q"), (k, "k"), (v, "v"), (qpos, "qpos"), (kpos, "kpos"), (out, "out")):
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError(f"{name} must be on a ROCm device (got {t.device}); no CPU path")
        if t.device != q.device:
            raise RuntimeError(f"attention_rope: {name} is on {t.device}, q on {q.device}")
    if out is None:
        out = torch.empty((B, Nq, row), dtype=torch.float32, device=q.device)
    if B * Nq * H == 0:
        return out
    a = AttnArgs()
    a.q, a.k, a.v, a.out, a.qpos, a.kpos = _p(q), _p(k), _p(v), _p(out), _p(qpos), _p(kpos)
    a.B, a.Nq, a.Nk, a.H, a.D = B, Nq, Nk, H, D
    a.q_sb, a.q_sn = _attn_strides(q, Nq, row)
    a.k_sb, a.k_sn = _attn_strides(k, Nk, row)
    a.v_sb, a.v_sn = _attn_strides(v, Nk, row)
    a.o_sb, a.o_sn = _attn_strides(out, Nq, row)
    a.base, a.f0, a.scale, a.dtype = float(base), float(f0), float(scale), ROPE_F32
    _raise(_lib.m3s_attn_rope(ctypes.byref(a), _stream(q.device)), "m3s_attn_rope")
    return out


# --------------------------------------------------------------- head ---
_HEAD_DTYPES = {torch.float32: HEAD_F32, torch.float16: HEAD_F16}
_HEAD_OUT = ("X", "C", "D", "Q")


def _head_mode(mode, name):
    try:
        vmin, vmax = (float(v) for v in mode)
    except (TypeError, ValueError):
        raise RuntimeError(f"{name} must be (vmin, vmax)") from None
    if not math.isfinite(vmin) or not vmax >= vmin:
        raise RuntimeError(f"{name} must be a finite vmin and a vmax >= vmin (got {mode})")
    return vmin, vmax


def head_postprocess(pts, feat, patch_size, desc_dim, *, conf=(1.0, float("inf")), desc_conf=(0.0, float("inf")),
                     downsample=1, desc_dtype=torch.float32, out=None, generic=False):
    """The tail of MASt3R's catmlp+dpt head in one launch (new entry point;
    m3s_head_postprocess; catmlp_dpt_head.py:25-39, 82-96, dust3r
    heads/postprocess.py:22-58 and the stack / downsample / .half() of the SLAM
    side, mast3r_utils.py:43-52, 73-79).

    pts [B,4,H,W] f32 contiguous: the DPT output (x, y, z, raw confidence). feat
    [B,S,(F+1)*P*P] f32 contiguous: head_local_features' output, S =
    (H/P)*(W/P), P = patch_size, F = desc_dim. conf and desc_conf are the
    (vmin, vmax) of the two 'exp' confidence modes. downsample = k keeps the
    pixels [::k, ::k].

    -> (X [B,Ho,Wo,3] f32, C [B,Ho,Wo] f32, D [B,Ho,Wo,F] desc_dtype (float32 or
    float16, the fp32 value rounded once), Q [B,Ho,Wo] f32). out=(X, C, D, Q)
    writes into the caller's tensors instead: each image of each must be
    contiguous, the batch stride is free, so slot k of a stacked [4,B,Ho,Wo,.]
    buffer, or rows of a wider one, are taken as they are. generic=True takes
    the element-wise kernel whatever the shape (the same values, bitwise). On
    the current stream; no allocation when out is given; no host
    synchronisation."""
    a, out = _head_args(pts, feat, patch_size, desc_dim, conf, desc_conf, downsample, desc_dtype, out, generic)
    if a is not None:
        _raise(_lib.m3s_head_postprocess(ctypes.byref(a), _stream(pts.device)), "m3s_head_postprocess")
    return out


def _head_args(pts, feat, patch_size, desc_dim, conf, desc_conf, downsample, desc_dtype, out, generic):
    """Validate and fill an ``m3s_head_args``; -> (args or None when there is
    nothing to do, (X, C, D, Q))."""
    # layout and dtype first, the device last, in the order of rope_2d
    for t, name in ((pts, "pts"), (feat, "feat")):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{name} must be a tensor")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name} must be {torch.float32} (got {t.dtype})")
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous")
    P, F, ds = int(patch_size), int(desc_dim), int(downsample)
    for v, name in ((P, "patch_size"), (F, "desc_dim"), (ds, "downsample")):
        if v < 1:
            raise RuntimeError(f"{name} must be >= 1 (got {v})")
    if pts.dim() != 4 or pts.shape[1] != 4:
        raise RuntimeError(f"pts must be [B, 4, H, W] (got {tuple(pts.shape)})")
    B, _, H, W = (int(x) for x in pts.shape)
    if H % P or W % P:
        raise RuntimeError(f"pts: H = {H} and W = {W} must be multiples of patch_size = {P}")
    want = (B, (H // P) * (W // P), (F + 1) * P * P)
    if tuple(feat.shape) != want:
        raise RuntimeError(f"feat must be {list(want)} (got {tuple(feat.shape)})")
    if desc_dtype not in _HEAD_DTYPES:
        raise RuntimeError(f"desc_dtype must be float32 or float16 (got {desc_dtype})")
    conf, desc_conf = _head_mode(conf, "conf"), _head_mode(desc_conf, "desc_conf")
    Ho, Wo = -(-H // ds), -(-W // ds)
    shapes = ((B, Ho, Wo, 3), (B, Ho, Wo), (B, Ho, Wo, F), (B, Ho, Wo))
    dtypes = (torch.float32, torch.float32, desc_dtype, torch.float32)
    strides = [math.prod(s[1:]) for s in shapes]
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 4:
            raise RuntimeError("out must be (X, C, D, Q)")
        for k, (t, name, shape, dtype) in enumerate(zip(out, _HEAD_OUT, shapes, dtypes)):
            if not isinstance(t, torch.Tensor):
                raise RuntimeError(f"out {name} must be a tensor")
            if tuple(t.shape) != shape:
                raise RuntimeError(f"out {name} must be {list(shape)} (got {tuple(t.shape)})")
            if t.dtype != dtype:
                raise RuntimeError(f"out {name} must be {dtype} (got {t.dtype})")
            if t.numel() and not t[0].is_contiguous():
                raise RuntimeError(f"out {name}: every image must be contiguous (only the batch stride is free)")
            # the stride of a dimension of size 1 is arbitrary: keep the dense value
            if B > 1:
                if t.stride(0) < strides[k]:
                    raise RuntimeError(f"out {name}: the images overlap (batch stride {t.stride(0)} < {strides[k]})")
                strides[k] = t.stride(0)
    for t, name in ((pts, "pts"), (feat, "feat")) + tuple((t, f"out {n}") for t, n in zip(out or (), _HEAD_OUT)):
        if t.device.type != "cuda":
            raise RuntimeError(f"{name} must be on a ROCm device (got {t.device}); no CPU path")
        if t.device != pts.device:
            raise RuntimeError(f"head_postprocess: {name} is on {t.device}, pts on {pts.device}")
    if out is None:
        out = tuple(torch.empty(s, dtype=d, device=pts.device) for s, d in zip(shapes, dtypes))
    if B * H * W == 0:
        return None, tuple(out)
    a = HeadArgs()
    a.pts, a.feat = _p(pts), _p(feat)
    a.X, a.C, a.D, a.Q = (_p(t) for t in out)
    a.B, a.H, a.W, a.P, a.F, a.ds = B, H, W, P, F, ds
    a.sbX, a.sbC, a.sbD, a.sbQ = strides
    (a.conf_vmin, a.conf_vmax), (a.dconf_vmin, a.dconf_vmax) = conf, desc_conf
    a.desc_dtype = _HEAD_DTYPES[desc_dtype]
    a.flags = HEAD_GENERIC if generic else 0
    return a, tuple(out)


# ---------------------------------------------------------- retrieval ---
def asmk_store_layout(cap_images, cap_entries, D):
    """Byte offsets of the store's sections (ASMK_STORE_SECTIONS)."""
    offs = (ctypes.c_size_t * len(ASMK_STORE_SECTIONS))()
    _lib.m3s_asmk_store_layout(int(cap_images), int(cap_entries), int(D), offs)
    return dict(zip(ASMK_STORE_SECTIONS, list(offs)))


def asmk_workspace_layout(Kc, D, cap_images):
    """Byte offsets of the workspace's sections (ASMK_WS_SECTIONS)."""
    offs = (ctypes.c_size_t * len(ASMK_WS_SECTIONS))()
    _lib.m3s_asmk_workspace_layout(int(Kc), int(D), int(cap_images), offs)
    return dict(zip(ASMK_WS_SECTIONS, list(offs)))


def asmk_store_size(cap_images, cap_entries, D):
    return int(_lib.m3s_asmk_store_size(int(cap_images), int(cap_entries), int(D)))


def asmk_workspace_size(Kc, D, cap_images):
    return int(_lib.m3s_asmk_workspace_size(int(Kc), int(D), int(cap_images)))


class AsmkHandle:
    """One database for the m3s_asmk_* entry points: the store and workspace
    tensors (uint8, on a ROCm device), the geometry and the filled
    ``m3s_asmk_db``. ``section(name)`` / ``ws_section(name)`` are typed views of
    the documented sections, for the caller's one read and for tests."""

    def __init__(self, store, workspace, cap_images, cap_entries, Kc, D):
        _check(store, "store", torch.uint8)
        _check(workspace, "workspace", torch.uint8)
        if store.device != workspace.device:
            raise RuntimeError("asmk: store and workspace must be on one device")
        self.cap_images, self.cap_entries, self.Kc, self.D = int(cap_images), int(cap_entries), int(Kc), int(D)
        if min(self.cap_images, self.cap_entries, self.Kc, self.D) < 1:
            raise RuntimeError("asmk: cap_images, cap_entries, Kc and D must be >= 1")
        self.D32 = (self.D + 31) // 32
        self.store_off = asmk_store_layout(self.cap_images, self.cap_entries, self.D)
        self.ws_off = asmk_workspace_layout(self.Kc, self.D, self.cap_images)
        if store.numel() < self.store_off["total"] or workspace.numel() < self.ws_off["total"]:
            raise RuntimeError("asmk: store or workspace smaller than its size function says")
        if store.data_ptr() % 16 or workspace.data_ptr() % 16:
            raise RuntimeError("asmk: store and workspace must be 16-byte aligned")
        self.store, self.workspace, self.device = store, workspace, store.device
        d = AsmkDb()
        d.store, d.store_bytes = _p(store), store.numel()
        d.workspace, d.workspace_bytes = _p(workspace), workspace.numel()
        d.cap_images, d.cap_entries, d.Kc, d.D = self.cap_images, self.cap_entries, self.Kc, self.D
        self.db = d

    @staticmethod
    def _view(buf, off, count, dtype):
        nbytes = count * torch.empty(0, dtype=dtype).element_size()
        return buf[off:off + nbytes].view(dtype)

    def section(self, name):
        o = self.store_off[name]
        if name == "header":
            return self._view(self.store, o, 16, torch.int32)
        if name == "img_ptr":
            return self._view(self.store, o, self.cap_images + 1, torch.int32)
        if name == "word":
            return self._view(self.store, o, self.cap_entries, torch.int32)
        if name == "codes":  # uint32 bit patterns as int32
            return self._view(self.store, o, self.cap_entries * self.D32, torch.int32).view(-1, self.D32)
        raise KeyError(name)

    def ws_section(self, name):
        o = self.ws_off[name]
        if name == "counts":
            return self._view(self.workspace, o, 16, torch.int32)
        if name == "slot":
            return self._view(self.workspace, o, self.Kc, torch.int32)
        if name in ("words", "members"):
            return self._view(self.workspace, o, 2 * ASMK_MAX_PAIRS, torch.int32).view(2, -1)
        if name == "start":
            return self._view(self.workspace, o, 2 * (ASMK_MAX_PAIRS + 16), torch.int32).view(2, -1)
        if name == "codes":
            return self._view(self.workspace, o, 2 * ASMK_MAX_PAIRS * self.D32, torch.int32).view(2, -1, self.D32)
        if name == "scores":
            return self._view(self.workspace, o, self.cap_images, torch.float64)
        if name == "out":
            return self.workspace[o:o + ctypes.sizeof(AsmkOut)]
        raise KeyError(name)


def asmk_reset(h: AsmkHandle):
    """Empty the store and clear the word table (m3s_asmk_reset)."""
    _raise(_lib.m3s_asmk_reset(ctypes.byref(h.db), _stream(h.device)), "m3s_asmk_reset")


def asmk_aggregate(h: AsmkHandle, des, centroids, assign, query_ma, build_ma):
    """m3s_asmk_aggregate: des [n, D] f32, centroids [Kc, D] f32, assign [n, ma]
    int64 -> the query rows (first query_ma columns) and the build rows (first
    build_ma columns) of the workspace. With query_ma > 0 an asmk_search must
    follow before the next aggregate (it clears the word table)."""
    _check(des, "des", torch.float32)
    _check(centroids, "centroids", torch.float32)
    _check(assign, "assign", torch.int64)
    if des.dim() != 2 or des.shape[1] != h.D:
        raise RuntimeError(f"asmk_aggregate: des must be [n, {h.D}]")
    if tuple(centroids.shape) != (h.Kc, h.D):
        raise RuntimeError(f"asmk_aggregate: centroids must be [{h.Kc}, {h.D}]")
    n = int(des.shape[0])
    if assign.dim() != 2 or assign.shape[0] != n:
        raise RuntimeError("asmk_aggregate: assign must be [n, ma]")
    ma, query_ma, build_ma = int(assign.shape[1]), int(query_ma), int(build_ma)
    if not (0 <= query_ma <= ma and 0 <= build_ma <= ma and query_ma + build_ma > 0 and n >= 1):
        raise RuntimeError("asmk_aggregate: need n >= 1 and 0 <= query_ma, build_ma <= ma, not both 0")
    if n * max(query_ma, build_ma) > ASMK_MAX_PAIRS:
        raise RuntimeError(f"asmk_aggregate: n * multiple_assignment exceeds {ASMK_MAX_PAIRS}")
    for name, t in (("des", des), ("centroids", centroids), ("assign", assign)):
        if t.device != h.device:
            raise RuntimeError(f"asmk_aggregate: {name} is on {t.device}, the database on {h.device}")
    a = AsmkAggregateArgs()
    a.db = h.db
    a.des, a.centroids, a.assign = _p(des), _p(centroids), _p(assign)
    a.n, a.ma, a.query_ma, a.build_ma = n, ma, query_ma, build_ma
    _raise(_lib.m3s_asmk_aggregate(ctypes.byref(a), _stream(h.device)), "m3s_asmk_aggregate")


def asmk_search(h: AsmkHandle, n_images, k, alpha=3.0, similarity_threshold=0.0, min_thresh=0.0):
    """m3s_asmk_search: scores of the query rows against the first n_images
    stored images -> h.ws_section("scores")[:n_images], selection ->
    h.ws_section("out") (an AsmkOut). No host synchronisation."""
    n_images, k = int(n_images), int(k)
    if not 1 <= n_images <= h.cap_images:
        raise RuntimeError(f"asmk_search: n_images must be in [1, {h.cap_images}]")
    if not 1 <= k <= ASMK_MAX_K:
        raise RuntimeError(f"asmk_search: k must be in [1, {ASMK_MAX_K}]")
    a = AsmkSearchArgs()
    a.db = h.db
    a.n_images, a.k = n_images, k
    a.alpha, a.similarity_threshold, a.min_thresh = float(alpha), float(similarity_threshold), float(min_thresh)
    _raise(_lib.m3s_asmk_search(ctypes.byref(a), _stream(h.device)), "m3s_asmk_search")


def asmk_append(h: AsmkHandle):
    """m3s_asmk_append: the build rows become the next stored image; at
    capacity nothing is written but ASMK_INFO_FULL in the store header."""
    _raise(_lib.m3s_asmk_append(ctypes.byref(h.db), _stream(h.device)), "m3s_asmk_append")


def asmk_read_out(h: AsmkHandle) -> AsmkOut:
    """The one device-to-host copy of a search: its ``m3s_asmk_out``."""
    return AsmkOut.from_buffer_copy(h.ws_section("out").cpu().numpy().tobytes())


def asmk_quantize_workspace_size(n_max, Kc, ma):
    """Bytes of scratch ``asmk_quantize`` needs for up to ``n_max`` features."""
    return int(_lib.m3s_asmk_quantize_workspace_size(int(n_max), int(Kc), int(ma)))


def asmk_centroid_norms(centroids):
    """m3s_asmk_centroid_norms: centroids [Kc, D] f32 -> |c|^2 [Kc] f32, once
    per codebook. One launch on the current stream."""
    _check(centroids, "centroids", torch.float32)
    if centroids.dim() != 2 or centroids.shape[0] < 1 or centroids.shape[1] < 1:
        raise RuntimeError("asmk_centroid_norms: centroids must be [Kc, D]")
    Kc, D = (int(x) for x in centroids.shape)
    norms = torch.empty(Kc, dtype=torch.float32, device=centroids.device)
    _raise(_lib.m3s_asmk_centroid_norms(_p(centroids), Kc, D, _p(norms), _stream(centroids.device)),
           "m3s_asmk_centroid_norms")
    return norms


def asmk_quantize(feat, centroids, norms, ma, workspace, out=None, dist=None):
    """m3s_asmk_quantize: feat [n, D] f32, centroids [Kc, D] f32, norms [Kc]
    (asmk_centroid_norms) -> the ``ma`` nearest words of every feature, nearest
    first, [n, ma] int64 (``out``, or a new tensor): the ``assign`` of
    asmk_aggregate. ``workspace`` is a uint8 buffer of at least
    asmk_quantize_workspace_size(n, Kc, ma) bytes; ``dist`` ([n, ma] f32,
    optional) receives the ranked values |c|^2 - 2 q.c. Two launches on the
    current stream, no allocation when ``out`` is given, no host
    synchronisation."""
    _check(feat, "feat", torch.float32)
    _check(centroids, "centroids", torch.float32)
    _check(norms, "norms", torch.float32)
    _check(workspace, "workspace", torch.uint8)
    if feat.dim() != 2 or centroids.dim() != 2 or feat.shape[1] != centroids.shape[1]:
        raise RuntimeError("asmk_quantize: feat must be [n, D] and centroids [Kc, D]")
    n, D = (int(x) for x in feat.shape)
    Kc, ma = int(centroids.shape[0]), int(ma)
    if tuple(norms.shape) != (Kc,):
        raise RuntimeError(f"asmk_quantize: norms must be [{Kc}]")
    if not 1 <= ma <= min(ASMK_QUANTIZE_MAX_MA, Kc):
        raise RuntimeError(f"asmk_quantize: ma must be in [1, min({ASMK_QUANTIZE_MAX_MA}, Kc)]")
    if n < 1 or n * ma > ASMK_MAX_PAIRS:
        raise RuntimeError(f"asmk_quantize: need n >= 1 and n * ma <= {ASMK_MAX_PAIRS}")
    if workspace.numel() < asmk_quantize_workspace_size(n, Kc, ma):
        raise RuntimeError("asmk_quantize: workspace smaller than asmk_quantize_workspace_size(n, Kc, ma)")
    if out is None:
        out = torch.empty((n, ma), dtype=torch.int64, device=feat.device)
    _check(out, "out", torch.int64)
    if tuple(out.shape) != (n, ma):
        raise RuntimeError(f"asmk_quantize: out must be [{n}, {ma}]")
    if dist is not None:
        _check(dist, "dist", torch.float32)
        if tuple(dist.shape) != (n, ma):
            raise RuntimeError(f"asmk_quantize: dist must be [{n}, {ma}]")
    for name, t in (("centroids", centroids), ("norms", norms), ("workspace", workspace), ("out", out), ("dist", dist)):
        if t is not None and t.device != feat.device:
            raise RuntimeError(f"asmk_quantize: {name} is on {t.device}, feat on {feat.device}")
    a = AsmkQuantizeArgs()
    a.des, a.centroids, a.norms = _p(feat), _p(centroids), _p(norms)
    a.n, a.Kc, a.D, a.ma = n, Kc, D, ma
    a.assign, a.dist = _p(out), _p(dist)
    a.workspace, a.workspace_bytes = _p(workspace), workspace.numel()
    _raise(_lib.m3s_asmk_quantize(ctypes.byref(a), _stream(feat.device)), "m3s_asmk_quantize")
    return out


# ------------------------------------------------------------ tracker ---
def _track(fn, Xf, Xk, T_WCf, T_WCk, Qk, valid, K, img_size, sigma_a, sigma_b, huber_k,
           max_iters, rel_error, delta_norm, pixel_border=0, z_eps=0.0, sync_every=5, workspace=None):
    _check(Xf, "Xf", torch.float32)
    _check(Xk, "Xk", torch.float32)
    _check(Qk, "Qk", torch.float32)
    _check(valid, "valid", torch.bool)
    T_WCf = T_WCf.contiguous()
    T_WCk = T_WCk.contiguous()
    _check(T_WCf, "T_WCf", torch.float32)
    _check(T_WCk, "T_WCk", torch.float32)
    if K is not None:
        _check(K, "K", torch.float32)
    HW = int(Xk.shape[0])
    if Xf.numel() != 3 * HW or Xk.numel() != 3 * HW or Qk.numel() != HW or valid.numel() != HW:
        raise RuntimeError("tracker inputs must be Xf/Xk [HW,3], Qk/valid [HW,1]")
    dev = Xk.device
    out_f = torch.empty(1, 8, dtype=torch.float32, device=dev)
    out_r = torch.empty(1, 8, dtype=torch.float32, device=dev)
    info = torch.zeros(8, dtype=torch.int32, device=dev)
    need = _lib.m3s_track_workspace_size(HW)
    if workspace is None:
        ws = _workspace(need, dev)
    else:  # caller-owned (tests: reused / poisoned workspaces)
        _check(workspace, "workspace", torch.uint8)
        if workspace.device != dev or workspace.numel() < need:
            raise RuntimeError(f"tracker workspace must be a uint8 tensor of >= {need} bytes on {dev}")
        ws = workspace
    a = TrackArgs()
    a.Xf, a.Xk, a.Qk, a.valid = _p(Xf), _p(Xk), _p(Qk), _p(valid)
    a.T_WCf, a.T_WCk, a.K = _p(T_WCf), _p(T_WCk), _p(K)
    a.HW = HW
    h, w = (int(img_size[0]), int(img_size[1])) if img_size is not None else (0, 0)
    a.height, a.width, a.pixel_border, a.z_eps = h, w, int(pixel_border), float(z_eps)
    a.sigma_a, a.sigma_b, a.huber_k = float(sigma_a), float(sigma_b), float(huber_k)
    a.max_iters, a.rel_error, a.delta_norm = int(max_iters), float(rel_error), float(delta_norm)
    a.sync_every = int(sync_every)
    a.T_WCf_out, a.T_CkCf_out, a.info = _p(out_f), _p(out_r), _p(info)
    a.workspace, a.workspace_bytes = _p(ws), ws.numel()
    rc = getattr(_lib, fn)(ctypes.byref(a), _stream(dev))
    _raise(rc, fn)
    del ws  # stream-ordered by the caching allocator
    return out_f, out_r, info


def track_workspace_size(HW):
    """Bytes of the tracker workspace for an image of HW pixels."""
    return int(_lib.m3s_track_workspace_size(int(HW)))


def track_rays_sim3(Xf, Xk, T_WCf, T_WCk, Qk, valid, sigma_ray, sigma_dist, huber_k, max_iters,
                    rel_error, delta_norm, sync_every=5, workspace=None):
    """Device form of FrameTracker.opt_pose_ray_dist_sim3 (tracker.py:173-214).
    Returns (T_WCf [1,8], T_CkCf [1,8], info int32[8]); info[1] != 0 means the
    Cholesky failed (the reference raises; tracker.py:91-93)."""
    return _track("m3s_track_rays_sim3", Xf, Xk, T_WCf, T_WCk, Qk, valid, None, None, sigma_ray,
                  sigma_dist, huber_k, max_iters, rel_error, delta_norm, sync_every=sync_every,
                  workspace=workspace)


def track_calib_sim3(Xf, Xk, T_WCf, T_WCk, Qk, valid, K, img_size, sigma_pixel, sigma_depth,
                     huber_k, max_iters, rel_error, delta_norm, pixel_border, z_eps, sync_every=5,
                     workspace=None):
    """Device form of FrameTracker.opt_pose_calib_sim3 (tracker.py:216-266);
    Xf/Xk already constrained to rays, meas_k formed on device."""
    return _track("m3s_track_calib_sim3", Xf, Xk, T_WCf, T_WCk, Qk, valid, K, img_size,
                  sigma_pixel, sigma_depth, huber_k, max_iters, rel_error, delta_norm,
                  pixel_border=pixel_border, z_eps=z_eps, sync_every=sync_every, workspace=workspace)


def track_frame_workspace_size(HW):
    """Bytes of the track_frame workspace for an image of HW pixels."""
    return int(_lib.m3s_track_frame_workspace_size(int(HW)))


def track_frame(Xf_canon, Cf_sum, Nf, Xk_canon, Ck_sum, Nk, idx_f2k, valid_match, Qk, T_WCf, T_WCk,
                K, img_size, C_conf, Q_conf, sigma_a, sigma_b, huber_k, max_iters, rel_error,
                delta_norm, pixel_border=0, z_eps=0.0, sync_every=0, workspace=None,
                return_prepared=False, out=None):
    """FrameTracker.track from the matches to the refined pose on the device
    (new entry point; m3s_track_frame): get_points_poses (tracker.py:129-154),
    valid_opt / valid_kf (:60-65) and the three counts behind match_frac,
    match_frac_k and unique_frac_f (:67, :104-108) in three launches, then the
    launches of track_rays_sim3 (K is None) or track_calib_sim3 on the result.

    Xf_canon, Xk_canon [HW,3] f32; Cf_sum, Ck_sum [HW(,1)] f32, the summed
    confidences (Pointmap.C) with their update counts Nf, Nk (Pointmap.N);
    idx_f2k [HW] (or [1,HW]) int32 as match_dense writes it, every entry in
    [0, HW) -- not scanned; valid_match [HW(,1)] bool; Qk [HW(,1)] f32; T_WCf,
    T_WCk [8] or [1,8]; K [3,3] f32 or None (rays mode); img_size (H, W) with
    H * W == HW; sigma_a / sigma_b as track_rays_sim3 (rays) or
    track_calib_sim3 (calib) name them.

    -> (T_WCf [1,8], T_CkCf [1,8], info int32[8], stats int32[4]) with stats =
    (n_opt, n_kf, n_unique, 0); with return_prepared=True also (Xf_g [HW,3],
    Xk_g [HW,3], valid_opt [HW,1] bool), the rows the tracker launches read.
    out: an int32 [12] device tensor; info and stats are then its views [:8]
    and [8:], so that one copy brings both to the host. No host
    synchronisation here (calib mode: the tracker entry point's one read of K)."""
    _check(Xf_canon, "Xf_canon", torch.float32)
    _check(Cf_sum, "Cf_sum", torch.float32)
    _check(Xk_canon, "Xk_canon", torch.float32)
    _check(Ck_sum, "Ck_sum", torch.float32)
    _check(idx_f2k, "idx_f2k", torch.int32)
    _check(valid_match, "valid_match", torch.bool)
    _check(Qk, "Qk", torch.float32)
    T_WCf = T_WCf.contiguous()
    T_WCk = T_WCk.contiguous()
    _check(T_WCf, "T_WCf", torch.float32)
    _check(T_WCk, "T_WCk", torch.float32)
    if K is not None:
        _check(K, "K", torch.float32)
        if K.numel() != 9:
            raise RuntimeError("track_frame: K must be [3,3]")
    if T_WCf.numel() != 8 or T_WCk.numel() != 8:
        raise RuntimeError("track_frame: T_WCf / T_WCk must be [8] or [1,8]")
    HW = int(Xk_canon.shape[0])
    H, W = int(img_size[0]), int(img_size[1])
    if H < 1 or W < 1 or H * W != HW:
        raise RuntimeError(f"track_frame: img_size {H} x {W} does not hold HW = {HW} pixels")
    if Xf_canon.numel() != 3 * HW or Xk_canon.numel() != 3 * HW:
        raise RuntimeError("track_frame: Xf_canon / Xk_canon must be [HW,3]")
    for name, t in (("Cf_sum", Cf_sum), ("Ck_sum", Ck_sum), ("idx_f2k", idx_f2k),
                    ("valid_match", valid_match), ("Qk", Qk)):
        if t.numel() != HW:
            raise RuntimeError(f"track_frame: {name} must hold HW = {HW} elements (got {tuple(t.shape)})")
    Nf, Nk = int(Nf), int(Nk)
    if Nf < 1 or Nk < 1:
        raise RuntimeError("track_frame: Nf and Nk must be >= 1 (an initialised pointmap)")
    dev = Xk_canon.device
    for name, t in (("Xf_canon", Xf_canon), ("Cf_sum", Cf_sum), ("Ck_sum", Ck_sum), ("idx_f2k", idx_f2k),
                    ("valid_match", valid_match), ("Qk", Qk), ("T_WCf", T_WCf), ("T_WCk", T_WCk), ("K", K)):
        if t is not None and t.device != dev:
            raise RuntimeError(f"track_frame: {name} is on {t.device}, Xk_canon on {dev}")
    if out is None:
        out = torch.empty(12, dtype=torch.int32, device=dev)  # written by the call's first launches
    else:
        _check(out, "out", torch.int32)
        if out.numel() != 12 or out.device != dev:
            raise RuntimeError(f"track_frame: out must be an int32 [12] tensor on {dev}")
    info, stats = out.view(-1)[:8], out.view(-1)[8:]
    out_f = torch.empty(1, 8, dtype=torch.float32, device=dev)
    out_r = torch.empty(1, 8, dtype=torch.float32, device=dev)
    need = track_frame_workspace_size(HW)
    if workspace is None:
        ws = _workspace(need, dev)
    else:  # caller-owned (tests: reused / poisoned workspaces)
        _check(workspace, "workspace", torch.uint8)
        if workspace.device != dev or workspace.numel() < need:
            raise RuntimeError(f"track_frame workspace must be a uint8 tensor of >= {need} bytes on {dev}")
        ws = workspace
    Xf_g = Xk_g = valid_opt = None
    if return_prepared:
        Xf_g = torch.empty(HW, 3, dtype=torch.float32, device=dev)
        Xk_g = torch.empty(HW, 3, dtype=torch.float32, device=dev)
        valid_opt = torch.empty(HW, 1, dtype=torch.bool, device=dev)
    a = TrackFrameArgs()
    a.Xf_canon, a.Cf_sum, a.Xk_canon, a.Ck_sum = _p(Xf_canon), _p(Cf_sum), _p(Xk_canon), _p(Ck_sum)
    a.idx_f2k, a.valid_match, a.Qk = _p(idx_f2k), _p(valid_match), _p(Qk)
    a.T_WCf, a.T_WCk, a.K = _p(T_WCf), _p(T_WCk), _p(K)
    a.HW, a.Nf, a.Nk, a.height, a.width = HW, Nf, Nk, H, W
    a.C_conf, a.Q_conf = float(C_conf), float(Q_conf)
    a.pixel_border, a.z_eps = int(pixel_border), float(z_eps)
    a.sigma_a, a.sigma_b, a.huber_k = float(sigma_a), float(sigma_b), float(huber_k)
    a.max_iters, a.rel_error, a.delta_norm = int(max_iters), float(rel_error), float(delta_norm)
    a.sync_every = int(sync_every)
    a.T_WCf_out, a.T_CkCf_out, a.info, a.stats = _p(out_f), _p(out_r), _p(info), _p(stats)
    a.Xf_out, a.Xk_out, a.valid_opt_out = _p(Xf_g), _p(Xk_g), _p(valid_opt)
    a.workspace, a.workspace_bytes = _p(ws), ws.numel()
    _raise(_lib.m3s_track_frame(ctypes.byref(a), _stream(dev)), "m3s_track_frame")
    del ws  # stream-ordered by the caching allocator
    if return_prepared:
        return out_f, out_r, info, stats, Xf_g, Xk_g, valid_opt
    return out_f, out_r, info, stats


# -------------------------------------------------- stepwise (sharded) ---
def gn_prepare(a, keep):
    _raise(_lib.m3s_gn_prepare(ctypes.byref(a), _stream(keep["Xs"].device)), "m3s_gn_prepare")


def gn_linearize(a, keep, edge_begin, edge_end, edge_sums):
    _check(edge_sums, "edge_sums", torch.float64)
    rc = _lib.m3s_gn_linearize(ctypes.byref(a), int(edge_begin), int(edge_end), _p(edge_sums),
                               _stream(keep["Xs"].device))
    _raise(rc, "m3s_gn_linearize")


def gn_release(a, keep):
    _raise(_lib.m3s_gn_release(ctypes.byref(a), _stream(keep["Xs"].device)), "m3s_gn_release")


def gn_solve(a, keep, edge_sums):
    _check(edge_sums, "edge_sums", torch.float64)
    rc = _lib.m3s_gn_solve(ctypes.byref(a), _p(edge_sums), _stream(keep["Xs"].device))
    _raise(rc, "m3s_gn_solve")

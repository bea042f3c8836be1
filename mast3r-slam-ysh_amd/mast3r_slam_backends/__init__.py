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

``dpt_tail`` (new; include/m3s_dpt.h) is what stands directly in front of it:
the last four modules of the DPT head (bilinear x2 upsampling, the 3x3
convolution 128 -> 128, ReLU, the 1x1 convolution to the 4 output channels) in
one launch on the fp32 MFMA, from weights ``dpt_tail_pack`` packs once per
model; ``mast3r_slam_amd.dpt`` puts it into a loaded model.
"""
from __future__ import annotations

import ctypes
import os

# one module per public header: its public names are the package's, and its
# _SIGNATURES (symbol -> (restype, argtypes)) declares each of its symbols once
from . import attn, dpt, fuse, gn, head, match, retrieval, rope
from ._abi import *  # noqa: F401,F403  (the M3S_* return codes)
from ._abi import _call, _check, _p, _raise, _stream, _workspace  # noqa: F401  (used by distributed, tools and tests)
from .attn import *  # noqa: F401,F403
from .dpt import *  # noqa: F401,F403
from .fuse import *  # noqa: F401,F403
from .gn import *  # noqa: F401,F403
from .head import *  # noqa: F401,F403
from .match import *  # noqa: F401,F403
from .retrieval import *  # noqa: F401,F403
from .rope import *  # noqa: F401,F403

_run_gn, _head_args, _match_dense = gn._run_gn, head._head_args, match._match_dense  # used by tests and tools
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libm3s_gn.so"
LIB_PATH = os.environ.get("M3S_LIB") or os.path.join(_HERE, LIB_NAME)  # override: experiments only
# the same sources built with -DM3S_TEST_PATHS: the A/B reference solver paths
# and test hooks, for the tests that compare against them (never the product)
TEST_LIB_PATH = os.path.join(_HERE, "libm3s_gn_test.so")

_MODULES = (gn, match, fuse, retrieval, rope, attn, head)
# every symbol include/m3s_gn.h, m3s_match.h and m3s_fuse.h declare
EXPORTS = tuple(s for m in (gn, match, fuse) for s in m._SIGNATURES)
RETRIEVAL_EXPORTS = tuple(retrieval._SIGNATURES)  # every symbol include/m3s_retrieval.h declares
ROPE_EXPORTS = tuple(rope._SIGNATURES)  # ... include/m3s_rope.h
ATTN_EXPORTS = tuple(attn._SIGNATURES)  # ... include/m3s_attn.h
HEAD_EXPORTS = tuple(head._SIGNATURES)  # ... include/m3s_head.h
DPT_EXPORTS = tuple(dpt._SIGNATURES)  # ... include/m3s_dpt.h


def _load(path=LIB_PATH):
    if not os.path.exists(path):
        raise ImportError(
            f"mast3r_slam_backends: {path} is missing; build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)"
        )
    lib = ctypes.CDLL(path)
    for module in _MODULES + (dpt,):  # _MODULES: the seven tables tests/test_backend_package.py holds together
        for symbol, (restype, argtypes) in module._SIGNATURES.items():
            fn = getattr(lib, symbol)
            fn.restype, fn.argtypes = restype, argtypes
    return lib


# the library every wrapper calls, looked up here at each call (_abi._sym): assign
# another build to it (load_test_library(), _load(path)) and they all follow
_lib = _load()


def load_test_library():
    """The test build of the library (A/B reference paths, test hooks)."""
    return _load(TEST_LIB_PATH)

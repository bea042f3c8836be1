"""include/m3s_retrieval.h: the ASMK retrieval steps on an ``AsmkHandle``, and the quantize."""
import ctypes

import torch

from ._abi import _F32, _F64, _I32, _I64, _INT, _P, _SIZE, _VP, _call, _check, _layout, _p, _same_device, _stream, _sym

ASMK_MAX_PAIRS, ASMK_MAX_K = 4096, 64
ASMK_QUANTIZE_MAX_MA = 8
ASMK_INFO_BAD_WORD, ASMK_INFO_FULL = 1, 2
ASMK_STORE_SECTIONS = ("header", "img_ptr", "word", "codes", "total")
ASMK_WS_SECTIONS = ("counts", "slot", "words", "start", "members", "codes", "scores", "out", "total")


class AsmkOut(ctypes.Structure):
    """Mirror of ``m3s_asmk_out`` (include/m3s_retrieval.h)."""

    _fields_ = [
        ("count", _I32), ("n_images", _I32), ("info", _I32), ("n_query_words", _I32), ("idx", _I32 * ASMK_MAX_K),
        ("score", _F64 * ASMK_MAX_K),
    ]


class AsmkDb(ctypes.Structure):
    """Mirror of ``m3s_asmk_db`` (include/m3s_retrieval.h)."""

    _fields_ = [
        ("store", _VP), ("store_bytes", _SIZE), ("workspace", _VP), ("workspace_bytes", _SIZE), ("cap_images", _I64),
        ("cap_entries", _I64), ("Kc", _I64), ("D", _I64),
    ]


class AsmkAggregateArgs(ctypes.Structure):
    """Mirror of ``m3s_asmk_aggregate_args`` (include/m3s_retrieval.h)."""

    _fields_ = [
        ("db", AsmkDb), ("des", _VP), ("centroids", _VP), ("assign", _VP), ("n", _I64), ("ma", _I64),
        ("query_ma", _INT), ("build_ma", _INT),
    ]


class AsmkSearchArgs(ctypes.Structure):
    """Mirror of ``m3s_asmk_search_args`` (include/m3s_retrieval.h)."""

    _fields_ = [
        ("db", AsmkDb), ("n_images", _I64), ("k", _INT), ("alpha", _F32), ("similarity_threshold", _F32),
        ("min_thresh", _F64),
    ]


class AsmkQuantizeArgs(ctypes.Structure):
    """Mirror of ``m3s_asmk_quantize_args`` (include/m3s_retrieval.h)."""

    _fields_ = [
        ("des", _VP), ("centroids", _VP), ("norms", _VP), ("n", _I64), ("Kc", _I64), ("D", _I64), ("ma", _INT),
        ("assign", _VP), ("dist", _VP), ("workspace", _VP), ("workspace_bytes", _SIZE),
    ]


# symbol -> (restype, argtypes): include/m3s_retrieval.h
_SIGNATURES = {
    "m3s_asmk_store_size": (_SIZE, [_I64] * 3),
    "m3s_asmk_workspace_size": (_SIZE, [_I64] * 3),
    "m3s_asmk_store_layout": (_SIZE, [_I64] * 3 + [_P(_SIZE)]),
    "m3s_asmk_workspace_layout": (_SIZE, [_I64] * 3 + [_P(_SIZE)]),
    "m3s_asmk_reset": (_INT, [_P(AsmkDb), _VP]),
    "m3s_asmk_aggregate": (_INT, [_P(AsmkAggregateArgs), _VP]),
    "m3s_asmk_search": (_INT, [_P(AsmkSearchArgs), _VP]),
    "m3s_asmk_append": (_INT, [_P(AsmkDb), _VP]),
    "m3s_asmk_quantize_workspace_size": (_SIZE, [_I64, _I64, _INT]),
    "m3s_asmk_centroid_norms": (_INT, [_VP, _I64, _I64, _VP, _VP]),
    "m3s_asmk_quantize": (_INT, [_P(AsmkQuantizeArgs), _VP]),
}


def asmk_store_layout(cap_images, cap_entries, D):
    """Byte offsets of the store's sections (ASMK_STORE_SECTIONS)."""
    return _layout("m3s_asmk_store_layout", ASMK_STORE_SECTIONS, cap_images, cap_entries, D)


def asmk_workspace_layout(Kc, D, cap_images):
    """Byte offsets of the workspace's sections (ASMK_WS_SECTIONS)."""
    return _layout("m3s_asmk_workspace_layout", ASMK_WS_SECTIONS, Kc, D, cap_images)


def asmk_store_size(cap_images, cap_entries, D):
    return int(_sym("m3s_asmk_store_size")(int(cap_images), int(cap_entries), int(D)))


def asmk_workspace_size(Kc, D, cap_images):
    return int(_sym("m3s_asmk_workspace_size")(int(Kc), int(D), int(cap_images)))


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
    _call("m3s_asmk_reset", ctypes.byref(h.db), _stream(h.device))


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
    _same_device("asmk_aggregate", (("des", des), ("centroids", centroids), ("assign", assign)),
                 "the database", h.device)
    a = AsmkAggregateArgs()
    a.db = h.db
    a.des, a.centroids, a.assign = _p(des), _p(centroids), _p(assign)
    a.n, a.ma, a.query_ma, a.build_ma = n, ma, query_ma, build_ma
    _call("m3s_asmk_aggregate", ctypes.byref(a), _stream(h.device))


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
    _call("m3s_asmk_search", ctypes.byref(a), _stream(h.device))


def asmk_append(h: AsmkHandle):
    """m3s_asmk_append: the build rows become the next stored image; at
    capacity nothing is written but ASMK_INFO_FULL in the store header."""
    _call("m3s_asmk_append", ctypes.byref(h.db), _stream(h.device))


def asmk_read_out(h: AsmkHandle) -> AsmkOut:
    """The one device-to-host copy of a search: its ``m3s_asmk_out``."""
    return AsmkOut.from_buffer_copy(h.ws_section("out").cpu().numpy().tobytes())


def asmk_quantize_workspace_size(n_max, Kc, ma):
    """Bytes of scratch ``asmk_quantize`` needs for up to ``n_max`` features."""
    return int(_sym("m3s_asmk_quantize_workspace_size")(int(n_max), int(Kc), int(ma)))


def asmk_centroid_norms(centroids):
    """m3s_asmk_centroid_norms: centroids [Kc, D] f32 -> |c|^2 [Kc] f32, once
    per codebook. One launch on the current stream."""
    _check(centroids, "centroids", torch.float32)
    if centroids.dim() != 2 or centroids.shape[0] < 1 or centroids.shape[1] < 1:
        raise RuntimeError("asmk_centroid_norms: centroids must be [Kc, D]")
    Kc, D = (int(x) for x in centroids.shape)
    norms = torch.empty(Kc, dtype=torch.float32, device=centroids.device)
    _call("m3s_asmk_centroid_norms", _p(centroids), Kc, D, _p(norms), _stream(centroids.device))
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
    for name, t in (("feat", feat), ("centroids", centroids), ("norms", norms)):
        _check(t, name, torch.float32)
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
    _same_device("asmk_quantize", (("centroids", centroids), ("norms", norms), ("workspace", workspace),
                                   ("out", out), ("dist", dist)), "feat", feat.device)
    a = AsmkQuantizeArgs()
    a.des, a.centroids, a.norms = _p(feat), _p(centroids), _p(norms)
    a.n, a.Kc, a.D, a.ma = n, Kc, D, ma
    a.assign, a.dist = _p(out), _p(dist)
    a.workspace, a.workspace_bytes = _p(workspace), workspace.numel()
    _call("m3s_asmk_quantize", ctypes.byref(a), _stream(feat.device))
    return out

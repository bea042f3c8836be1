"""Device-resident ASMK retrieval: the reference's RetrievalDatabase
(mast3r_slam/retrieval_database.py:43-166) without asmk, its Cython extension,
faiss, the per-keyframe copy of the features to the host and the Python loops
over visual words.

The quantize (``quantize_custom``, :96-105) is torch on the device, as in the
reference, or with ``quantizer="device"`` the fused distance and top-MA kernel
``mast3r_slam_backends.asmk_quantize`` (no distance matrix). Everything after
it -- residual aggregation, binarisation and packing, the inverted file, the
Hamming similarity, the score accumulation and the top-k -- is the HIP code
behind ``mast3r_slam_backends.asmk_*`` (include/m3s_retrieval.h). The
parameters are the ones MASt3R fixes (mast3r/retrieval/processor.py:91-96):
binary kernel, no idf, multiple assignment 1 for the build and 5 for the query,
alpha 3, similarity threshold 0.

The retrieval network and ``prep_features`` are not part of this class: ``feat``
is what ``prep_features`` returns.
"""
from __future__ import annotations

import torch

import mast3r_slam_backends as be


def backend_edges(idx, retrieval_inds, n_consec=1):
    """The graph construction of run_backend (main.py:103-125) for keyframe
    ``idx`` and what ``update`` returned for it: the ``n_consec`` previous
    keyframes, united with the retrieved ones, without ``idx`` itself.
    -> (ii, jj), the lists FactorGraph.add_factors / add_factors_dense take."""
    kf_idx = []
    for j in range(min(n_consec, idx)):
        kf_idx.append(idx - 1 - j)
    kf_idx += list(retrieval_inds)
    kf_idx = set(kf_idx)  # remove duplicates
    kf_idx.discard(idx)  # remove the current keyframe if included
    kf_idx = list(kf_idx)
    return kf_idx, [idx] * len(kf_idx)


class RetrievalDatabase:
    """``update(feat, add_after_query, k, min_thresh)`` as the reference's, on
    the device: one host read per call (the selection), none when the database
    is empty."""

    def __init__(self, centroids, capacity=512, max_features=300, query_ma=5, build_ma=1, alpha=3.0,
                 similarity_threshold=0.0, *, use_idf=False, binary=True, quantizer="torch"):
        if use_idf:
            raise ValueError("RetrievalDatabase: use_idf=True is not supported (idf is 1 throughout)")
        if binary not in (True, "bin"):
            raise ValueError("RetrievalDatabase: only the binary ASMK kernel is supported")
        if quantizer not in ("torch", "device"):
            raise ValueError(f"RetrievalDatabase: quantizer must be 'torch' or 'device' (got {quantizer!r})")
        capacity, max_features, query_ma, build_ma = int(capacity), int(max_features), int(query_ma), int(build_ma)
        if capacity < 1 or max_features < 1 or build_ma < 1 or query_ma < build_ma:
            raise ValueError("RetrievalDatabase: need capacity, max_features >= 1 and 1 <= build_ma <= query_ma")
        if quantizer == "device" and query_ma > be.ASMK_QUANTIZE_MAX_MA:
            raise ValueError(f"RetrievalDatabase: quantizer='device' takes query_ma <= {be.ASMK_QUANTIZE_MAX_MA}")
        if max_features * query_ma > be.ASMK_MAX_PAIRS:
            raise ValueError(f"RetrievalDatabase: max_features * query_ma = {max_features * query_ma} exceeds "
                             f"{be.ASMK_MAX_PAIRS} (n * multiple_assignment of one aggregate)")
        if not isinstance(centroids, torch.Tensor) or centroids.device.type != "cuda":
            raise RuntimeError("RetrievalDatabase: centroids must be a tensor on a ROCm device; no CPU path")
        if centroids.dim() != 2:
            raise RuntimeError("RetrievalDatabase: centroids must be [Kc, D]")
        self.centroids = centroids.to(torch.float32).contiguous()
        self.device = self.centroids.device
        self.Kc, self.D = (int(x) for x in self.centroids.shape)
        self.capacity, self.max_features = capacity, max_features
        self.query_ma, self.build_ma = query_ma, build_ma
        self.alpha, self.similarity_threshold = float(alpha), float(similarity_threshold)
        self.centroids_sq = torch.sum(self.centroids**2, dim=1)  # |c|^2, once per database
        cap_entries = capacity * max_features * build_ma
        store = torch.empty(be.asmk_store_size(capacity, cap_entries, self.D), dtype=torch.uint8, device=self.device)
        ws = torch.empty(be.asmk_workspace_size(self.Kc, self.D, capacity), dtype=torch.uint8, device=self.device)
        self.handle = be.AsmkHandle(store, ws, capacity, cap_entries, self.Kc, self.D)
        be.asmk_reset(self.handle)
        self.quantizer = quantizer
        if quantizer == "device":  # everything m3s_asmk_quantize needs, once: no allocation per call
            if query_ma > self.Kc:
                raise ValueError(f"RetrievalDatabase: query_ma = {query_ma} exceeds the {self.Kc} centroids")
            self.centroid_norms = be.asmk_centroid_norms(self.centroids)
            self._quantize_ws = torch.empty(be.asmk_quantize_workspace_size(max_features, self.Kc, query_ma),
                                            dtype=torch.uint8, device=self.device)
            self._assign = torch.empty(max_features * query_ma, dtype=torch.int64, device=self.device)
        self.kf_counter = 0
        self.kf_ids = []

    # ------------------------------------------------------------ pieces --
    def _features(self, feat):
        if not isinstance(feat, torch.Tensor) or feat.device != self.device:
            raise RuntimeError(f"RetrievalDatabase: feat must be a tensor on {self.device}; no CPU path")
        if feat.dim() == 3:
            if feat.shape[0] != 1:
                raise RuntimeError("RetrievalDatabase: one frame at a time (feat [1, n, D])")
            feat = feat[0]
        if feat.dim() != 2 or feat.shape[1] != self.D:
            raise RuntimeError(f"RetrievalDatabase: feat must be [n, {self.D}] or [1, n, {self.D}]")
        if not 1 <= feat.shape[0] <= self.max_features:
            raise RuntimeError(f"RetrievalDatabase: n = {feat.shape[0]} features, max_features = {self.max_features}")
        return feat.to(torch.float32).contiguous()

    def quantize(self, feat, multiple_assignment):
        """quantize_custom (:96-105): the ``multiple_assignment`` nearest
        centroids of every feature, nearest first -> [n, ma] int64. With
        ``quantizer="device"`` it is m3s_asmk_quantize and the result is a view
        of the database's own buffer, valid until the next quantize."""
        if self.quantizer == "device":
            n, ma = int(feat.shape[0]), int(multiple_assignment)
            if not (1 <= n <= self.max_features and 1 <= ma <= self.query_ma):
                raise RuntimeError(f"RetrievalDatabase: the device quantizer was sized for n <= {self.max_features} "
                                   f"and multiple_assignment <= {self.query_ma}")
            return be.asmk_quantize(feat, self.centroids, self.centroid_norms, ma, self._quantize_ws,
                                    out=self._assign[:n * ma].view(n, ma))
        l2_dists = (
            torch.sum(feat**2, dim=1)[:, None]
            + self.centroids_sq[None, :]
            - 2 * (feat @ self.centroids.mT)
        )
        return torch.topk(l2_dists, multiple_assignment, dim=1, largest=False).indices

    def _search(self, feat, build_ma, k, min_thresh):
        assign = self.quantize(feat, self.query_ma)
        be.asmk_aggregate(self.handle, feat, self.centroids, assign, self.query_ma, build_ma)
        be.asmk_search(self.handle, self.kf_counter, k, self.alpha, self.similarity_threshold, min_thresh)

    def _append(self):
        full = self.kf_counter >= self.capacity
        be.asmk_append(self.handle)  # at capacity the device refuses it and sets ASMK_INFO_FULL
        if full:
            raise RuntimeError(f"RetrievalDatabase: full ({self.capacity} images); nothing was added")
        self.kf_ids.append(self.kf_counter)
        self.kf_counter += 1

    # ------------------------------------------------------------ public --
    def update(self, feat, add_after_query, k, min_thresh=0.0):
        """retrieval_database.py:43-72 -> the ids of at most ``k`` stored images
        with score > ``min_thresh``, best first (equal scores: lower id first)."""
        feat = self._features(feat)
        k = int(k)
        if not 1 <= k <= be.ASMK_MAX_K:
            raise RuntimeError(f"RetrievalDatabase: k must be in [1, {be.ASMK_MAX_K}]")
        topk_image_inds = []
        if self.kf_counter > 0:  # only query if there is an image already
            self._search(feat, self.build_ma if add_after_query else 0, k, float(min_thresh))
            out = be.asmk_read_out(self.handle)  # the call's one host read
            topk_image_inds = list(out.idx[:out.count])
        elif add_after_query:
            be.asmk_aggregate(self.handle, feat, self.centroids, self.quantize(feat, self.build_ma), 0, self.build_ma)
        if add_after_query:
            self._append()
        return topk_image_inds

    def query(self, feat):
        """The scores of ``feat`` against every stored image: float64
        [n_images] on the device (a copy; no host read)."""
        feat = self._features(feat)
        if self.kf_counter == 0:
            return torch.zeros(0, dtype=torch.float64, device=self.device)
        self._search(feat, 0, 1, 0.0)
        return self.handle.ws_section("scores")[:self.kf_counter].clone()

    def add_to_database(self, feat):
        """Add ``feat`` as the next image without a query (:89-94, :138-166)."""
        feat = self._features(feat)
        be.asmk_aggregate(self.handle, feat, self.centroids, self.quantize(feat, self.build_ma), 0, self.build_ma)
        self._append()

    def info(self):
        """The store's sticky info bits (be.ASMK_INFO_*): a host read, for
        diagnostics."""
        return int(self.handle.section("header")[2])

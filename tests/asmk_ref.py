"""Numpy restatement of the ASMK path of the reference's RetrievalDatabase.update
with the parameters MASt3R fixes (binary kernel, use_idf=False):
ASMKKernel.aggregate_image (asmk/kernel.py:26-39), hamming.pyx's
binarize_and_pack_2D and hamming_cdist_packed, ASMKKernel.similarity
(kernel.py:56-68), functional.asmk_kernel, IVF.add / IVF.search
(inverted_file.py:56-108), the selection of retrieval_database.py:59-67 and the
fp64 form of quantize_custom (:96-105).

TEST INFRASTRUCTURE ONLY (tests/test_retrieval_ref.py checks it against
fixtures written by the reference's own modules; tests/test_gpu_retrieval.py and
tools/retrieval_time.py compare the device code with it). It restates the
reference's arithmetic, operation for operation and with its dtypes, in this
project's own words; the store keeps the reference's per-word posting lists so
that every score sums its terms in the reference's order.
"""
import numpy as np


def quantize(des, centroids, ma):
    """The `ma` nearest centroids of every descriptor, nearest first, from fp64
    distances |q|^2 + |c|^2 - 2 q.c -> (words [n, ma] int64, sorted distances
    [n, Kc] fp64)."""
    q, c = des.astype(np.float64), centroids.astype(np.float64)
    d = (q**2).sum(1)[:, None] + (c**2).sum(1)[None, :] - 2 * (q @ c.T)
    order = np.argsort(d, axis=1, kind="stable")
    return order[:, :ma].astype(np.int64), np.take_along_axis(d, order, axis=1)


def binarize_and_pack_2D(arr):
    """hamming.pyx:79-109: bit = value > 0, the first component in the most
    significant bit of each uint32, a short last word shifted left."""
    n, D = arr.shape
    D32 = -(-D // 32)
    out = np.zeros((n, D32), np.uint32)
    for j in range(D32):
        seg = arr[:, 32 * j:min(32 * j + 32, D)] > 0
        tmp = np.zeros(n, np.uint64)
        for b in range(seg.shape[1]):
            tmp = (tmp << np.uint64(1)) + seg[:, b].astype(np.uint64)
        out[:, j] = (tmp << np.uint64(32 * j + 32 - min(32 * j + 32, D))).astype(np.uint32)
    return out


def popcount32(x):
    x = x.astype(np.uint32)
    n = np.zeros(x.shape, np.int32)
    for b in range(32):
        n += ((x >> np.uint32(b)) & np.uint32(1)).astype(np.int32)
    return n


def hamming_cdist_packed(qcode, codes):
    """hamming.pyx:33-42,128-152 for one query code: the int bit count over the
    float32 padded length 32 * D32, a float32 division -> float32 [m]."""
    pop = popcount32(codes ^ qcode[None, :]).sum(1).astype(np.int32)
    return (pop.astype(np.float32) / np.float32(32 * codes.shape[1])).astype(np.float32)


def aggregate_image(des, word_ids, centroids):
    """kernel.py:26-39 (binary): -> (codes [U, D32] uint32, words [U])."""
    unique_ids = np.unique(word_ids)
    ades = np.empty((unique_ids.shape[0], des.shape[1]), dtype=np.float32)
    for i, word in enumerate(unique_ids):
        ades[i] = (des[(word_ids == word).any(axis=1)] - centroids[word]).sum(0)
    return binarize_and_pack_2D(ades), unique_ids


class IVF:
    """inverted_file.py with use_idf=False: per-word posting lists."""

    def __init__(self, codebook_size):
        self.vecs = [[] for _ in range(codebook_size)]
        self.image_ids = [[] for _ in range(codebook_size)]
        self.norm_factor = np.zeros(0)  # float64, as np.concatenate(([], zeros)) makes it
        self.n_images = 0

    def add(self, codes, words):
        """IVF.add for one image, the next id."""
        imid = self.n_images
        self.norm_factor = np.concatenate((self.norm_factor, np.zeros(1)))
        self.n_images += 1
        for code, word in zip(codes, words):
            self.vecs[word].append(code)
            self.image_ids[word].append(imid)
            self.norm_factor[imid] += 1

    def search(self, codes, words, alpha=3.0, similarity_threshold=0.0):
        """IVF.search with topk=None, before the ranking: scores float64 [n_images]."""
        scores = np.zeros(self.n_images)
        q_norm_factor = 0
        for qvec, word in zip(codes, words):
            q_norm_factor += np.float32(1)  # idf[word], a float32 one
            if not self.image_ids[word]:
                continue  # empty visual word
            image_ids = np.array(self.image_ids[word])
            norm_hdist = hamming_cdist_packed(qvec, np.stack(self.vecs[word]))
            sim = -2 * norm_hdist + 1  # float32, in [-1, 1]
            mask = sim >= similarity_threshold  # functional.asmk_kernel
            image_ids, sim = image_ids[mask], np.power(sim[mask], alpha)
            sim *= np.float32(1)  # idf
            sim /= np.sqrt(self.norm_factor[image_ids])  # a float64 quotient stored as float32
            scores[image_ids] += sim
        return scores / np.sqrt(q_norm_factor)


def select(scores, k, min_thresh):
    """retrieval_database.py:59-67: the min(k, n) highest scores, those
    > min_thresh, best first; equal scores go to the lower id."""
    order = np.argsort(-scores, kind="stable")[:min(k, scores.shape[0])]
    return [int(i) for i in order if scores[i] > min_thresh]


def assignment_gap(sorted_d, ma):
    """Per feature, the gap between its ma-th and (ma+1)-th smallest distance
    relative to the ma-th: how unambiguous the top-ma assignment is."""
    return (sorted_d[:, ma] - sorted_d[:, ma - 1]) / sorted_d[:, ma - 1]


def selection_margin(scores, k, min_thresh):
    """The smallest relative distance that decides select(scores, k,
    min_thresh): between the k-th and (k+1)-th score, and between each of the
    top-k scores and min_thresh. inf when nothing is to decide."""
    s = np.sort(scores)[::-1]
    m = np.inf
    if s.shape[0] > k:
        m = min(m, abs(s[k - 1] - s[k]) / max(abs(s[k - 1]), abs(s[k]), 1e-300))
    for v in s[:k]:
        m = min(m, abs(v - min_thresh) / max(abs(v), abs(min_thresh), 1e-300))
    return m


def make_scene(Kc, n, D, n_images, seed, noise=0.15, gap=1e-3):
    """Synthetic retrieval inputs: unit-variance centroids [Kc, D], and images
    that see n of 2n landmarks on a ring (image i the window starting at
    i * (n // 4), wrapping), so that neighbours share most landmarks, distant
    images none, and the last images close the loop with the first. A landmark
    is a centroid plus a fixed offset; an observation adds fresh noise. A
    feature whose 1st/2nd or 5th/6th fp64 distances are closer than `gap`
    (relative) is drawn again, so every top-1 and top-5 assignment is
    unambiguous in fp32 as well. -> (centroids f32, [des f32 [n, D]] * n_images)."""
    rng = np.random.default_rng(seed)
    centroids = rng.standard_normal((Kc, D)).astype(np.float32)
    L = 2 * n
    lm_word = rng.integers(0, Kc, L)
    lm_off = (0.3 * rng.standard_normal((L, D))).astype(np.float32)
    images = []
    for i in range(n_images):
        lm = (i * (n // 4) + np.arange(n)) % L
        des = np.empty((n, D), np.float32)
        todo = np.arange(n)
        while todo.size:
            des[todo] = (centroids[lm_word[lm[todo]]] + lm_off[lm[todo]]
                         + (noise * rng.standard_normal((todo.size, D))).astype(np.float32))
            _, sd = quantize(des[todo], centroids, 6)
            todo = todo[(assignment_gap(sd, 1) <= gap) | (assignment_gap(sd, 5) <= gap)]
        images.append(des)
    return centroids, images


class Database:
    """RetrievalDatabase.update on given word assignments (the caller
    quantizes): assign [n, query_ma]; the build uses its first build_ma columns."""

    def __init__(self, centroids, query_ma=5, build_ma=1, alpha=3.0, similarity_threshold=0.0):
        self.centroids = np.ascontiguousarray(centroids, dtype=np.float32)
        self.ivf = IVF(self.centroids.shape[0])
        self.query_ma, self.build_ma = query_ma, build_ma
        self.alpha, self.similarity_threshold = alpha, similarity_threshold
        self.kf_counter = 0

    def query(self, des, assign):
        codes, words = aggregate_image(des, assign[:, :self.query_ma], self.centroids)
        return self.ivf.search(codes, words, self.alpha, self.similarity_threshold)

    def add(self, des, assign):
        codes, words = aggregate_image(des, assign[:, :self.build_ma], self.centroids)
        self.ivf.add(codes, words)
        self.kf_counter += 1
        return codes, words

    def update(self, des, assign, add_after_query, k, min_thresh=0.0):
        """-> (selection, scores or None)."""
        inds, scores = [], None
        if self.kf_counter > 0:
            scores = self.query(des, assign)
            inds = select(scores, k, min_thresh)
        if add_after_query:
            self.add(des, assign)
        return inds, scores

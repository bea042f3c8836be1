"""The device quantize (m3s_asmk_quantize: fused distance and top-MA on the f32
MFMA, no distance matrix) against asmk_ref.quantize, the fp64 stable-order
reference the retrieval tests use.

Cases (Kc, n, D, images): the two fixtures (97, 37, 64 / 40: one ragged
centroid tile, a feature tail, and at D = 40 a k tail), the d1024 scene
(512, 300, 1024: four centroid tiles, three feature tiles), and an off-tile
scene (1000, 70, 96: eight centroid tiles with a ragged last one, D = 3 k
tiles). Every comparison of assignments is exact (zero differing rows), after
asserting in fp64 on the CPU that each feature's MA-th and (MA+1)-th distances
differ by more than 1e-4 of the distance.

`dist` is |c|^2 - 2 q.c: a k-ordered fp32 fmaf chain (error about
1.5e-7 * sum |q_k c_k| at K <= 1024, doubled by the factor 2), the fp32 norm
(one rounding of an fp64 sum, 6e-8 |c|^2) and the final fmaf's rounding;
atol = 4e-7 * (|c|^2 + 2 sum |q_k c_k|) per entry is about twice that.
Observed maximum of |error| / that scale on an MI355X: see DESIGN.md §4."""
import os

import numpy as np
import pytest
import torch

import asmk_ref

pytestmark = pytest.mark.gpu

QUERY_MA, BUILD_MA = 5, 1
K, MIN_THRESH = 3, 5e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


def load_case(name, golden_dir):
    if name == "d1024":
        return asmk_ref.make_scene(512, 300, 1024, 12, seed=31)
    if name == "offtile":
        return asmk_ref.make_scene(1000, 70, 96, 2, seed=37)
    fx = np.load(os.path.join(golden_dir, f"retrieval_{name}.npz"))
    return fx["centroids"], list(fx["des"])


@pytest.fixture(scope="module", params=["d64", "d40", "d1024", "offtile"])
def case(request, golden_dir):
    """Inputs and the fp64 reference, computed once: per image the words in
    stable distance order (8 of them) and the sorted fp64 distances."""
    centroids, images = load_case(request.param, golden_dir)
    ref = [asmk_ref.quantize(d, centroids, 8) for d in images]
    return dict(name=request.param, centroids=centroids, images=images, words=[r[0] for r in ref],
                sorted_d=[r[1] for r in ref])


class Quantizer:
    """be.asmk_quantize on one codebook with preallocated buffers."""

    def __init__(self, be, centroids, n_max, ma_max, dev):
        self.be = be
        self.centroids = torch.from_numpy(np.ascontiguousarray(centroids)).to(dev)
        self.norms = be.asmk_centroid_norms(self.centroids)
        self.ws = torch.empty(be.asmk_quantize_workspace_size(n_max, centroids.shape[0], ma_max), dtype=torch.uint8,
                              device=dev)

    def __call__(self, des, ma, with_dist=False):
        feat = des if isinstance(des, torch.Tensor) else torch.from_numpy(des).to(self.centroids.device)
        dist = torch.empty((feat.shape[0], ma), dtype=torch.float32, device=feat.device) if with_dist else None
        assign = self.be.asmk_quantize(feat, self.centroids, self.norms, ma, self.ws, dist=dist)
        return (assign, dist) if with_dist else assign


def check_exact(case, be, dev, ma):
    qz = Quantizer(be, case["centroids"], case["images"][0].shape[0], ma, dev)
    for i, des in enumerate(case["images"]):
        assert asmk_ref.assignment_gap(case["sorted_d"][i], ma).min() > 1e-4, i  # in fp64 on the CPU
        got = qz(des, ma).cpu().numpy()
        assert got.dtype == np.int64 and got.shape == (des.shape[0], ma)
        assert int((got != case["words"][i][:, :ma]).any(axis=1).sum()) == 0, (case["name"], ma, i)


@pytest.mark.parametrize("ma", [5, 1])
def test_assignment_equals_fp64_assignment(case, be, dev, ma):
    check_exact(case, be, dev, ma)


def test_assignment_ma8(be, dev, golden_dir):
    centroids, images = load_case("offtile", golden_dir)
    ref = [asmk_ref.quantize(d, centroids, 9) for d in images]
    case = dict(name="offtile", centroids=centroids, images=images, words=[r[0] for r in ref],
                sorted_d=[r[1] for r in ref])
    check_exact(case, be, dev, 8)


def test_ma_equal_to_codebook_size(be, dev):
    """Kc = 5 = ma: every word exactly once per row, in distance order; the 123
    rows of the centroid tile past Kc never take a slot."""
    rng = np.random.default_rng(5)
    centroids = rng.standard_normal((5, 8)).astype(np.float32)
    des = rng.standard_normal((3, 8)).astype(np.float32)
    words, sd = asmk_ref.quantize(des, centroids, 5)
    assert (np.diff(sd, axis=1) / sd[:, :-1]).min() > 1e-4
    got = Quantizer(be, centroids, 3, 5, dev)(des, 5).cpu().numpy()
    assert np.array_equal(np.sort(got, axis=1), np.tile(np.arange(5), (3, 1)))
    assert np.array_equal(got, words)


def test_dist_is_the_ranked_value(case, be, dev):
    centroids = case["centroids"].astype(np.float64)
    qz = Quantizer(be, case["centroids"], case["images"][0].shape[0], QUERY_MA, dev)
    worst = 0.0
    for i, des in enumerate(case["images"][:3]):
        assign, dist = qz(des, QUERY_MA, with_dist=True)
        assign, dist = assign.cpu().numpy(), dist.cpu().numpy()
        assert np.array_equal(assign, case["words"][i][:, :QUERY_MA])
        q, c = des.astype(np.float64)[:, None, :], centroids[assign]  # [n, 1, D], [n, ma, D]
        ref = (c**2).sum(-1) - 2 * (q * c).sum(-1)
        scale = (c**2).sum(-1) + 2 * np.abs(q * c).sum(-1)
        err = np.abs(dist.astype(np.float64) - ref)
        worst = max(worst, float((err / scale).max()))
        print(f"{case['name']} image {i}: max |dist - fp64| / (|c|^2 + 2 sum|q c|) = {float((err / scale).max()):.3e}")
        assert (err <= 4e-7 * scale).all(), (case["name"], i, float((err / scale).max()))
        assert (np.diff(dist, axis=1) >= 0).all()  # nearest first
    print(f"{case['name']}: worst {worst:.3e} of the 4e-7 allowed")


def tie_scene():
    """A codebook whose row B is a bitwise copy of row A, 280 rows (two
    centroid tiles) apart; a third of the features lie near that centroid."""
    rng = np.random.default_rng(11)
    Kc, n, D, A, B = 400, 70, 64, 20, 300
    centroids = rng.standard_normal((Kc, D)).astype(np.float32)
    centroids[B] = centroids[A]
    des = np.empty((n, D), np.float32)
    todo = np.arange(n)
    while todo.size:  # as make_scene: draw again what is ambiguous, or has A last in its list
        des[todo] = rng.standard_normal((todo.size, D)).astype(np.float32)
        near = todo[todo % 3 == 0]
        des[near] = centroids[A] + (0.3 * rng.standard_normal((near.size, D))).astype(np.float32)
        words, sd = asmk_ref.quantize(des[todo], centroids, QUERY_MA + 1)
        gaps = np.diff(sd[:, :QUERY_MA + 1], axis=1) / sd[:, :QUERY_MA]
        gaps[(words[:, :-1] == A) & (words[:, 1:] == B)] = 1.0
        todo = todo[(gaps.min(axis=1) <= 1e-3) | (words[:, QUERY_MA - 1] == A)]
    return centroids, des, A, B


def test_equal_distances_come_out_lower_word_first(be, dev):
    centroids, des, A, B = tie_scene()
    assert centroids[A].tobytes() == centroids[B].tobytes() and B - A >= 150
    words, sd = asmk_ref.quantize(des, centroids, QUERY_MA + 1)  # stable: A before B
    # the pair never straddles the end of the list, and nothing else is close to a swap
    assert not (words[:, QUERY_MA - 1] == A).any()
    gaps = np.diff(sd[:, :QUERY_MA + 1], axis=1) / sd[:, :QUERY_MA]
    pair = (words[:, :-1] == A) & (words[:, 1:] == B)
    assert (gaps[pair] == 0).all() and gaps[~pair].min() > 1e-4
    assign, dist = Quantizer(be, centroids, des.shape[0], QUERY_MA, dev)(des, QUERY_MA, with_dist=True)
    got, dist = assign.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(got, words[:, :QUERY_MA])
    rows = 0
    for r in range(got.shape[0]):
        row = got[r].tolist()
        if A in row or B in row:
            assert A in row and B in row and row.index(B) == row.index(A) + 1, (r, row)
            assert dist[r, row.index(A)].tobytes() == dist[r, row.index(B)].tobytes()
            rows += 1
    assert rows >= des.shape[0] // 3


def test_second_call_and_poisoned_workspace_are_bitwise_identical(case, be, dev):
    des = case["images"][0]
    qz = Quantizer(be, case["centroids"], des.shape[0], QUERY_MA, dev)
    a, da = qz(des, QUERY_MA, with_dist=True)
    b, db_ = qz(des, QUERY_MA, with_dist=True)
    qz.ws.fill_(0xFF)
    c, dc = qz(des, QUERY_MA, with_dist=True)
    for x, y in ((a, b), (a, c), (da, db_), (da, dc)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


# ------------------------------------------------------------ end to end --
def u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", ["d64", "d40", "d1024"])
def test_update_sequence_with_device_quantizer_matches_reference(name, be, dev, golden_dir):
    """update(add_after_query=True) for every image, as
    test_gpu_retrieval.py::test_update_sequence_matches_reference requires of
    the torch path: words, codes and img_ptr bitwise, scores at rtol 1e-6,
    selections exact."""
    from mast3r_slam_amd.retrieval import RetrievalDatabase

    centroids, images = load_case(name, golden_dir)
    assigns = [asmk_ref.quantize(d, centroids, QUERY_MA)[0] for d in images]
    ref = asmk_ref.Database(centroids, QUERY_MA, BUILD_MA)
    db = RetrievalDatabase(torch.from_numpy(centroids).to(dev), capacity=16, max_features=images[0].shape[0],
                           quantizer="device")
    assert db.quantizer == "device"
    ref_words, ref_codes = [], []
    for i, (des, assign) in enumerate(zip(images, assigns)):
        qa = asmk_ref.aggregate_image(des, assign[:, :QUERY_MA], centroids)
        ba = asmk_ref.aggregate_image(des, assign[:, :BUILD_MA], centroids)
        ref_inds, ref_scores = ref.update(des, assign, True, K, MIN_THRESH)
        if ref_scores is not None:
            assert asmk_ref.selection_margin(ref_scores, K, MIN_THRESH) > 1e-5, i
        feat = torch.from_numpy(des).to(dev)
        inds = db.update(feat[None] if i % 2 else feat, True, K, MIN_THRESH)
        for s, (codes_ref, words_ref) in ((0, qa), (1, ba)):
            if s == 0 and i == 0:
                continue  # the first image is added without a query
            U = int(db.handle.ws_section("counts")[s])
            assert np.array_equal(db.handle.ws_section("words")[s, :U].cpu().numpy(), words_ref), (s, i)
            assert np.array_equal(u32(db.handle.ws_section("codes")[s, :U]), codes_ref), (s, i)
        if i:
            scores = db.handle.ws_section("scores")[:i].cpu().numpy()
            assert np.allclose(scores, ref_scores, rtol=1e-6, atol=0.0), i
        assert inds == ref_inds, (i, inds, ref_inds)
        ref_codes.append(ba[0]), ref_words.append(ba[1])
    h = db.handle
    words, codes = np.concatenate(ref_words), np.concatenate(ref_codes)
    ptr = np.concatenate(([0], np.cumsum([w.shape[0] for w in ref_words])))
    hdr = h.section("header").cpu().numpy()
    assert (int(hdr[0]), int(hdr[1]), int(hdr[2])) == (words.shape[0], len(images), 0)
    assert np.array_equal(h.section("img_ptr").cpu().numpy()[:len(images) + 1], ptr)
    assert np.array_equal(h.section("word").cpu().numpy()[:words.shape[0]], words)
    assert np.array_equal(u32(h.section("codes"))[:words.shape[0]], codes)


def peak_of_one_update(db, feat):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    db.update(feat, False, K, MIN_THRESH)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def test_no_distance_matrix_is_allocated(be, dev, golden_dir):
    from mast3r_slam_amd.retrieval import RetrievalDatabase

    centroids, images = load_case("d1024", golden_dir)
    n, Kc = images[0].shape[0], centroids.shape[0]
    cent = torch.from_numpy(centroids).to(dev)
    feats = [torch.from_numpy(d).to(dev) for d in images[:3]]
    peaks = {}
    for quantizer in ("device", "torch"):
        db = RetrievalDatabase(cent, capacity=4, max_features=n, quantizer=quantizer)
        db.update(feats[0], True, K, MIN_THRESH)
        db.update(feats[1], False, K, MIN_THRESH)  # warm-up of the measured call's path
        peaks[quantizer] = peak_of_one_update(db, feats[2])
    print(f"peak bytes above the baseline during one update: {peaks}; a distance matrix is {n * Kc * 4}")
    assert peaks["device"] < n * Kc * 4
    assert peaks["torch"] > n * Kc * 4  # the check measures something

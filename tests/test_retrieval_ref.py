"""tests/asmk_ref.py (the numpy restatement the device retrieval is compared
with) reproduces the fixtures that tests/golden/make_retrieval_golden.py wrote
from the reference's own ASMKKernel / IVF / asmk_kernel / hamming code: the words
are equal, the packed codes bitwise equal, the scores equal to 1e-12, the
selections equal. D = 40 exercises the shifted last word and the normalisation
by the padded bit count. CPU only."""
import os

import numpy as np
import pytest

import asmk_ref

QUERY_MA, BUILD_MA = 5, 1


@pytest.fixture(scope="module", params=[64, 40])
def fx(request, golden_dir):
    return dict(np.load(os.path.join(golden_dir, f"retrieval_d{request.param}.npz")))


def test_fixture_shapes_and_provenance(fx):
    n_images, n, D = fx["des"].shape
    assert (n_images, n) == (10, 37) and D in (64, 40) and fx["centroids"].shape == (97, D)
    assert fx["assign"].shape == (n_images, n, QUERY_MA)
    assert "hamming" in str(fx["hamming_impl"])
    assert int(fx["k"]) == 3 and float(fx["min_thresh"]) == 5e-3
    assert fx["q_codes_0"].dtype == np.uint32 and fx["q_codes_0"].shape[1] == -(-D // 32)


def test_fixture_assignments_are_unambiguous(fx):
    """The assignments stored are the fp64 nearest centroids, and each is
    decided by more than 1e-4 of the distance (what the GPU test relies on)."""
    for i, des in enumerate(fx["des"]):
        assign, sd = asmk_ref.quantize(des, fx["centroids"], QUERY_MA)
        assert np.array_equal(assign, fx["assign"][i])
        assert asmk_ref.assignment_gap(sd, BUILD_MA).min() > 1e-4
        assert asmk_ref.assignment_gap(sd, QUERY_MA).min() > 1e-4


def test_aggregates_match_reference_bitwise(fx):
    for i, des in enumerate(fx["des"]):
        assign = fx["assign"][i]
        for tag, ma in (("q", QUERY_MA), ("b", BUILD_MA)):
            codes, words = asmk_ref.aggregate_image(des, assign[:, :ma], fx["centroids"])
            assert np.array_equal(words, fx[f"{tag}_words_{i}"]), (tag, i)
            assert codes.dtype == np.uint32 and np.array_equal(codes, fx[f"{tag}_codes_{i}"]), (tag, i)


def test_short_last_word_is_shifted_left(fx):
    D = fx["des"].shape[2]
    if D % 32:
        low = np.uint32((1 << (32 - D % 32)) - 1)
        assert not (fx["q_codes_3"][:, -1] & low).any()  # the padding bits are the low ones, all zero
        assert (fx["q_codes_3"][:, -1] >> np.uint32(32 - D % 32)).any()


def test_scores_and_selections_match_reference(fx):
    db = asmk_ref.Database(fx["centroids"], QUERY_MA, BUILD_MA)
    k, min_thresh = int(fx["k"]), float(fx["min_thresh"])
    for i, des in enumerate(fx["des"]):
        inds, scores = db.update(des, fx["assign"][i], True, k, min_thresh)
        assert inds == list(fx["sel"][i, :fx["sel_len"][i]]), i
        if i == 0:
            assert scores is None
            continue
        ref = fx[f"scores_{i}"]
        assert scores.dtype == np.float64 and scores.shape == ref.shape == (i,)
        assert np.abs(scores - ref).max() <= 1e-12, i
        # the selection is decided by more than 1e-5 relative (what the GPU test relies on)
        assert asmk_ref.selection_margin(ref, k, min_thresh) > 1e-5, i
    assert np.array_equal(db.ivf.norm_factor, fx["norm_factor"])


def test_padded_normalisation():
    """h divides by 32 * ceil(D / 32), not by D (hamming.pyx:36-37)."""
    a = np.array([0xFF000000, 0x00000000], np.uint32)  # D = 40 would be 2 words
    b = np.zeros((1, 2), np.uint32)
    assert asmk_ref.hamming_cdist_packed(a, b)[0] == np.float32(8 / 64)


def test_select_ties_and_threshold():
    s = np.array([0.2, 0.5, 0.5, 0.1, 0.0])
    assert asmk_ref.select(s, 3, 0.0) == [1, 2, 0]
    assert asmk_ref.select(s, 3, 0.2) == [1, 2]  # strictly greater
    assert asmk_ref.select(s[:2], 3, 0.0) == [1, 0]  # min(k, n_images)

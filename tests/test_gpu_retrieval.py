"""Device ASMK retrieval (mast3r_slam_amd.retrieval.RetrievalDatabase over the
m3s_asmk_* kernels) against tests/asmk_ref.py, the numpy restatement that
tests/test_retrieval_ref.py ties to the reference's own code.

Cases: the two fixtures (Kc = 97, n = 37, 10 images, D = 64 and D = 40: the
shifted last word and the padded normalisation) and one synthetic case at the
descriptor size of the real network (D = 1024, Kc = 512, n = 300, 12 images).

What is compared, and how tightly:
* the torch assignment with the fp64 one: zero differing rows. Every feature's
  MA-th and (MA+1)-th distances differ by more than 1e-4 of the distance
  (asserted in fp64 first), far above the fp32 error of the distance;
* codes and words of both aggregates, img_ptr and the counters: bitwise. The
  residual sums add the features in ascending order one after the other on both
  sides, in fp32, so there is nothing to allow for;
* scores: rtol 1e-6. Every term is non-negative; a device term and a numpy term
  differ by at most the fp32 rounding of the cube and of the division
  (~2.4e-7 relative); both sides accumulate in fp64;
* selections: exactly, after asserting on the reference that each is decided by
  more than 1e-5 relative.
"""
import ctypes
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


def reference_run(centroids, images, assigns):
    """The whole update(add_after_query=True) sequence on the CPU, once per
    case: per image the two aggregates, the scores and the selection."""
    db = asmk_ref.Database(centroids, QUERY_MA, BUILD_MA)
    steps = []
    for des, assign in zip(images, assigns):
        q = asmk_ref.aggregate_image(des, assign[:, :QUERY_MA], centroids)
        b = asmk_ref.aggregate_image(des, assign[:, :BUILD_MA], centroids)
        inds, scores = db.update(des, assign, True, K, MIN_THRESH)
        steps.append(dict(q=q, b=b, inds=inds, scores=scores))
    return steps


@pytest.fixture(scope="module", params=["d64", "d40", "d1024"])
def case(request, golden_dir):
    if request.param == "d1024":
        centroids, images = asmk_ref.make_scene(512, 300, 1024, 12, seed=31)
        assigns, fixture_sel = [asmk_ref.quantize(d, centroids, QUERY_MA)[0] for d in images], None
    else:
        fx = np.load(os.path.join(golden_dir, f"retrieval_{request.param}.npz"))
        centroids, images, assigns = fx["centroids"], list(fx["des"]), list(fx["assign"])
        fixture_sel = [list(s[:n]) for s, n in zip(fx["sel"], fx["sel_len"])]
        assert int(fx["k"]) == K and float(fx["min_thresh"]) == MIN_THRESH
    steps = reference_run(centroids, images, assigns)
    for i, st in enumerate(steps):  # (b): every selection is decided by a clear margin
        if st["scores"] is not None:
            assert asmk_ref.selection_margin(st["scores"], K, MIN_THRESH) > 1e-5, i
    if fixture_sel is not None:
        assert [st["inds"] for st in steps] == fixture_sel
    return dict(name=request.param, centroids=centroids, images=images, assigns=assigns, steps=steps)


def new_db(case, dev, **kw):
    from mast3r_slam_amd.retrieval import RetrievalDatabase

    kw.setdefault("capacity", 16)
    kw.setdefault("max_features", case["images"][0].shape[0])
    return RetrievalDatabase(torch.from_numpy(case["centroids"]).to(dev), **kw)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def device_aggregate(db, s, be):
    """(codes uint32 [U, D32], words [U]) of workspace set s (0 query, 1 build)."""
    U = int(db.handle.ws_section("counts")[s])
    return u32(db.handle.ws_section("codes")[s, :U]), db.handle.ws_section("words")[s, :U].cpu().numpy()


def store_state(db):
    h = db.handle
    hdr = h.section("header").cpu().numpy()
    return dict(n_entries=int(hdr[0]), n_images=int(hdr[1]), info=int(hdr[2]),
                img_ptr=h.section("img_ptr").cpu().numpy().copy(), word=h.section("word").cpu().numpy().copy(),
                codes=u32(h.section("codes")).copy())


def run_sequence(case, dev, be, check=True):
    """update(add_after_query=True) for every image on a fresh database ->
    (db, [scores per image])."""
    db = new_db(case, dev)
    all_scores = []
    for i, (des, st) in enumerate(zip(case["images"], case["steps"])):
        feat = torch.from_numpy(des).to(dev)
        inds = db.update(feat[None] if i % 2 else feat, True, K, MIN_THRESH)  # [1, n, D] and [n, D]
        scores = db.handle.ws_section("scores")[:i].cpu().numpy().copy() if i else None
        all_scores.append(scores)
        if not check:
            continue
        for s, tag in ((0, "q"), (1, "b")):
            if s == 0 and i == 0:
                continue  # the first image is added without a query
            codes, words = device_aggregate(db, s, be)
            ref_codes, ref_words = st[tag]
            assert np.array_equal(words, ref_words), (tag, i)
            assert np.array_equal(codes, ref_codes), (tag, i, int((codes != ref_codes).sum()))
        if i:
            print(f"{case['name']} image {i}: max rel score error "
                  f"{np.max(np.abs(scores - st['scores']) / np.maximum(st['scores'], 1e-300)):.3e}")
            assert np.allclose(scores, st["scores"], rtol=1e-6, atol=0.0), i
        assert inds == st["inds"], (i, inds, st["inds"])
        assert all(type(j) is int for j in inds)
    return db, all_scores


def test_torch_assignment_equals_fp64_assignment(case, dev):
    db = new_db(case, dev)
    for i, (des, assign) in enumerate(zip(case["images"], case["assigns"])):
        _, sd = asmk_ref.quantize(des, case["centroids"], QUERY_MA)
        assert asmk_ref.assignment_gap(sd, QUERY_MA).min() > 1e-4  # (a), in fp64 on the CPU
        assert asmk_ref.assignment_gap(sd, BUILD_MA).min() > 1e-4
        feat = torch.from_numpy(des).to(dev)
        got = db.quantize(feat, QUERY_MA).cpu().numpy()
        assert got.dtype == np.int64
        assert int((got != assign).any(axis=1).sum()) == 0, i
        assert np.array_equal(db.quantize(feat, BUILD_MA).cpu().numpy(), assign[:, :BUILD_MA]), i


def test_update_sequence_matches_reference(case, dev, be):
    db, _ = run_sequence(case, dev, be)
    n_img = len(case["images"])
    st = store_state(db)
    words = np.concatenate([s["b"][1] for s in case["steps"]])
    codes = np.concatenate([s["b"][0] for s in case["steps"]])
    ptr = np.concatenate(([0], np.cumsum([s["b"][1].shape[0] for s in case["steps"]])))
    assert st["n_images"] == n_img == db.kf_counter and db.kf_ids == list(range(n_img))
    assert st["n_entries"] == words.shape[0] and st["info"] == 0
    assert np.array_equal(st["img_ptr"][:n_img + 1], ptr)
    assert np.array_equal(st["word"][:words.shape[0]], words)
    assert np.array_equal(st["codes"][:words.shape[0]], codes)
    # the word table is clear again after every search
    assert int((db.handle.ws_section("slot") != -1).sum()) == 0
    # query(): the scores of the last image against all of them, itself included
    q = db.query(torch.from_numpy(case["images"][-1]).to(dev))
    assert q.dtype == torch.float64 and q.shape == (n_img,) and q.device.type == "cuda"
    ref = asmk_ref.Database(case["centroids"], QUERY_MA, BUILD_MA)
    for des, assign in zip(case["images"], case["assigns"]):
        ref.add(des, assign)
    assert np.allclose(q.cpu().numpy(), ref.query(case["images"][-1], case["assigns"][-1]), rtol=1e-6, atol=0.0)


def test_second_run_is_bitwise_identical(case, dev, be):
    _, a = run_sequence(case, dev, be, check=False)
    _, b = run_sequence(case, dev, be, check=False)
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()


def test_relocalisation_sequence(case, dev, be):
    """main.py:33-58: a query on an empty database, a query that adds nothing,
    then the same features added exactly once."""
    db = new_db(case, dev)
    f0, f1 = (torch.from_numpy(case["images"][i]).to(dev) for i in (0, 1))
    assert db.update(f0, False, K, MIN_THRESH) == [] and db.kf_counter == 0
    assert store_state(db)["n_images"] == 0
    assert db.query(f0).shape == (0,)
    assert db.update(f0, True, K, MIN_THRESH) == [] and db.kf_counter == 1
    before = store_state(db)
    got = db.update(f1, False, K, MIN_THRESH)  # lost frame: query only
    assert got == case["steps"][1]["inds"]
    after = store_state(db)
    assert all(np.array_equal(before[k], after[k]) for k in before) and db.kf_counter == 1
    assert db.update(f1, True, K, MIN_THRESH) == got  # relocalised: the same query, then one append
    end = store_state(db)
    assert end["n_images"] == 2 == db.kf_counter and db.kf_ids == [0, 1]
    nb = [case["steps"][i]["b"][1].shape[0] for i in (0, 1)]
    assert list(end["img_ptr"][:3]) == [0, nb[0], nb[0] + nb[1]] and end["n_entries"] == nb[0] + nb[1]
    assert np.array_equal(end["word"][nb[0]:nb[0] + nb[1]], case["steps"][1]["b"][1])


def test_query_word_without_entries_counts_in_the_norm(case, dev, be):
    """IVF.search adds idf to q_norm_factor before it looks at the posting list
    (inverted_file.py:94-97)."""
    db = new_db(case, dev)
    last = len(case["images"]) // 2  # half way round the ring: shares no landmark with image 0
    db.add_to_database(torch.from_numpy(case["images"][0]).to(dev))
    scores = db.query(torch.from_numpy(case["images"][last]).to(dev)).cpu().numpy()
    out = be.asmk_read_out(db.handle)
    q_words = case["steps"][last]["q"][1]
    stored = set(case["steps"][0]["b"][1].tolist())
    assert out.n_query_words == q_words.shape[0] > sum(1 for w in q_words.tolist() if w in stored)
    ref = asmk_ref.Database(case["centroids"], QUERY_MA, BUILD_MA)
    ref.add(case["images"][0], case["assigns"][0])
    assert np.allclose(scores, ref.query(case["images"][last], case["assigns"][last]), rtol=1e-6, atol=0.0)


def test_full_store_refuses_and_stays_unchanged(case, dev, be):
    db = new_db(case, dev, capacity=3)
    feats = [torch.from_numpy(d).to(dev) for d in case["images"][:4]]
    for f in feats[:3]:
        db.update(f, True, K, MIN_THRESH)
    before = store_state(db)
    assert before["n_images"] == 3 and before["info"] == 0 and db.info() == 0
    with pytest.raises(RuntimeError, match="full"):
        db.update(feats[3], True, K, MIN_THRESH)
    after = store_state(db)
    assert after["info"] & be.ASMK_INFO_FULL and db.info() & be.ASMK_INFO_FULL
    assert all(np.array_equal(before[k], after[k]) for k in before if k != "info")
    assert db.kf_counter == 3 and db.update(feats[3], False, K, MIN_THRESH) == case["steps"][3]["inds"]
    # the entry capacity, through the entry points: room for the first image only
    n0 = case["steps"][0]["b"][1].shape[0]
    cap_entries = n0 + case["steps"][1]["b"][1].shape[0] - 1
    D, Kc = case["centroids"].shape[1], case["centroids"].shape[0]
    h = be.AsmkHandle(torch.empty(be.asmk_store_size(8, cap_entries, D), dtype=torch.uint8, device=dev),
                      torch.empty(be.asmk_workspace_size(Kc, D, 8), dtype=torch.uint8, device=dev),
                      8, cap_entries, Kc, D)
    be.asmk_reset(h)
    cent = torch.from_numpy(case["centroids"]).to(dev)
    for i in (0, 1):
        be.asmk_aggregate(h, feats[i], cent, torch.from_numpy(case["assigns"][i]).to(dev), 0, BUILD_MA)
        be.asmk_append(h)
        hdr = h.section("header").cpu().numpy()
        assert (int(hdr[0]), int(hdr[1]), int(hdr[2])) == ((n0, 1, 0) if i == 0 else (n0, 1, be.ASMK_INFO_FULL))
    assert np.array_equal(h.section("word")[:n0].cpu().numpy(), case["steps"][0]["b"][1])
    assert list(h.section("img_ptr")[:2].cpu().numpy()) == [0, n0]


def test_out_of_range_word_sets_flag_and_is_skipped(case, dev, be):
    D, Kc = case["centroids"].shape[1], case["centroids"].shape[0]
    des, assign = case["images"][2], case["assigns"][2].copy()
    assign[3, 1], assign[5, 0], assign[7, 4] = Kc, -1, Kc + 5
    h = be.AsmkHandle(torch.empty(be.asmk_store_size(4, 4096, D), dtype=torch.uint8, device=dev),
                      torch.empty(be.asmk_workspace_size(Kc, D, 4), dtype=torch.uint8, device=dev), 4, 4096, Kc, D)
    be.asmk_reset(h)
    be.asmk_aggregate(h, torch.from_numpy(des).to(dev), torch.from_numpy(case["centroids"]).to(dev),
                      torch.from_numpy(assign).to(dev), 0, QUERY_MA)  # returns normally
    torch.cuda.synchronize()
    counts = h.ws_section("counts").cpu().numpy()
    assert counts[3] == 1 and counts[2] == 0 and counts[0] == 0
    # the reference on the same rows with the three bad entries out of every word's reach
    pad = np.concatenate((case["centroids"], np.zeros((7, D), np.float32)))
    ref_assign = assign.copy()
    ref_assign[5, 0] = Kc + 6
    ref_codes, ref_words = asmk_ref.aggregate_image(des, ref_assign, pad)
    keep = ref_words < Kc
    U = int(counts[1])
    assert U == int(keep.sum())
    assert np.array_equal(h.ws_section("words")[1, :U].cpu().numpy(), ref_words[keep])
    assert np.array_equal(u32(h.ws_section("codes")[1, :U]), ref_codes[keep])
    assert int((h.ws_section("slot") != -1).sum()) == 0  # a build-only aggregate leaves the table alone


def test_one_update_makes_one_device_to_host_copy(case, dev, be):
    from torch.profiler import ProfilerActivity, profile

    db = new_db(case, dev)
    feats = [torch.from_numpy(d).to(dev) for d in case["images"][:4]]
    for f in feats[:3]:  # also the warm-up: code objects, the allocator's blocks
        db.update(f, True, K, MIN_THRESH)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        inds = db.update(feats[3], True, K, MIN_THRESH)
        torch.cuda.synchronize()
    assert inds == case["steps"][3]["inds"]
    device_type = torch.autograd.DeviceType
    on_device = [e.name for e in prof.events() if e.device_type == device_type.CUDA]
    copies = [n for n in on_device if "memcpy" in n.lower()]
    # the runtime's own view, for where the profiler has no device tracing
    api = [e.name for e in prof.events() if e.device_type == device_type.CPU and e.name.startswith("hipMemcpy")]
    print("device copies:", copies, "runtime copy calls:", api, "device records:", len(on_device))
    assert on_device or api, "the profiler recorded neither device activity nor runtime calls"
    if on_device:
        assert len(copies) == 1, copies
        assert "htod" not in copies[0].lower() and "dtod" not in copies[0].lower(), copies
    if api:
        assert len(api) == 1, api
    out = be.asmk_read_out(db.handle)
    assert ctypes.sizeof(out) == ctypes.sizeof(be.AsmkOut) and out.n_images == 3

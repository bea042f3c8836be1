"""The device retrieval update against the reference-shaped path it replaces,
at the sizes of the real system (n = 300 features, D = 1024, a codebook of
Kc = 20 000 words), with 64 and with 512 stored images -- GPU box:

    python tools/retrieval_time.py [--out profiles/retrieval/retrieval_time.json]

device   RetrievalDatabase.update(feat, add_after_query=False, k=3): the torch
         quantize, m3s_asmk_aggregate, m3s_asmk_search and the one host read
         of the selection.
host     what retrieval_database.py does: the same torch quantize on the
         device, the features and the assignment copied to the host, then
         tests/asmk_ref.py (the numpy restatement of asmk's aggregate_image,
         IVF.search and the selection; its Hamming distance is vectorised
         numpy where the reference calls a Cython loop) on the CPU.

Both run in this process, interleaved round by round (device, host, device,
...); a round is `reps` calls by the wall clock, the device idle before and
after; the figure is the median round, the spread its min..max. The selections
and the scores of the two paths are compared before anything is timed. The
share of the device update that is the torch quantize is the quantize alone,
timed the same way, over the device figure. Prints one JSON line; --out also
writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam-ysh_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import asmk_ref  # noqa: E402
import mast3r_slam_backends as be  # noqa: E402
from mast3r_slam_amd.retrieval import RetrievalDatabase  # noqa: E402

N, D, KC, K, MIN_THRESH = 300, 1024, 20000, 3, 5e-3


def scene(n_images, dev, seed=7):
    """Centroids and images that see N of the landmarks of a ring (a landmark:
    a centroid plus a fixed offset; an observation adds noise), 75 landmarks on
    from one image to the next, so that neighbours score high and the rest low."""
    gen = torch.Generator().manual_seed(seed)
    centroids = torch.randn(KC, D, generator=gen)
    L = 75 * n_images + N
    word = torch.randint(0, KC, (L,), generator=gen)
    off = 0.3 * torch.randn(L, D, generator=gen)
    images = []
    for i in range(n_images + 1):  # the last one is the query: a revisit of the middle
        s = 75 * (i if i < n_images else n_images // 2)
        lm = torch.arange(s, s + N)
        images.append((centroids[word[lm]] + off[lm] + 0.15 * torch.randn(N, D, generator=gen)).to(dev))
    return centroids.to(dev), images


def wall(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def measure(n_images, dev, rounds, reps_device, reps_host):
    centroids, images = scene(n_images, dev)
    db = RetrievalDatabase(centroids, capacity=n_images)
    ref = asmk_ref.Database(centroids.cpu().numpy())
    cent_np = ref.centroids
    for feat in images[:n_images]:  # the same assignment (the device's) on both sides
        db.update(feat, True, K, MIN_THRESH)
        ref.add(feat.cpu().numpy(), db.quantize(feat, db.build_ma).cpu().numpy())
    query = images[n_images]

    def device():
        return db.update(query, False, K, MIN_THRESH)

    def host():
        assign = db.quantize(query, db.query_ma).cpu().numpy()
        des = query.cpu().numpy()
        codes, words = asmk_ref.aggregate_image(des, assign, cent_np)
        scores = ref.ivf.search(codes, words, ref.alpha, ref.similarity_threshold)
        return asmk_ref.select(scores, K, MIN_THRESH), scores

    def quantize():
        return db.quantize(query, db.query_ma)

    sel_d = device()
    scores_d = db.handle.ws_section("scores")[:n_images].cpu().numpy()
    sel_h, scores_h = host()
    same = sel_d == sel_h and bool(np.allclose(scores_d, scores_h, rtol=1e-6, atol=0.0))
    for fn, r in ((device, 5), (host, 1), (quantize, 5)):  # warm-up
        wall(fn, r)
    times = {"device": [], "host": [], "quantize": []}
    for _ in range(rounds):
        times["device"].append(wall(device, reps_device))
        times["host"].append(wall(host, reps_host))
        times["quantize"].append(wall(quantize, reps_device))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"stored_images": n_images, "stored_entries": int(db.handle.section("header")[0]),
           "query_words": int(be.asmk_read_out(db.handle).n_query_words), "selection": sel_d,
           "outputs_match": same, "max_rel_score_diff": float(np.max(np.abs(scores_d - scores_h)
                                                                        / np.maximum(scores_h, 1e-300)))}
    for k in times:
        out["ms_" + k] = round(med[k], 4)
        out["ms_" + k + "_min_max"] = [round(min(times[k]), 4), round(max(times[k]), 4)]
    out["host_over_device"] = round(med["host"] / med["device"], 2)
    out["quantize_share_of_device"] = round(med["quantize"] / med["device"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=(64, 512))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps-device", type=int, default=20)
    ap.add_argument("--reps-host", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("retrieval_time: no GPU; this tool only measures on the device")
    dev = torch.device("cuda:0")
    res = {"workload": "update(add_after_query=False, k=%d): n=%d features, D=%d, Kc=%d, query MA 5, build MA 1"
                       % (K, N, D, KC),
           "clock": "wall clock per call, device idle before and after; median of the rounds",
           "rounds": a.rounds, "reps_per_round": {"device": a.reps_device, "host": a.reps_host},
           "cases": [measure(n, dev, a.rounds, a.reps_device, a.reps_host) for n in a.sizes],
           "device": torch.cuda.get_device_name(0), "lib": be.version()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

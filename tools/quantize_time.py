"""The device quantize (m3s_asmk_quantize) against the torch quantize it can
replace, at the sizes of the real system (n = 300 features, D = 1024, a
codebook of Kc = 20 000 words) -- GPU box:

    python tools/quantize_time.py [--out profiles/retrieval/quantize_time.json]

(a) quantize  RetrievalDatabase.quantize of a quantizer="device" database and
              of a quantizer="torch" database on the same codebook and
              features, at multiple assignment 5 (the query) and 1 (the build).
(b) update    update(feat, add_after_query=False, k=3) of both databases with
              64 and with 512 stored images: the quantize, m3s_asmk_aggregate,
              m3s_asmk_search and the one host read of the selection.

Both paths run in this process, interleaved round by round (device, torch,
device, ...); a round is `reps` calls by the wall clock, the device idle before
and after; the figure is the median round, the spread its min..max. The
assignments of the two paths (and the selections and scores of the two
updates) are asserted equal before anything is timed; so that equality is a
fair demand of two fp32 evaluations, every feature of the scene has its six
nearest centroids more than 1e-4 (relative, in fp64) apart from one another --
a feature that has not is drawn again. f32_peak_fraction is the 2 n Kc D flop of
the distance product over the device quantize's time, as a fraction of the
157 TF f32 peak. Prints one JSON line; --out also writes it to
a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam-ysh_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import mast3r_slam_backends as be  # noqa: E402
from mast3r_slam_amd.retrieval import RetrievalDatabase  # noqa: E402
from retrieval_time import D, K, KC, MIN_THRESH, N, wall  # noqa: E402

F32_PEAK_TFLOPS = 157.0
MIN_GAP = 1e-4


def scene(n_images, dev, seed=7):
    """tools/retrieval_time.py's scene (a ring of landmarks, 75 on from one
    image to the next; the last image is the query, a revisit of the middle),
    with every feature's six nearest centroids MIN_GAP apart in fp64."""
    gen = torch.Generator().manual_seed(seed)
    centroids = torch.randn(KC, D, generator=gen)
    L = 75 * n_images + N
    word = torch.randint(0, KC, (L,), generator=gen)
    off = 0.3 * torch.randn(L, D, generator=gen)
    c64 = centroids.to(dev, torch.float64)
    c_sq = (c64**2).sum(1)
    images = []
    for i in range(n_images + 1):
        s = 75 * (i if i < n_images else n_images // 2)
        lm = torch.arange(s, s + N)
        base = (centroids[word[lm]] + off[lm]).to(dev)
        des = torch.empty(N, D, device=dev)
        todo = torch.arange(N, device=dev)
        while todo.numel():
            des[todo] = base[todo] + (0.15 * torch.randn(todo.numel(), D, generator=gen)).to(dev)
            q = des[todo].to(torch.float64)
            d = (q**2).sum(1)[:, None] + c_sq[None, :] - 2 * (q @ c64.mT)
            near = torch.topk(d, 6, dim=1, largest=False).values
            todo = todo[((near[:, 1:] - near[:, :-1]) / near[:, :-1]).min(1).values <= MIN_GAP]
        images.append(des)
    return centroids.to(dev), images


def rounds_of(fns, rounds, reps):
    """{name: [ms per call, one per round]}, the functions taking turns."""
    for fn in fns.values():  # warm-up
        wall(fn, 5)
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(wall(fn, reps))
    return times


def figures(times):
    out = {}
    for k, v in times.items():
        out["ms_" + k] = round(statistics.median(v), 4)
        out["ms_" + k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
    return out


def measure_quantize(dbs, query, ma, rounds, reps):
    got = {k: db.quantize(query, ma).clone() for k, db in dbs.items()}
    assert torch.equal(got["device"], got["torch"]), f"the two quantizers differ at ma = {ma}"
    t = rounds_of({k: (lambda db=db: db.quantize(query, ma)) for k, db in dbs.items()}, rounds, reps)
    out = {"ma": ma, "assignments_equal": True, **figures(t)}
    out["torch_over_device"] = round(out["ms_torch"] / out["ms_device"], 2)
    tflops = 2.0 * N * KC * D / (out["ms_device"] * 1e-3) / 1e12
    out["device_tflops"] = round(tflops, 1)
    out["f32_peak_fraction"] = round(tflops / F32_PEAK_TFLOPS, 3)
    return out


def measure_update(n_images, dev, rounds, reps):
    centroids, images = scene(n_images, dev)
    dbs = {q: RetrievalDatabase(centroids, capacity=n_images, quantizer=q) for q in ("device", "torch")}
    for feat in images[:n_images]:
        for db in dbs.values():
            db.update(feat, True, K, MIN_THRESH)
    query = images[n_images]
    sel, scores = {}, {}
    for q, db in dbs.items():
        sel[q] = db.update(query, False, K, MIN_THRESH)
        scores[q] = db.handle.ws_section("scores")[:n_images].clone()
    assert sel["device"] == sel["torch"] and torch.equal(scores["device"], scores["torch"]), "the two updates differ"
    t = rounds_of({q: (lambda db=db: db.update(query, False, K, MIN_THRESH)) for q, db in dbs.items()}, rounds, reps)
    out = {"stored_images": n_images, "selection": sel["device"], "outputs_equal": True, **figures(t)}
    out["torch_over_device"] = round(out["ms_torch"] / out["ms_device"], 2)
    return out, dbs, query


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=(64, 512))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.rounds < 7:
        sys.exit("quantize_time: at least 7 rounds")
    if not torch.cuda.is_available():
        sys.exit("quantize_time: no GPU; this tool only measures on the device")
    dev = torch.device("cuda:0")
    updates, quantizes = [], []
    for n_images in a.sizes:
        res, dbs, query = measure_update(n_images, dev, a.rounds, a.reps)
        updates.append(res)
        if not quantizes:  # the quantize does not depend on the store
            quantizes = [measure_quantize(dbs, query, ma, a.rounds, a.reps) for ma in (5, 1)]
        del dbs
    res = {"workload": "n=%d features, D=%d, Kc=%d; update(add_after_query=False, k=%d), query MA 5" % (N, D, KC, K),
           "clock": "wall clock per call, device idle before and after; median of the rounds",
           "rounds": a.rounds, "reps_per_round": a.reps, "f32_peak_tflops": F32_PEAK_TFLOPS,
           "quantize": quantizes, "update": updates,
           "device": torch.cuda.get_device_name(0), "lib": be.version()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

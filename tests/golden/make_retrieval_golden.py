"""Writes tests/golden/retrieval_d{64,40}.npz from the reference's own ASMK code.

    python tests/golden/make_retrieval_golden.py <reference checkout>

It needs the reference's source tree and runs only where that is present; the
tests read the fixtures it leaves. The modules asmk/kernel.py,
asmk/inverted_file.py, asmk/functional.py and asmk/io_helpers.py of
<reference>/thirdparty/mast3r/asmk are loaded from their files under a stub
`asmk` package (asmk/__init__ pulls in faiss, which the path under test does
not use), and asmk.hamming is built from the reference's cython/hamming.c into
a temporary directory. If that does not build, the three hamming functions are
taken from tests/asmk_ref.py instead and the fixture's `hamming_impl` says so.

The sequence is RetrievalDatabase.update(add_after_query=True) for 10 images:
query with multiple assignment 5 (ASMKKernel.aggregate_image, IVF.search with
ASMKKernel.similarity / functional.asmk_kernel, alpha 3, threshold 0), then add
with the first column (ASMKKernel.aggregate, IVF.add). The word assignments are
the fp64 nearest centroids of tests/asmk_ref.quantize; inputs come from
tests/asmk_ref.make_scene.
"""
import importlib.machinery
import importlib.util
import os
import subprocess
import sys
import sysconfig
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import asmk_ref  # noqa: E402

KC, N, N_IMAGES, K, MIN_THRESH = 97, 37, 10, 3, 5e-3
QUERY_MA, BUILD_MA, ALPHA, SIM_THRESH = 5, 1, 3.0, 0.0


def load_reference(ref_root):
    """-> (kernel module, inverted_file module, hamming_impl)."""
    asmk_dir = os.path.join(ref_root, "thirdparty", "mast3r", "asmk")
    pkg = types.ModuleType("asmk")
    pkg.__path__ = []
    sys.modules["asmk"] = pkg

    def from_file(name, path):
        spec = importlib.util.spec_from_file_location("asmk." + name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["asmk." + name] = mod
        spec.loader.exec_module(mod)
        setattr(pkg, name, mod)
        return mod

    impl = "reference cython/hamming.c"
    try:
        tmp = tempfile.mkdtemp(prefix="asmk_hamming_")
        so = os.path.join(tmp, "hamming" + importlib.machinery.EXTENSION_SUFFIXES[0])
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-w", "-I", sysconfig.get_paths()["include"],
                               "-I", np.get_include(), os.path.join(asmk_dir, "cython", "hamming.c"), "-o", so])
        from_file("hamming", so)
    except Exception as exc:  # noqa: BLE001
        print("hamming.c did not build or load:", exc)
        impl = "tests/asmk_ref.py restatement"
        ham = types.ModuleType("asmk.hamming")
        ham.binarize_and_pack_2D = asmk_ref.binarize_and_pack_2D
        ham.hamming_cdist_packed = lambda a, b: np.stack([asmk_ref.hamming_cdist_packed(q, b) for q in a])
        sys.modules["asmk.hamming"] = ham
        pkg.hamming = ham
    for name in ("io_helpers", "functional", "kernel", "inverted_file"):
        from_file(name, os.path.join(asmk_dir, "asmk", name + ".py"))
    return sys.modules["asmk.kernel"], sys.modules["asmk.inverted_file"], impl


def make(D, seed, kernel_mod, ivf_mod, impl):
    centroids, images = asmk_ref.make_scene(KC, N, D, N_IMAGES, seed)
    codebook = types.SimpleNamespace(centroids=centroids)
    kern = kernel_mod.ASMKKernel(codebook, binary=True)
    ivf = ivf_mod.IVF.initialize_empty(codebook_size=KC, use_idf=False)
    similarity = lambda *x: kern.similarity(*x, alpha=ALPHA, similarity_threshold=SIM_THRESH)  # noqa: E731
    out = dict(centroids=centroids, des=np.stack(images), hamming_impl=np.array(impl),
               k=np.array(K), min_thresh=np.array(MIN_THRESH))
    assigns, sel, sel_len = [], np.full((N_IMAGES, K), -1, np.int64), np.zeros(N_IMAGES, np.int64)
    for i, des in enumerate(images):
        assign, _ = asmk_ref.quantize(des, centroids, QUERY_MA)
        assigns.append(assign)
        # the query aggregate (kept for every image; image 0 has nothing to search)
        q_codes, q_words = kern.aggregate_image(des, assign)
        out[f"q_codes_{i}"], out[f"q_words_{i}"] = q_codes, q_words
        if i > 0:
            ranks, ranked = ivf.search(q_codes, q_words, similarity_func=similarity, topk=None)
            scores = np.empty_like(ranked)
            scores[ranks] = ranked  # retrieval_database.py:59-60
            out[f"scores_{i}"] = scores
            order = np.argsort(-scores, kind="stable")[:min(K, i)]
            keep = [int(j) for j in order if scores[j] > MIN_THRESH]
            sel[i, :len(keep)], sel_len[i] = keep, len(keep)
        b_codes, b_words, b_imids = kern.aggregate(des, assign[:, :BUILD_MA], np.full(N, i, np.int64))
        out[f"b_codes_{i}"], out[f"b_words_{i}"] = b_codes, b_words
        ivf.add(b_codes, b_words, b_imids)
    out["assign"], out["sel"], out["sel_len"] = np.stack(assigns), sel, sel_len
    out["norm_factor"] = np.asarray(ivf.norm_factor)
    path = os.path.join(HERE, f"retrieval_d{D}.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", impl, "; selections", [list(s[:n]) for s, n in zip(sel, sel_len)])


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    mods = load_reference(sys.argv[1])
    make(64, 11, *mods)
    make(40, 12, *mods)

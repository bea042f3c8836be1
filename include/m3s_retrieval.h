/*
 * m3s_retrieval.h — C ABI of the MI355X ASMK retrieval kernels of MASt3R-SLAM.
 *
 * The part of RetrievalDatabase.update (retrieval_database.py:43-166) that the
 * reference runs on the host in numpy and Cython, after its torch quantize:
 *
 *   aggregate   ASMKKernel.aggregate_image (asmk/kernel.py:26-39) with the
 *               binary kernel: per visual word the fp32 sum of the residuals
 *               of its features, in ascending feature order, sign-binarised and
 *               packed as hamming.pyx:24-30,99-107 packs it
 *   search      IVF.search (asmk/inverted_file.py:86-108) with use_idf=False,
 *               ASMKKernel.similarity (kernel.py:56-68), functional.asmk_kernel
 *               and the top-k of retrieval_database.py:59-67
 *   append      IVF.add (inverted_file.py:56-84) with use_idf=False
 *
 * and that quantize itself (quantize_custom, retrieval_database.py:96-105), so
 * that a C caller can run a whole retrieval: norms once, then per frame
 * quantize -> aggregate -> search -> append.
 *
 * Plain C: device pointers, sizes, the caller's hipStream_t as `void *`, an int
 * status (M3S_OK / M3S_EINVAL / M3S_ELAUNCH of m3s_gn.h). No allocation and no
 * host synchronisation in any entry point; the caller reads the `out` section
 * of the workspace when it wants the result.
 *
 * The store is append-only and laid out image by image (not word by word):
 * searching is one coalesced pass over it, one workgroup per stored image, so
 * every image's score has a fixed summation order and needs no atomics.
 */
#ifndef M3S_RETRIEVAL_H
#define M3S_RETRIEVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M3S_ASMK_MAX_PAIRS 4096 /* n * multiple_assignment of one aggregate   */
#define M3S_ASMK_MAX_K 64       /* images one search can select               */

/* info bits: store header word 2 (sticky until reset), `out` header word 2 */
#define M3S_ASMK_INFO_BAD_WORD 1 /* an assignment outside [0, Kc) was skipped */
#define M3S_ASMK_INFO_FULL 2     /* an append was refused: capacity reached   */

/* Sections of the store, byte offsets from its base (m3s_asmk_store_layout). */
#define M3S_ASMK_STORE_HEADER 0  /* int32[16]: n_entries, n_images, info      */
#define M3S_ASMK_STORE_IMG_PTR 1 /* int32[cap_images + 1]: first entry of each */
#define M3S_ASMK_STORE_WORD 2    /* int32[cap_entries]: visual word of entry   */
#define M3S_ASMK_STORE_CODES 3   /* uint32[cap_entries, ceil(D/32)]            */
#define M3S_ASMK_STORE_TOTAL 4   /* = m3s_asmk_store_size                      */
#define M3S_ASMK_STORE_SECTIONS 5

/* Sections of the workspace (m3s_asmk_workspace_layout). Set 0 is the query
 * aggregate, set 1 the build aggregate; each has M3S_ASMK_MAX_PAIRS rows. */
#define M3S_ASMK_WS_COUNTS 0  /* int32[16]: U_query, U_build, bad_query, bad_build */
#define M3S_ASMK_WS_SLOT 1    /* int32[Kc]: word -> row of the query set, or -1    */
#define M3S_ASMK_WS_WORDS 2   /* int32[2, MAX_PAIRS]: sorted unique words          */
#define M3S_ASMK_WS_START 3   /* int32[2, MAX_PAIRS + 16]: member range of a word  */
#define M3S_ASMK_WS_MEMBERS 4 /* int32[2, MAX_PAIRS]: feature of each sorted pair  */
#define M3S_ASMK_WS_CODES 5   /* uint32[2, MAX_PAIRS, ceil(D/32)]                  */
#define M3S_ASMK_WS_SCORES 6  /* double[cap_images]: the scores of the last search */
#define M3S_ASMK_WS_OUT 7     /* m3s_asmk_out                                      */
#define M3S_ASMK_WS_TOTAL 8   /* = m3s_asmk_workspace_size                         */
#define M3S_ASMK_WS_SECTIONS 9

/* What one search leaves for the host: one small copy. */
typedef struct m3s_asmk_out {
  int32_t count;               /* selected images with score > min_thresh         */
  int32_t n_images;            /* images searched                                 */
  int32_t info;                /* store info | this query's M3S_ASMK_INFO_BAD_WORD */
  int32_t n_query_words;       /* unique words of the query (the query norm)      */
  int32_t idx[M3S_ASMK_MAX_K]; /* image ids by descending score, lower id first   */
  double score[M3S_ASMK_MAX_K];
} m3s_asmk_out;

/* One database: its two buffers and its geometry. */
typedef struct m3s_asmk_db {
  void *store;     /* >= m3s_asmk_store_size(cap_images, cap_entries, D) bytes */
  size_t store_bytes;
  void *workspace; /* >= m3s_asmk_workspace_size(Kc, D, cap_images) bytes      */
  size_t workspace_bytes;
  int64_t cap_images, cap_entries;
  int64_t Kc; /* codebook size, < 2^20 */
  int64_t D;  /* descriptor dimension  */
} m3s_asmk_db;

size_t m3s_asmk_store_size(int64_t cap_images, int64_t cap_entries, int64_t D);
size_t m3s_asmk_workspace_size(int64_t Kc, int64_t D, int64_t cap_images);
/* offs[M3S_ASMK_STORE_SECTIONS] / offs[M3S_ASMK_WS_SECTIONS]; return the total */
size_t m3s_asmk_store_layout(int64_t cap_images, int64_t cap_entries, int64_t D, size_t *offs);
size_t m3s_asmk_workspace_layout(int64_t Kc, int64_t D, int64_t cap_images, size_t *offs);

/* Empty the store and clear the workspace's word table. One launch. Must run
 * once before the first use of the two buffers. */
int m3s_asmk_reset(const m3s_asmk_db *db, void *stream);

/*
 * Aggregate one image's features into the workspace rows of the query set (the
 * first query_ma columns of `assign`) and of the build set (the first build_ma
 * columns); a set with 0 columns is not produced. Two launches: one workgroup
 * per set sorts its (word, feature) pairs in LDS and derives the unique words
 * and their member ranges; then one workgroup per (word, 256 components) sums
 * and packs. The query set also fills the word -> row table that the search
 * reads; m3s_asmk_search clears it again, so with query_ma > 0 a search must
 * follow before the next aggregate. n * query_ma and n * build_ma are at most
 * M3S_ASMK_MAX_PAIRS (else M3S_EINVAL). A word outside [0, Kc) sets
 * bad_query / bad_build and is skipped; it is never used as an index.
 */
typedef struct m3s_asmk_aggregate_args {
  m3s_asmk_db db;
  const float *des;       /* [n, D] local descriptors                       */
  const float *centroids; /* [Kc, D] codebook                               */
  const int64_t *assign;  /* [n, ma] nearest words, nearest first           */
  int64_t n, ma;
  int query_ma; /* <= ma; 0: no query set */
  int build_ma; /* <= ma; 0: no build set */
} m3s_asmk_aggregate_args;

int m3s_asmk_aggregate(const m3s_asmk_aggregate_args *a, void *stream);

/*
 * Score the query set against the first n_images stored images, select and
 * clear the word table. Two launches. Per stored entry whose word the query
 * has: h = popcount(xor) / (32 * ceil(D/32)), sim = 1 - 2h (fp32); when
 * sim >= similarity_threshold, fp32(sim^alpha) / sqrt(entries of the image),
 * rounded to fp32, is added to the image's fp64 score (entry order within a
 * lane, fixed tree across lanes). Scores are divided by sqrt(unique query
 * words) and left in the workspace; the min(k, n_images) highest with
 * score > min_thresh go to `out`.
 */
typedef struct m3s_asmk_search_args {
  m3s_asmk_db db;
  int64_t n_images; /* the caller's count of successful appends, >= 1 */
  int k;            /* 1 .. M3S_ASMK_MAX_K */
  float alpha;
  float similarity_threshold;
  double min_thresh;
} m3s_asmk_search_args;

int m3s_asmk_search(const m3s_asmk_search_args *a, void *stream);

/* Append the build set as the next image. One launch. When either capacity
 * would be exceeded nothing is written but M3S_ASMK_INFO_FULL. */
int m3s_asmk_append(const m3s_asmk_db *db, void *stream);

/*
 * The quantize (quantize_custom, retrieval_database.py:96-105): the `ma`
 * nearest centroids of every feature, nearest first, into the `assign` that
 * m3s_asmk_aggregate takes. Ranked by |c|^2 - 2 q.c in exact fp32 (the
 * f32-input MFMA; |q|^2 is the same for every centroid of a feature), in the
 * order (value ascending, word ascending): exactly equal values come out
 * lower word first, and a second run is bitwise identical. No [n, Kc] matrix
 * is ever stored: one launch keeps the smallest pairs of every (feature, tile
 * of 128 centroids) in registers and writes `ma` of them per tile to the
 * workspace, a second launch merges the tiles of each feature. The workspace
 * is scratch of its own (not the database's); nothing in it outlives a call.
 *
 * M3S_EINVAL, before any launch: a null pointer (`dist` may be null), n < 1,
 * n * ma > M3S_ASMK_MAX_PAIRS, ma < 1, ma > M3S_ASMK_QUANTIZE_MAX_MA, ma > Kc,
 * Kc >= 2^20, D < 1, a workspace smaller than its size function says or not
 * 8-byte aligned. Any other n, Kc and D work.
 */
#define M3S_ASMK_QUANTIZE_MAX_MA 8

typedef struct m3s_asmk_quantize_args {
  const float *des;       /* [n, D] local descriptors                          */
  const float *centroids; /* [Kc, D] codebook                                  */
  const float *norms;     /* [Kc] |c|^2 (m3s_asmk_centroid_norms)              */
  int64_t n, Kc, D;
  int ma;           /* 1 .. min(M3S_ASMK_QUANTIZE_MAX_MA, Kc)                  */
  int64_t *assign;  /* out [n, ma]: nearest words, nearest first               */
  float *dist;      /* out [n, ma] or null: the ranked values |c|^2 - 2 q.c    */
  void *workspace;  /* >= m3s_asmk_quantize_workspace_size(n, Kc, ma) bytes    */
  size_t workspace_bytes;
} m3s_asmk_quantize_args;

/* Bytes of scratch for the partial candidate lists of n <= n_max features. */
size_t m3s_asmk_quantize_workspace_size(int64_t n_max, int64_t Kc, int ma);

/* norms[c] = |centroids[c]|^2, summed in fp64 and rounded once to fp32. One
 * launch, once per database. M3S_EINVAL: a null pointer, Kc < 1, Kc >= 2^20,
 * D < 1. */
int m3s_asmk_centroid_norms(const float *centroids, int64_t Kc, int64_t D, float *norms, void *stream);

/* Two launches on `stream`. */
int m3s_asmk_quantize(const m3s_asmk_quantize_args *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* M3S_RETRIEVAL_H */

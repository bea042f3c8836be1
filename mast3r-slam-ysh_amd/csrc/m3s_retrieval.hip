// m3s_retrieval.hip — MI355X (gfx950) ASMK retrieval kernels
// (include/m3s_retrieval.h): what RetrievalDatabase.update runs on the host in
// the reference (numpy loops over visual words, a Cython Hamming kernel, per-word
// posting lists) as six launches on the caller's stream, and its torch quantize
// as two more (the quantize section below).
//
//   aggregate  sort_pairs_kernel   one workgroup per set: bitonic sort of the
//                                  (word, feature) keys in LDS, unique words,
//                                  member ranges, the word -> row table
//              pack_kernel         one workgroup per (word, 256 components):
//                                  sequential fp32 residual sum, ballot, pack
//   search     score_kernel        one workgroup per stored image
//              select_kernel       scale, top-k, threshold, clear the table
//   append     append_kernel       one workgroup: copy, then bump the counters
//   reset      reset_kernel
//   quantize   quantize_tile_kernel, quantize_merge_kernel (centroid_norms_kernel
//              once per database)
//
// Every sum has a fixed order: the residual sums add features in ascending
// order one after the other (numpy's .sum(0) over rows), the scores add in
// entry order within a lane and in a fixed tree across lanes. No atomics on
// floating-point data anywhere.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "m3s_gn.h"
#include "m3s_retrieval.h"

namespace {

constexpr int kSortThreads = 1024;
constexpr int kPackThreads = 256;
constexpr int kScoreThreads = 256;
constexpr int kSelectThreads = 256;
constexpr int kAppendThreads = 1024;
constexpr int kMaxPairs = M3S_ASMK_MAX_PAIRS;
constexpr int kStartStride = kMaxPairs + 16;
constexpr int kFeatBits = 12;  // a feature index < kMaxPairs
constexpr uint32_t kBadKey = 0xffffffffu;
constexpr int64_t kMaxWords = (1 << 20) - 1;
static_assert((1 << kFeatBits) == kMaxPairs, "key packing");

inline int launch_status() { return hipGetLastError() == hipSuccess ? M3S_OK : M3S_ELAUNCH; }

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

inline int64_t words32(int64_t D) { return (D + 31) / 32; }

size_t store_layout(int64_t cap_images, int64_t cap_entries, int64_t D, size_t *o) {
  const size_t ci = cap_images > 0 ? (size_t)cap_images : 0, ce = cap_entries > 0 ? (size_t)cap_entries : 0;
  const size_t d32 = D > 0 ? (size_t)words32(D) : 0;
  size_t t[M3S_ASMK_STORE_SECTIONS];
  t[M3S_ASMK_STORE_HEADER] = 0;
  t[M3S_ASMK_STORE_IMG_PTR] = 64;
  t[M3S_ASMK_STORE_WORD] = align_up(t[M3S_ASMK_STORE_IMG_PTR] + 4 * (ci + 1));
  t[M3S_ASMK_STORE_CODES] = align_up(t[M3S_ASMK_STORE_WORD] + 4 * ce);
  t[M3S_ASMK_STORE_TOTAL] = align_up(t[M3S_ASMK_STORE_CODES] + 4 * ce * d32);
  if (o)
    for (int k = 0; k < M3S_ASMK_STORE_SECTIONS; k++) o[k] = t[k];
  return t[M3S_ASMK_STORE_TOTAL];
}

size_t workspace_layout(int64_t Kc, int64_t D, int64_t cap_images, size_t *o) {
  const size_t kc = Kc > 0 ? (size_t)Kc : 0, ci = cap_images > 0 ? (size_t)cap_images : 0;
  const size_t d32 = D > 0 ? (size_t)words32(D) : 0;
  size_t t[M3S_ASMK_WS_SECTIONS];
  t[M3S_ASMK_WS_COUNTS] = 0;
  t[M3S_ASMK_WS_SLOT] = 64;
  t[M3S_ASMK_WS_WORDS] = align_up(t[M3S_ASMK_WS_SLOT] + 4 * kc);
  t[M3S_ASMK_WS_START] = align_up(t[M3S_ASMK_WS_WORDS] + 4 * 2 * (size_t)kMaxPairs);
  t[M3S_ASMK_WS_MEMBERS] = align_up(t[M3S_ASMK_WS_START] + 4 * 2 * (size_t)kStartStride);
  t[M3S_ASMK_WS_CODES] = align_up(t[M3S_ASMK_WS_MEMBERS] + 4 * 2 * (size_t)kMaxPairs);
  t[M3S_ASMK_WS_SCORES] = align_up(t[M3S_ASMK_WS_CODES] + 4 * 2 * (size_t)kMaxPairs * d32);
  t[M3S_ASMK_WS_OUT] = align_up(t[M3S_ASMK_WS_SCORES] + 8 * ci);
  t[M3S_ASMK_WS_TOTAL] = align_up(t[M3S_ASMK_WS_OUT] + sizeof(m3s_asmk_out));
  if (o)
    for (int k = 0; k < M3S_ASMK_WS_SECTIONS; k++) o[k] = t[k];
  return t[M3S_ASMK_WS_TOTAL];
}

// The device view of one database: section pointers and geometry.
struct Db {
  int32_t *hdr;      // store: n_entries, n_images, info
  int32_t *img_ptr;  // store [cap_images + 1]
  int32_t *sword;    // store [cap_entries]
  uint32_t *scodes;  // store [cap_entries, D32]
  int32_t *counts;   // workspace: U_query, U_build, bad_query, bad_build
  int32_t *slot;     // [Kc]
  int32_t *words;    // [2, kMaxPairs]
  int32_t *start;    // [2, kStartStride]
  int32_t *members;  // [2, kMaxPairs]
  uint32_t *codes;   // [2, kMaxPairs, D32]
  double *scores;    // [cap_images]
  m3s_asmk_out *out;
  int32_t cap_images, cap_entries, Kc, D, D32;
};

bool make_db(const m3s_asmk_db *d, Db *v) {
  if (!d || !d->store || !d->workspace) return false;
  if (d->cap_images < 1 || d->cap_entries < 1 || d->Kc < 1 || d->Kc > kMaxWords || d->D < 1) return false;
  if (d->cap_images > (1 << 24) || d->cap_entries > (1ll << 30) || d->D > (1 << 20)) return false;
  size_t so[M3S_ASMK_STORE_SECTIONS], wo[M3S_ASMK_WS_SECTIONS];
  if (store_layout(d->cap_images, d->cap_entries, d->D, so) > d->store_bytes) return false;
  if (workspace_layout(d->Kc, d->D, d->cap_images, wo) > d->workspace_bytes) return false;
  char *s = static_cast<char *>(d->store), *w = static_cast<char *>(d->workspace);
  v->hdr = reinterpret_cast<int32_t *>(s + so[M3S_ASMK_STORE_HEADER]);
  v->img_ptr = reinterpret_cast<int32_t *>(s + so[M3S_ASMK_STORE_IMG_PTR]);
  v->sword = reinterpret_cast<int32_t *>(s + so[M3S_ASMK_STORE_WORD]);
  v->scodes = reinterpret_cast<uint32_t *>(s + so[M3S_ASMK_STORE_CODES]);
  v->counts = reinterpret_cast<int32_t *>(w + wo[M3S_ASMK_WS_COUNTS]);
  v->slot = reinterpret_cast<int32_t *>(w + wo[M3S_ASMK_WS_SLOT]);
  v->words = reinterpret_cast<int32_t *>(w + wo[M3S_ASMK_WS_WORDS]);
  v->start = reinterpret_cast<int32_t *>(w + wo[M3S_ASMK_WS_START]);
  v->members = reinterpret_cast<int32_t *>(w + wo[M3S_ASMK_WS_MEMBERS]);
  v->codes = reinterpret_cast<uint32_t *>(w + wo[M3S_ASMK_WS_CODES]);
  v->scores = reinterpret_cast<double *>(w + wo[M3S_ASMK_WS_SCORES]);
  v->out = reinterpret_cast<m3s_asmk_out *>(w + wo[M3S_ASMK_WS_OUT]);
  v->cap_images = (int32_t)d->cap_images, v->cap_entries = (int32_t)d->cap_entries;
  v->Kc = (int32_t)d->Kc, v->D = (int32_t)d->D, v->D32 = (int32_t)words32(d->D);
  return true;
}

__global__ void __launch_bounds__(256) reset_kernel(Db db) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  for (int w = g; w < db.Kc; w += gridDim.x * 256) db.slot[w] = -1;
  if (g < 16) db.hdr[g] = 0, db.counts[g] = 0;
  if (g == 0) db.img_ptr[0] = 0;
}

struct AggArgs {
  const float *des;
  const float *centroids;
  const int64_t *assign;
  int32_t n, ma, query_ma, build_ma;
};

// One workgroup per set. The (word, feature) pairs of the set's columns become
// keys word << 12 | feature; their ascending order is the order of
// np.unique(word_ids) with each word's features ascending.
__global__ void __launch_bounds__(kSortThreads) sort_pairs_kernel(Db db, AggArgs A) {
  __shared__ uint32_t keys[kMaxPairs];
  __shared__ int32_t sums[kSortThreads];
  __shared__ int32_t n_valid, bad;
  const int set = blockIdx.x, tid = threadIdx.x;
  const int ma = set == 0 ? A.query_ma : A.build_ma;
  const int npairs = A.n * ma;  // <= kMaxPairs (host check)
  if (ma == 0) {
    if (tid == 0) db.counts[set] = 0, db.counts[2 + set] = 0;
    return;
  }
  int P = 2;
  while (P < npairs) P <<= 1;
  if (tid == 0) n_valid = 0, bad = 0;
  __syncthreads();
  for (int p = tid; p < P; p += kSortThreads) {
    uint32_t key = kBadKey;
    if (p < npairs) {
      const int f = p / ma, c = p - f * ma;
      const int64_t w = A.assign[(int64_t)f * A.ma + c];
      if (w >= 0 && w < db.Kc)
        key = ((uint32_t)w << kFeatBits) | (uint32_t)f;
      else
        bad = 1;  // every writer stores the same value
    }
    keys[p] = key;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += kSortThreads) {
        const int x = i ^ j;
        if (x > i) {
          const uint32_t a = keys[i], b = keys[x];
          const bool up = (i & k) == 0;
          if ((a > b) == up) keys[i] = b, keys[x] = a;
        }
      }
      __syncthreads();
    }
  }
  // heads of the runs of equal words: four consecutive positions per thread
  constexpr int kPer = kMaxPairs / kSortThreads;
  const int p0 = tid * kPer;
  int heads = 0, valid = 0;
#pragma unroll
  for (int q = 0; q < kPer; q++) {
    const int p = p0 + q;
    if (p < P && keys[p] != kBadKey) {
      valid++;
      if (p == 0 || (keys[p] >> kFeatBits) != (keys[p - 1] >> kFeatBits)) heads++;
    }
  }
  if (valid) atomicAdd(&n_valid, valid);
  sums[tid] = heads;
  __syncthreads();
  for (int off = 1; off < kSortThreads; off <<= 1) {  // inclusive scan
    const int v = tid >= off ? sums[tid - off] : 0;
    __syncthreads();
    sums[tid] += v;
    __syncthreads();
  }
  int u = sums[tid] - heads;  // unique words before this thread's positions
  int32_t *words = db.words + set * kMaxPairs, *start = db.start + set * kStartStride;
  int32_t *members = db.members + set * kMaxPairs;
#pragma unroll
  for (int q = 0; q < kPer; q++) {
    const int p = p0 + q;
    if (p < P && keys[p] != kBadKey) {
      const uint32_t key = keys[p];
      const int w = (int)(key >> kFeatBits);
      if (p == 0 || (key >> kFeatBits) != (keys[p - 1] >> kFeatBits)) {
        words[u] = w, start[u] = p;
        if (set == 0) db.slot[w] = u;
        u++;
      }
      // a word twice in one feature's row counts once ((word_ids == word).any(axis=1))
      members[p] = (p > 0 && keys[p - 1] == key) ? -1 : (int)(key & (kMaxPairs - 1));
    }
  }
  if (tid == kSortThreads - 1) {
    start[sums[tid]] = n_valid;
    db.counts[set] = sums[tid];
    db.counts[2 + set] = bad;
  }
}

#pragma clang fp contract(off)

// One workgroup per (row of a set, 256 components). Row x < n * query_ma is
// row x of the query set, the rest are rows of the build set; rows past the
// set's unique-word count leave at once.
__global__ void __launch_bounds__(kPackThreads) pack_kernel(Db db, AggArgs A) {
  const int rows_q = A.n * A.query_ma;
  const int set = (int)blockIdx.x < rows_q ? 0 : 1;
  const int u = set == 0 ? blockIdx.x : blockIdx.x - rows_q;
  if (u >= db.counts[set]) return;
  const int32_t *start = db.start + set * kStartStride, *members = db.members + set * kMaxPairs;
  const int w = db.words[set * kMaxPairs + u];
  const int s = start[u], e = start[u + 1];
  const int d = blockIdx.y * kPackThreads + threadIdx.x;
  const bool live = d < db.D;
  const float c = live ? A.centroids[(int64_t)w * db.D + d] : 0.f;
  float acc = 0.f;
  for (int p = s; p < e; p++) {
    const int f = members[p];
    if (f < 0) continue;
    if (live) acc = acc + (A.des[(int64_t)f * db.D + d] - c);
  }
  // hamming.pyx: the first component is the most significant bit; a short last
  // word is shifted left, which is the same as zero bits for the missing ones
  const unsigned long long m = __ballot(live && acc > 0.f);
  const int lane = threadIdx.x & 63;
  if ((lane & 31) == 0 && d < db.D32 * 32) {
    const uint32_t half = lane == 0 ? (uint32_t)m : (uint32_t)(m >> 32);
    db.codes[((int64_t)set * kMaxPairs + u) * db.D32 + (d >> 5)] = __brev(half);
  }
}

struct SearchArgs {
  int32_t n_images, k;
  float alpha, similarity_threshold;
  double min_thresh;
};

// One workgroup per stored image; thread t takes entries t, t + 256, ...
__global__ void __launch_bounds__(kScoreThreads) score_kernel(Db db, SearchArgs A) {
  __shared__ double part[kScoreThreads / 64];
  const int img = blockIdx.x, tid = threadIdx.x;
  const int n_stored = min(db.hdr[1], db.cap_images);
  double acc = 0.0;
  if (img < n_stored) {
    const int e0 = max(db.img_ptr[img], 0), e1 = min(db.img_ptr[img + 1], db.cap_entries);
    const double norm = sqrt((double)(e1 - e0));
    const float bits = (float)(32 * db.D32);
    const int ia = (int)A.alpha;
    const bool int_alpha = (float)ia == A.alpha && ia >= 1 && ia <= 8;
    for (int e = e0 + tid; e < e1; e += kScoreThreads) {
      const int w = db.sword[e];
      if (w < 0 || w >= db.Kc) continue;
      const int q = db.slot[w];
      if (q < 0 || q >= kMaxPairs) continue;
      const uint32_t *a = db.scodes + (int64_t)e * db.D32, *b = db.codes + (int64_t)q * db.D32;
      int pop = 0;
      if ((db.D32 & 3) == 0) {
        const uint4 *a4 = reinterpret_cast<const uint4 *>(a), *b4 = reinterpret_cast<const uint4 *>(b);
        for (int c = 0; c < db.D32 / 4; c++) {
          const uint4 x = a4[c], y = b4[c];
          pop += __popc(x.x ^ y.x) + __popc(x.y ^ y.y) + __popc(x.z ^ y.z) + __popc(x.w ^ y.w);
        }
      } else {
        for (int c = 0; c < db.D32; c++) pop += __popc(a[c] ^ b[c]);
      }
      const float h = (float)pop / bits;
      const float sim = -2.f * h + 1.f;
      if (!(sim >= A.similarity_threshold)) continue;
      float s;
      if (int_alpha) {
        s = sim;
        for (int r = 1; r < ia; r++) s = s * sim;
      } else {
        s = powf(sim, A.alpha);
      }
      acc += (double)(float)((double)s / norm);
    }
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) db.scores[img] = ((part[0] + part[1]) + (part[2] + part[3]));
}

// Scale by the query norm, select, threshold, and clear the word table.
__global__ void __launch_bounds__(kSelectThreads) select_kernel(Db db, SearchArgs A) {
  __shared__ double best_s[kSelectThreads];
  __shared__ int32_t best_i[kSelectThreads];
  const int tid = threadIdx.x;
  const int U = min(max(db.counts[0], 0), kMaxPairs);
  const int n = min(A.n_images, min(db.hdr[1], db.cap_images));
  // q_norm_factor accumulates float32 ones; np.sqrt of it is a float32
  const double qn = (double)sqrtf((float)U);
  for (int i = tid; i < A.n_images; i += kSelectThreads) db.scores[i] = (i < n && U > 0) ? db.scores[i] / qn : 0.0;
  for (int u = tid; u < U; u += kSelectThreads) {
    const int w = db.words[u];
    if (w >= 0 && w < db.Kc) db.slot[w] = -1;
  }
  __syncthreads();
  const int k = min(A.k, n);
  double last_s = 0.0;
  int last_i = -1, count = 0;
  for (int r = 0; r < k; r++) {
    // the next image in (score descending, id ascending) order after the last one
    double bs = 0.0;
    int bi = -1;
    for (int i = tid; i < n; i += kSelectThreads) {
      const double s = db.scores[i];
      const bool after = last_i < 0 || s < last_s || (s == last_s && i > last_i);
      if (after && (bi < 0 || s > bs)) bs = s, bi = i;  // i ascends: ties keep the lower id
    }
    best_s[tid] = bs, best_i[tid] = bi;
    __syncthreads();
    for (int off = kSelectThreads / 2; off > 0; off >>= 1) {
      if (tid < off) {
        const double s2 = best_s[tid + off];
        const int i2 = best_i[tid + off];
        const int i1 = best_i[tid];
        if (i2 >= 0 && (i1 < 0 || s2 > best_s[tid] || (s2 == best_s[tid] && i2 < i1))) best_s[tid] = s2, best_i[tid] = i2;
      }
      __syncthreads();
    }
    last_s = best_s[0], last_i = best_i[0];
    __syncthreads();
    if (last_i < 0) break;  // NaN scores only: nothing orders after them
    if (tid == 0) db.out->idx[r] = last_i, db.out->score[r] = last_s;
    if (last_s > A.min_thresh) count = r + 1;
  }
  if (tid == 0) {
    db.out->count = count;
    db.out->n_images = n;
    db.out->info = db.hdr[2] | (db.counts[2] ? M3S_ASMK_INFO_BAD_WORD : 0);
    db.out->n_query_words = U;
  }
}

#pragma clang fp contract(on)

// One workgroup: every thread reads the counters, the copy follows, and one
// thread bumps them behind a barrier.
__global__ void __launch_bounds__(kAppendThreads) append_kernel(Db db) {
  const int tid = threadIdx.x;
  const int n_entries = db.hdr[0], n_images = db.hdr[1];
  const int U = db.counts[1];
  const bool ok = U >= 0 && U <= kMaxPairs && n_entries >= 0 && n_images >= 0 && n_images < db.cap_images &&
                  n_entries <= db.cap_entries - U;
  __syncthreads();
  if (!ok) {
    if (tid == 0) db.hdr[2] |= M3S_ASMK_INFO_FULL;
    return;
  }
  const int32_t *words = db.words + kMaxPairs;
  const uint32_t *codes = db.codes + (int64_t)kMaxPairs * db.D32;
  for (int u = tid; u < U; u += kAppendThreads) db.sword[n_entries + u] = words[u];
  const int64_t nw = (int64_t)U * db.D32;
  uint32_t *dst = db.scodes + (int64_t)n_entries * db.D32;
  for (int64_t i = tid; i < nw; i += kAppendThreads) dst[i] = codes[i];
  __syncthreads();
  if (tid == 0) {
    db.hdr[0] = n_entries + U;
    db.hdr[1] = n_images + 1;
    db.img_ptr[n_images + 1] = n_entries + U;
    if (db.counts[3]) db.hdr[2] |= M3S_ASMK_INFO_BAD_WORD;
  }
}

// ------------------------------------------------------------- quantize --
// The nearest `ma` centroids of every feature by |c|^2 - 2 q.c (|q|^2 is the
// same for every centroid of a feature), without a distance matrix.
//
//   quantize_tile_kernel   one workgroup per (128 centroids, 128 features):
//                          the f32 MFMA product over D through LDS, then per
//                          feature the ma smallest (value, word) pairs
//                          of the tile -> workspace [n, tiles, ma]
//   quantize_merge_kernel  one wave per feature: the smallest `ma` pairs over
//                          its tiles -> assign (and dist)
//
// The order is (value ascending, word ascending) everywhere, a strict total
// order on the pairs of one feature, so no merge order can change the result.

constexpr int kQTile = 128;       // centroids and features per workgroup
constexpr int kQK = 32;           // k per LDS tile
constexpr int kQChain = 128;      // components per fmaf chain
constexpr int kQStride = kQK + 4; // row stride in floats: ds_read_b128 of 16 rows hits 16 distinct 16-B slots
constexpr int kQThreads = 256;
constexpr int kQMaxMa = M3S_ASMK_QUANTIZE_MAX_MA;

typedef float f32x16 __attribute__((ext_vector_type(16)));

inline int64_t quantize_tiles(int64_t Kc) { return (Kc + kQTile - 1) / kQTile; }

size_t quantize_workspace(int64_t n_max, int64_t Kc, int ma) {
  if (n_max < 1 || Kc < 1 || ma < 1) return 0;
  return align_up((size_t)n_max * (size_t)quantize_tiles(Kc) * (size_t)ma * sizeof(uint64_t));
}

// A (value, word) pair as one 64-bit key whose unsigned order is (value
// ascending, word ascending): the value's bits made monotone (sign flipped for
// v >= 0, all bits for v < 0; -0 is +0 first, so that equal values have equal
// bits) above the word.
__device__ inline uint64_t pair_key(float v, uint32_t w) {
  const uint32_t b = __float_as_uint(v + 0.f);
  return ((uint64_t)(b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u)) << 32) | w;
}
__device__ inline float key_value(uint64_t k) {
  const uint32_t u = (uint32_t)(k >> 32);
  return __uint_as_float(u ^ ((u & 0x80000000u) ? 0x80000000u : 0xffffffffu));
}
constexpr uint64_t kNoPair = ~0ull;  // an empty slot: after every pair of a word < 2^20

// The M smallest keys seen, ascending, in registers (every loop is unrolled).
template <int M>
struct TopList {
  uint64_t key[M];
  __device__ inline void clear() {
#pragma unroll
    for (int j = 0; j < M; j++) key[j] = kNoPair;
  }
  __device__ inline void insert(uint64_t k) {  // one bubble pass: the largest of the M + 1 falls out
#pragma unroll
    for (int j = 0; j < M; j++) {
      const bool lt = k < key[j];
      const uint64_t lo = lt ? k : key[j];
      k = lt ? key[j] : k;
      key[j] = lo;
    }
  }
  // the list of the lane `mask` away joins this one (both lanes end up equal)
  __device__ inline void merge_xor(int mask) {
    uint64_t other[M];
#pragma unroll
    for (int j = 0; j < M; j++) other[j] = __shfl_xor((unsigned long long)key[j], mask, 64);
#pragma unroll
    for (int j = 0; j < M; j++) insert(other[j]);
  }
};

struct QuantArgs {
  const float *des;
  const float *centroids;
  const float *norms;
  int64_t *assign;
  float *dist;
  uint64_t *cand;  // [n, tiles, ma]: pair keys
  int64_t D;
  int32_t n, Kc, tiles, vec;
};

// One wave per centroid: lane l adds the squares of components l, l + 64, ...
// in fp64, a fixed tree joins the lanes, one rounding to fp32.
__global__ void __launch_bounds__(256) centroid_norms_kernel(const float *centroids, int32_t Kc, int64_t D, float *norms) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= Kc) return;
  const float *row = centroids + (int64_t)c * D;
  double acc = 0.0;
  for (int64_t k = lane; k < D; k += 64) acc += (double)row[k] * (double)row[k];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) norms[c] = (float)acc;
}

// Rows row0 + r (r = tid / 8 + 32 i) of a [rows, D] matrix, components
// k0 + 4 (tid % 8) .. + 3, zero outside the matrix.
__device__ inline void quantize_fetch(const float *base, int64_t rows, int64_t D, int64_t row0, int64_t k0, bool vec,
                                      int tid, float4 (&reg)[4]) {
  const int64_t k = k0 + 4 * (tid & 7);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int64_t r = row0 + (tid >> 3) + 32 * i;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows) {
      const float *p = base + r * D + k;
      if (vec) {
        if (k < D) x = *reinterpret_cast<const float4 *>(p);  // D % 4 == 0: all four or none
      } else {
        if (k < D) x.x = p[0];
        if (k + 1 < D) x.y = p[1];
        if (k + 2 < D) x.z = p[2];
        if (k + 3 < D) x.w = p[3];
      }
    }
    reg[i] = x;
  }
}

__device__ inline void quantize_stage(float *tile, int tid, const float4 (&reg)[4]) {
#pragma unroll
  for (int i = 0; i < 4; i++)
    *reinterpret_cast<float4 *>(tile + ((tid >> 3) + 32 * i) * kQStride + 4 * (tid & 7)) = reg[i];
}

// Wave w of four takes centroids 64 (w / 2) .. + 63 and features 64 (w % 2)
// .. + 63 of the workgroup's tile as 2 x 2 MFMA tiles: centroids on the row
// index (A), features on the column index (B, the lane), so the 16
// accumulators of a lane are 16 centroids of one feature. Lane half h takes
// components 16 h .. 16 h + 15 of a 32-component LDS tile in its 16 k-steps
// (A and B alike, so every product pairs the same component).
template <int MA>
__global__ void __launch_bounds__(kQThreads, 2) quantize_tile_kernel(QuantArgs A) {
  __shared__ __attribute__((aligned(16))) float As[kQTile * kQStride];
  __shared__ __attribute__((aligned(16))) float Bs[kQTile * kQStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
  const int64_t c0 = (int64_t)blockIdx.x * kQTile, f0 = (int64_t)blockIdx.y * kQTile;
  const bool vec = A.vec != 0;

  // acc: the fmaf chain of the current kQChain components; dot: the sum of
  // the finished chains. One chain over all of D loses too much when every
  // product has the same sign (a feature next to its own centroid): at
  // D = 1024 its error reaches 1e-6 of |c|^2 + 2 sum |q_k c_k|, eight chains
  // of 128 stay below 2e-7.
  f32x16 acc[2][2], dot[2][2];
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int nn = 0; nn < 2; nn++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[m][nn][r] = 0.f, dot[m][nn][r] = 0.f;

  float4 ra[4], rb[4];
  quantize_fetch(A.centroids, A.Kc, A.D, c0, 0, vec, tid, ra);
  quantize_fetch(A.des, A.n, A.D, f0, 0, vec, tid, rb);
  for (int64_t k0 = 0; k0 < A.D; k0 += kQK) {
    quantize_stage(As, tid, ra);
    quantize_stage(Bs, tid, rb);
    __syncthreads();
    if (k0 + kQK < A.D) {  // the next tile's loads fly under this tile's products
      quantize_fetch(A.centroids, A.Kc, A.D, c0, k0 + kQK, vec, tid, ra);
      quantize_fetch(A.des, A.n, A.D, f0, k0 + kQK, vec, tid, rb);
    }
    const float *ap = As + (wm * 64 + li) * kQStride + 16 * lh;
    const float *bp = Bs + (wn * 64 + li) * kQStride + 16 * lh;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const float4 a0 = *reinterpret_cast<const float4 *>(ap + 4 * q);
      const float4 a1 = *reinterpret_cast<const float4 *>(ap + 32 * kQStride + 4 * q);
      const float4 b0 = *reinterpret_cast<const float4 *>(bp + 4 * q);
      const float4 b1 = *reinterpret_cast<const float4 *>(bp + 32 * kQStride + 4 * q);
      const float av[2][4] = {{a0.x, a0.y, a0.z, a0.w}, {a1.x, a1.y, a1.z, a1.w}};
      const float bv[2][4] = {{b0.x, b0.y, b0.z, b0.w}, {b1.x, b1.y, b1.z, b1.w}};
#pragma unroll
      for (int s = 0; s < 4; s++)
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
          for (int nn = 0; nn < 2; nn++)
            acc[m][nn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][s], bv[nn][s], acc[m][nn], 0, 0, 0);
    }
    if ((k0 + kQK) % kQChain == 0 || k0 + kQK >= A.D) {
#pragma unroll
      for (int m = 0; m < 2; m++)
#pragma unroll
        for (int nn = 0; nn < 2; nn++)
#pragma unroll
          for (int r = 0; r < 16; r++) dot[m][nn][r] += acc[m][nn][r], acc[m][nn][r] = 0.f;
    }
    __syncthreads();
  }

  // this lane's 32 centroids of each of its two features, then the other lane
  // half's (the centroids 4 rows on)
  TopList<MA> top[2];
#pragma unroll
  for (int nn = 0; nn < 2; nn++) {
    top[nn].clear();
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int64_t c = c0 + wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        // a row past Kc never takes a slot
        top[nn].insert(c < A.Kc ? pair_key(fmaf(-2.f, dot[m][nn][r], A.norms[c]), (uint32_t)c) : kNoPair);
      }
    top[nn].merge_xor(32);
  }
  // the upper centroid half's lists go through LDS (the k loop's last barrier
  // has passed: the tiles are free) to the lower half's waves
  uint64_t *xch = reinterpret_cast<uint64_t *>(As);  // [MA][2][2 feature halves * 32 lanes]
  if (wm == 1 && lh == 0) {
#pragma unroll
    for (int nn = 0; nn < 2; nn++)
#pragma unroll
      for (int j = 0; j < MA; j++) xch[(j * 2 + nn) * 64 + wn * 32 + li] = top[nn].key[j];
  }
  __syncthreads();
  if (wm == 0 && lh == 0) {
#pragma unroll
    for (int nn = 0; nn < 2; nn++) {
#pragma unroll
      for (int j = 0; j < MA; j++) top[nn].insert(xch[(j * 2 + nn) * 64 + wn * 32 + li]);
      const int64_t f = f0 + wn * 64 + nn * 32 + li;
      if (f < A.n) {  // feature tail: computed and dropped
        uint64_t *out = A.cand + (f * A.tiles + blockIdx.x) * MA;
#pragma unroll
        for (int j = 0; j < MA; j++) out[j] = top[nn].key[j];
      }
    }
  }
}

// One wave per feature: lane l takes candidates l, l + 64, ... of the
// feature's tiles * ma, a butterfly joins the lanes, lane j writes rank j.
template <int MA>
__global__ void __launch_bounds__(256) quantize_merge_kernel(QuantArgs A) {
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (f >= A.n) return;
  const int64_t count = (int64_t)A.tiles * MA;
  const uint64_t *cand = A.cand + (int64_t)f * count;
  TopList<MA> top;
  top.clear();
  for (int64_t e = lane; e < count; e += 64) top.insert(cand[e]);
  for (int off = 32; off > 0; off >>= 1) top.merge_xor(off);
#pragma unroll
  for (int j = 0; j < MA; j++)
    if (lane == j) {
      // ma <= Kc: an empty slot can only come out of non-finite input; it is
      // -1, which m3s_asmk_aggregate skips as a bad word
      const uint32_t w = (uint32_t)top.key[j];
      A.assign[(int64_t)f * MA + j] = w < (uint32_t)A.Kc ? (int64_t)w : -1;
      if (A.dist) A.dist[(int64_t)f * MA + j] = w < (uint32_t)A.Kc ? key_value(top.key[j]) : INFINITY;
    }
}

template <int MA>
int launch_quantize(const QuantArgs &A, hipStream_t st) {
  const dim3 grid((unsigned)A.tiles, (unsigned)((A.n + kQTile - 1) / kQTile));
  quantize_tile_kernel<MA><<<grid, kQThreads, 0, st>>>(A);
  if (launch_status() != M3S_OK) return M3S_ELAUNCH;
  quantize_merge_kernel<MA><<<(unsigned)((A.n + 3) / 4), 256, 0, st>>>(A);
  return launch_status();
}

}  // namespace

extern "C" {

size_t m3s_asmk_store_size(int64_t cap_images, int64_t cap_entries, int64_t D) {
  return store_layout(cap_images, cap_entries, D, nullptr);
}

size_t m3s_asmk_workspace_size(int64_t Kc, int64_t D, int64_t cap_images) {
  return workspace_layout(Kc, D, cap_images, nullptr);
}

size_t m3s_asmk_store_layout(int64_t cap_images, int64_t cap_entries, int64_t D, size_t *offs) {
  return store_layout(cap_images, cap_entries, D, offs);
}

size_t m3s_asmk_workspace_layout(int64_t Kc, int64_t D, int64_t cap_images, size_t *offs) {
  return workspace_layout(Kc, D, cap_images, offs);
}

int m3s_asmk_reset(const m3s_asmk_db *d, void *stream) {
  Db db;
  if (!make_db(d, &db)) return M3S_EINVAL;
  const unsigned blocks = (unsigned)((db.Kc + 255) / 256);
  reset_kernel<<<blocks < 1024 ? blocks : 1024, 256, 0, static_cast<hipStream_t>(stream)>>>(db);
  return launch_status();
}

int m3s_asmk_aggregate(const m3s_asmk_aggregate_args *a, void *stream) {
  Db db;
  if (!a || !make_db(&a->db, &db)) return M3S_EINVAL;
  if (!a->des || !a->centroids || !a->assign) return M3S_EINVAL;
  if (a->n < 1 || a->ma < 1 || a->query_ma < 0 || a->build_ma < 0) return M3S_EINVAL;
  if (a->query_ma > a->ma || a->build_ma > a->ma || a->query_ma + a->build_ma == 0) return M3S_EINVAL;
  if (a->n > kMaxPairs || a->n * a->query_ma > kMaxPairs || a->n * a->build_ma > kMaxPairs) return M3S_EINVAL;
  AggArgs A;
  A.des = a->des, A.centroids = a->centroids, A.assign = a->assign;
  A.n = (int32_t)a->n, A.ma = (int32_t)a->ma, A.query_ma = a->query_ma, A.build_ma = a->build_ma;
  hipStream_t st = static_cast<hipStream_t>(stream);
  sort_pairs_kernel<<<2, kSortThreads, 0, st>>>(db, A);
  if (launch_status() != M3S_OK) return M3S_ELAUNCH;
  const dim3 grid((unsigned)(A.n * (A.query_ma + A.build_ma)), (unsigned)((db.D + kPackThreads - 1) / kPackThreads));
  pack_kernel<<<grid, kPackThreads, 0, st>>>(db, A);
  return launch_status();
}

int m3s_asmk_search(const m3s_asmk_search_args *a, void *stream) {
  Db db;
  if (!a || !make_db(&a->db, &db)) return M3S_EINVAL;
  if (a->n_images < 1 || a->n_images > a->db.cap_images || a->k < 1 || a->k > M3S_ASMK_MAX_K) return M3S_EINVAL;
  if (!(a->alpha == a->alpha) || !(a->similarity_threshold == a->similarity_threshold)) return M3S_EINVAL;
  SearchArgs A;
  A.n_images = (int32_t)a->n_images, A.k = a->k;
  A.alpha = a->alpha, A.similarity_threshold = a->similarity_threshold, A.min_thresh = a->min_thresh;
  hipStream_t st = static_cast<hipStream_t>(stream);
  score_kernel<<<(unsigned)A.n_images, kScoreThreads, 0, st>>>(db, A);
  if (launch_status() != M3S_OK) return M3S_ELAUNCH;
  select_kernel<<<1, kSelectThreads, 0, st>>>(db, A);
  return launch_status();
}

int m3s_asmk_append(const m3s_asmk_db *d, void *stream) {
  Db db;
  if (!make_db(d, &db)) return M3S_EINVAL;
  append_kernel<<<1, kAppendThreads, 0, static_cast<hipStream_t>(stream)>>>(db);
  return launch_status();
}

size_t m3s_asmk_quantize_workspace_size(int64_t n_max, int64_t Kc, int ma) { return quantize_workspace(n_max, Kc, ma); }

int m3s_asmk_centroid_norms(const float *centroids, int64_t Kc, int64_t D, float *norms, void *stream) {
  if (!centroids || !norms || Kc < 1 || Kc > kMaxWords || D < 1) return M3S_EINVAL;
  centroid_norms_kernel<<<(unsigned)((Kc + 3) / 4), 256, 0, static_cast<hipStream_t>(stream)>>>(centroids, (int32_t)Kc, D,
                                                                                                 norms);
  return launch_status();
}

int m3s_asmk_quantize(const m3s_asmk_quantize_args *a, void *stream) {
  if (!a || !a->des || !a->centroids || !a->norms || !a->assign || !a->workspace) return M3S_EINVAL;
  if (a->n < 1 || a->ma < 1 || a->ma > kQMaxMa || a->ma > a->Kc || a->n * a->ma > kMaxPairs) return M3S_EINVAL;
  if (a->Kc > kMaxWords || a->D < 1) return M3S_EINVAL;
  if (a->workspace_bytes < quantize_workspace(a->n, a->Kc, a->ma) || ((uintptr_t)a->workspace & 7)) return M3S_EINVAL;
  QuantArgs A;
  A.des = a->des, A.centroids = a->centroids, A.norms = a->norms, A.assign = a->assign, A.dist = a->dist;
  A.cand = static_cast<uint64_t *>(a->workspace);
  A.D = a->D, A.n = (int32_t)a->n, A.Kc = (int32_t)a->Kc, A.tiles = (int32_t)quantize_tiles(a->Kc);
  A.vec = (a->D % 4 == 0 && (((uintptr_t)a->des | (uintptr_t)a->centroids) & 15) == 0) ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (a->ma) {  // the list length is a compile-time constant: the lists live in registers
    case 1: return launch_quantize<1>(A, st);
    case 2: return launch_quantize<2>(A, st);
    case 3: return launch_quantize<3>(A, st);
    case 4: return launch_quantize<4>(A, st);
    case 5: return launch_quantize<5>(A, st);
    case 6: return launch_quantize<6>(A, st);
    case 7: return launch_quantize<7>(A, st);
    default: return launch_quantize<8>(A, st);
  }
}

}  // extern "C"

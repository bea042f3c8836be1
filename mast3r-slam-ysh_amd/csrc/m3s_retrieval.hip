// m3s_retrieval.hip — MI355X (gfx950) ASMK retrieval kernels
// (include/m3s_retrieval.h): what RetrievalDatabase.update runs on the host in
// the reference (numpy loops over visual words, a Cython Hamming kernel, per-word
// posting lists) as six launches on the caller's stream.
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

}  // extern "C"

// gn/prologue.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The per-call setup on the device: ProArgs, the block scan / min-max /
// lower-bound helpers, gn_prologue_kernel (ranks the edge ids, writes the
// linearize edge order, flags, info, dx) and its launch sizes (prologue_lds,
// prologue_p2; host).
// Relies on nothing but kFlagStop (gn/layout.h).

// ------------------------------------------------------ call prologue --
// The per-call setup of a GN call on the device, so the call's first
// linearize can be enqueued right behind it and nothing waits for the host:
// the edge ids are ranked (the reference's torch::_unique(cat(ii, jj), sorted,
// return_inverse), gn_kernels.cu:1154-1160) by a bitonic sort of the 2E ids in
// LDS, the ranks and the linearize edge order (edges grouped by KF j,
// block_task; the order inside a KF bucket is free: partials are indexed by
// task, so the sums do not depend on it) go to the workspace, flags / edge
// counters / info /
// dx_out are initialised, and ii, jj, K are copied into pinned host memory
// for the host's symbolic analysis, which then runs while the first linearize
// kernel does (host_finish).
constexpr int kProThreads = 1024;
constexpr int kProMaxE = 2048;  // 2E ids sorted in LDS; larger edge sets take the host path
static_assert(kProMaxE % kProThreads == 0, "prologue: whole edges per thread");
struct ProArgs {
  const int64_t *ii, *jj;
  const float *K;      // calib: 3x3 (else null)
  int64_t *down_ii, *down_jj;
  float *down_K;       // host-mapped pinned copies
  int E, N, P2;        // P2: power of two >= 2E
  int32_t *flags, *rank_i, *rank_j, *eorder, *info;
  uint32_t *edge_cnt;
  float *dx_out;
  int n_dx;
};

// exclusive prefix of one int per thread over the block; *total = block sum
__device__ int block_excl_scan(int v, int *wsum, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int w = 0; w < nw; w++) {
      const int t = wsum[w];
      wsum[w] = acc;
      acc += t;
    }
    wsum[16] = acc;
  }
  __syncthreads();
  const int r = wsum[wave] + x - v;
  *total = wsum[16];
  __syncthreads();
  return r;
}

// minimum and maximum of one int64 pair per thread over the block (every
// thread gets both)
__device__ void block_minmax_i64(int64_t &lo, int64_t &hi, int64_t *red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int64_t a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
    lo = a < lo ? a : lo, hi = b > hi ? b : hi;
  }
  if (lane == 0) red[wave] = lo, red[16 + wave] = hi;
  __syncthreads();
  lo = red[0], hi = red[16];
  for (int w = 1; w < nw; w++) lo = red[w] < lo ? red[w] : lo, hi = red[16 + w] > hi ? red[16 + w] : hi;
  __syncthreads();
}

__device__ __forceinline__ int lower_bound_i64(const int64_t *u, int n, int64_t v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (u[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kProThreads) gn_prologue_kernel(ProArgs A) {
  extern __shared__ __attribute__((aligned(16))) int64_t pro_smem[];
  __shared__ int wsum[17];
  __shared__ int64_t red64[32];
  const int E = A.E, P2 = A.P2, tid = threadIdx.x;
  constexpr int64_t kPad = 0x7fffffffffffffffLL;
  int64_t *keys = pro_smem, *uniq = keys + P2;
  int32_t *cnt = reinterpret_cast<int32_t *>(uniq + P2);  // [P2]: KF bucket counts, then offsets
  int32_t *erj = cnt + P2;  // [E]
  // this thread's edges e = tid, tid + 1024 (E <= kProMaxE): their ids stay in registers
  constexpr int kPer = kProMaxE / kProThreads;
  int64_t ei[kPer], ej[kPer];
#pragma unroll
  for (int u = 0; u < kPer; u++) {
    const int e = tid + u * kProThreads;
    ei[u] = e < E ? A.ii[e] : 0, ej[u] = e < E ? A.jj[e] : 0;
  }
  int64_t lo = kPad, hi = -kPad - 1;  // id range (keyframe ids: small non-negative integers in practice)
#pragma unroll
  for (int u = 0; u < kPer; u++) {
    const int e = tid + u * kProThreads;
    if (e < E) {
      A.down_ii[e] = ei[u], A.down_jj[e] = ej[u];
      keys[e] = ei[u], keys[E + e] = ej[u];
      lo = ei[u] < lo ? ei[u] : lo, hi = ei[u] > hi ? ei[u] : hi;
      lo = ej[u] < lo ? ej[u] : lo, hi = ej[u] > hi ? ej[u] : hi;
    }
  }
  for (int q = 2 * E + tid; q < P2; q += kProThreads) keys[q] = kPad;
  if (A.K && tid < 9) A.down_K[tid] = A.K[tid];
  for (int q = tid; q <= E; q += kProThreads) A.edge_cnt[q] = 0u;
  for (int q = tid; q < A.n_dx; q += kProThreads) A.dx_out[q] = 0.0f;
  if (tid < 64) A.flags[tid] = 0;
  block_minmax_i64(lo, hi, red64);  // threads without edges hold (max, min): neutral
  // bitmap of 64 P2 bits in the uniq region (P2 int64), its word prefix in the keys region
  int nu = 0;
  if (E > 0 && (uint64_t)hi - (uint64_t)lo < (uint64_t)64 * P2) {
    // rank = number of distinct ids below: a presence bitmap over [lo, hi] and
    // a prefix of its word popcounts (4 barriers instead of the sort's
    // log2(P2)(log2(P2)+1)/2)
    uint32_t *bm = reinterpret_cast<uint32_t *>(uniq);
    int32_t *pre = reinterpret_cast<int32_t *>(keys);
    const int nwu = (int)(((uint64_t)hi - (uint64_t)lo) >> 5) + 1;
    for (int q = tid; q < nwu; q += kProThreads) bm[q] = 0u;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPer; u++) {
      if (tid + u * kProThreads < E) {
        const uint64_t di = (uint64_t)ei[u] - (uint64_t)lo, dj = (uint64_t)ej[u] - (uint64_t)lo;
        atomicOr(&bm[di >> 5], 1u << (di & 31));
        atomicOr(&bm[dj >> 5], 1u << (dj & 31));
      }
    }
    __syncthreads();
    const int segw = (nwu + kProThreads - 1) / kProThreads;
    int pc = 0;
    for (int q = 0; q < segw; q++) {
      const int w = tid * segw + q;
      pc += w < nwu ? __builtin_popcount(bm[w]) : 0;
    }
    int off0 = block_excl_scan(pc, wsum, &nu);
    for (int q = 0; q < segw; q++) {
      const int w = tid * segw + q;
      if (w < nwu) pre[w] = off0, off0 += __builtin_popcount(bm[w]);
    }
    __syncthreads();
    auto rank = [&](int64_t v) {
      const uint64_t d = (uint64_t)v - (uint64_t)lo;
      return pre[d >> 5] + __builtin_popcount(bm[d >> 5] & ((1u << (d & 31)) - 1u));
    };
#pragma unroll
    for (int u = 0; u < kPer; u++) {
      const int e = tid + u * kProThreads;
      if (e < E) {
        const int ri = rank(ei[u]), rj = rank(ej[u]);
        A.rank_i[e] = ri, A.rank_j[e] = rj;
        erj[e] = rj;
      }
    }
  } else {
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1)  // bitonic sort, ascending
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < P2; i += kProThreads) {
          const int l = i ^ j;
          if (l > i) {
            const int64_t x = keys[i], y = keys[l];
            if ((x > y) == ((i & k) == 0)) keys[i] = y, keys[l] = x;
          }
        }
        __syncthreads();
      }
    // the sorted unique ids, in order (each thread a run of <= 4 sorted keys)
    const int seg = (P2 + kProThreads - 1) / kProThreads;
    auto first = [&](int i) { return i < P2 && keys[i] != kPad && (i == 0 || keys[i] != keys[i - 1]); };
    int nf = 0;
    for (int q = 0; q < seg; q++) nf += first(tid * seg + q) ? 1 : 0;
    int at_ = block_excl_scan(nf, wsum, &nu);
    for (int q = 0; q < seg; q++)
      if (first(tid * seg + q)) uniq[at_++] = keys[tid * seg + q];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPer; u++) {
      const int e = tid + u * kProThreads;
      if (e < E) {
        const int ri = lower_bound_i64(uniq, nu, ei[u]), rj = lower_bound_i64(uniq, nu, ej[u]);
        A.rank_i[e] = ri, A.rank_j[e] = rj;
        erj[e] = rj;
      }
    }
  }
  const bool bad = nu > A.N;
  if (tid < 8) A.info[tid] = tid == M3S_INFO_N_UNIQUE ? nu : (tid == M3S_INFO_BAD_EDGE && bad) ? 1 : 0;
  if (tid == 0 && bad) A.flags[kFlagStop] = 1;  // every launch of the call is a no-op
  if (bad || E == 0) return;                     // (uniform)
  for (int q = tid; q < nu; q += kProThreads) cnt[q] = 0;
  __syncthreads();
  for (int e = tid; e < E; e += kProThreads) atomicAdd(&cnt[erj[e]], 1);
  __syncthreads();
  const int segn = (nu + kProThreads - 1) / kProThreads;  // <= 4
  int cl[4] = {0, 0, 0, 0}, sum = 0;
  for (int q = 0; q < segn; q++) {
    const int i = tid * segn + q;
    cl[q] = i < nu ? cnt[i] : 0;
    sum += cl[q];
  }
  int tot = 0;
  int off = block_excl_scan(sum, wsum, &tot);
  for (int q = 0; q < segn; q++) {
    const int i = tid * segn + q;
    if (i < nu) cnt[i] = off, off += cl[q];
  }
  __syncthreads();
  for (int e = tid; e < E; e += kProThreads) A.eorder[atomicAdd(&cnt[erj[e]], 1)] = e;
}
inline size_t prologue_lds(int E, int P2) {
  return sizeof(int64_t) * 2 * (size_t)P2 + sizeof(int32_t) * ((size_t)P2 + (size_t)E);
}
inline int prologue_p2(int64_t E) {
  int p = 2;
  while (p < 2 * E) p <<= 1;
  return p;
}

// gn/linearize.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// LinArgs, the per-pixel gather (gather_pixel), block_task, the wave and
// block reductions (block_reduce_store, xreduce36 and its DPP forms,
// sum_xor16_32, wave_sum_pl, xred_index, xreduceN_dpp, store_partial),
// finalize_edge, the last-chunk tails (edge_tail, track_tail),
// linearize_kernel<MODE, TRACK, VEC, WPACK>, the LDS-DMA helpers (buf_lds16*,
// kFarOff, lds_xj6, M3S_XRD) and linearize_packed_kernel<MODE>.
// Relies on gn/layout.h (kThreads, kPixPerThread, kBlockPix, TrackState, the
// track_solve_block declaration), the vector typedefs of m3s_gn.hip and the
// residuals of m3s_device.h.

// ------------------------------------------------------------- linearize --
struct LinArgs {
  const float *Twc;        // backend: poses (rank order)
  const float *T_rel;      // tracker: T_CkCf (single pose), else null
  const float *Xs;
  const float *Cs;
  const float *Xsrc;       // tracker: Xf (source points); backend: unused
  const int64_t *idx;
  int idx32;  // idx holds int32 (m3s_gn_args.idx_i32)
  const uint8_t *valid;
  const float *Q;
  const int32_t *rank_i;
  const int32_t *rank_j;
  const int32_t *stop;
  const int32_t *eorder;   // the launch's edges sorted by KF j (block_task); null: block = task
  int64_t per, E_loc;      // block_task: 8 runs of `per` blocks; edges of the launch
  uint32_t cnt_base;       // edge_cnt arrivals before this launch in the call (edge_tail)
  float *planes;           // per-edge target-side planes (PixIn), [E_loc][kPlanes][HW]
  float *partials;         // [task][36]
  uint32_t *edge_cnt;      // non-null: the last chunk of an edge to finish also finalizes it into fin
  double *esum;            // non-null (stepwise API): that chunk writes the edge's fp64 sums here instead
  double *fin;             // [E][kFin] per-edge blocks M L M^T, M g (fused finalize)
  TrackState *track;       // tracker: the last chunk of an iteration runs the 7x7 solve (else null)
  int32_t *info;           // tracker outputs / convergence rule
  float *T_WCf_out, *T_CkCf_out;
  float rel_error, delta_norm;
  int64_t HW, edge_begin, chunks, chunk_pix;
  ResidualParams P;
  const float *Kd;  // calib backend: the caller's 3x3 K (device), read by the kernels (P.fx.. unset)
};

// The residual parameters of a launch: the intrinsics of a calib backend
// launch come from the caller's K on the device (uniform loads), so the first
// linearize of a call can be enqueued before the host has read anything back.
__device__ __forceinline__ ResidualParams kparams(const LinArgs &A) {
  ResidualParams P = A.P;
  if (A.Kd) P.fx = A.Kd[0], P.fy = A.Kd[4], P.cx = A.Kd[2], P.cy = A.Kd[5];
  return P;
}

// one pixel's gathered inputs -> target-side inputs (shared by all paths)
template <int MODE, bool TRACK>
__device__ __forceinline__ PixIn<MODE> gather_pixel(const LinArgs &A, const float *Xs_i, const float *Cs_i,
                                                    int64_t p, bool vm, int64_t id_raw, float q, float cj) {
  const int64_t id = TRACK ? p : (vm ? id_raw : 0);
  const float Xi[3] = {Xs_i[3 * id + 0], Xs_i[3 * id + 1], Xs_i[3 * id + 2]};
  bool ok;
  if (TRACK) {
    ok = vm;
  } else {
    const float ci = Cs_i[id];
    ok = vm && (q > A.P.Q_thresh) && (ci > A.P.C_thresh) && (cj > A.P.C_thresh);
  }
  int u_t = 0, v_t = 0;
  if (MODE == M3S_MODE_CALIB) {  // ind_Xi % width, ind_Xi / width (gn_kernels.cu:1360-1361)
    const int iid = (int)id;
    int vv = (int)((float)iid * (1.0f / (float)A.P.width));
    if (vv * A.P.width > iid) vv--;
    if ((vv + 1) * A.P.width <= iid) vv++;
    v_t = vv;
    u_t = iid - vv * A.P.width;
  }
  return make_pixin<MODE>(A.P, Xi, ok, q, u_t, v_t);
}

// block -> task (e_loc * chunks + c). The E_loc x chunks tasks sorted by
// (chunk, KF j) are cut into 8 contiguous runs and run x is dealt to blocks
// x, x + 8, x + 16, ...: the edges that stream the same Xj chunk run back to
// back on one XCD (blocks b and b + 8 share an XCD under round-robin
// placement; speed only: partials are indexed by task). -1: idle padding.
__device__ __forceinline__ int64_t block_task(const LinArgs &A) {
  if (!A.eorder) return (int64_t)blockIdx.x;
  const int64_t b = blockIdx.x, t = (b & 7) * A.per + (b >> 3);
  if (t >= A.E_loc * A.chunks) return -1;
  const int64_t c = t / A.E_loc;
  return (int64_t)A.eorder[t - c * A.E_loc] * A.chunks + c;
}

// The block partial is stored write-through (sc1), so the edge's last chunk
// can read it from another XCD without a release fence (guide §6 G16 R1).
__device__ __forceinline__ void store_sc1(float *p, float v) {
  __hip_atomic_store(reinterpret_cast<uint32_t *>(p), __float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// Block reduction of the 36 per-thread sums through LDS: every thread stores
// its row (16-B stores), then 252 threads each add a 1/7 slice of one column,
// then 36 threads combine the 7 slices. ~100 instructions per thread instead
// of 36 wave-wide shuffle trees.
constexpr int kRedW = kNP / 2;  // values per pass (36 or 18)
__device__ __forceinline__ void block_reduce_store(const float *acc, float *out) {
  __shared__ __attribute__((aligned(16))) float red[kThreads * kRedW];
  __shared__ float part[kRedW][8];
  const int t = threadIdx.x;
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    if (pass) __syncthreads();
    float2 *row = reinterpret_cast<float2 *>(red + (size_t)t * kRedW);
#pragma unroll
    for (int k = 0; k < kRedW / 2; k++)
      row[k] = make_float2(acc[pass * kRedW + 2 * k], acc[pass * kRedW + 2 * k + 1]);
    __syncthreads();
    constexpr int S = (kThreads + kRedW * 7 - 1) / (kRedW * 7) * 7 > 0 ? 7 : 7;
    constexpr int per = (kThreads + S - 1) / S;
    if (t < kRedW * S) {
      const int v = t / S, s = t % S;
      const int r0 = s * per, r1 = (r0 + per < kThreads) ? r0 + per : kThreads;
      float x = 0.0f;
      for (int r = r0; r < r1; r++) x += red[r * kRedW + v];
      part[v][s] = x;
    }
    __syncthreads();
    if (t < kRedW) {
      float x = 0.0f;
#pragma unroll
      for (int s = 0; s < S; s++) x += part[t][s];
      store_sc1(out + pass * kRedW + t, x);
    }
  }
}

template <typename T>
__device__ __forceinline__ T ld_stream(const T *p) {
  return __builtin_nontemporal_load(p);
}


// Per edge: H_jj = M L M^T and g_j = M l in fp64 (M = Adj(T_i)^-T), written
// as fin[0:49] (row-major) and fin[49:56], from the edge's 36 local sums `es`
// (LDS). Threads 0..63 of the block work; every thread of the block must call
// it (block barriers). Mc: M already in LDS (the fused finalize forms it on
// its second wave while the first loads the partials); else lanes 0..48 form
// it here, one entry each.
constexpr int kFin = 56;
__device__ __forceinline__ void finalize_edge(const double *es, const float *Ti, double *fin,
                                              const double (*Mc)[7] = nullptr) {
  __shared__ double Mo[7][7], Lm[7][7], T1[7][7], l[7];
  const double(*M)[7] = Mc ? Mc : Mo;
  const int t = threadIdx.x;
  if (!Mc && t < 49) Mo[t / 7][t % 7] = adjT_inv_entry(Ti, t / 7, t % 7);
  if (t < 49) {
    const int a = t / 7, c = t % 7;
    Lm[a][c] = es[kL + tri(a < c ? a : c, a < c ? c : a)];
  }
  if (t < 7) l[t] = es[kG + t];
  __syncthreads();
  if (t < 49) {
    const int a = t / 7, c = t % 7;
    double sm = 0.0;
    for (int k = 0; k < 7; k++) sm += M[a][k] * Lm[k][c];
    T1[a][c] = sm;
  } else if (t < 56) {
    const int a = t - 49;
    double sm = 0.0;
    for (int k = 0; k < 7; k++) sm += M[a][k] * l[k];
    fin[49 + a] = sm;
  }
  __syncthreads();
  if (t < 49) {
    const int a = t / 7, c = t % 7;
    double sm = 0.0;
    for (int k = 0; k < 7; k++) sm += T1[a][k] * M[c][k];
    fin[t] = sm;
  }
}

// Each lane owns 4 consecutive pixels (one 16-B vector per stream); a wave
// sweeps 256 pixels per trip, a block 1024.
// 36 per-thread sums -> one block partial
// Transposed wave reduction of N values: each butterfly step (xor 32, 16,
// ..., 1) a lane keeps one half of its values and sends the other half to its
// partner, so the count halves every step: 18 + 9 + 5 + 3 + 2 + 1 = 38
// shuffles for 36 values instead of 36 x 6. Lane l ends with the full sum of
// value index `idx` (valid when the path never took a padding slot).
template <int N, int M, typename T>
__device__ __forceinline__ void xreduce_step(const T (&v)[N], T (&o)[(N + 1) / 2], bool hi) {
  constexpr int H = (N + 1) / 2;
#pragma unroll
  for (int i = 0; i < H; i++) {
    const T lo_v = v[i];
    const T hi_v = (i + H < N) ? v[i + H] : T(0);
    const T keep = hi ? hi_v : lo_v, send = hi ? lo_v : hi_v;
    o[i] = keep + __shfl_xor(send, M, 64);
  }
}
template <typename T>
__device__ __forceinline__ T xreduce36(const T (&v)[kNP], int lane, int &idx, bool &valid) {
  T a[18], b[9], c[5], d[3], e[2], f[1];
  xreduce_step<36, 32>(v, a, lane & 32);
  xreduce_step<18, 16>(a, b, lane & 16);
  xreduce_step<9, 8>(b, c, lane & 8);
  xreduce_step<5, 4>(c, d, lane & 4);
  xreduce_step<3, 2>(d, e, lane & 2);
  xreduce_step<2, 1>(e, f, lane & 1);
  // the value index a lane ends with: array sizes 36, 18, 9, 5, 3, 2 (the
  // halves H are compile-time); r = real (non-padding) values on the path
  int base = 0, r = kNP, sz = kNP;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int h = (sz + 1) / 2;
    if (lane & m)
      base += h, r = r > h ? r - h : 0;
    else
      r = r < h ? r : h;
    sz = h;
  }
  idx = base;
  valid = r == 1;
  return f[0];
}

// The same transposed reduction on the VALU's cross-lane paths instead of
// ds_bpermute (an LDS round trip per shuffle, ~6 dependent ones per call on
// the tracker's per-iteration critical path): xor 32 and xor 16 by the gfx950
// v_permlane32_swap / v_permlane16_swap (one swap exchanges the halves of a
// value pair: each side then adds what it keeps to what it received), xor 8
// by DPP row_ror:8, then DPP row_half_mirror (lane i of a half-row pairs with
// 7 - i: the pairs still split on lane bit 2, so the keep rule and the final
// index are xreduce36's), quad_perm [2,3,0,1] and [1,0,3,2]. Every sum is
// keep + partner as before; only the xor-4 step's partner (and so the fp
// rounding of the result) differs from xreduce36's.
template <typename T>
__device__ __forceinline__ void xr_swap(bool s32, T &x, T &y) {  // {x, y} -> {x_lo|y_lo, x_hi|y_hi}
  if constexpr (sizeof(T) == 4) {
    const auto r = s32 ? __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false)
                       : __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    x = __uint_as_float(r[0]), y = __uint_as_float(r[1]);
  } else {
    const unsigned long long xb = (unsigned long long)__double_as_longlong(x), yb = (unsigned long long)__double_as_longlong(y);
    const unsigned xl = (unsigned)xb, xh = (unsigned)(xb >> 32), yl = (unsigned)yb, yh = (unsigned)(yb >> 32);
    const auto rl = s32 ? __builtin_amdgcn_permlane32_swap(xl, yl, false, false) : __builtin_amdgcn_permlane16_swap(xl, yl, false, false);
    const auto rh = s32 ? __builtin_amdgcn_permlane32_swap(xh, yh, false, false) : __builtin_amdgcn_permlane16_swap(xh, yh, false, false);
    x = __longlong_as_double((long long)(((unsigned long long)rh[0] << 32) | rl[0]));
    y = __longlong_as_double((long long)(((unsigned long long)rh[1] << 32) | rl[1]));
  }
}
template <int CTRL, typename T>
__device__ __forceinline__ T xr_dpp(T v) {  // the DPP partner's value
  if constexpr (sizeof(T) == 4) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
  } else {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
  }
}
// u + (u of lane ^ 16), then + (that of lane ^ 32): the two butterfly steps of
// `u += __shfl_xor(u, 16); u += __shfl_xor(u, 32)` by v_permlane16/32_swap of
// u with itself (each side gets its partner's value; the sums are the same
// additions, so bitwise the same result) instead of two ds_bpermute LDS round
// trips (the dense tail's back-substitution chain, round 5)
__device__ __forceinline__ double sum_xor16_32(double u) {
  double a = u, b = u;
  xr_swap(false, a, b);
  u = a + b;
  a = u, b = u;
  xr_swap(true, a, b);
  return a + b;
}
// whole-wave sum on every lane by the same exchanges (permlane swaps of the
// value with itself for xor 32 / 16, then DPP; the xor-4 partner is 7 - i
// within a half-row): the solve tails' ||dx|| sums (round 5)
__device__ __forceinline__ float wave_sum_pl(float u) {
  float a = u, b = u;
  xr_swap(true, a, b);
  u = a + b;
  a = u, b = u;
  xr_swap(false, a, b);
  u = a + b;
  u += xr_dpp<0x128>(u);
  u += xr_dpp<0x141>(u);
  u += xr_dpp<0x4E>(u);
  u += xr_dpp<0xB1>(u);
  return u;
}
template <int N, bool S32, typename T>
__device__ __forceinline__ void xr_swap_step(const T (&v)[N], T (&o)[(N + 1) / 2]) {
  constexpr int H = (N + 1) / 2;
#pragma unroll
  for (int i = 0; i < H; i++) {
    T x = v[i], y = (i + H < N) ? v[i + H] : T(0);
    xr_swap(S32, x, y);
    o[i] = x + y;
  }
}
template <int N, int CTRL, typename T>
__device__ __forceinline__ void xr_dpp_step(const T (&v)[N], T (&o)[(N + 1) / 2], bool hi) {
  constexpr int H = (N + 1) / 2;
#pragma unroll
  for (int i = 0; i < H; i++) {
    const T lo_v = v[i];
    const T hi_v = (i + H < N) ? v[i + H] : T(0);
    const T keep = hi ? hi_v : lo_v, send = hi ? lo_v : hi_v;
    o[i] = keep + xr_dpp<CTRL>(send);
  }
}
template <typename T>
__device__ __forceinline__ T xreduce36_dpp(const T (&v)[kNP], int lane, int &idx, bool &valid) {
  T a[18], b[9], c[5], d[3], e[2], f[1];
  xr_swap_step<36, true>(v, a);
  xr_swap_step<18, false>(a, b);
  xr_dpp_step<9, 0x128>(b, c, lane & 8);  // row_ror:8
  xr_dpp_step<5, 0x141>(c, d, lane & 4);  // row_half_mirror
  xr_dpp_step<3, 0x4E>(d, e, lane & 2);   // quad_perm [2,3,0,1]
  xr_dpp_step<2, 0xB1>(e, f, lane & 1);   // quad_perm [1,0,3,2]
  int base = 0, r = kNP, sz = kNP;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int h = (sz + 1) / 2;
    if (lane & m)
      base += h, r = r > h ? r - h : 0;
    else
      r = r < h ? r : h;
    sz = h;
  }
  idx = base;
  valid = r == 1;
  return f[0];
}
// The same transposed reduction for N <= 64 values (xreduce36_dpp's steps);
// xred_index gives the value index a lane ends with and whether it is real.
template <int N>
__device__ __forceinline__ void xred_index(int lane, int &idx, bool &valid) {
  int base = 0, r = N, sz = N;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int h = (sz + 1) / 2;
    if (lane & m)
      base += h, r = r > h ? r - h : 0;
    else
      r = r < h ? r : h;
    sz = h;
  }
  idx = base;
  valid = r == 1;
}
template <int N, typename T>
__device__ __forceinline__ T xreduceN_dpp(const T (&v)[N], int lane) {
  constexpr int S1 = (N + 1) / 2, S2 = (S1 + 1) / 2, S3 = (S2 + 1) / 2, S4 = (S3 + 1) / 2, S5 = (S4 + 1) / 2;
  T a[S1], b[S2], c[S3], d[S4], e[S5], f[(S5 + 1) / 2];
  xr_swap_step<N, true>(v, a);
  xr_swap_step<S1, false>(a, b);
  xr_dpp_step<S2, 0x128>(b, c, lane & 8);
  xr_dpp_step<S3, 0x141>(c, d, lane & 4);
  xr_dpp_step<S4, 0x4E>(d, e, lane & 2);
  xr_dpp_step<S5, 0xB1>(e, f, lane & 1);
  return f[0];
}
// the linearize kernels' block partials on xreduce36_dpp (1) or xreduce36 (0):
// within noise for the packed kernel (an A/B of the first-listed library reads
// ~2-3% slow in tools/ab_linearize.py either way, profiles/r05/ab_pkw_*.txt),
// so the round-4 rounding stays
template <typename T>
__device__ __forceinline__ T xreduce36_trk(const T (&v)[kNP], int lane, int &idx, bool &valid) {
  return xreduce36_dpp(v, lane, idx, valid);
}

__device__ __forceinline__ void store_partial(const float *acc, float *out) {
  __shared__ float red[kThreads / 64][kNP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float v[kNP];
#pragma unroll
  for (int k = 0; k < kNP; k++) v[k] = acc[k];
  int idx;
  bool valid;
  const float s = xreduce36(v, lane, idx, valid);
  if (valid) red[wave][idx] = s;
  __syncthreads();
  if (threadIdx.x < kNP) {
    float t = 0.0f;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) t += red[w][threadIdx.x];
    store_sc1(out + threadIdx.x, t);
  }
}

// Fused finalize (single-GPU solve): after its chunk partial is stored, a
// block draws a ticket from its edge's counter; the edge's last chunk
// (ticket = chunks - 1 mod chunks: the counter runs on over a call's GN
// iterations and is zeroed per call) sums the edge's chunk partials in fp64
// in chunk order with sc1 loads (the same sums as edge_reduce_kernel /
// finalize_edges_kernel) and writes fin[e] - the finalize launch disappears.
// Stepwise API (a sharded rank's range): the same chunk writes the 36 sums
// to esum[e_loc] - the edge_reduce launch disappears (bitwise the same sums).
__device__ __forceinline__ void edge_tail(const LinArgs &A, int64_t e_loc, int64_t e) {
  __shared__ double esl[kNP], Ms[7][7];
  __shared__ int last_s;
  const int t = threadIdx.x;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its sc1 stores
  __syncthreads();
  if (t == 0) {
    const uint32_t ch = (uint32_t)A.chunks;
    const uint32_t old = __hip_atomic_fetch_add(A.edge_cnt + e_loc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_s = ((old - A.cnt_base) % ch) == ch - 1;
  }
  __syncthreads();
  if (!last_s) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no loads above the ticket
  if (t < kNP) {
    const uint32_t *p = reinterpret_cast<const uint32_t *>(A.partials + (size_t)e_loc * A.chunks * kNP + t);
    double acc = 0.0;
    int64_t c = 0;
    for (; c + 8 <= A.chunks; c += 8) {
      uint32_t v[8];
#pragma unroll
      for (int k = 0; k < 8; k++)
        v[k] = __hip_atomic_load(p + (size_t)(c + k) * kNP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int k = 0; k < 8; k++) acc += (double)__uint_as_float(v[k]);
    }
    for (; c < A.chunks; c++)
      acc += (double)__uint_as_float(__hip_atomic_load(p + (size_t)c * kNP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (A.esum)
      A.esum[(size_t)e_loc * kNP + t] = acc;
    else
      esl[t] = acc;
  } else if (!A.esum && t >= 64 && t < 64 + 49) {  // the second wave forms M under the first's loads
    const int q = t - 64;
    Ms[q / 7][q % 7] = adjT_inv_entry(A.Twc + 8 * (size_t)A.rank_i[e], q / 7, q % 7);
  }
  if (A.esum) return;
  __syncthreads();
  finalize_edge(esl, A.Twc + 8 * (size_t)A.rank_i[e], A.fin + (size_t)e * kFin, Ms);
}

// Fused tracker solve: the iteration's last chunk to arrive (ticket =
// chunks - 1 mod chunks; the counter runs over the call's iterations and is
// zeroed by track_init_kernel) reduces the partials and updates the pose.
__device__ __forceinline__ void track_tail(const LinArgs &A) {
  __shared__ int last_t;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this block's sc1 partial is stored
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t ch = (uint32_t)A.chunks;
    const uint32_t old = __hip_atomic_fetch_add(&A.track->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_t = (old % ch) == ch - 1;
  }
  __syncthreads();
  if (!last_t) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // the other chunks' partials, not stale L1 lines
  track_solve_block(A);
}

// WPACK: also store the target-side planes for the packed kernel (first GN
// iteration of a solve call).
template <int MODE, bool TRACK, bool VEC, bool WPACK>
__global__ void __launch_bounds__(kThreads) linearize_kernel(LinArgs A) {
  if (*A.stop) return;
  const int64_t b = block_task(A);
  if (b < 0) return;
  const int64_t e_loc = b / A.chunks;
  const int64_t c = b - e_loc * A.chunks;
  const int64_t e = A.edge_begin + e_loc;
  const int64_t HW = A.HW;
  const ResidualParams P = kparams(A);

  Sim3f Tij;
  const float *Xs_i, *Xs_j, *Cs_i = nullptr, *Cs_j = nullptr;
  if (TRACK) {
    Tij = load_sim3(A.T_rel);
    Xs_i = A.Xs;    // Xk (target, pixel-aligned)
    Xs_j = A.Xsrc;  // Xf (source, already gathered by idx_f2k)
  } else {
    const int ri = A.rank_i[e], rj = A.rank_j[e];
    Tij = relative(load_sim3(A.Twc + 8 * ri), load_sim3(A.Twc + 8 * rj));
    Xs_i = A.Xs + (size_t)ri * HW * 3;
    Xs_j = A.Xs + (size_t)rj * HW * 3;
    Cs_i = A.Cs + (size_t)ri * HW;
    Cs_j = A.Cs + (size_t)rj * HW;
  }
  const Sim3Mat Tm = sim3_matrix(Tij);
  // edge data (idx/valid/Q) is addressed relative to the launch's edge slice
  const size_t eoff = TRACK ? 0 : (size_t)e_loc * HW;
  const int64_t *__restrict__ idx = TRACK ? nullptr : A.idx + eoff;
  const int32_t *__restrict__ idx32 = TRACK ? nullptr : reinterpret_cast<const int32_t *>(A.idx) + eoff;
  const uint8_t *__restrict__ valid = A.valid + eoff;
  const float *__restrict__ Qe = A.Q + eoff;
  constexpr int NPL = PixIn<MODE>::kPlanes;
  float *__restrict__ pl = WPACK ? A.planes + (size_t)e_loc * NPL * HW : nullptr;

  // scalar accumulators here: 4 pixels of raw inputs stay live in this kernel
  AccumFlat acc;
  acc.zero();

  const int64_t p_begin = c * A.chunk_pix;
  const int64_t p_end = (p_begin + A.chunk_pix < HW) ? p_begin + A.chunk_pix : HW;

  if (VEC) {
    for (int64_t p0 = p_begin + kPixPerThread * threadIdx.x; p0 < p_end; p0 += kBlockPix) {
      // edge data is read once per iteration: non-temporal, so the pointmaps
      // (re-read by every edge that touches a keyframe) keep the caches
      const uint32_t vb = ld_stream(reinterpret_cast<const uint32_t *>(valid + p0));
      const f32x4 q4 = ld_stream(reinterpret_cast<const f32x4 *>(Qe + p0));
      int64_t ids[4] = {0, 0, 0, 0};
      if (!TRACK) {
        if (A.idx32) {  // uniform branch: 16 B of int32 ids
          typedef int i32x4 __attribute__((ext_vector_type(4)));
          const i32x4 i4 = ld_stream(reinterpret_cast<const i32x4 *>(idx32 + p0));
          ids[0] = i4.x, ids[1] = i4.y, ids[2] = i4.z, ids[3] = i4.w;
        } else {
          const i64x2 i01 = ld_stream(reinterpret_cast<const i64x2 *>(idx + p0));
          const i64x2 i23 = ld_stream(reinterpret_cast<const i64x2 *>(idx + p0 + 2));
          ids[0] = i01.x, ids[1] = i01.y, ids[2] = i23.x, ids[3] = i23.y;
        }
      }
      const f32x4 *xj4 = reinterpret_cast<const f32x4 *>(Xs_j + 3 * p0);
      const f32x4 xa = xj4[0], xb = xj4[1], xc = xj4[2];
      f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
      if (!TRACK) c4 = *reinterpret_cast<const f32x4 *>(Cs_j + p0);
      const float Xj[4][3] = {{xa.x, xa.y, xa.z}, {xa.w, xb.x, xb.y}, {xb.z, xb.w, xc.x}, {xc.y, xc.z, xc.w}};
      const float qs[4] = {q4.x, q4.y, q4.z, q4.w};
      const float cjs[4] = {c4.x, c4.y, c4.z, c4.w};
      PixIn<MODE> in[4];
#pragma unroll
      for (int s = 0; s < 4; s++)
        in[s] = gather_pixel<MODE, TRACK>(A, Xs_i, Cs_i, p0 + s, ((vb >> (8 * s)) & 0xffu) != 0, ids[s],
                                          qs[s], cjs[s]);
      {
#pragma unroll
        for (int s = 0; s < 4; s++) {
          float Y[3];
          act(Tm, Xj[s], Y);
          pixel_contrib<MODE>(acc, P, in[s], Y);
        }
      }
      if (WPACK) {
#pragma unroll
        for (int k = 0; k < NPL; k++) {
          const f32x4 v = {in[0].v[k], in[1].v[k], in[2].v[k], in[3].v[k]};
          // streamed past L2, where the pointmaps that other edges re-read live
          // (first call 258 -> 251 us at C3, 1172 -> 1134 us at 128 KFs rays)
          __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(pl + (size_t)k * HW + p0));
        }
      }
    }
  } else {
    for (int64_t p = p_begin + threadIdx.x; p < p_end; p += kThreads) {
      const bool vm = valid[p] != 0;
      const int64_t id = TRACK ? p : (A.idx32 ? (int64_t)idx32[p] : idx[p]);
      const float Xj[3] = {Xs_j[3 * p], Xs_j[3 * p + 1], Xs_j[3 * p + 2]};
      const float cj = TRACK ? 0.0f : Cs_j[p];
      const PixIn<MODE> in = gather_pixel<MODE, TRACK>(A, Xs_i, Cs_i, p, vm, id, Qe[p], cj);
      {
        float Y[3];
        act(Tm, Xj, Y);
        pixel_contrib<MODE>(acc, P, in, Y);
      }
      if (WPACK) {
#pragma unroll
        for (int k = 0; k < NPL; k++) pl[(size_t)k * HW + p] = in.v[k];
      }
    }
  }
  float sums[kNP];
#pragma unroll
  for (int k = 0; k < kNP; k++) sums[k] = 0.0f;
  acc.fold(sums);
  store_partial(sums, A.partials + (size_t)b * kNP);
  if (A.edge_cnt) edge_tail(A, e_loc, e);
  if (TRACK && A.track) track_tail(A);
}

// Later GN iterations of a solve call: target-side inputs from the planes the
// first iteration stored, Xj streamed (shared through L2 by the edges of one
// keyframe, which the task table places on one XCD back to back). No gathers.
// calib / points fit 128 VGPRs (4 waves per SIMD); rays keeps 84 accumulator
// VGPRs and is left unbounded (164, 3 waves)
// 16 B per lane from a buffer resource straight into LDS (lane-linear at
// m0 = lds): wave-uniform soffset, per-lane voffset (nt: streamed once)
__device__ __forceinline__ void buf_lds16_nt(__amdgpu_buffer_rsrc_t R, __attribute__((address_space(3))) void *lds,
                                             int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(R, lds, 16, voff, soff, 0, 2);
}
__device__ __forceinline__ void buf_lds16(__amdgpu_buffer_rsrc_t R, __attribute__((address_space(3))) void *lds,
                                          int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(R, lds, 16, voff, soff, 0, 0);
}
__device__ __forceinline__ void buf_lds16_sc0(__amdgpu_buffer_rsrc_t R, __attribute__((address_space(3))) void *lds,
                                              int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(R, lds, 16, voff, soff, 0, 1);
}
// A buffer offset past every resource's range (num_records < 2^31): the load
// returns zeros and makes no memory access.
constexpr int kFarOff = 0x7fff0000;
// Xj floats 6h .. 6h + 5 of a lane's 12 (its 4 pixels x y z, interleaved over
// three 16-B LDS rows 1 KB apart, from xs), one ds_read_b32 each straight
// into the half of the pair that uses it: plain loads merge into 16-B reads
// whose halves then need 5 v_mov per pair to regroup by pixel. LDS reads
// complete in order, so the compiler's own counted waits stay correct; ours
// is explicit.
__device__ __forceinline__ void lds_xj6(const float *xs, int h, float (&xf)[6]) {
  const uint32_t xa = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) const float *)xs);
#define M3S_XRD(q_, f_) \
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(xf[q_]) : "v"(xa), "i"(4 * (256 * ((f_) >> 2) + ((f_) & 3))))
  if (h == 0) {
    M3S_XRD(0, 0); M3S_XRD(1, 1); M3S_XRD(2, 2); M3S_XRD(3, 3); M3S_XRD(4, 4); M3S_XRD(5, 5);
  } else {
    M3S_XRD(0, 6); M3S_XRD(1, 7); M3S_XRD(2, 8); M3S_XRD(3, 9); M3S_XRD(4, 10); M3S_XRD(5, 11);
  }
#undef M3S_XRD
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xf[0]), "+v"(xf[1]), "+v"(xf[2]), "+v"(xf[3]), "+v"(xf[4]), "+v"(xf[5]));
}
#ifndef M3S_PK_WAVES  // packed linearize: minimum waves per SIMD (register bound 512 / w)
#define M3S_PK_WAVES 3
#endif
#ifndef M3S_PK_WAVES_RAYS
#define M3S_PK_WAVES_RAYS 2
#endif
template <int MODE>
__global__ void __launch_bounds__(kThreads, MODE == 1 ? M3S_PK_WAVES_RAYS : M3S_PK_WAVES)
    linearize_packed_kernel(LinArgs A) {
  if (*A.stop) return;
  const int64_t b = block_task(A);
  if (b < 0) return;
  const int64_t e_loc = b / A.chunks;
  const int64_t c = b - e_loc * A.chunks;
  const int64_t e = A.edge_begin + e_loc;
  const int64_t HW = A.HW;
  const int ri = A.rank_i[e], rj = A.rank_j[e];
  const Sim3f Tij = relative(load_sim3(A.Twc + 8 * ri), load_sim3(A.Twc + 8 * rj));
  const Sim3Mat Tm = sim3_matrix(Tij);
  const ResidualParams P = kparams(A);
  const float *__restrict__ Xs_j = A.Xs + (size_t)rj * HW * 3;
  constexpr int NPL = PixIn<MODE>::kPlanes;
  const float *__restrict__ pl = A.planes + (size_t)e_loc * NPL * HW;

  AccumPP acc;
  acc.zero();
  const int64_t p_begin = c * A.chunk_pix;
  const int64_t p_end = (p_begin + A.chunk_pix < HW) ? p_begin + A.chunk_pix : HW;
  float sink = 0.0f;  // the memory-floor build only (M3S_PK_FLOOR=1)
  // Prefetch one trip ahead through LDS with no VGPR cost: each wave's next
  // trip (NPL plane vectors + 3 Xj vectors, 16 B per lane each) is loaded by
  // buffer_load_dwordx4 ... lds into the wave's own LDS slot while the wave
  // computes the current trip from registers. Lane l's 16 B land at slot +
  // 16 l (lane-linear), so every lane reads back exactly what it loaded.
  // Round 3: buffer loads with wave-uniform soffsets (the trip's first pixel)
  // and per-lane voffsets fixed for the whole kernel, and the LDS slot (m0)
  // from a wave-uniform wave index: no per-load VALU address arithmetic
  // (17 VALU per trip before). One resource per plane, sized HW floats.
  // one slot per wave (a 2-deep prefetch measured slower)
  constexpr int DEPTH = 1;
  __shared__ __attribute__((aligned(16))) f32x4 stage[DEPTH][kThreads / 64][NPL + 3][64];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), ln = threadIdx.x & 63;
  __amdgpu_buffer_rsrc_t Rp[NPL];
#pragma unroll
  for (int k = 0; k < NPL; k++)
    Rp[k] = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pl + (size_t)k * HW), 0, (int)(4 * HW), 0x00020000);
  const __amdgpu_buffer_rsrc_t Rx =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Xs_j), 0, (int)(12 * HW), 0x00020000);
  const int vo_p = 16 * ln, vo_x = 48 * ln;
  const int pend = (int)p_end;
  // pw: the wave's first pixel of a trip (wave-uniform); lane pixels pw + 4 ln
  auto issue = [&](int pw, int sl_) {
#if defined(M3S_PK_FLOOR) && M3S_PK_FLOOR == 2  // compute floor (A/B only): no loads
    return;
#endif
    // A trip that runs past the chunk's end (a partial last trip only): its
    // lanes past the end take an offset beyond every resource, which reads
    // zeros with no memory access. The buffer range check covers voffset (+
    // the instruction offset), not soffset, so the wave-uniform trip base in
    // soffset alone would let them read past the last plane / pointmap.
    // Round 5: the partial trip has loads of its own with other cache bits
    // (sc0, no nt): with the same intrinsic calls on both sides the compiler
    // merged the two paths into per-lane selects of the offsets on every trip
    // (round 4: 277 -> 283 VALU per calib trip, tools/isa_loop.py).
    if (pw + kPixPerThread * 64 > pend) {  // wave-uniform: the full trips keep the fixed offsets
      const bool out = pw + kPixPerThread * ln >= pend;
      const int vp = out ? kFarOff : vo_p, vx = out ? kFarOff : vo_x;
#pragma unroll
      for (int k = 0; k < NPL; k++)
        buf_lds16_sc0(Rp[k], (__attribute__((address_space(3))) void *)(&stage[sl_][wv][k][0]), vp, 4 * pw);
#pragma unroll
      for (int k = 0; k < 3; k++)
        buf_lds16_sc0(Rx, (__attribute__((address_space(3))) void *)(&stage[sl_][wv][NPL + k][0]), vx, 12 * pw + 16 * k);
      return;
    }
#pragma unroll
    for (int k = 0; k < NPL; k++)
      buf_lds16_nt(Rp[k], (__attribute__((address_space(3))) void *)(&stage[sl_][wv][k][0]), vo_p, 4 * pw);
#pragma unroll
    for (int k = 0; k < 3; k++)
      buf_lds16(Rx, (__attribute__((address_space(3))) void *)(&stage[sl_][wv][NPL + k][0]), vo_x, 12 * pw + 16 * k);
  };
  int pw0 = (int)p_begin + kPixPerThread * 64 * wv;
  if (pw0 < pend) issue(pw0, 0);
  if (DEPTH > 1 && pw0 + kBlockPix < pend) issue(pw0 + kBlockPix, 1 % DEPTH);
  // One trip; PARTIAL: the wave's last trip runs past the chunk's end. The
  // full trips are a loop of their own and the partial one is peeled after
  // it, so the full trips carry no per-lane end test (2 VALU per trip).
  auto trip_body = [&](const int pw, const int trip, const bool PARTIAL) {  // (inlined: PARTIAL folds)
    const int cur = DEPTH > 1 ? (trip & 1) : 0;
    if (DEPTH > 1 && pw + kBlockPix < pend) {
      // this trip's loads are done once at most the next trip's NPL + 3 are in flight
      if constexpr (NPL == 3) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // lanes past the chunk's end (a partial last trip only) read back zeros
    // from the resources and take no part (their exec bit is off)
    if (PARTIAL && pw + kPixPerThread * ln >= pend) return;
    // each pixel pair's operands are read from the LDS slot just before its
    // math (8-B reads: 2 NPL + 6 VGPRs live instead of 4 (NPL + 3)); the slot
    // is refilled once the second pair's operands are in registers
    const float *sl = reinterpret_cast<const float *>(&stage[cur][wv][0][ln]);
#pragma unroll
    for (int h = 0; h < 2; h++) {
      f32x2 in[NPL], X[3];
#pragma unroll
      for (int k = 0; k < NPL; k++) in[k] = *reinterpret_cast<const f32x2 *>(sl + 256 * k + 2 * h);
      // Xj of pixels 2h, 2h + 1: floats 6h .. 6h + 5 of the lane's 12
      const float *xs = sl + 256 * NPL;
      float xf[6];
      lds_xj6(xs, h, xf);
      X[0] = f32x2{xf[0], xf[3]}, X[1] = f32x2{xf[1], xf[4]}, X[2] = f32x2{xf[2], xf[5]};
      if (h == 1) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // slot read back before it is refilled
        if (pw + DEPTH * kBlockPix < pend) issue(pw + DEPTH * kBlockPix, cur);
      }
#if defined(M3S_PK_FLOOR) && M3S_PK_FLOOR == 1  // memory floor (A/B only): no math
      sink += in[0].x + in[NPL - 1].y + X[0].x + X[2].y;
#else
      f32x2 Y[3];
      act2(Tm, X, Y);
      pixel_contrib2<MODE, NPL, false>(acc, P, in, Y);
#endif
    }
  };
  int trip = 0;
  for (; pw0 + kPixPerThread * 64 <= pend; pw0 += kBlockPix, trip++) trip_body(pw0, trip, false);
  if (pw0 < pend) trip_body(pw0, trip, true);
  float sums[kNP];
#pragma unroll
  for (int k = 0; k < kNP; k++) sums[k] = 0.0f;
  if constexpr (MODE == 2) acc.cal25_fixup();
  acc.fold(sums);
  sums[0] += sink;
  store_partial(sums, A.partials + (size_t)b * kNP);
  if (A.edge_cnt) edge_tail(A, e_loc, e);
}

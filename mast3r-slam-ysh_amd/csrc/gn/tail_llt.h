// gn/tail_llt.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The dense top of the elimination tree: kTailNW, kTailRows, TailArgs,
// TailSrc / tail_src / tail_entry, the diagonal-tile routines
// (tail_diag_mfma_t, tail_diag_full, tail_diag_part, tail_diag_mfma,
// tail_diag_warm), tail_tile, tail_load and tail_llt_kernel (one workgroup).
// gn/tail_cyc.h and gn/tail_pair.h build on all of these.
// Relies on gn/layout.h (kTailMaxT, kFlagStop, kFlagSplitFail) and
// gn/llt_blocks.h (f64x4, rsqrt_nr, wave_lds_fence).

// ------------------------------------------- dense tail on the f64 MFMA --
// The top clique of the elimination tree (nc block columns, n = 7 nc scalar
// columns; SparsePlan::nc) after its border updates is a dense SPD system:
// a chain of n dependent pivots. sparse_llt_kernel factored it with 7x7 block
// products on one CU's dependent global-memory round trips (B1/B2, ~440 us at
// 256 KFs). Here one workgroup of 4 waves (one per SIMD) factors it
// left-looking over 16x16 fp64 tiles on v_mfma_f64_16x16x4f64, per tile
// column k:
//   update  A(I,k) -= sum_{j<k} L(I,j) L(k,j)^T for I >= k, accumulated in
//           registers (wave w owns the rows I = k + w (mod 4)); the finished
//           L tiles stream from L2 (written once, read by later columns);
//   diag    wave 0: A(k,k) -> L_kk (register Cholesky, readlane broadcasts),
//           W_k = L_kk^-1 into LDS (and global, for the back-substitution);
//   panel   L(I,k)^T = W_k A(I,k)^T on the MFMA, stored to L2.
// The RHS y is row n of the augmented matrix, so row n of the factor is
// y' = L^-1 y; then L^T x = y' by tile columns from the bottom. Every sum
// runs in a fixed order: bitwise reproducible (the sharded ranks rely on it).
// Replaces the dense-tail part of SimplicialLLT (gn_kernels.cu:132-153).
//
// Layouts. An accumulator tile holds A(I,k)^T in the MFMA C layout: lane l,
// register r = A(I,k)[l & 15][(l >> 4) + 4 r], which is also the operand
// order q = r of a product X . A(I,k)^T. Finished tiles are stored in that
// order, [tile][lane][4] (32 B per lane): every MFMA operand is one load.
constexpr int kTailNW = 4;     // waves (one per SIMD)
constexpr int kTailRows = (kTailMaxT + kTailNW - 1) / kTailNW;  // tile rows per wave and column

struct TailArgs {
  const double *Ad;  // bordered tail, dense symmetric [n][ld] (border_kernel writes it)
  int ld;
  double *rhs;       // y [m][7] in; x of the tail columns out (same place)
  double *Lg;        // finished L tiles, [tile (I,J) = I (I + 1) / 2 + J][64][4]
  double *Wg;        // [TC][16][16]: W_k of every tile column
  int32_t *flags;
  int nc, c0;        // tail columns, first tail column
};

// augmented tail matrix entry (i, j): padding columns are identity (and the
// unused (n, n)), padding rows zero, row n the RHS y of the tail columns
// Both loads are buffer loads, unconditional: an out-of-range offset reads 0
// (kFar), so a workgroup's initial tiles are all in flight at once (a
// guarded pointer load became one branch and one vmcnt(0) per entry).
struct TailSrc {
  __amdgpu_buffer_rsrc_t ad, rhs;
};
__device__ __forceinline__ TailSrc tail_src(const TailArgs &A, int n) {
  return {__builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(A.Ad), 0, n * A.ld * 8, 0x00020000),
          __builtin_amdgcn_make_buffer_rsrc(A.rhs + 7 * A.c0, 0, n * 8, 0x00020000)};
}
__device__ __forceinline__ double tail_entry(const TailArgs &A, const TailSrc &T, int n, int i, int j) {
  constexpr int kFar = 0x7fff0000;
  const bool pad = j >= n || i > n, rrow = i == n;
  const int ao = (!pad && !rrow) ? (i * A.ld + j) * 8 : kFar;
  const int ro = (!pad && rrow) ? j * 8 : kFar;
  const unsigned long long a = __builtin_bit_cast(unsigned long long, __builtin_amdgcn_raw_buffer_load_b64(T.ad, ao, 0, 0));
  const unsigned long long r = __builtin_bit_cast(unsigned long long, __builtin_amdgcn_raw_buffer_load_b64(T.rhs, ro, 0, 0));
  // at most one of the three is non-zero (the other loads read 0): OR, not a
  // select, so the loads stay unconditional
  const unsigned long long p = (pad && j >= n && i == j) ? 0x3ff0000000000000ull : 0ull;
  return __builtin_bit_cast(double, a | r | p);
}

// Diagonal tile (one wave, round 2): the tile stays in the MFMA C layout it
// was accumulated in (lane l, register r = A[(l >> 4) + 4 r][l & 15]) and is
// factored in four steps of 4 columns on the f64 MFMA. Step b: the 4x4 block
// D_b goes to every lane through LDS (the only LDS round trip of the step);
// every lane factors it in registers (L_D, W_D = L_D^-1); the panel
// P = A[:, 4b..4b+3] W_D^T is ONE MFMA (W_D x register b of the tile, which
// is the B operand as it stands, and the result lands in A-operand order);
// the trailing update A -= P P^T is one more. W = L^-1 is accumulated as the
// product of the elementary block-column inverses (two MFMAs per step, off
// the critical path). Round 1's by-rows form broadcast every column through
// LDS and ran ~2000 f64 instructions on one wave (~4 us per tile; this form
// is ~4x fewer). Padding columns / rows (>= jv, incl. the RHS row's own
// column) are identity; the RHS row's panel values are y' (-> yv_k). W ->
// Wk[16][17] (row-major). Returns true on a non-positive pivot (computed on
// with pivot 1; the step becomes dx = 0).
template <bool FULL>  // FULL: jv == 16 (every tile column but possibly the last): no padding masks
__device__ __forceinline__ bool tail_diag_mfma_t(f64x4 a, double (*Wk)[17], double *yv_k, int jv, int rhs_row,
                                                 int lane) {
  if (FULL) jv = 16;
  __shared__ double xd[4][16], xw[4][16];
  const int lr = lane & 15, lk = lane >> 4;
  f64x4 M;  // W accumulator, identity
#pragma unroll
  for (int r = 0; r < 4; r++) M[r] = (lk + 4 * r == lr) ? 1.0 : 0.0;
  bool bad = false;
#pragma unroll
  for (int b = 0; b < 4; b++) {
    const int c0 = 4 * b;
    // D_b[i][j] = A[c0 + i][c0 + j]: register b of the lanes with column lr in the block
    if (lr >= c0 && lr < c0 + 4) xd[b][4 * lk + lr - c0] = a[b];
    wave_lds_fence();
    bool real[4];
#pragma unroll
    for (int m = 0; m < 4; m++) real[m] = FULL || c0 + m < jv;
    double D[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j <= i; j++) {
        const double v = xd[b][4 * i + j];
        D[i][j] = (real[i] && real[j]) ? v : (i == j ? 1.0 : 0.0);
      }
    // 4x4 Cholesky and W_D = L_D^-1, on every lane
    double L[4][4], Wd[4][4], iv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      double d = D[j][j];
      bad |= real[j] && !(d > 0.0);
      d = d > 0.0 ? d : 1.0;
      iv[j] = rsqrt_nr(d);
#pragma unroll
      for (int i = j + 1; i < 4; i++) L[i][j] = D[i][j] * iv[j];
#pragma unroll
      for (int i = j + 1; i < 4; i++)
#pragma unroll
        for (int k = j + 1; k <= i; k++) D[i][k] -= L[i][j] * L[k][j];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      Wd[i][i] = iv[i];
#pragma unroll
      for (int j = 0; j < i; j++) {
        double s = 0.0;
#pragma unroll
        for (int k = j; k < i; k++) s += L[i][k] * Wd[k][j];
        Wd[i][j] = -s * iv[i];
      }
    }
    // A operands: Wpad[lr][lk] = W_D[lr][lk] (lr < 4); A1[lr][lk] = (W_D - I)[lr - c0][lk] (lr in the
    // block): W_D through LDS (every lane holds it; lane 0 writes, each lane reads its entry)
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) xw[b][4 * i + k] = k <= i ? Wd[i][k] : 0.0;
    }
    wave_lds_fence();
    const double wpad = lr < 4 ? xw[b][4 * lr + lk] : 0.0;
    const double a1 =
        (lr >= c0 && lr < c0 + 4) ? xw[b][4 * (lr - c0) + lk] - (lr - c0 == lk ? 1.0 : 0.0) : 0.0;
    // panel P[lr][lk] = L[lr][c0 + lk] (rows above the block and padding columns 0)
    double p = __builtin_amdgcn_mfma_f64_16x16x4f64(wpad, a[b], f64x4{0.0, 0.0, 0.0, 0.0}, 0, 0, 0)[0];
    p = (lr >= c0 && (FULL || c0 + lk < jv)) ? p : 0.0;
    if (!FULL && lr == rhs_row && c0 + lk < jv) yv_k[c0 + lk] = p;
    a = __builtin_amdgcn_mfma_f64_16x16x4f64(-p, p, a, 0, 0, 0);  // A -= P P^T
    // W <- (elementary inverse of block column b) W: the block rows by W_D,
    // then the real rows below lose P_below times them
    const f64x4 Y = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, M[b], M, 0, 0, 0);
    const double a2 = (lr >= c0 + 4 && (FULL || lr < jv)) ? -p : 0.0;
    M = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, Y[b], Y, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; r++) Wk[lk + 4 * r][lr] = M[r];
  return bad;
}
// Not inlined: each tail workgroup factors its diagonal tile(s) once, so the
// ~600 instructions run from a cold instruction cache (measured ~2.5 us per
// tile, ~4x the MFMA / LDS latencies it is made of). One copy of the code, run
// once on a dummy tile while the workgroup waits for its updates
// (tail_diag_warm), is then hot when the real tile arrives.
// Round 6 measured a right-looking by-columns form on DPP row broadcasts
// (v_mov_b64_dpp row_newbcast, no LDS or MFMA on the chain):
// 8.7k cycles per hot call against 5.4k for this one
// (profiles/r06/r6h_ubench_diag16.txt, tools/ubench_diag16.hip): a 64-bit
// DPP broadcast feeding an FMA costs ~30 cycles, 120 of them per tile.
__device__ __noinline__ bool tail_diag_full(f64x4 a, double (*Wk)[17], double *yv_k, int lane) {
  return tail_diag_mfma_t<true>(a, Wk, yv_k, 16, -1, lane);
}
__device__ __noinline__ bool tail_diag_part(f64x4 a, double (*Wk)[17], double *yv_k, int jv, int rhs_row, int lane) {
  return tail_diag_mfma_t<false>(a, Wk, yv_k, jv, rhs_row, lane);
}
__device__ __forceinline__ bool tail_diag_mfma(f64x4 a, double (*Wk)[17], double *yv_k, int jv, int rhs_row,
                                               int lane) {
  return jv == 16 ? tail_diag_full(a, Wk, yv_k, lane) : tail_diag_part(a, Wk, yv_k, jv, rhs_row, lane);
}
// the warm-up: an identity tile through the same call (W lands in Wk before
// the real factor overwrites it; y' goes to the dummy yv_k)
__device__ __forceinline__ void tail_diag_warm(double (*Wk)[17], double *yv_dummy, int jv, int rhs_row, int lane) {
  const int lr = lane & 15, lk = lane >> 4;
  f64x4 e;
#pragma unroll
  for (int r = 0; r < 4; r++) e[r] = (lk + 4 * r == lr) ? 1.0 : 0.0;
  (void)tail_diag_mfma(e, Wk, yv_dummy, jv, rhs_row, lane);
}

__device__ __forceinline__ int tail_tile(int I, int J) { return I * (I + 1) / 2 + J; }

// one finished tile's operand registers (32 B per lane, L2)
__device__ __forceinline__ f64x4 tail_load(const double *Lg, int t, int lane) {
  const f64x4 *p = reinterpret_cast<const f64x4 *>(Lg + (size_t)t * 256) + lane;
  return __builtin_nontemporal_load(p);
}

__global__ void __launch_bounds__(64 * kTailNW, 1) tail_llt_kernel(TailArgs A) {
  if (A.flags[kFlagStop]) return;
  __shared__ double Wk[16][17];  // W_k of the current step
  __shared__ double yv[16 * kTailMaxT], xv[16 * kTailMaxT];
  __shared__ int fail_s;
  const int n = 7 * A.nc;
  const TailSrc TS = tail_src(A, n);
  const int TC = (n + 15) / 16, TR = (n + 16) / 16;  // tile columns; tile rows incl. the RHS row n
  const int In = n / 16, rn = n - 16 * In;             // RHS row: tile row, local row
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  double *Lg = A.Lg, *Wg = A.Wg;
  if (tid == 0) fail_s = 0;
  for (int q = tid; q < 16 * kTailMaxT; q += 64 * kTailNW) yv[q] = 0.0, xv[q] = 0.0;
  __syncthreads();
#ifdef M3S_TAIL_STAMPS
  int64_t *stamp = reinterpret_cast<int64_t *>(Wg + (size_t)kTailMaxT * 256);
#define M3S_STAMP(i) if (tid == 0) stamp[i] = wall_clock64();
#else
#define M3S_STAMP(i)
#endif
  M3S_STAMP(0)
  for (int k = 0; k < TC; k++) {
    // column k: wave w holds the rows I = k + w + 4u (u < kTailRows)
    f64x4 acc[kTailRows];
#pragma unroll
    for (int u = 0; u < kTailRows; u++) {
      const int I = k + wave + kTailNW * u;
      f64x4 v = {0.0, 0.0, 0.0, 0.0};
      if (I < TR) {
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = tail_entry(A, TS, n, 16 * I + lr, 16 * k + lk + 4 * r);
      }
      acc[u] = v;
    }
    // A(I,k)^T -= L(k,j) L(I,j)^T, j ascending; the operands of j + 2 are
    // in flight while j's products run (3-deep register ring)
    f64x4 rk[3], ri[3][kTailRows];
#define M3S_TAIL_ISSUE(j_, b_)                                                           \
  do {                                                                                   \
    rk[b_] = tail_load(Lg, tail_tile(k, (j_)), lane);                                    \
    for (int u = 0; u < kTailRows; u++) {                                                \
      const int I = k + wave + kTailNW * u;                                              \
      if (I < TR) ri[b_][u] = tail_load(Lg, tail_tile(I, (j_)), lane);                   \
    }                                                                                    \
  } while (0)
#define M3S_TAIL_UPD(b_)                                                                 \
  do {                                                                                   \
    for (int u = 0; u < kTailRows; u++) {                                                \
      const int I = k + wave + kTailNW * u;                                              \
      if (I < TR) {                                                                      \
        for (int q = 0; q < 4; q++)                                                      \
          acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(-rk[b_][q], ri[b_][u][q], acc[u], 0, 0, 0); \
      }                                                                                  \
    }                                                                                    \
  } while (0)
    if (k > 0) M3S_TAIL_ISSUE(0, 0);
    if (k > 1) M3S_TAIL_ISSUE(1, 1);
    for (int j = 0; j < k; j += 3) {
      if (j + 2 < k) M3S_TAIL_ISSUE(j + 2, 2);
      M3S_TAIL_UPD(0);
      if (j + 1 >= k) break;
      if (j + 3 < k) M3S_TAIL_ISSUE(j + 3, 0);
      M3S_TAIL_UPD(1);
      if (j + 2 >= k) break;
      if (j + 4 < k) M3S_TAIL_ISSUE(j + 4, 1);
      M3S_TAIL_UPD(2);
    }
#undef M3S_TAIL_ISSUE
#undef M3S_TAIL_UPD
    M3S_STAMP(1 + 3 * k)
    if (wave == 0) {  // diag: tile (k, k) is wave 0's u = 0
      if (tail_diag_mfma(acc[0], Wk, yv + 16 * k, min(16, n - 16 * k), In == k ? rn : -1, lane) && lane == 0)
        fail_s = 1;
      wave_lds_fence();
      if (lane < 16) {
#pragma unroll
        for (int r = 0; r < 16; r++) Wg[(size_t)k * 256 + r * 16 + lane] = Wk[r][lane];
      }
    }
    M3S_STAMP(2 + 3 * k)
    __syncthreads();  // W_k
    // panel: L(I,k)^T = W_k A(I,k)^T for I > k, stored in operand order
#pragma unroll
    for (int u = 0; u < kTailRows; u++) {
      const int I = k + wave + kTailNW * u;
      if (I < TR && I > k) {
        f64x4 d = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 4; q++) d = __builtin_amdgcn_mfma_f64_16x16x4f64(Wk[lr][4 * q + lk], acc[u][q], d, 0, 0, 0);
        reinterpret_cast<f64x4 *>(Lg + (size_t)tail_tile(I, k) * 256)[lane] = d;
        if (I == In && lr == rn) {  // y' of this column from the RHS row
#pragma unroll
          for (int r = 0; r < 4; r++) yv[16 * k + lk + 4 * r] = d[r];
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // L(., k) in L2 before any wave loads it
    __syncthreads();
    M3S_STAMP(3 + 3 * k)
  }
  // back-substitution L^T x = y', tile columns from the bottom; yv
  // accumulates the updates of each column in decreasing K (fixed order).
  // Thread (J, c) (two per thread: 16 (K - 1) <= 496 pairs) sums column c of
  // tile (K, J), L(K,J)[r][c] at lane 16 (c % 4) + r, register c / 4; the next
  // row's tiles and W are loaded while this row runs.
  constexpr int kBP = (16 * kTailMaxT + 64 * kTailNW - 1) / (64 * kTailNW);  // pairs per thread
  double lb[kBP][16], wb[16];
  auto bs_load = [&](int K) {
#pragma unroll
    for (int pp = 0; pp < kBP; pp++) {
      const int q = tid + 64 * kTailNW * pp, J = q >> 4, c = q & 15;
      if (J < K) {
        const double *T = Lg + (size_t)tail_tile(K, J) * 256 + (c >> 2);
#pragma unroll
        for (int r = 0; r < 16; r++) lb[pp][r] = __builtin_nontemporal_load(T + 4 * (16 * (c & 3) + r));
      }
    }
    if (wave == 0 && lane < 16) {
#pragma unroll
      for (int i = 0; i < 16; i++) wb[i] = Wg[(size_t)K * 256 + i * 16 + lane];
    }
  };
  if (TC > 0) bs_load(TC - 1);
  for (int K = TC - 1; K >= 0; K--) {
    const int jv = min(16, n - 16 * K);
    if (wave == 0 && lane < 16) {
      double x = 0.0;
#pragma unroll
      for (int i = 0; i < 16; i++) x += wb[i] * yv[16 * K + i];
      xv[16 * K + lane] = lane < jv ? x : 0.0;
    }
    __syncthreads();
    double u[kBP];
#pragma unroll
    for (int pp = 0; pp < kBP; pp++) {
      u[pp] = 0.0;
      const int q = tid + 64 * kTailNW * pp, J = q >> 4;
      if (J < K) {
#pragma unroll
        for (int r = 0; r < 16; r++) u[pp] += lb[pp][r] * xv[16 * K + r];
      }
    }
    if (K > 0) bs_load(K - 1);
#pragma unroll
    for (int pp = 0; pp < kBP; pp++) {
      const int q = tid + 64 * kTailNW * pp, J = q >> 4, c = q & 15;
      if (J < K) yv[16 * J + c] -= u[pp];
    }
    __syncthreads();
  }
  M3S_STAMP(100)
  for (int j = tid; j < n; j += 64 * kTailNW) A.rhs[7 * A.c0 + j] = xv[j];
  if (tid == 0 && fail_s) A.flags[kFlagSplitFail] = 1;
#undef M3S_STAMP
}

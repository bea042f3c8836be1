// gn/tail_cyc.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The dense tail with one tile column per workgroup: TailSync, the sc1 tile
// loads and stores, the tagged 16-B granules of the hand-offs (GranTile,
// gran_*), tail_backsub_wg and tail_cyc_kernel (the A/B reference of
// tail_pair_kernel, behind the test-only tail_pair knob). The part closes
// with the introduction of tail_pair_kernel ("Round 4"); the kernel stands in
// gn/tail_pair.h, behind the code it shares a launch with.
// Relies on gn/layout.h (kTailMaxT and the flags), sum_xor16_32
// (gn/linearize.h), gn/llt_blocks.h (f64x4, ld_sc1 / st_sc1, poll_b128,
// wave_lds_fence), gn/col_tasks.h (kColSpins, M3S_CSTAMP) and gn/tail_llt.h
// (TailArgs, tail_src / tail_entry, tail_diag_mfma, tail_diag_warm,
// tail_tile, kTailNW).

// ----------------------------- dense tail over many workgroups (default) --
// The same left-looking 16x16-tile factorisation as tail_llt_kernel, with
// tile column J on workgroup J (TC workgroups of 4 waves, wave w holding the
// rows I = J + w (mod 4) in MFMA accumulator registers). Workgroup J applies
// the update of every finished column k < J as soon as column k is published
// (A(I,J)^T -= L(J,k) L(I,k)^T, k ascending: the single-workgroup kernel's
// order, so the result is bitwise the same), then factors its diagonal tile,
// forms its panel L(I,J)^T = W_J A(I,J)^T, and publishes the panel, W_J and
// y'_J (write-through stores drained before an epoch flag). The critical
// path per tile column is one hand-off + one tile update + the diagonal
// factor, instead of the whole left-looking sweep of one CU (281 us at 256
// KFs). The last workgroup then runs the back-substitution L^T x = y' over
// the published tiles (sc1 loads).
struct TailSync {
  int32_t *tflag;    // [TC] epoch flags: tile column published (W_J, y'_J, the LgT tiles: back-substitution)
  int epoch;
  double *ypg;     // y' of every tile column [16 TC]
  double *LgT;     // the L tiles again, L(I,J) (not transposed) in the MFMA C layout, [tile][2][64 lanes][2] (back-substitution A operands)
  double *LgG;     // the L tiles as tagged granules, [tile][4][64 lanes] x {double, epoch tag, 0} (16 B; zeroed per call)
  int warm;        // 1: warm the diagonal factor's code on a dummy tile first (tail_diag_warm)
};
constexpr size_t kTailGranBytes = (size_t)kTailMaxT * (kTailMaxT + 1) / 2 * 64 * 4 * 16;

__device__ __forceinline__ f64x4 ld_sc1_f64x4(const double *p) {
  f64x4 v;
#pragma unroll
  for (int r = 0; r < 4; r++) v[r] = ld_sc1(p + r);
  return v;
}
__device__ __forceinline__ void st_sc1_f64x4(double *p, f64x4 v) {
#pragma unroll
  for (int r = 0; r < 4; r++) st_sc1(p + r, v[r]);
}

// Tagged-granule tile hand-off (MI355X_MICROARCH.md, handoff-1to1 / R2): each
// entry is one 16-B write-through store {value, epoch tag}, read back by a
// 16-B sc1 buffer load; the consumer checks the tags, so there is no flag, no
// producer drain and no second round trip (flag, then payload).
struct GranTile {
  u32x4 v[4];
};
__device__ __forceinline__ __amdgpu_buffer_rsrc_t gran_rsrc(double *p) {
  return __builtin_amdgcn_make_buffer_rsrc(p, 0, (int)kTailGranBytes, 0x00020000);
}
__device__ __forceinline__ void gran_load(__amdgpu_buffer_rsrc_t R, int tile, int lane, GranTile &g) {
#pragma unroll
  for (int r = 0; r < 4; r++) g.v[r] = poll_b128(R, ((tile * 4 + r) * 64 + lane) * 16);
}
__device__ __forceinline__ bool gran_ready(const GranTile &g, int want) {  // wave-uniform
  const bool ok = g.v[0].z == (unsigned)want && g.v[1].z == (unsigned)want && g.v[2].z == (unsigned)want &&
                  g.v[3].z == (unsigned)want;
  return __ballot(!ok) == 0;
}
__device__ __forceinline__ f64x4 gran_val(const GranTile &g) {
  f64x4 d;
#pragma unroll
  for (int r = 0; r < 4; r++) d[r] = __longlong_as_double((long long)(((unsigned long long)g.v[r].y << 32) | g.v[r].x));
  return d;
}
// Granule r of every lane of a tile is one 1-KB run ([tile][4][64 lanes]):
// each 16-B store / load instruction of the wave covers whole lines (round 4;
// lane-major [tile][64][4] made every instruction a 25 %-dense 4-KB stride of
// partial-line write-through stores)
__device__ __forceinline__ void gran_store(__amdgpu_buffer_rsrc_t R, int tile, int lane, f64x4 d, int want) {
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(d[r]);
    const u32x4 w = {(unsigned)(b & 0xffffffffu), (unsigned)(b >> 32), (unsigned)want, 0u};
    __builtin_amdgcn_raw_buffer_store_b128(w, R, ((tile * 4 + r) * 64 + lane) * 16, 0, 16);
  }
}

// The last workgroup of a tail launch: back-substitution L^T x = y' over the
// published tiles (after every column flag), x of the tail columns to A.rhs.
__device__ __forceinline__ void tail_backsub_wg(const TailArgs &A, const TailSync &S, double *yv, double *xv) {
  const int n = 7 * A.nc;
  const int TC = (n + 15) / 16;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const int want = S.epoch + 1;
  double *Wg = A.Wg;
  // The last workgroup: back-substitution L^T x = y' over the published tiles
  // (every column k < J was waited for above). Wave w owns the tile rows
  // J' = w (mod 4) of y' (it alone updates them); x_K is formed by the owner
  // of row K as soon as its own updates from x_{K+1..} are in, then handed to
  // the other waves through LDS with a flag: no workgroup barrier per step.
  // The same sums in the same order as tail_llt_kernel's loop.
  __shared__ int xflag[kTailMaxT];
  if (wave == 0) {  // every column's W, y' and LgT tiles are out (column flags, one per lane)
    int spins = 0;
    while (__ballot(lane < TC && __hip_atomic_load(S.tflag + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != want)) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > kColSpins) {
        if (lane == 0) __hip_atomic_store(A.flags + kFlagSplitFail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
    }
  }
  __syncthreads();
  if (tid == 0) M3S_CSTAMP(2, 698, 0);
  // every W_K^T to LDS (rows padded to 17: conflict-free column reads)
  __shared__ double WlT[kTailMaxT * 16 * 17];
  {  // all loads in flight at once (16-B sc1 buffer loads; out of range past TC reads zeros)
    constexpr int kWL = kTailMaxT * 256 / (2 * 64 * kTailNW);
    const __amdgpu_buffer_rsrc_t RW = __builtin_amdgcn_make_buffer_rsrc(Wg, 0, kTailMaxT * 256 * 8, 0x00020000);
    u32x4 wv[kWL];
#pragma unroll
    for (int i = 0; i < kWL; i++) {
      const int q2 = 2 * (tid + 64 * kTailNW * i);
      wv[i] = __builtin_amdgcn_raw_buffer_load_b128(RW, q2 < 256 * TC ? q2 * 8 : 0x7fffff00, 0, 16);
    }
    double yl[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int q = tid + 64 * kTailNW * i;
      yl[i] = q < 16 * TC ? ld_sc1(S.ypg + q) : 0.0;
    }
#pragma unroll
    for (int i = 0; i < kWL; i++) {
      const int q2 = 2 * (tid + 64 * kTailNW * i);
      WlT[(q2 >> 4) * 17 + (q2 & 15)] = __longlong_as_double((long long)(((unsigned long long)wv[i].y << 32) | wv[i].x));
      WlT[(q2 >> 4) * 17 + (q2 & 15) + 1] =
          __longlong_as_double((long long)(((unsigned long long)wv[i].w << 32) | wv[i].z));
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int q = tid + 64 * kTailNW * i;
      if (q < 16 * TC) yv[q] = yl[i];
    }
  }
  for (int q = tid; q < 16 * kTailMaxT; q += 64 * kTailNW) xv[q] = 0.0;
  if (tid < kTailMaxT) xflag[tid] = 0;
  __syncthreads();
  // y_J -= L(K, J)^T x_K from the LgT tile (operand order: 32 B per lane).
  // The operands of the next step are in flight while this one runs: every
  // load is a 16-B sc1 buffer load issued unconditionally (rows a step does
  // not need read out of range, which returns zeros without a memory access),
  // so each step issues the same number of loads and the compiler waits for
  // exactly the older step's (24 per wave, two steps = 48 < the 63 vmcnt).
  // Per step K the owner of row K - 1 applies x_K to that row first and forms
  // x_{K-1} at once (the chain per step is one tile update + one 16-term
  // dot product), then applies x_K to its other rows. Each row still takes
  // its updates in decreasing K (the same sums).
  constexpr int kTW = (kTailMaxT + kTailNW - 1) / kTailNW;  // tile rows J' of one wave
  constexpr int kRing = 3;
  const __amdgpu_buffer_rsrc_t RT =
      __builtin_amdgcn_make_buffer_rsrc(S.LgT, 0, kTailMaxT * (kTailMaxT + 1) / 2 * 256 * 8, 0x00020000);
  constexpr int kFar = 0x7fffff00;  // out of range
  f64x4 lt[kRing][kTW];
  auto ld2 = [&](int off, double &x0, double &x1) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(RT, off, 0, 16);
    x0 = __longlong_as_double((long long)(((unsigned long long)v.y << 32) | v.x));
    x1 = __longlong_as_double((long long)(((unsigned long long)v.w << 32) | v.z));
  };
  auto bs_load = [&](int K, int slot) {
#pragma unroll
    for (int t = 0; t < kTW; t++) {
      const int Jc = wave + kTailNW * t;
      // tile layout [tile][2 halves][64 lanes][2 doubles] (every 16-B access of
      // the wave covers whole lines)
      const bool in = K >= 0 && Jc < K;
      const int off = in ? (tail_tile(K, Jc) * 256 + 2 * lane) * 8 : kFar;
      double x0, x1, x2, x3;
      ld2(off, x0, x1);
      ld2(in ? off + 1024 : kFar, x2, x3);
      lt[slot][t] = f64x4{x0, x1, x2, x3};
    }
  };
  auto form_x = [&](int K) {  // the owner of row K, all of whose updates are in
    const int jv = min(16, n - 16 * K);
    // x_K[r] = sum_i W_K^T[r][i] y'_K[i]: lane r + 16 g sums i in [4 g, 4 g + 4),
    // then the four groups by the permlane swaps (4 dependent FMAs + 2 swap
    // steps on the chain instead of 16 FMAs, round 5)
    if (lane < 16) {
      double x = 0.0;
#pragma unroll
      for (int i = 0; i < 16; i++) x += WlT[(K * 16 + lane) * 17 + i] * yv[16 * K + i];
      xv[16 * K + lane] = lane < jv ? x : 0.0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) __hip_atomic_store(xflag + K, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (lane == 0) M3S_CSTAMP(2, 700 + K, 0);
  };
#pragma unroll
  for (int d = 0; d < kRing; d++) bs_load(TC - 1 - d, d);
  if (tid == 0) M3S_CSTAMP(2, 699, 0);
  if ((TC - 1) % kTailNW == wave) form_x(TC - 1);
  for (int K0 = TC - 1; K0 >= 0; K0 -= kRing) {
#pragma unroll
    for (int d = 0; d < kRing; d++) {
      const int K = K0 - d;
      if (K >= 0) {
        if (K % kTailNW != wave) {  // (the owner formed x_K itself, in the step before)
          int spins = 0;
          while (__hip_atomic_load(xflag + K, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0 &&
                 spins < (1 << 22))
            spins++;
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        double xb[4];
#pragma unroll
        for (int q = 0; q < 4; q++) xb[q] = xv[16 * K + 4 * q + lk];
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
#pragma unroll
          for (int t = 0; t < kTW; t++) {
            const int Jc = wave + kTailNW * t;
            if (pass == 0 ? Jc == K - 1 : Jc < K - 1) {
              // (L^T x)[m], m = lr: lane l holds L(K,Jc)^T[lr][lk + 4q]; the 4 lanes of
              // one m add their partial sums (VALU: the MFMA form spent 15/16 of its work
              // on copies of x)
              double u = 0.0;
#pragma unroll
              for (int q = 0; q < 4; q++) u += lt[d][t][q] * xb[q];
              u = sum_xor16_32(u);
              if (lane < 16) yv[16 * Jc + lane] -= u;
              if (pass == 0) {
                wave_lds_fence();  // row K - 1's y' before this wave reads it
                form_x(K - 1);
              }
            }
          }
        }
        wave_lds_fence();
      }
      bs_load(K - kRing, d);
    }
  }
  __syncthreads();  // every x_K
  for (int j = tid; j < n; j += 64 * kTailNW) A.rhs[7 * A.c0 + j] = xv[j];
  if (tid == 0) M3S_CSTAMP(2, 511, 0);
}


// Round 2: the L tiles go from workgroup to workgroup as tagged granules
// (one hop = one store + one polled load), the panel follows the updates
// without a workgroup barrier (waves 1..3 wait for W_J on an LDS flag), and
// the column flag only guards what the back-substitution reads.
__global__ void __launch_bounds__(64 * kTailNW, 1) tail_cyc_kernel(TailArgs A, TailSync S) {
  if (A.flags[kFlagStop]) return;
  __shared__ double Wk[16][17];
  __shared__ double yv[16 * kTailMaxT], xv[16 * kTailMaxT];
  __shared__ int fail_s, wready;
  const int n = 7 * A.nc;
  const TailSrc TS = tail_src(A, n);
  const int TC = (n + 15) / 16, TR = (n + 16) / 16;
  const int In = n / 16, rn = n - 16 * In;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const int J = blockIdx.x;
  const int want = S.epoch + 1;
  double *Wg = A.Wg;
  const __amdgpu_buffer_rsrc_t R = gran_rsrc(S.LgG);
  // rows: wave 0 holds only the diagonal tile (its factor is the critical
  // path), waves 1..3 the rows below it, I = J + w + 3 u
  constexpr int kRC = (kTailMaxT + 2) / 3;
  auto rowI = [&](int u) { return wave == 0 ? (u == 0 ? J : -1) : J + wave + 3 * u; };
  auto live = [&](int u) {
    const int I = rowI(u);
    return I >= 0 && I < TR;
  };
  if (tid == 0) fail_s = 0, wready = 0;
  for (int q = tid; q < 16 * kTailMaxT; q += 64 * kTailNW) yv[q] = 0.0;
  __syncthreads();
  f64x4 acc[kRC];
#pragma unroll
  for (int u = 0; u < kRC; u++) {
    f64x4 v = {0.0, 0.0, 0.0, 0.0};
    if (live(u)) {
#pragma unroll
      for (int r = 0; r < 4; r++) v[r] = tail_entry(A, TS, n, 16 * rowI(u) + lr, 16 * J + lk + 4 * r);
    }
    acc[u] = v;
  }
  // updates from the finished columns, k ascending (the single-workgroup
  // kernel's order: bitwise the same sums), each tile as soon as it lands
  auto poll_tile = [&](int t, GranTile &g) {
    int spins = 0;
    for (;;) {
      gran_load(R, t, lane, g);
      if (gran_ready(g, want)) break;
      __builtin_amdgcn_s_sleep(1);
      if (++spins > kColSpins) {
        if (lane == 0) fail_s = 1;
        break;
      }
    }
  };
  if (wave == 0 && J > 0 && S.warm) tail_diag_warm(Wk, xv + 16 * J, min(16, n - 16 * J), In == J ? rn : -1, lane);
  f64x4 rk_last = {0.0, 0.0, 0.0, 0.0};  // tile L(J, J-1): waves 1..3 apply column J - 1 row by row below
  for (int k = 0; k < J; k++) {
    GranTile gk;
    poll_tile(tail_tile(J, k), gk);
    const f64x4 rk = gran_val(gk);
    if (wave == 0) {
#pragma unroll
      for (int q = 0; q < 4; q++) acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(-rk[q], rk[q], acc[0], 0, 0, 0);
    } else if (k + 1 == J) {
      rk_last = rk;
    } else {
      // every row's tile of column k: all loads in flight at once, the rows
      // that have landed are applied, the rest polled again
      unsigned pend = 0;
#pragma unroll
      for (int u = 0; u < kRC; u++)
        if (live(u)) pend |= 1u << u;
      int spins = 0;
      while (pend) {
        GranTile g[kRC];
#pragma unroll
        for (int u = 0; u < kRC; u++)
          if (pend & (1u << u)) gran_load(R, tail_tile(rowI(u), k), lane, g[u]);
#pragma unroll
        for (int u = 0; u < kRC; u++) {
          if ((pend & (1u << u)) && gran_ready(g[u], want)) {
            const f64x4 ri = gran_val(g[u]);
#pragma unroll
            for (int q = 0; q < 4; q++) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(-rk[q], ri[q], acc[u], 0, 0, 0);
            pend &= ~(1u << u);
          }
        }
        if (pend) {
          __builtin_amdgcn_s_sleep(1);
          if (++spins > kColSpins) {
            if (lane == 0) fail_s = 1;
            break;
          }
        }
      }
    }
  }
  if (wave == 0) {  // the diagonal tile: factor, W_J
    if (tid == 0) M3S_CSTAMP(2, J, 1);
    if (tid == 0) M3S_CSTAMP(2, 600 + J, 0);
    if (tail_diag_mfma(acc[0], Wk, yv + 16 * J, min(16, n - 16 * J), In == J ? rn : -1, lane) && lane == 0)
      fail_s = 1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // Wk (and y') before the flag
    if (lane == 0) __hip_atomic_store(&wready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (tid == 0) M3S_CSTAMP(2, J, 2);
    // W^T ([16][16] row-major, element e = 16 l + r holds W[r][l]): four
    // stores of 64 consecutive elements, whole lines each
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int e = 64 * i + lane;
      st_sc1(Wg + (size_t)J * 256 + e, Wk[e & 15][e >> 4]);
    }
    if (In == J && lane < 16) st_sc1(S.ypg + 16 * J + lane, yv[16 * J + lane]);
  } else {
    // row by row, the sub-diagonal tile first: the update from column J - 1
    // (as its tile lands), then the panel tile L(I, J)^T = W_J A(I, J)^T,
    // handed off as granules at once
    bool have_w = false;
#pragma unroll
    for (int u = 0; u < kRC; u++) {
      const int I = rowI(u);
      if (live(u)) {
        if (J > 0) {
          GranTile g;
          poll_tile(tail_tile(I, J - 1), g);
          const f64x4 ri = gran_val(g);
#pragma unroll
          for (int q = 0; q < 4; q++) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(-rk_last[q], ri[q], acc[u], 0, 0, 0);
        }
        if (!have_w) {
          int spins = 0;
          while (__hip_atomic_load(&wready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0 &&
                 spins < (1 << 20)) {
            __builtin_amdgcn_s_sleep(1);
            spins++;
          }
          if (spins >= (1 << 20) && lane == 0) fail_s = 1;
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
          have_w = true;
        }
        f64x4 d = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 4; q++) d = __builtin_amdgcn_mfma_f64_16x16x4f64(Wk[lr][4 * q + lk], acc[u][q], d, 0, 0, 0);
        gran_store(R, tail_tile(I, J), lane, d, want);
        if (I == J + 1 && tid == 64) M3S_CSTAMP(2, J, 0);
        if (I == In && lr == rn) {  // y' of this column from the RHS row
#pragma unroll
          for (int r = 0; r < 4; r++) st_sc1(S.ypg + 16 * J + lk + 4 * r, d[r]);
        }
      }
    }
    // L(I, J) itself (operands swapped: A(I, J) W^T) for the back-substitution,
    // after every hand-off of this wave (16-B write-through stores)
    const __amdgpu_buffer_rsrc_t RT =
        __builtin_amdgcn_make_buffer_rsrc(S.LgT, 0, kTailMaxT * (kTailMaxT + 1) / 2 * 256 * 8, 0x00020000);
#pragma unroll
    for (int u = 0; u < kRC; u++) {
      const int I = rowI(u);
      if (live(u) && I < TC) {
        f64x4 dt = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 4; q++) dt = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[u][q], Wk[lr][4 * q + lk], dt, 0, 0, 0);
        const unsigned long long b0 = __double_as_longlong(dt[0]), b1 = __double_as_longlong(dt[1]),
                                 b2 = __double_as_longlong(dt[2]), b3 = __double_as_longlong(dt[3]);
        const u32x4 w0 = {(unsigned)b0, (unsigned)(b0 >> 32), (unsigned)b1, (unsigned)(b1 >> 32)};
        const u32x4 w1 = {(unsigned)b2, (unsigned)(b2 >> 32), (unsigned)b3, (unsigned)(b3 >> 32)};
        const int off = (tail_tile(I, J) * 256 + 2 * lane) * 8;  // (halves of 1 KB: whole lines per store)
        __builtin_amdgcn_raw_buffer_store_b128(w0, RT, off, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b128(w1, RT, off + 1024, 0, 16);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every store of this wave has left
  __syncthreads();
  if (tid == 0) {
    if (fail_s) __hip_atomic_store(A.flags + kFlagSplitFail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(S.tflag + J, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    M3S_CSTAMP(2, J, 3);
  }
  if (J != TC - 1) return;
  tail_backsub_wg(A, S, yv, xv);
}


// Round 4: two tile columns per workgroup (J0 = 2 b, J1 = J0 + 1). The
// chain per tile column of tail_cyc_kernel is a hand-off (~1.3 us) + the
// diagonal factor (~2.4 us) + a panel tile; here the second column of a pair
// takes its sub-diagonal panel tile L(J1, J0) and the update of its diagonal
// from the first column inside the workgroup (wave 0, no hand-off), so the
// chain has one hand-off per two columns. Wave 0 holds the tiles (J0, J0),
// (J1, J0), (J1, J1); waves 1..3 the rows below, I = J1 + w + 3 u, for both
// columns. Per tile the same updates in the same order as tail_cyc_kernel
// (columns k ascending, then the pair's own first column): bitwise the same
// factor; the back-substitution is the same code (tail_backsub_wg).
// RC: row tiles per wave (waves 1..3 hold rows J1 + w + 3 u, u < RC): 7 up to
// 23 tile rows (the register arrays of 11 spill), 11 up to kTailMaxT

// gn/tail_pair.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The dense-tail launch of the large graphs: GArgs, g_poll / g_wait_flags and
// gcol_worker (the sparse columns' back-substitution, run by the launch's
// extra workgroups while the tail factors), then tail_pair_kernel<RC> (two
// tile columns per workgroup; introduced at the end of gn/tail_cyc.h).
// Relies on gn/layout.h (kTailMaxT and the flags), the wave sums of
// gn/linearize.h (xred_index, xreduceN_dpp), gn/llt_blocks.h (f64x4, ld_sc1 /
// st_sc1, wave_lds_fence), gn/col_tasks.h (ColArgs, kColSpins, M3S_CSTAMP,
// set_fail, wave_gticket), col_finish (gn/dataflow.h), gn/tail_llt.h
// (TailArgs, the diagonal tile, tail_tile, kTailNW) and gn/tail_cyc.h
// (TailSync, the granules, tail_backsub_wg).

// ------------------------ sparse back-substitution beside the dense tail --
// Round 5: the sparse back-substitution off the critical path. The sparse
// columns' x is affine in the tail's: x_s = L_ss^-T (y_s - L_ts^T x_t), so
// for every sparse column k
//   X_k = [a_k | B_k] = W_k^T (R_k - sum_{i sparse in struct(k)} L_ik^T X_i),
//   R_k = [y_k | 0] - sum_{i tail in struct(k)} L_ik^T [0 | E_i]
// (E_i picks x_i out of x_t), and x_k = a_k + B_k x_t. The X_k recursion
// needs only the factor, so extra workgroups of the dense tail's launch run
// it (column tasks in reverse level order, the X_i of the sparse ancestors
// by epoch flags) while the tail factors on its own workgroups; once the
// tail's x_t is out, x_k = a_k + B_k x_t is one short dot product per entry
// and col_backsub_kernel's chain of dependent hand-offs (9 levels, ~27 us,
// plus its launch at 256 KFs) leaves the critical path. x_k differs from the
// substitution by fp64 round-off (a different summation order).
struct GArgs {
  double *X;     // [m][7][nx] row-major per column (nx = 1 + 7 nc, padded)
  int nx, n_pairs;
  int32_t *task, *comb, *fin, *xt_ready;  // ticket / ticket / counter / flag words (colsync; zeroed per call)
  int32_t *cnt;                           // [m] chunks of X_k done (colsync; zeroed per call)
};
constexpr int kGBat = 8;    // sparse ancestors' X_i loads in flight per lane
constexpr int kGCapS = 24;  // sparse ancestors' L_ik staged in LDS per wave (the rest read from global)
constexpr int kGMaxS = 512; // sparse ancestors of one column: < m <= 512 on the chip-wide path
constexpr int kGTmap = kTailMaxT * 16 / 7 + 8;
#ifndef M3S_GSLEEP
#define M3S_GSLEEP 8
#endif
__device__ __forceinline__ bool g_poll(const int32_t *flag, int want) {  // bounded wait for one epoch flag
  for (int spins = 0; __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != want; spins++) {
    if (spins > kColSpins) return false;
    __builtin_amdgcn_s_sleep(M3S_GSLEEP);
  }
  return true;
}
// wait_flags with the workers' poll interval (they wait beside the tail's hand-offs)
__device__ __forceinline__ bool g_wait_flags(const int32_t *flag, const int32_t *idx, int q0, int q1, int lim, int want,
                                             int lane) {
  int spins = 0;
  for (int qb = q0; qb < q1; qb += 64) {
    const int q = qb + lane;
    const int i = q < q1 ? idx[q] : -1;
    for (;;) {
      const bool ok = i < 0 || i >= lim ||
                      __hip_atomic_load(flag + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == want;
      if (__ballot(!ok) == 0) break;
      __builtin_amdgcn_s_sleep(M3S_GSLEEP);
      if (++spins > kColSpins) return false;
    }
  }
  return true;
}
// Per wave, task (k, ch): the 64 columns c = 64 ch + lane of X_k (a column of
// ~300 c at 256 KFs is ~170 KB of X_i reads: one CU's fabric bandwidth made a
// whole-column task ~10 us, so a column is spread over S = nx / 64 waves on
// as many CUs); the last of its S chunks to finish (per-column counter
// G.cnt, epoch-based) publishes done2[k].
__device__ void gcol_worker(const ColArgs &C, const GArgs &G) {
  __shared__ double Lw[kTailNW][kGCapS * 49], Ww[kTailNW][49];
  __shared__ int tmapw[kTailNW][kGTmap];  // tail block (i - c0) -> its position q in struct(k), or -1
  __shared__ int sqw[kTailNW][kGMaxS];    // the sparse ancestors' positions q in struct(k), list order
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t *pl = C.plan;
  const int32_t *col_ptr = pl + C.off[kSec_col_ptr], *col_row = pl + C.off[kSec_col_row],
                *col_slot = pl + C.off[kSec_col_slot], *corder = pl + C.off[kSec_corder];
  const int want = C.epoch + 1, c0 = C.c0, nct = C.m - c0, nx = G.nx, nt = 7 * nct;
  const int nG = (int)gridDim.x - G.n_pairs;
  const int S = (nx + 63) / 64;
  double *Lk = Lw[wave], *Wk = Ww[wave];
  int *tmap = tmapw[wave], *sq = sqw[wave];
  // 1. the X_k recursion, column chunks in reverse level order
  const int base = C.epoch * (C.ncols * S + kTailNW * nG);
  for (;;) {
    const int t = wave_gticket(G.task) - base;
    if (t >= C.ncols * S) break;
    const int ci = t / S, ch = t - S * ci;
    const int k = corder[C.ncols - 1 - ci];
    const int q0 = col_ptr[k], q1 = col_ptr[k + 1];
    if (lane == 0 && ch == 0) M3S_CSTAMP(1, k, 0);
    for (int q = lane; q < nct; q += 64) tmap[q] = -1;
    wave_lds_fence();
    int ns = 0;
    for (int qb = q0; qb < q1; qb += 64) {  // tail positions; sparse ancestors compacted in list order
      const int q = qb + lane;
      const int i = q < q1 ? col_row[q] : c0;
      if (q < q1 && i >= c0) tmap[i - c0] = q - q0;
      const uint64_t sm = __ballot(q < q1 && i < c0);
      const int pos = ns + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(sm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)sm, 0u));
      if (q < q1 && i < c0 && pos < kGMaxS) sq[pos] = q - q0;
      ns += __popcll(sm);
    }
    ns = min(ns, kGMaxS);
    wave_lds_fence();
    // the factor is final: the ancestors' L_ik and W_k by plain loads
    for (int e = lane; e < 49 * min(ns, kGCapS); e += 64) Lk[e] = C.L[(size_t)col_slot[q0 + sq[e / 49]] * 49 + e % 49];
    if (lane < 49) Wk[lane] = C.Dinv[(size_t)k * 49 + lane];
    const int c = 64 * ch + lane;
    const bool cv = c < nx;
    double r[7];
    {  // R_k: [y_k | 0] minus, for the tail block i holding dof j = c - 1, row j of L_ik^T
      const int j = c - 1;
      const int q = c > 0 && j < nt ? tmap[j / 7] : -1;
      const double *Lq = C.L + (size_t)col_slot[q0 + (q >= 0 ? q : 0)] * 49 + (j % 7) * 7;
#pragma unroll
      for (int a = 0; a < 7; a++) r[a] = (c == 0 ? C.y[(size_t)k * 7 + a] : 0.0) - (q >= 0 ? Lq[a] : 0.0);
    }
    if (!g_wait_flags(C.done2, col_row, q0, q1, c0, want, lane) && lane == 0) set_fail(C.flags);  // sparse ancestors' X_i
    wave_lds_fence();
    if (lane == 0 && ch == 0) M3S_CSTAMP(1, k, 1);
    const int cl = cv ? c : 0;
    for (int u0 = 0; u0 < ns; u0 += kGBat) {  // - L_ik^T X_i, ancestors in list order
      double xi[kGBat][7];
#pragma unroll
      for (int v = 0; v < kGBat; v++) {
        const double *Xi = G.X + (size_t)col_row[q0 + sq[min(u0 + v, ns - 1)]] * 7 * nx + cl;
#pragma unroll
        for (int b = 0; b < 7; b++) xi[v][b] = ld_sc1(Xi + (size_t)b * nx);
      }
#pragma unroll
      for (int v = 0; v < kGBat; v++) {
        const int u = u0 + v;
        if (u >= ns) break;
        const double *Lq = u < kGCapS ? Lk + 49 * u : C.L + (size_t)col_slot[q0 + sq[u]] * 49;
#pragma unroll
        for (int a = 0; a < 7; a++) {
          double sm = 0.0;
#pragma unroll
          for (int b = 0; b < 7; b++) sm += Lq[b * 7 + a] * xi[v][b];
          r[a] -= sm;
        }
      }
    }
    double *Xk = G.X + (size_t)k * 7 * nx;
    if (cv) {
#pragma unroll
      for (int a = 0; a < 7; a++) {  // X_k = W_k^T r
        double x = 0.0;
#pragma unroll
        for (int b = 0; b < 7; b++) x += Wk[b * 7 + a] * r[b];
        st_sc1(Xk + (size_t)a * nx + c, x);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this chunk's X_k stores have left
    if (lane == 0) {
      const int o = __hip_atomic_fetch_add(G.cnt + k, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (o == want * S - 1) {  // the column's last chunk
        __hip_atomic_store(C.done2 + k, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        M3S_CSTAMP(1, k, 2);
      }
    }
    wave_lds_fence();  // before the next task rewrites this wave's LDS
  }
  // 2. x_k = a_k + B_k x_t: one column per wave over every worker wave; B_k
  // is in registers (ready once X_k is) before the tail's x_t is out, so
  // after its flag only x_t is read (one round trip) and summed
  const int cbase = C.epoch * (C.ncols + kTailNW * nG);
  constexpr int kCU = 16 * kTailMaxT / 64;  // tail dofs per lane (nt < 16 kTailMaxT)
  int ri;
  bool rv;
  xred_index<7>(lane, ri, rv);
  for (;;) {
    const int t = wave_gticket(G.comb) - cbase;
    if (t >= C.ncols) break;
    const int k = corder[C.ncols - 1 - t];  // root side first: those X_k are out first
    const double *Xk = G.X + (size_t)k * 7 * nx;
    if (lane == 0 && !g_poll(C.done2 + k, want)) set_fail(C.flags);  // X_k of another workgroup
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double bx[kCU][7];
#pragma unroll
    for (int u = 0; u < kCU; u++) {
      const int j = lane + 64 * u;
#pragma unroll
      for (int a = 0; a < 7; a++) bx[u][a] = j < nt ? ld_sc1(Xk + (size_t)a * nx + 1 + j) : 0.0;
    }
    const double a0 = ld_sc1(Xk + (size_t)(rv ? ri : 0) * nx);  // a_k[ri]: this lane's row of the result
    if (lane == 0 && !g_poll(G.xt_ready, want)) set_fail(C.flags);  // the tail's x_t
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double acc[7];
#pragma unroll
    for (int a = 0; a < 7; a++) acc[a] = 0.0;
#pragma unroll
    for (int u = 0; u < kCU; u++) {
      const int j = lane + 64 * u;
      const double xt = j < nt ? ld_sc1(C.y + (size_t)7 * c0 + j) : 0.0;
#pragma unroll
      for (int a = 0; a < 7; a++) acc[a] += bx[u][a] * xt;
    }
    // the 7 wave sums by the transposed reduction (permlane swaps + DPP):
    // lane ri-holder ends with row ri's sum
    const double v = xreduceN_dpp<7>(acc, lane);
    if (rv) st_sc1(C.y + (size_t)k * 7 + ri, a0 + v);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // x_k (and any failure flag) out before the ticket
    if (lane == 0) M3S_CSTAMP(1, k, 3);
    const int f = wave_gticket(G.fin);  // the wave that combines the last column finishes the step
    if (f - C.epoch * C.ncols == C.ncols - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      col_finish(C, lane);
    }
  }
}

template <int RC>
__global__ void __launch_bounds__(64 * kTailNW, 1) tail_pair_kernel(TailArgs A, TailSync S, ColArgs C, GArgs G) {
  if (A.flags[kFlagStop]) return;
  if (G.X && (int)blockIdx.x >= G.n_pairs) {  // the sparse back-substitution's workers
    gcol_worker(C, G);
    return;
  }
  __shared__ double Wk[2][16][17];
  __shared__ double yv[16 * kTailMaxT], xv[16 * kTailMaxT];
  __shared__ f64x4 Lsub[64];  // L(J1, J0) in operand order (waves 1..3 update their J1 tiles with it)
  __shared__ int fail_s, wready[2], lready;
  const int n = 7 * A.nc;
  const TailSrc TS = tail_src(A, n);
  const int TC = (n + 15) / 16, TR = (n + 16) / 16;
  const int In = n / 16, rn = n - 16 * In;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  const int J0 = 2 * (int)blockIdx.x, jn = min(2, TC - J0), J1 = J0 + 1, Jl = J0 + jn - 1;
  const int want = S.epoch + 1;
  double *Wg = A.Wg;
  const __amdgpu_buffer_rsrc_t R = gran_rsrc(S.LgG);
  constexpr int kRC = RC;
  auto rowI = [&](int u) { return wave == 0 ? (u < jn ? J0 + u : -1) : Jl + wave + 3 * u; };
  auto live = [&](int u) {
    const int I = rowI(u);
    return I >= 0 && I < TR;
  };
  if (tid == 0) fail_s = 0, wready[0] = 0, wready[1] = 0, lready = 0;
  for (int q = tid; q < 16 * kTailMaxT; q += 64 * kTailNW) yv[q] = 0.0;
  __syncthreads();
  // acc0[u]: tile (I, J0)^T; acc1[u]: tile (I, J1)^T (rows I >= J1)
  f64x4 acc0[kRC], acc1[kRC];
#pragma unroll
  for (int u = 0; u < kRC; u++) {
    f64x4 v0 = {0.0, 0.0, 0.0, 0.0}, v1 = {0.0, 0.0, 0.0, 0.0};
    if (live(u)) {
      const int I = rowI(u);
#pragma unroll
      for (int r = 0; r < 4; r++) v0[r] = tail_entry(A, TS, n, 16 * I + lr, 16 * J0 + lk + 4 * r);
      if (jn == 2 && I >= J1) {
#pragma unroll
        for (int r = 0; r < 4; r++) v1[r] = tail_entry(A, TS, n, 16 * I + lr, 16 * J1 + lk + 4 * r);
      }
    }
    acc0[u] = v0;
    acc1[u] = v1;
  }
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
  auto mma = [&](f64x4 &acc, const f64x4 &key, const f64x4 &ri) {
#pragma unroll
    for (int q = 0; q < 4; q++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-key[q], ri[q], acc, 0, 0, 0);
  };
  if (wave == 0 && J0 > 0 && S.warm)
    tail_diag_warm(Wk[0], xv + 16 * J0, min(16, n - 16 * J0), In == J0 ? rn : -1, lane);
  f64x4 rk0_last = {0.0, 0.0, 0.0, 0.0}, rk1_last = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < J0; k++) {
    // the pair's two key tiles L(J0, k), L(J1, k): both loads in flight, one poll
    GranTile g0, g1;
    {
      int spins = 0;
      for (;;) {
        gran_load(R, tail_tile(J0, k), lane, g0);
        if (jn == 2) gran_load(R, tail_tile(J1, k), lane, g1);
        if (gran_ready(g0, want) && (jn < 2 || gran_ready(g1, want))) break;
        __builtin_amdgcn_s_sleep(1);
        if (++spins > kColSpins) {
          if (lane == 0) fail_s = 1;
          break;
        }
      }
    }
    const f64x4 rk0 = gran_val(g0);
    f64x4 rk1 = {0.0, 0.0, 0.0, 0.0};
    if (jn == 2) rk1 = gran_val(g1);
    if (wave == 0) {
      mma(acc0[0], rk0, rk0);
      if (jn == 2) {
        mma(acc0[1], rk0, rk1);
        mma(acc1[1], rk1, rk1);
      }
    } else if (k + 1 == J0) {
      rk0_last = rk0, rk1_last = rk1;
    } else {
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
            mma(acc0[u], rk0, ri);
            if (jn == 2) mma(acc1[u], rk1, ri);
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
  const __amdgpu_buffer_rsrc_t RT =
      __builtin_amdgcn_make_buffer_rsrc(S.LgT, 0, kTailMaxT * (kTailMaxT + 1) / 2 * 256 * 8, 0x00020000);
  // L(I, J) itself (A(I, J) W^T: operands swapped) for the back-substitution
  auto store_lgt = [&](int I, int J, const f64x4 &a, int slot) {
    f64x4 dt = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; q++) dt = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], Wk[slot][lr][4 * q + lk], dt, 0, 0, 0);
    const unsigned long long b0 = __double_as_longlong(dt[0]), b1 = __double_as_longlong(dt[1]),
                             b2 = __double_as_longlong(dt[2]), b3 = __double_as_longlong(dt[3]);
    const u32x4 w0 = {(unsigned)b0, (unsigned)(b0 >> 32), (unsigned)b1, (unsigned)(b1 >> 32)};
    const u32x4 w1 = {(unsigned)b2, (unsigned)(b2 >> 32), (unsigned)b3, (unsigned)(b3 >> 32)};
    const int off = (tail_tile(I, J) * 256 + 2 * lane) * 8;  // (halves of 1 KB: whole lines per store)
    __builtin_amdgcn_raw_buffer_store_b128(w0, RT, off, 0, 16);
    __builtin_amdgcn_raw_buffer_store_b128(w1, RT, off + 1024, 0, 16);
  };
  auto panel = [&](const f64x4 &a, int slot) {  // L(I, J)^T = W_J A(I, J)^T, operand order
    f64x4 d = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; q++) d = __builtin_amdgcn_mfma_f64_16x16x4f64(Wk[slot][lr][4 * q + lk], a[q], d, 0, 0, 0);
    return d;
  };
  auto wait_lds = [&](int *f) {
    int spins = 0;
    while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0 && spins < (1 << 20)) {
      __builtin_amdgcn_s_sleep(1);
      spins++;
    }
    if (spins >= (1 << 20) && lane == 0) fail_s = 1;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  };
  if (wave == 0) {
    // diagonal J0, then (jn == 2) the pair's sub-diagonal tile, the second
    // diagonal's update from it, the second diagonal
    if (tid == 0) M3S_CSTAMP(2, J0, 1);
    if (tid == 0) M3S_CSTAMP(2, 600 + J0, 0);
    if (tail_diag_mfma(acc0[0], Wk[0], yv + 16 * J0, min(16, n - 16 * J0), In == J0 ? rn : -1, lane) && lane == 0)
      fail_s = 1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) __hip_atomic_store(&wready[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (tid == 0) M3S_CSTAMP(2, J0, 2);
    if (jn == 2) {
      const f64x4 d = panel(acc0[1], 0);  // L(J1, J0)^T
      Lsub[lane] = d;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 0) __hip_atomic_store(&lready, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (J1 == In && lr == rn) {  // y' of column J0 from the RHS row
#pragma unroll
        for (int r = 0; r < 4; r++) st_sc1(S.ypg + 16 * J0 + lk + 4 * r, d[r]);
      }
      mma(acc1[1], d, d);
      if (tid == 0) M3S_CSTAMP(2, J1, 1);
      if (tid == 0) M3S_CSTAMP(2, 600 + J1, 0);
      if (tail_diag_mfma(acc1[1], Wk[1], yv + 16 * J1, min(16, n - 16 * J1), In == J1 ? rn : -1, lane) && lane == 0)
        fail_s = 1;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 0) __hip_atomic_store(&wready[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (tid == 0) M3S_CSTAMP(2, J1, 2);
    }
    // W^T of each column ([16][16] row-major: element e = 16 l + r holds
    // W[r][l]): four stores of 64 consecutive elements, whole lines each
    // (lane l storing its row of 16 was 16 partial-line write-through stores)
#pragma unroll
    for (int j = 0; j < jn; j++) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int e = 64 * i + lane;
        st_sc1(Wg + (size_t)(J0 + j) * 256 + e, Wk[j][e & 15][e >> 4]);
      }
      if (In == J0 + j && lane < 16) st_sc1(S.ypg + 16 * (J0 + j) + lane, yv[16 * (J0 + j) + lane]);
    }
    if (jn == 2) store_lgt(J1, J0, acc0[1], 0);
  } else {
    // The wave's first row first, on its own (in waves 1 and 2 it carries
    // the next pair's chain: its two tiles go out before any other work):
    // the deferred update from column J0 - 1 as its tile lands, the panel
    // tile L(I, J0), the update of (I, J1) from the pair's first column
    // (L(J1, J0) from wave 0), the panel tile L(I, J1), each handed off at
    // once. Then the other rows phase by phase, every row's MFMA chain of a
    // phase interleaved with the others' (one row at a time left each
    // row's ~12 dependent MFMAs and stores exposed: ~1.5 us per row,
    // profiles/r04/tail_stamps_pair_rows_fine.txt). Per tile the same
    // updates in the same order.
    if (lane == 0) M3S_CSTAMP(2, 1000 + 16 * J0 + 15, wave);
    auto deferred = [&](int u) {
      GranTile g;
      poll_tile(tail_tile(rowI(u), J0 - 1), g);
      const f64x4 ri = gran_val(g);
      mma(acc0[u], rk0_last, ri);
      if (jn == 2) mma(acc1[u], rk1_last, ri);
    };
    auto put_y = [&](int I, int J, const f64x4 &d) {  // y' of column J from the RHS row
      if (I == In && lr == rn) {
#pragma unroll
        for (int r = 0; r < 4; r++) st_sc1(S.ypg + 16 * J + lk + 4 * r, d[r]);
      }
    };
    f64x4 ls = {0.0, 0.0, 0.0, 0.0};
    if (live(0)) {
      const int I = rowI(0);
      if (J0 > 0) deferred(0);
      if (tid == 64) M3S_CSTAMP(2, 1300 + 16 * J0, 0);
      wait_lds(&wready[0]);
      const f64x4 d0 = panel(acc0[0], 0);
      gran_store(R, tail_tile(I, J0), lane, d0, want);
      if (tid == 64) M3S_CSTAMP(2, 1300 + 16 * J0, 1);
      put_y(I, J0, d0);
      if (jn == 2) {
        wait_lds(&lready);
        ls = Lsub[lane];
        mma(acc1[0], ls, d0);
        wait_lds(&wready[1]);
        const f64x4 d = panel(acc1[0], 1);
        gran_store(R, tail_tile(I, J1), lane, d, want);
        if (tid == 64) M3S_CSTAMP(2, 1300 + 16 * J0, 3);
        if (I == J1 + 1 && tid == 64) M3S_CSTAMP(2, J1, 0);
        put_y(I, J1, d);
      }
      if (lane == 0) M3S_CSTAMP(2, 1000 + 16 * J0, wave);
    }
    if (live(1)) {  // (rows are dealt in order: live(1) implies live(0))
      // the deferred update: every remaining row's tile in flight at once,
      // applied as they land
      if (J0 > 0) {
        unsigned pend = 0;
#pragma unroll
        for (int u = 1; u < kRC; u++)
          if (live(u)) pend |= 1u << u;
        int spins = 0;
        while (pend) {
          GranTile g[kRC];
#pragma unroll
          for (int u = 1; u < kRC; u++)
            if (pend & (1u << u)) gran_load(R, tail_tile(rowI(u), J0 - 1), lane, g[u]);
#pragma unroll
          for (int u = 1; u < kRC; u++) {
            if ((pend & (1u << u)) && gran_ready(g[u], want)) {
              const f64x4 ri = gran_val(g[u]);
              mma(acc0[u], rk0_last, ri);
              if (jn == 2) mma(acc1[u], rk1_last, ri);
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
      if (tid == 64) M3S_CSTAMP(2, 1300 + 16 * J0 + 1, 0);
      // (a wave whose row 0 is dead has no rows at all, so the flags below
      // were already seen by row 0)
      f64x4 d0[kRC];
#pragma unroll
      for (int u = 1; u < kRC; u++) {
        d0[u] = f64x4{0.0, 0.0, 0.0, 0.0};
        if (live(u)) d0[u] = panel(acc0[u], 0);
      }
#pragma unroll
      for (int u = 1; u < kRC; u++)
        if (live(u)) {
          gran_store(R, tail_tile(rowI(u), J0), lane, d0[u], want);
          put_y(rowI(u), J0, d0[u]);
        }
      if (tid == 64) M3S_CSTAMP(2, 1300 + 16 * J0 + 1, 1);
      if (jn == 2) {
#pragma unroll
        for (int u = 1; u < kRC; u++)
          if (live(u)) mma(acc1[u], ls, d0[u]);
        f64x4 d1[kRC];
#pragma unroll
        for (int u = 1; u < kRC; u++) {
          d1[u] = f64x4{0.0, 0.0, 0.0, 0.0};
          if (live(u)) d1[u] = panel(acc1[u], 1);
        }
#pragma unroll
        for (int u = 1; u < kRC; u++)
          if (live(u)) {
            gran_store(R, tail_tile(rowI(u), J1), lane, d1[u], want);
            put_y(rowI(u), J1, d1[u]);
          }
        if (tid == 64) M3S_CSTAMP(2, 1300 + 16 * J0 + 1, 3);
      }
      if (lane == 0) M3S_CSTAMP(2, 1000 + 16 * J0 + 1, wave);
    }
    // the L tiles for the back-substitution, after every hand-off
#pragma unroll
    for (int u = 0; u < kRC; u++) {
      const int I = rowI(u);
      if (live(u) && I < TC) {
        store_lgt(I, J0, acc0[u], 0);
        if (jn == 2) store_lgt(I, J1, acc1[u], 1);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every store of this wave has left
  __syncthreads();
  if (tid == 0) {
    if (fail_s) {  // out before the column flags (the back-substitution workers may finish the step early)
      __hip_atomic_store(A.flags + kFlagSplitFail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    for (int j = 0; j < jn; j++) __hip_atomic_store(S.tflag + J0 + j, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int j = 0; j < jn; j++) M3S_CSTAMP(2, J0 + j, 3);
  }
  if ((int)blockIdx.x != (G.X ? G.n_pairs : (int)gridDim.x) - 1) return;
  tail_backsub_wg(A, S, yv, xv);
  if (G.X) {  // x_t is out (plain stores): release, then the workers combine
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(G.xt_ready, S.epoch + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

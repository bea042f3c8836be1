// gn/dataflow.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The large graphs' factorisation over the chip: DfArgs, kDfWaves,
// df_factor_kernel, then col_finish (retraction and stop flag after a
// chip-wide solve) and col_backsub_kernel.
// Relies on gn/layout.h (kFlagStop, kFlagSplitFail), wave_sum_pl
// (gn/linearize.h), gn/llt_blocks.h (ld_sc1 / st_sc1, poll_b128, readlane_d,
// wave_lds_fence, kStageDoubles, the block operations through border_task)
// and gn/col_tasks.h (ColArgs, kColSpins, M3S_CSTAMP, set_fail, wave_gticket,
// wait_flags).

// ------------------------------------ wave-level dataflow factorisation --
// Large graphs: every block of the sparse columns' factor is its own work
// item on one wave, dispatched over the whole chip from one ticket counter in
// a topological order (level order; DIAG(k) before the OFF tasks of column k;
// the dense-tail border tasks last):
//   DIAG(k)    D_k - sum_p L_kp L_kp^T -> L_kk, W_k = L_kk^-1, y_k; waits for
//              the slots L_kp of its update list (dtr);
//   OFF(t)     L_ik = (A_ik - sum_p L_ip L_kp^T) W_k^T; waits for DIAG(k) and
//              the slots of its update list (tr_a / tr_b);
//   BORDER(b)  one dense-tail block minus its updates from the sparse columns
//              (and the tail RHS), written to the factor and densely for
//              tail_llt_kernel; waits for the slots of its update prefix.
// Every block slot has an epoch flag (diagonal slots = DIAG done, which also
// covers y_k); a finished block is published with write-through (sc1) stores
// drained before the flag, and read with sc1 loads. A wave waits only for
// items with smaller tickets (all dispatched to running waves earlier), so
// progress does not depend on residency. The columns' OFF tasks no longer
// queue behind one workgroup's 4 waves: the top of the elimination tree (33
// OFF blocks in one column at 256 KFs) runs its blocks side by side.
// (SimplicialLLT's factor, gn_kernels.cu:132-153.)
struct DfArgs {
  const int32_t *plan;
  int off[kPlanSections];
  const int32_t *items;  // dispatch list: -1-k DIAG(k), t < n_tasks OFF(t), n_tasks + b BORDER(b)
  int n_items, n_tasks, m, c0, nc, epoch;
  double *L, *Dinv, *y;
  int32_t *sdone;  // [S] slot epoch flags
  int32_t *ctr;    // ticket counter
  int32_t *flags;
  double *tail_A;
  int tail_ld;
  double *Wgr;     // [m][49] W_k as {value, epoch tag} 16-B granules (round 3)
};
constexpr int kDfWaves = 4;

__global__ void __launch_bounds__(64 * kDfWaves) df_factor_kernel(DfArgs D) {
  if (D.flags[kFlagStop]) return;
  __shared__ __attribute__((aligned(16))) double stage[kDfWaves][kStageDoubles];
  __shared__ double scratch[kDfWaves][64];
  __shared__ double Wsh[kDfWaves][49];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int32_t *pl = D.plan;
  const int32_t *dtr_ptr = pl + D.off[kSec_dtr_ptr], *dtr_slot = pl + D.off[kSec_dtr_slot],
                *dtr_p = pl + D.off[kSec_dtr_p], *task_dst = pl + D.off[kSec_task_dst],
                *task_col = pl + D.off[kSec_task_col], *task_tr_ptr = pl + D.off[kSec_task_tr_ptr],
                *tr_a = pl + D.off[kSec_tr_a], *tr_b = pl + D.off[kSec_tr_b];
  const int32_t *clq = pl + D.off[kSec_clq];
  const int r = lane / 7, c = lane % 7;
  const bool act49 = lane < 49;
  const int lane49 = act49 ? lane : 0, r7 = act49 ? r * 7 : 0, c7 = act49 ? c * 7 : 0;
  const int lane7 = lane < 7 ? lane : 0, l7 = lane7 * 7;
  double *stg = stage[wave], *scr = scratch[wave], *W = Wsh[wave];
  const int want = D.epoch + 1;
  // First round: wave g of the grid takes item g (no atomic: 1024 waves on
  // one counter cost ~10 us of arrival skew); later rounds draw tickets from
  // the counter. Every wave of this grid is resident at once (at most 1024
  // waves of 28 KB-LDS workgroups: >= 4 per CU), so a wave only ever waits
  // for items held by running waves. Draws per launch are fixed (the
  // successful ones plus one failing draw per wave that reaches the
  // counter), which gives the epoch base of the counter.
  const int nW = (int)gridDim.x * kDfWaves, gw = (int)blockIdx.x * kDfWaves + wave;
  const int draws = (D.n_items > nW ? D.n_items - nW : 0) + (D.n_items < nW ? D.n_items : nW);
  const int base = D.epoch * draws;
  double *L = D.L;
  const int BIG = 1 << 30;
  for (int round = 0;; round++) {
    const int t = round == 0 ? gw : nW + wave_gticket(D.ctr) - base;
    if (t >= D.n_items) break;
    const int code = D.items[t];
    if (code < 0) {  // DIAG(k)
      const int k = -1 - code;
      const int q0 = dtr_ptr[k], q1 = dtr_ptr[k + 1];
      if (lane == 0) M3S_CSTAMP(0, k, 0);
      double v = L[(size_t)k * 49 + lane49];  // assembled by the previous launch
      double bb = D.y[(size_t)k * 7 + lane7];
      bool ok = true;  // the update list is waited for batch by batch
      diag_updates_sc1(v, bb, L, dtr_slot, dtr_p, q0, q1, D.y, r7, c7, lane7, lane49, lane, stg, D.sdone, want, &ok);
      if (!ok && lane == 0) set_fail(D.flags);
      if (lane == 0) M3S_CSTAMP(0, k, 1);
      double wcol[7];
      if (diag_factor<true>(v, k, L, D.Dinv, scr, lane, l7, wcol) && lane == 0) set_fail(D.flags);
      fwd_solve_store<true>(bb, wcol, scr, D.y + (size_t)k * 7, lane);
      if (lane == 0) M3S_CSTAMP(0, k, 2);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_store(D.sdone + k, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (lane < 7) {
        // W_k as tagged granules (after the drain: an OFF item that sees a
        // tag also sees y_k and L_kk): entry qq * 7 + lane of Dinv[k]
        const __amdgpu_buffer_rsrc_t RG =
            __builtin_amdgcn_make_buffer_rsrc(D.Wgr, 0, (int)(16 * 49 * (D.m + 1)), 0x00020000);
#pragma unroll
        for (int qq = 0; qq < 7; qq++) {
          const unsigned long long bw = (unsigned long long)__double_as_longlong(wcol[qq]);
          const u32x4 gw = {(unsigned)(bw & 0xffffffffu), (unsigned)(bw >> 32), (unsigned)want, 0u};
          __builtin_amdgcn_raw_buffer_store_b128(gw, RG, (k * 49 + qq * 7 + lane) * 16, 0, 16);
        }
      }
      if (lane == 0) M3S_CSTAMP(0, k, 3);
    } else if (code < D.n_tasks) {  // OFF(t)
      const int dst = task_dst[code], k = task_col[code];
      const int q0 = task_tr_ptr[code], q1 = task_tr_ptr[code + 1];
      if (lane == 0) M3S_CSTAMP(3, dst, 0);
      // the update sum first (its blocks are usually final before DIAG(k)),
      // then DIAG(k)'s W_k
      bool ok = true;
      double v = L[(size_t)dst * 49 + lane49];
      v = sub_products<true, false, true>(v, L, tr_a, tr_b, q0, q1, r7, c7, lane49, lane, stg, D.sdone, want, &ok);
      if (lane == 0) M3S_CSTAMP(3, dst, 1);
      {  // W_k from its tagged granules: the poll and the payload are one load
        const __amdgpu_buffer_rsrc_t RG =
            __builtin_amdgcn_make_buffer_rsrc(D.Wgr, 0, (int)(16 * 49 * (D.m + 1)), 0x00020000);
        int spins = 0;
        for (;;) {
          const u32x4 g = poll_b128(RG, (k * 49 + lane49) * 16);
          if (__ballot(act49 && g.z != (unsigned)want) == 0) {
            if (act49) W[lane] = __longlong_as_double((long long)(((unsigned long long)g.y << 32) | g.x));
            break;
          }
          __builtin_amdgcn_s_sleep(1);
          if (++spins > kColSpins) {
            ok = false;
            break;
          }
        }
      }
      if (!ok && lane == 0) set_fail(D.flags);
      if (lane == 0) M3S_CSTAMP(3, dst, 2);
      if (act49) scr[lane] = v;
      wave_lds_fence();
      double x = 0.0;
#pragma unroll
      for (int mm = 0; mm < 7; mm++) x += scr[r7 + mm] * W[c7 + mm];
      if (act49) st_sc1(L + (size_t)dst * 49 + lane, x);
      wave_lds_fence();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_store(D.sdone + dst, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (lane == 0) M3S_CSTAMP(3, dst, 3);
    } else {  // BORDER(b): border_task over its update prefix (sc1 reads)
      const int bt = code - D.n_tasks, nc = D.nc;
      // the blocks of the update list waited for batch by batch, as they are
      // loaded (round 5: waiting for the whole list first put every product
      // of the tail border behind the last sparse level: ~20 us of the launch
      // at 256 KFs after the last column was published)
      bool ok = true;
      border_task<true, true>(bt, nc, D.c0, pl, D.off, L, D.y, r7, c7, lane49, lane, lane7, act49, stg, D.tail_A,
                              D.tail_ld, D.sdone, want, &ok);
      if (!ok && lane == 0) set_fail(D.flags);
    }
  }
}


// dx = -x (original order), retraction, ||dx|| test (one wave). x is read
// from C.y with plain loads: the acquire below makes every other workgroup's
// released x visible, whichever caller this is (the callers also acquire
// after their final ticket; a kernel boundary precedes the ncols == 0 call).
__device__ void col_finish(const ColArgs &C, int lane) {
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  __shared__ float dxs[7 * 512];
  const int32_t *perm = C.plan + C.off[kSec_perm];
  const int m = C.m;
  const bool failed =
      __hip_atomic_load(C.flags + kFlagSplitFail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
  if (failed) {
    for (int k = lane; k < 7 * m; k += 64) C.dx_out[k] = 0.0f;
    if (lane == 0) {
      C.flags[kFlagSplitFail] = 0;
      C.info[M3S_INFO_ITERS] += 1;
      C.info[M3S_INFO_SOLVE_FAIL] += 1;
      if (0.0f < C.delta_thresh) {
        C.info[M3S_INFO_CONVERGED] = 1;
        C.flags[kFlagStop] = 1;
      }
    }
    return;
  }
  // the poses this wave retracts, all in flight now (clamped indices, no
  // guards: a guarded load per pose was one dependent round trip each, round 5)
  // every x_k was published before this workgroup's ticket and the caller's
  // agent-scope acquire: plain loads, all in flight at once (one relaxed
  // atomic load per entry was one dependent fabric round trip each: ~28 per
  // lane at 256 KFs, ~10 us of the kernel, round 5)
  float part = 0.0f;
  constexpr int kFinB = 8;
  for (int i0 = 0; i0 < 7 * m; i0 += 64 * kFinB) {
    double xv[kFinB];
#pragma unroll
    for (int u = 0; u < kFinB; u++) {
      const int idx = i0 + 64 * u + lane;
      xv[u] = idx < 7 * m ? C.y[idx] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kFinB; u++) {
      const int idx = i0 + 64 * u + lane;
      if (idx < 7 * m) {
        const int vn = idx / 7, q = idx - 7 * vn;
        const int vo = perm[vn];
        const float v = -(float)xv[u];
        C.dx_out[vo * 7 + q] = v;
        dxs[vo * 7 + q] = v;
        part += v * v;
      }
    }
  }
  part = wave_sum_pl(part);
  wave_lds_fence();
  for (int p = lane; p < m; p += 64) {
    const Sim3f T = load_sim3(C.Twc + 8 * (size_t)(p + 1));
    float xi[7];
#pragma unroll
    for (int q = 0; q < 7; q++) xi[q] = dxs[p * 7 + q];
    store_sim3(C.Twc + 8 * (size_t)(p + 1), retract_f64(xi, T));
  }
  if (lane == 0) {
    C.info[M3S_INFO_ITERS] += 1;
    if (sqrtf(part) < C.delta_thresh) {
      C.info[M3S_INFO_CONVERGED] = 1;
      C.flags[kFlagStop] = 1;
    }
  }
}

constexpr int kBsCap = 40;  // L_ik blocks of a column prefetched into LDS (the rest staged)
__global__ void __launch_bounds__(64) col_backsub_kernel(ColArgs C) {
  if (C.flags[kFlagStop]) return;
  __shared__ __attribute__((aligned(16))) double stage[kStageDoubles];
  __shared__ double Lst[kBsCap * 49], xst[kBsCap * 7];
  const int lane = threadIdx.x;
  const int32_t *pl = C.plan;
  const int32_t *col_ptr = pl + C.off[kSec_col_ptr], *col_row = pl + C.off[kSec_col_row],
                *col_slot = pl + C.off[kSec_col_slot], *corder = pl + C.off[kSec_corder];
  const int lane7 = lane < 7 ? lane : 0;
  const int lane49 = lane < 49 ? lane : 0;
  const int base = C.epoch * (C.ncols + (int)gridDim.x);
  if (C.ncols == 0) {  // no sparse columns: the tail kernel solved everything
    if (blockIdx.x == 0) col_finish(C, lane);
    return;
  }
  for (;;) {
    const int t = wave_gticket(C.ctr + 1) - base;
    if (t >= C.ncols) break;
    const int k = corder[C.ncols - 1 - t];
    const int q0 = col_ptr[k], q1 = col_ptr[k + 1];
    if (lane == 0) M3S_CSTAMP(1, k, 0);
    // the factor is final (earlier launches): its blocks L_ik of this column
    // and W_k are fetched BEFORE waiting, so only the x_i hand-off is left on
    // the critical path
    const int npre = (q1 - q0 < kBsCap) ? q1 - q0 : kBsCap;
    for (int bq = 0; bq < npre; bq++)
      if (lane < 49) Lst[bq * 49 + lane] = C.L[(size_t)col_slot[q0 + bq] * 49 + lane];
    double wk[7];
#pragma unroll
    for (int mm = 0; mm < 7; mm++) wk[mm] = C.Dinv[(size_t)k * 49 + mm * 7 + lane7];
    double rr = C.y[(size_t)k * 7 + lane7];
    if (!wait_flags(C.done2, col_row, q0, q1, C.c0, C.epoch + 1, lane) && lane == 0) set_fail(C.flags);
    if (lane == 0) M3S_CSTAMP(1, k, 1);
    for (int idx = lane; idx < 7 * npre; idx += 64) {
      const int bq = idx / 7;
      xst[idx] = ld_sc1(C.y + (size_t)col_row[q0 + bq] * 7 + (idx - 7 * bq));
    }
    wave_lds_fence();
    for (int bq = 0; bq < npre; bq++) {  // sub_matvec<TRANS>'s per-block sums, same order
      double t0 = 0.0;
#pragma unroll
      for (int mm = 0; mm < 7; mm++) t0 += Lst[bq * 49 + mm * 7 + lane7] * xst[bq * 7 + mm];
      rr -= t0;
    }
    wave_lds_fence();
    rr = sub_matvec<true, true, true>(rr, C.L, col_slot, col_row, q0 + npre, q1, C.y, lane7, lane49, lane, stage);
    double xk = 0.0;
#pragma unroll
    for (int mm = 0; mm < 7; mm++) xk += wk[mm] * readlane_d(rr, mm);
    if (lane < 7) st_sc1(C.y + (size_t)k * 7 + lane, xk);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_store(C.done2 + k, C.epoch + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lane == 0) M3S_CSTAMP(1, k, 2);
    // the workgroup that finishes the last column finishes the step
    const int fin = wave_gticket(C.ctr + 2);
    if (fin - C.epoch * C.ncols == C.ncols - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      col_finish(C, lane);
    }
  }
}

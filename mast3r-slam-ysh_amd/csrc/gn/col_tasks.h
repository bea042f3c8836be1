// gn/col_tasks.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The chip-wide solvers' common ground: ColArgs, kColSpins, the
// M3S_COL_STAMPS stamps (M3S_CSTAMP), set_fail, wave_gticket, wait_flags,
// and, in the test build only (-DM3S_TEST_PATHS), col_factor_kernel, the A/B
// reference of df_factor_kernel.
// Relies on gn/layout.h (kFlagStop, kFlagSplitFail) and gn/llt_blocks.h
// (st_sc1, wave_lds_fence, kStageDoubles, sub_products, sub_matvec,
// diag_factor, fwd_solve_store).

// ------------------------------------- column tasks over many workgroups --
// Large graphs (factor in global memory): the sparse columns of the
// elimination tree below the dense tail are factored as column tasks spread
// over the chip instead of as dataflow items on one workgroup's 16 waves. A
// task is column k: DIAG (D_k - sum_p L_kp L_kp^T -> L_kk, W_k = L_kk^-1, the
// forward step y_k) on wave 0, then its OFF blocks L_ik = (A_ik - sum_p L_ip
// L_kp^T) W_k^T on all 4 waves. Column k reads exactly the columns p with
// L_kp != 0 (its dtr list), all earlier in the level-order dispatch list, so
// a workgroup waits only for tasks running workgroups drew before it
// (progress does not depend on co-residency). Hand-off: sc1 stores drained
// before the column's flag, sc1 loads after polling it. Flags and tickets
// carry an epoch (solve launch count since m3s_gn_prepare zeroed them):
// nothing is reset between launches. col_backsub_kernel runs the tasks in
// reverse (x_k = W_k^T (y_k - sum_i L_ik^T x_i)) and the workgroup that
// finishes the last column writes dx, retracts and tests ||dx||.
// (Eigen SimplicialLLT factor + solve, gn_kernels.cu:132-153, with the
// reference's dx = 0 on failure and pose_retr_kernel :415-453.)
struct ColArgs {
  const int32_t *plan;
  int off[kPlanSections];
  int m, c0, ncols, epoch;  // ncols = c0 sparse columns (corder)
  double *L, *Dinv, *y;     // factor slots, W_k, RHS [m][7] (x after the back-substitution)
  int32_t *done, *done2;    // [m] epoch flags: column factored / x_k final
  int32_t *ctr;             // [0] factor ticket, [1] back-substitution ticket, [2] columns finished
  int32_t *flags;
  int32_t *info;
  float *Twc, *dx_out;
  int64_t N;
  float delta_thresh;
};
constexpr int kColSpins = 1 << 20;  // bounded waits: a plan bug becomes a solve failure, never a hang
#ifdef M3S_COL_STAMPS  // per-column wall-clock stamps (tools/col_stamps.py)
__device__ int64_t g_col_stamp[4][2048][4];
#define M3S_CSTAMP(ph, k, i)                                \
  do {                                                      \
    if ((k) < 2048) g_col_stamp[ph][k][i] = wall_clock64(); \
  } while (0)
#else
#define M3S_CSTAMP(ph, k, i) \
  do {                       \
  } while (0)
#endif
__device__ __forceinline__ void set_fail(int32_t *flags) {
  __hip_atomic_store(flags + kFlagSplitFail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// wave-uniform global ticket: the first active lane adds 64 and its old value
// / 64 is the ticket. Explicit rather than "every lane adds 1": that form is
// one add of 64 only when the atomic optimizer folds it, which needs the
// counter's address provably uniform; a pointer loaded through a reference in
// a non-inlined function (gcol_worker, round 5) got 64 per-lane adds
// interleaved with other waves' and duplicate tickets.
__device__ __forceinline__ int wave_gticket(int32_t *ctr) {
  const uint64_t ex = __builtin_amdgcn_read_exec();
  const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  int o = 0;
  if (lane == __builtin_ctzll(ex)) o = __hip_atomic_fetch_add(ctr, 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __builtin_amdgcn_readfirstlane(o) >> 6;
}

// wave-uniform wait until flag[idx[q]] == want for every q in [q0, q1) with
// idx[q] < lim (lanes poll 64 at a time, sc1 loads); false on timeout
__device__ __forceinline__ bool wait_flags(const int32_t *flag, const int32_t *idx, int q0, int q1, int lim, int want,
                                           int lane) {
  int spins = 0;
  for (int qb = q0; qb < q1; qb += 64) {
    const int q = qb + lane;
    const int i = q < q1 ? idx[q] : -1;
    for (;;) {
      const bool ok = i < 0 || i >= lim ||
                      __hip_atomic_load(flag + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == want;
      if (__ballot(!ok) == 0) break;
      __builtin_amdgcn_s_sleep(2);
      if (++spins > kColSpins) return false;
    }
  }
  return true;
}

#ifdef M3S_TEST_PATHS  // the column-task factor (A/B reference of df_factor_kernel)
__global__ void __launch_bounds__(256) col_factor_kernel(ColArgs C) {
  if (C.flags[kFlagStop]) return;
  __shared__ int tk_s;
  __shared__ double Wsh[49];
  __shared__ double scratch[4][64];
  __shared__ __attribute__((aligned(16))) double stage[4][kStageDoubles];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int32_t *pl = C.plan;
  const int32_t *col_ptr = pl + C.off[kSec_col_ptr], *dtr_ptr = pl + C.off[kSec_dtr_ptr],
                *dtr_slot = pl + C.off[kSec_dtr_slot], *dtr_p = pl + C.off[kSec_dtr_p],
                *task_dst = pl + C.off[kSec_task_dst], *task_tr_ptr = pl + C.off[kSec_task_tr_ptr],
                *tr_a = pl + C.off[kSec_tr_a], *tr_b = pl + C.off[kSec_tr_b], *corder = pl + C.off[kSec_corder],
                *ctask0 = pl + C.off[kSec_ctask0];
  const int r = lane / 7, c = lane % 7;
  const bool act49 = lane < 49;
  const int lane49 = act49 ? lane : 0, r7 = act49 ? r * 7 : 0, c7 = act49 ? c * 7 : 0;
  const int lane7 = lane < 7 ? lane : 0, l7 = lane7 * 7;
  double *stg = stage[wave], *scr = scratch[wave];
  const int base = C.epoch * (C.ncols + (int)gridDim.x);  // tickets drawn by earlier launches
  double *L = C.L;
  for (;;) {
    if (wave == 0) {
      const int t = wave_gticket(C.ctr + 0) - base;
      if (lane == 0) tk_s = t;
    }
    __syncthreads();
    const int t = tk_s;
    __syncthreads();
    if (t >= C.ncols) break;
    const int k = corder[t];
    const int q0 = dtr_ptr[k], q1 = dtr_ptr[k + 1];
    if (tid == 0) M3S_CSTAMP(0, k, 0);
    if (wave == 0) {
      if (!wait_flags(C.done, dtr_p, q0, q1, C.m, C.epoch + 1, lane) && lane == 0) set_fail(C.flags);
      if (lane == 0) M3S_CSTAMP(0, k, 1);
      // DIAG(k): the assembled D_k (previous launch: plain load) minus the
      // updates from the columns p (this launch: sc1)
      double v = L[(size_t)k * 49 + lane49];
      v = sub_products<true, true, true>(v, L, dtr_slot, dtr_slot, q0, q1, r7, c7, lane49, lane, stg);
      double wcol[7];
      if (diag_factor<true>(v, k, L, C.Dinv, scr, lane, l7, wcol, Wsh) && lane == 0) set_fail(C.flags);
      double bb = C.y[(size_t)k * 7 + lane7];
      bb = sub_matvec<true, false, true>(bb, L, dtr_slot, dtr_p, q0, q1, C.y, lane7, lane49, lane, stg);
      fwd_solve_store<true>(bb, wcol, scr, C.y + (size_t)k * 7, lane);
    }
    __syncthreads();  // W_k in LDS; the dependencies are final for every wave
    if (tid == 0) M3S_CSTAMP(0, k, 2);
    // OFF(i, k) for the |struct(k)| tasks of column k, one per wave
    const int tc0 = ctask0[k], ntask = col_ptr[k + 1] - col_ptr[k];
    for (int tt = wave; tt < ntask; tt += 4) {
      const int t2 = tc0 + tt, dst = task_dst[t2];
      double v = L[(size_t)dst * 49 + lane49];
      v = sub_products<true, false, true>(v, L, tr_a, tr_b, task_tr_ptr[t2], task_tr_ptr[t2 + 1], r7, c7, lane49,
                                          lane, stg);
      if (act49) scr[lane] = v;
      wave_lds_fence();
      double x = 0.0;
#pragma unroll
      for (int mm = 0; mm < 7; mm++) x += scr[r7 + mm] * Wsh[c7 + mm];
      if (act49) st_sc1(L + (size_t)dst * 49 + lane, x);
      wave_lds_fence();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every sc1 store of column k has left
    __syncthreads();
    if (tid == 0) __hip_atomic_store(C.done + k, C.epoch + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) M3S_CSTAMP(0, k, 3);
  }
}

#endif  // M3S_TEST_PATHS

// gn/sparse_llt.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The one-workgroup solver: the M3S_LLT_STAMPS stamps and
// sparse_llt_kernel<STORE, TAIL> (assembly, LLT, back-substitution,
// retraction, stop flag; it heads no rule line of its own: its section opens
// in gn/llt_blocks.h).
// Relies on gn/layout.h (kFlagStop, kFlagSplitFail), gn/linearize.h (kFin,
// wave_sum_pl, xr_dpp), fail_step (gn/assemble.h) and gn/llt_blocks.h
// (SparseDev, M3S_POLL, wait_flag, flag_set, wave_ticket, wave_lds_fence,
// readlane_d, kStageDoubles, M3S_TAIL_TR / _TC and the block operations).

#ifdef M3S_LLT_STAMPS  // per-item shader-clock stamps of sparse_llt_kernel<1> (tools/llt_stamps.py)
__device__ int64_t g_llt_stamp[2048][4];  // per dispatch slot: ticket, inputs summed, published, fwd done
__device__ int32_t g_llt_item[2048][2];   // item, wave
__device__ int64_t g_llt_phase[8];        // start, assembled, factored, back-substituted, end
#define M3S_LSTAMP(it, i) \
  if (STORE == 1 && lane == 0 && (it) < 2048) g_llt_stamp[it][i] = (int64_t)__builtin_readcyclecounter();
#define M3S_LPHASE(i) \
  if (STORE == 1 && tid == 0) g_llt_phase[i] = (int64_t)__builtin_readcyclecounter();
#else
#define M3S_LSTAMP(it, i)
#define M3S_LPHASE(i)
#endif

// STORE: 1 = factor, plan and flags in LDS (small graphs); 2 = factor and
// flags in LDS, plan in global memory; 0 = factor in global memory, flags and
// the per-wave stage areas in LDS (large graphs).
// TAIL: the phase-2 instance (tail factor and back-substitution only), with
// its own register budget (room for larger trailing-update tiles).
template <int STORE, bool TAIL = false>
__global__ void __launch_bounds__(1024) sparse_llt_kernel(SparseDev D) {
  if (D.flags[kFlagStop]) return;
  constexpr bool IN_LDS = STORE != 0;
  constexpr bool STAGE = STORE == 0;
  const int phase = TAIL ? 2 : STAGE ? D.phase : 0;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int fail_s, next_item, next_col, next_b0, next_tile;
  __shared__ float nrm[16];
  __shared__ double scratch[16][64];
  const int m = D.m, S = D.S;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  constexpr int NW = 16;
  M3S_LPHASE(0);
  double *Lb = IN_LDS ? smem : D.L;
  double *Di = IN_LDS ? smem + (size_t)S * 49 : D.Dinv;
  double *y = IN_LDS ? smem + (size_t)(S + m) * 49 : smem;
  int32_t *after_y = reinterpret_cast<int32_t *>(y + (size_t)m * 7);
  // index arrays: LDS copy (STORE 1) or global
  const int32_t *pl = STORE == 1 ? after_y : D.plan;
  const int32_t *perm = pl + D.off[kSec_perm], *col_ptr = pl + D.off[kSec_col_ptr],
                *col_row = pl + D.off[kSec_col_row], *col_slot = pl + D.off[kSec_col_slot],
                *lev_col = pl + D.off[kSec_lev_col], *dtr_ptr = pl + D.off[kSec_dtr_ptr],
                *dtr_slot = pl + D.off[kSec_dtr_slot], *dtr_p = pl + D.off[kSec_dtr_p],
                *task_dst = pl + D.off[kSec_task_dst], *task_col = pl + D.off[kSec_task_col],
                *task_tr_ptr = pl + D.off[kSec_task_tr_ptr], *tr_a = pl + D.off[kSec_tr_a],
                *tr_b = pl + D.off[kSec_tr_b], *asm_ptr = pl + D.off[kSec_asm_ptr],
                *asm_edge = pl + D.off[kSec_asm_edge], *g_ptr = pl + D.off[kSec_g_ptr],
                *g_edge = pl + D.off[kSec_g_edge], *wave_ptr = pl + D.off[kSec_wave_ptr],
                *witems = pl + D.off[kSec_witems], *part_q0 = pl + D.off[kSec_part_q0],
                *part_q1 = pl + D.off[kSec_part_q1], *part_tgt = pl + D.off[kSec_part_tgt],
                *dpart_ptr = pl + D.off[kSec_dpart_ptr], *opart_ptr = pl + D.off[kSec_opart_ptr];
  const int n_tasks = D.n_tasks;
  const bool split = D.n_parts > 0;
  // completion flags: sdone[slot] (factor block final; diagonal slot k also
  // means W_k final), ydone[k] (forward value y_k final), done2[k] (x_k final)
  int32_t *sdone = after_y + (STORE == 1 ? ((D.plan_len + 1) & ~1) : 0);
  int32_t *ydone = sdone + S;
  int32_t *done2 = ydone + m;
  int32_t *pdone = done2 + m;  // PART items
  const int n_flags = S + 2 * m + D.n_parts;
  double *stg = reinterpret_cast<double *>(sdone + ((n_flags + 1) & ~1)) + (size_t)wave * kStageDoubles;
  // the plan (STORE 1) and the per-edge blocks of the in-LDS assembly, every
  // load of both in flight at once (a loop of dependent load -> LDS store
  // rounds cost a memory latency each: ~5 us at C3)
  const bool asm_in = IN_LDS && D.asm_lds && phase != 2;
  const bool lazy_asm = asm_in && D.nc == 0 && phase == 0;
  double *fl = reinterpret_cast<double *>(sdone + ((n_flags + 1) & ~1));  // staged fin (asm_in)
  {
    // buffer loads: unconditional (an index past the end reads 0 with no
    // access), so all 12 of a round are in flight together; guarded pointer
    // loads compiled to one branch and one vmcnt(0) each (~5 us at C3)
    const int np_ = STORE == 1 ? D.plan_len : 0, nf_ = asm_in ? D.E * kFin : 0;
    const __amdgpu_buffer_rsrc_t Rpl = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t *>(D.plan), 0, 4 * np_, 0x00020000);
    const __amdgpu_buffer_rsrc_t Rfn = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(D.fin), 0, 8 * nf_, 0x00020000);
    for (int r = 0; r * 4096 < np_ || r * 8192 < nf_; r++) {
      int32_t pv[4];
      double fv[8];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int i = r * 4096 + u * 1024 + tid;
        pv[u] = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(Rpl, 4 * i, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int i = r * 8192 + u * 1024 + tid;
        fv[u] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(Rfn, 8 * i, 0, 0));
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int i = r * 4096 + u * 1024 + tid;
        if (i < np_) after_y[i] = pv[u];
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int i = r * 8192 + u * 1024 + tid;
        if (i < nf_) fl[i] = fv[u];
      }
    }
  }
  for (int q = tid; q < n_flags; q += 1024) sdone[q] = 0;
  __syncthreads();  // plan copy and fin staging complete
  const int r = lane / 7, c = lane % 7;
  const bool act49 = lane < 49;
  // clamped row offsets: lanes >= 49 (>= 7) load valid entries and discard them
  const int lane49 = act49 ? lane : 0, r7 = act49 ? r * 7 : 0, c7 = act49 ? c * 7 : 0;
  const int lane7 = lane < 7 ? lane : 0, l7 = lane7 * 7;
  double *scr = scratch[wave];
  // lazy assembly (lazy_asm): slot sl's entry lane49 / the RHS entry lane7 of
  // column k from the staged fin, the sums of the assembly loops below
  auto asm_slot = [&](int sl) {
    double v = 0.0;
    for (int q = asm_ptr[sl]; q < asm_ptr[sl + 1]; q++) v += fl[asm_edge[q] * kFin + lane49];
    return (sl < m) ? v : -v;
  };
  auto asm_rhs = [&](int k) {
    double v = 0.0;
    for (int q = g_ptr[k]; q < g_ptr[k + 1]; q++) {
      const int ent = g_edge[q];
      const double gj = fl[(ent >> 1) * kFin + 49 + lane7];
      v += (ent & 1) ? gj : -gj;
    }
    return v;
  };

  if (phase == 2) {  // after border_kernel: y and the failure flag from global memory
    for (int idx = tid; idx < m * 7; idx += 1024) y[idx] = D.rhs[idx];
    if (tid == 0) fail_s = D.flags[kFlagSplitFail], next_col = 0;
    __syncthreads();
  } else {
  // 0. assembly. LDS factor with room: the per-edge blocks (fin) are staged
  // in LDS with coalesced loads, then summed per slot in edge order (the sums
  // of assemble_slots_kernel); otherwise that kernel assembled into the global
  // factor array, copied in here.
  // lazy: no assembly phase; each DIAG / OFF item sums its own slot (and
  // DIAG(k) its RHS) from the staged fin when it starts, in the same order
  // (bitwise the same values), so the first items start right after the
  // staging (round 3; graphs without a dense tail, whose border tasks read
  // assembled slots)
  if (asm_in && !lazy_asm) {
    for (int idx = tid; idx < S * 49; idx += 1024) {
      const int sl = idx / 49, t = idx - sl * 49;
      double v = 0.0;
      for (int q = asm_ptr[sl]; q < asm_ptr[sl + 1]; q++) v += fl[asm_edge[q] * kFin + t];
      Lb[idx] = (sl < m) ? v : -v;
    }
    for (int idx = tid; idx < m * 7; idx += 1024) {
      const int vv = idx / 7, t = idx - vv * 7;
      double v = 0.0;
      for (int q = g_ptr[vv]; q < g_ptr[vv + 1]; q++) {
        const int ent = g_edge[q];
        const double gj = fl[(ent >> 1) * kFin + 49 + t];
        v += (ent & 1) ? gj : -gj;
      }
      y[idx] = v;
    }
  } else if (!asm_in) {
    if (IN_LDS)
      for (int idx = tid; idx < S * 49; idx += 1024) Lb[idx] = D.L[idx];
    for (int idx = tid; idx < m * 7; idx += 1024) y[idx] = D.rhs[idx];
  }
  if (tid == 0) fail_s = 0, next_item = 0, next_col = 0, next_b0 = 0;
  __syncthreads();
  M3S_LPHASE(1);
#if defined(M3S_LLT_EXIT) && M3S_LLT_EXIT == 1  // phase-timing builds only (tools/llt_phase_ab.py)
  return;
#endif

  // 1. factorisation + forward substitution as a dataflow over work items:
  // DIAG(k) (diagonal block and W_k = L_kk^-1, then the forward step of y_k),
  // OFF(i,k) (one off-diagonal block) and, for global factors, PART items
  // (the head of a long update list, summed early into a partial block). The
  // host list-schedules the items onto the 16 waves (m3s_symbolic.cpp,
  // schedule_items); each item waits on LDS completion flags of exactly the
  // blocks it reads and publishes its own. No workgroup barriers inside the
  // factorisation; the schedule's assignment order guarantees progress.
  const int n_disp = wave_ptr[1];
  for (;;) {
    // dynamic dispatch: the next item of the (topological) dispatch list
    const int it = wave_ticket(&next_item);
    if (it >= n_disp) break;
    const int item = witems[it];
    M3S_LSTAMP(it, 0);
#ifdef M3S_LLT_STAMPS
    if (STORE == 1 && lane == 0 && it < 2048) g_llt_item[it][0] = item, g_llt_item[it][1] = wave;
#endif
    if (item >= n_tasks) {  // PART: partial sum of the head of a long update list
      const int pi = item - n_tasks, tg = part_tgt[pi];
      const int q0 = part_q0[pi], q1 = part_q1[pi];
      double v, bp = 0.0;
      v = 0.0;
      if (tg < 0) {  // of DIAG(k): sum L_kp L_kp^T and sum L_kp y_p
        M3S_POLL(q0, q1, flag_set(&sdone[dtr_slot[q]]), (v = sub_products<STAGE, true>(v, Lb, dtr_slot, dtr_slot, qa, qb, r7, c7, lane49, lane, stg)));
        M3S_POLL(q0, q1, flag_set(&ydone[dtr_p[q]]), (bp = sub_matvec<STAGE, false>(bp, Lb, dtr_slot, dtr_p, qa, qb, y, lane7, lane49, lane, stg)));
      } else {  // of OFF(t): sum L_ip L_kp^T
        M3S_POLL(q0, q1, flag_set(&sdone[tr_a[q]]) && flag_set(&sdone[tr_b[q]]), (v = sub_products<STAGE, false>(v, Lb, tr_a, tr_b, qa, qb, r7, c7, lane49, lane, stg)));
      }
      double *pb = D.parts + (size_t)pi * 56;
      if (act49) pb[lane] = v;
      if (lane < 7) pb[49 + lane] = bp;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 0) __hip_atomic_store(&pdone[pi], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if (item < 0) {  // DIAG(k): D_k - sum_p L_kp L_kp^T -> L_kk, W_k; then y_k
      const int k = -1 - item;
      const int p0 = split ? dpart_ptr[k] : 0, p1 = split ? dpart_ptr[k + 1] : 0;
      const int q0 = (p1 > p0) ? part_q1[p1 - 1] : dtr_ptr[k], q1 = dtr_ptr[k + 1];
      for (int pi = p0; pi < p1; pi++) wait_flag(&pdone[pi], &fail_s);
      double v = lazy_asm ? asm_slot(k) : Lb[(size_t)k * 49 + lane49];
      for (int pi = p0; pi < p1; pi++) v += D.parts[(size_t)pi * 56 + lane49];
      M3S_POLL(q0, q1, flag_set(&sdone[dtr_slot[q]]), (v = sub_products<STAGE, true>(v, Lb, dtr_slot, dtr_slot, qa, qb, r7, c7, lane49, lane, stg)));
      M3S_LSTAMP(it, 1);
      double wcol[7];
      const bool bad = diag_factor<false, true>(v, k, Lb, Di, scr, lane, l7, wcol);
      if (bad && lane == 0) fail_s = 1;  // still published: no waiter hangs
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 0) __hip_atomic_store(&sdone[k], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      M3S_LSTAMP(it, 2);
      // forward step, off the factorisation's critical path:
      // y_k = L_kk^-1 (b_k - sum_p L_kp y_p)
      double bb = lazy_asm ? asm_rhs(k) : y[k * 7 + lane7];
      for (int pi = p0; pi < p1; pi++) bb += D.parts[(size_t)pi * 56 + 49 + lane7];
      M3S_POLL(q0, q1, flag_set(&ydone[dtr_p[q]]), (bb = sub_matvec<STAGE, false>(bb, Lb, dtr_slot, dtr_p, qa, qb, y, lane7, lane49, lane, stg)));
      fwd_solve_store(bb, wcol, scr, y + (size_t)k * 7, lane);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 0) __hip_atomic_store(&ydone[k], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      M3S_LSTAMP(it, 3);
    } else {  // OFF: L_ik = (A_ik - sum_p L_ip L_kp^T) W_k^T
      const int t2 = item;
      const int dst = task_dst[t2], k = task_col[t2];
      const int p0 = split ? opart_ptr[t2] : 0, p1 = split ? opart_ptr[t2 + 1] : 0;
      const int q0 = (p1 > p0) ? part_q1[p1 - 1] : task_tr_ptr[t2], q1 = task_tr_ptr[t2 + 1];
      // the updates first (their inputs L_ip, L_kp are older than DIAG(k)),
      // so only the W_k product waits for DIAG(k)
      for (int pi = p0; pi < p1; pi++) wait_flag(&pdone[pi], &fail_s);
      double v = lazy_asm ? asm_slot(dst) : Lb[(size_t)dst * 49 + lane49];
      for (int pi = p0; pi < p1; pi++) v += D.parts[(size_t)pi * 56 + lane49];
      M3S_POLL(q0, q1, flag_set(&sdone[tr_a[q]]) && flag_set(&sdone[tr_b[q]]), (v = sub_products<STAGE, false>(v, Lb, tr_a, tr_b, qa, qb, r7, c7, lane49, lane, stg)));
      M3S_LSTAMP(it, 1);
      wait_flag(&sdone[k], &fail_s);  // W_k
      M3S_LSTAMP(it, 3);
      if (act49) scr[lane] = v;
      wave_lds_fence();
      double x = 0.0;
#pragma unroll
      for (int mm = 0; mm < 7; mm++) x += scr[r7 + mm] * Di[(size_t)k * 49 + c7 + mm];
      if (act49) Lb[(size_t)dst * 49 + lane] = x;
      wave_lds_fence();
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 0) __hip_atomic_store(&sdone[dst], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      M3S_LSTAMP(it, 2);
    }
  }
  __syncthreads();
  M3S_LPHASE(2);
#if defined(M3S_LLT_EXIT) && M3S_LLT_EXIT == 2
  return;
#endif

  if (phase == 1) {  // hand y and the failure flag to border_kernel / phase 2
    for (int idx = tid; idx < m * 7; idx += 1024) const_cast<double *>(D.rhs)[idx] = y[idx];
    if (tid == 0) D.flags[kFlagSplitFail] = fail_s;
    return;
  }
  }  // phase != 2

  // 1b. dense tail: the top clique of the elimination tree (nc columns from
  // c0 whose structure is every later column) factored right-looking,
  // bulk-synchronously, after the dataflow items (which cover columns < c0,
  // including the border blocks L_ik, i >= c0 > k, and all y_p, p < c0).
  if (D.nc > 0 && D.tail_done) {  // tail_llt_kernel solved the dense tail: y holds x there
    for (int q = tid; q < D.nc; q += 1024) done2[m - D.nc + q] = 1;
    __syncthreads();
  } else if (D.nc > 0) {
    const int32_t *clq = pl + D.off[kSec_clq];
    const int nc = clq[0], c0 = clq[1];
    const int32_t *ct0 = clq + 2, *bend = clq + 2 + nc;
    // B0: border updates (columns p < c0) of every tail block and tail RHS
    const int nt0 = nc * (nc + 1) / 2;
    for (; phase == 0;) {
      const int t = wave_ticket(&next_b0);
      if (t >= nt0) break;
      border_task<STAGE>(t, nc, c0, pl, D.off, Lb, y, r7, c7, lane49, lane, lane7, act49, stg);
    }
    __syncthreads();
    // B1: per tail column k: L_kk, W_k, y_k (one wave) | L_ik = A_ik W_k^T,
    // y_i -= L_ik y_k (a wave per row; global factors also copy column k into
    // an LDS panel) | A_ij -= L_ik L_jk^T (kTR x kTC block tiles per wave,
    // their loads in flight together). Tail slots are arithmetic: the
    // off-diagonal blocks of the tail are the last slots, column-major.
    const int cbase = S - nc * (nc - 1) / 2;
    double *panel = stg - (size_t)wave * kStageDoubles;  // the stage areas (global factors only)
    // diagonal block kk: L_kk, W_k, forward step y_k (wave 0)
    auto tail_diag = [&](int kk) {
      const double v = Lb[(size_t)kk * 49 + lane49];
      double wcol[7];
      const bool bad = diag_factor<false, true>(v, kk, Lb, Di, scr, lane, l7, wcol);
      if (bad && lane == 0) fail_s = 1;
      fwd_solve_store(y[kk * 7 + lane7], wcol, scr, y + (size_t)kk * 7, lane);
    };
    // look-ahead: DIAG(k+1) runs on wave 0 inside step k's trailing update,
    // right after its first tile (which holds block (k+1, k+1)), so each
    // column costs two workgroup barriers instead of three
    if (wave == 0) tail_diag(c0);
    __syncthreads();
    for (int ci = 0; ci < nc; ci++) {
      const int k = c0 + ci;
      const int col0 = cbase + ci * nc - ci * (ci + 1) / 2;  // slot of L_{k+1, k}
      const int nr = nc - ci - 1;
      for (int rr = wave; rr < nr; rr += NW) {
        const int dst = col0 + rr;
        const double av = Lb[(size_t)dst * 49 + lane49];
        if (act49) scr[lane] = av;
        wave_lds_fence();
        double x = 0.0;
#pragma unroll
        for (int mm = 0; mm < 7; mm++) x += scr[r7 + mm] * Di[(size_t)k * 49 + c7 + mm];
        wave_lds_fence();
        if (act49) {
          Lb[(size_t)dst * 49 + lane] = x, scr[lane] = x;
          if (STAGE) panel[rr * 49 + lane] = x;
        }
        wave_lds_fence();
        double yv = 0.0;
#pragma unroll
        for (int mm = 0; mm < 7; mm++) yv += scr[l7 + mm] * y[k * 7 + mm];
        if (lane < 7) y[(k + 1 + rr) * 7 + lane] -= yv;
        wave_lds_fence();
      }
      if (tid == 0) next_tile = 64;  // trailing tiles 1.. by ticket (tile 0: wave 0)
      __syncthreads();
      const double *Pk = STAGE ? panel : Lb + (size_t)col0 * 49;  // L_{k+1+rr, k} at Pk + 49 rr
      // trailing tiles of kTR block rows x kTC block columns (rr >= cc): each
      // panel row is read from LDS once per tile and used for every block of
      // the tile ((kTR + kTC) * 7 LDS reads per lane for kTR * kTC blocks
      // instead of 14 per block)
      constexpr int kTR = TAIL ? 2 : M3S_TAIL_TR, kTC = TAIL ? 2 : M3S_TAIL_TC,
                    kTB = kTR * kTC;
      const int nrt = (nr + kTR - 1) / kTR, nct = (nr + kTC - 1) / kTC;
      int ntile = 0;
      for (int ct = 0; ct < nct; ct++) ntile += nrt - ct * kTC / kTR;
      // tile 0 holds block (k+1, k+1): wave 0 takes it, then runs DIAG(k+1),
      // then joins the others on the ticketed remaining tiles
      for (int t = wave == 0 ? 0 : wave_ticket(&next_tile); t < ntile; t = wave_ticket(&next_tile)) {
        int ct = 0, rem = t;  // t -> (ct, rt), rt >= ct * kTC / kTR, column-major
        while (rem >= nrt - ct * kTC / kTR) rem -= nrt - ct * kTC / kTR, ct++;
        const int r_0 = kTR * (ct * kTC / kTR + rem), c_0 = kTC * ct;
        int sd[kTB];
#pragma unroll
        for (int q = 0; q < kTB; q++) {
          const int rr = r_0 + q / kTC, cc = c_0 + q % kTC, cj = ci + 1 + cc;
          // destination (k + 1 + rr, k + 1 + cc); outside the triangle: a valid
          // block is loaded (branch-free loads, all in flight) and not stored
          sd[q] = !(rr < nr && cc <= rr) ? k + 1
                  : (rr == cc) ? k + 1 + rr : cbase + cj * nc - cj * (cj + 1) / 2 + (rr - cc - 1);
        }
        double vd[kTB];
#pragma unroll
        for (int q = 0; q < kTB; q++) vd[q] = Lb[(size_t)sd[q] * 49 + lane49];
        double Bv[kTC][7];
#pragma unroll
        for (int bq = 0; bq < kTC; bq++) {
          const double *B = Pk + (size_t)min(c_0 + bq, nr - 1) * 49;
#pragma unroll
          for (int mm = 0; mm < 7; mm++) Bv[bq][mm] = B[c7 + mm];
        }
#pragma unroll
        for (int aq = 0; aq < kTR; aq++) {
          const double *A = Pk + (size_t)min(r_0 + aq, nr - 1) * 49;
          double sm[kTC];
#pragma unroll
          for (int bq = 0; bq < kTC; bq++) sm[bq] = 0.0;
#pragma unroll
          for (int mm = 0; mm < 7; mm++) {
            const double a = A[r7 + mm];
#pragma unroll
            for (int bq = 0; bq < kTC; bq++) sm[bq] += a * Bv[bq][mm];
          }
#pragma unroll
          for (int bq = 0; bq < kTC; bq++) vd[kTC * aq + bq] -= sm[bq];
        }
        if (act49) {
#pragma unroll
          for (int q = 0; q < kTB; q++)
            if (r_0 + q / kTC < nr && c_0 + q % kTC <= r_0 + q / kTC) Lb[(size_t)sd[q] * 49 + lane] = vd[q];
        }
        if (t == 0) {  // wave 0: block (k+1, k+1) is final (this tile, rr = cc = 0)
          wave_lds_fence();
          tail_diag(k + 1);
        }
      }
      __syncthreads();
    }
    // B2: back-substitution of the tail, x_k = W_k^T y_k (one wave), then
    // y_j -= L_kj^T x_k for the tail columns j < k (a wave per column)
    for (int ci = nc - 1; ci >= 0; ci--) {
      const int k = c0 + ci;
      if (wave == 0) {
        const double rr = y[k * 7 + lane7];
        double xk = 0.0;
#pragma unroll
        for (int mm = 0; mm < 7; mm++) xk += Di[(size_t)k * 49 + mm * 7 + lane7] * readlane_d(rr, mm);
        if (lane < 7) y[k * 7 + lane] = xk;
      }
      __syncthreads();
      for (int cj = wave; cj < ci; cj += NW) {
        const int blk = cbase + cj * nc - cj * (cj + 1) / 2 + (ci - cj - 1);  // L_{k, c0 + cj}
        double t = 0.0;
#pragma unroll
        for (int mm = 0; mm < 7; mm++) t += Lb[(size_t)blk * 49 + mm * 7 + lane7] * y[k * 7 + mm];
        if (lane < 7) y[(c0 + cj) * 7 + lane] -= t;
      }
      __syncthreads();
    }
    for (int q = tid; q < nc; q += 1024) done2[c0 + q] = 1;
    __syncthreads();
  }

  if (fail_s) {
    fail_step(7 * m, D.dx_out, D.info, D.flags + kFlagStop, D.delta_thresh);
    return;
  }

  // the retraction's pose of this thread, loaded now: its latency hides
  // behind the back-substitution
  Sim3f T_pre;
  if (tid < m) T_pre = load_sim3(D.Twc + 8 * (size_t)(tid + 1));

  // 2. back-substitution L^T x = y in reverse level order (x overwrites y).
  // Level-synchronous (round 5): the columns of one elimination-tree level
  // run side by side on the waves, a workgroup barrier between levels (every
  // row of struct(k) is an ancestor, at a higher level). The per-column sums
  // are the dataflow's (sub_matvec in list order): bitwise the same x. The
  // dataflow form paid a flag poll (s_sleep granularity), a release fence and
  // an LDS ticket per column on the chain: ~2k cycles per level at C3.
  // Round 5 (factor in LDS): a column on 56 lanes, lane 8a + b
  // holding term b of row a: every block's L_ik and x_i entry of the lane in
  // one LDS load each, all blocks' loads in flight, the products summed over
  // the blocks per lane, then over b by three DPP steps; W_k^T r the same way
  // through the wave's scratch. The 7-lane form ran each block as 7 dependent
  // LDS-operand FMAs and the W product as 7 readlane broadcasts (~2k cycles
  // per level at C3). Another summation order: x within fp64 round-off.
  if (!STAGE) {
    const int32_t *lev_ptr = pl + D.off[kSec_lev_ptr];
    const int a8 = lane >> 3, b8 = lane & 7;
    const bool act = a8 < 7 && b8 < 7;
    const int ac = a8 < 7 ? a8 : 6, bc = b8 < 7 ? b8 : 6;
    for (int L = D.levels - 1; L >= 0; L--) {
      for (int c = lev_ptr[L] + wave; c < lev_ptr[L + 1]; c += NW) {
        const int k = lev_col[c];
        if (k >= m - D.nc) continue;  // dense tail: done above
        const int q0 = col_ptr[k], q1 = col_ptr[k + 1];
        double s0 = 0.0, s1 = 0.0;
        int q = q0;
        for (; q + 1 < q1; q += 2) {  // (L_ik^T x_i)[a] = sum_b L_ik[b][a] x_i[b]
          const double l0 = Lb[(size_t)col_slot[q] * 49 + bc * 7 + ac], l1 = Lb[(size_t)col_slot[q + 1] * 49 + bc * 7 + ac];
          const double x0 = y[col_row[q] * 7 + bc], x1 = y[col_row[q + 1] * 7 + bc];
          s0 += l0 * x0;
          s1 += l1 * x1;
        }
        if (q < q1) s0 += Lb[(size_t)col_slot[q] * 49 + bc * 7 + ac] * y[col_row[q] * 7 + bc];
        double sm = act ? s0 + s1 : 0.0;
        sm += xr_dpp<0x141>(sm);  // over b: half-row mirror, then quad_perm xor 2, xor 1
        sm += xr_dpp<0x4E>(sm);
        sm += xr_dpp<0xB1>(sm);
        if (b8 == 0 && a8 < 7) scr[a8] = y[k * 7 + a8] - sm;
        wave_lds_fence();
        double t = act ? Di[(size_t)k * 49 + bc * 7 + ac] * scr[bc] : 0.0;  // x_k[a] = sum_b W_k[b][a] r[b]
        t += xr_dpp<0x141>(t);
        t += xr_dpp<0x4E>(t);
        t += xr_dpp<0xB1>(t);
        if (b8 == 0 && a8 < 7) y[k * 7 + a8] = t;
        wave_lds_fence();  // the scratch is read before the next column rewrites it
      }
      __syncthreads();
    }
  } else {
    const int32_t *lev_ptr = pl + D.off[kSec_lev_ptr];
    for (int L = D.levels - 1; L >= 0; L--) {
      for (int c = lev_ptr[L] + wave; c < lev_ptr[L + 1]; c += NW) {
        const int k = lev_col[c];
        if (k >= m - D.nc) continue;  // dense tail: done above
        double rr = y[k * 7 + lane7];
        rr = sub_matvec<STAGE, true>(rr, Lb, col_slot, col_row, col_ptr[k], col_ptr[k + 1], y, lane7, lane49, lane, stg);
        double xk = 0.0;
#pragma unroll
        for (int mm = 0; mm < 7; mm++) xk += Di[(size_t)k * 49 + mm * 7 + lane7] * readlane_d(rr, mm);
        if (lane < 7) y[k * 7 + lane] = xk;
      }
      __syncthreads();
    }
  }
  for (; false;) {
    const int t = wave_ticket(&next_col);
    if (t >= m) break;
    const int k = lev_col[m - 1 - t];
    if (k >= m - D.nc) continue;  // dense tail: done above
    const int q0 = col_ptr[k], q1 = col_ptr[k + 1];
    double rr = y[k * 7 + lane7];
    M3S_POLL(q0, q1, flag_set(&done2[col_row[q]]), (rr = sub_matvec<STAGE, true>(rr, Lb, col_slot, col_row, qa, qb, y, lane7, lane49, lane, stg)));
    double xk = 0.0;
#pragma unroll
    for (int mm = 0; mm < 7; mm++) {
      const double rm = readlane_d(rr, mm);
      xk += Di[(size_t)k * 49 + mm * 7 + lane7] * rm;
    }
    if (lane < 7) y[k * 7 + lane] = xk;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) __hip_atomic_store(&done2[k], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  M3S_LPHASE(3);

  // 3. dx = -x in the original variable order, retraction, ||dx||; dx also
  // to LDS (the per-wave scratch, free now) when it fits, so the retraction
  // reads it there instead of back from global memory
  float *dxl = reinterpret_cast<float *>(&scratch[0][0]);
  const bool dx_lds = m * 7 <= (int)(sizeof(scratch) / sizeof(float));
  float part = 0.0f;
  for (int idx = tid; idx < m * 7; idx += 1024) {
    const int vn = idx / 7, q = idx - vn * 7;
    const int vo = perm[vn];
    const float v = -(float)y[idx];
    D.dx_out[vo * 7 + q] = v;
    if (dx_lds) dxl[vo * 7 + q] = v;
    part += v * v;
  }
  part = wave_sum_pl(part);
  if (lane == 0) nrm[wave] = part;
  __syncthreads();  // dx_out (global) written by this block is visible to it now
  for (int p = tid; p < m; p += 1024) {
    const Sim3f T = p == tid ? T_pre : load_sim3(D.Twc + 8 * (size_t)(p + 1));
    float xi[7];
#pragma unroll
    for (int q = 0; q < 7; q++) xi[q] = dx_lds ? dxl[p * 7 + q] : D.dx_out[p * 7 + q];
    store_sim3(D.Twc + 8 * (size_t)(p + 1), retract_f64(xi, T));
  }
  if (tid == 0) {
    float s2 = 0.0f;
    for (int w2 = 0; w2 < NW; w2++) s2 += nrm[w2];
    D.info[M3S_INFO_ITERS] += 1;
    if (sqrtf(s2) < D.delta_thresh) {
      D.info[M3S_INFO_CONVERGED] = 1;
      D.flags[kFlagStop] = 1;
    }
  }
  M3S_LPHASE(4);
}

// gn/llt_blocks.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// What the block-sparse solvers are built from: the f64x4 typedef,
// finalize_edges_kernel, assemble_slots_kernel, SparseDev, the flag and poll
// primitives (readlane_d, rsqrt_nr, wait_flag, M3S_POLL, wave_ticket,
// flag_set, wave_lds_fence, ld_sc1 / st_sc1, poll_b128, wait_lanes), the
// stage sizes (kStage, kSplitUpdates, kStageDoubles, M3S_TAIL_TR / _TC) and
// the 7x7 block operations (sub_products, sub_matvec, diag_updates_sc1,
// diag_factor, fwd_solve_store, border_task).
// Relies on finalize_edge and kFin (gn/linearize.h) and the f32x4 / u32x4
// typedefs of m3s_gn.hip.

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------- block-sparse LLT ----
// Per edge: H_jj = M L M^T and g_j = M l in fp64 (M = Adj(T_i)^-T), written
// as fin[e][0:49] (row-major) and fin[e][49:56]. One 64-thread block per edge.
// The edge's local sums come from edge_sums, or (single-GPU path) straight
// from the linearize chunk partials, summed in fp64 in chunk order exactly as
// edge_reduce_kernel does.
__global__ void __launch_bounds__(64) finalize_edges_kernel(const double *__restrict__ edge_sums,
                                                            const float *__restrict__ partials,
                                                            int64_t chunks,
                                                            const int32_t *__restrict__ rank_i,
                                                            const float *__restrict__ Twc,
                                                            double *__restrict__ fin,
                                                            const int32_t *__restrict__ stop) {
  if (*stop) return;
  const int64_t e = blockIdx.x;
  const int t = threadIdx.x;
  __shared__ double esl[kNP];
  if (t < kNP) {
    double acc = 0.0;
    if (partials) {
      const float *p = partials + (size_t)e * chunks * kNP + t;
      for (int64_t c = 0; c < chunks; c++) acc += (double)p[(size_t)c * kNP];
    } else {
      acc = edge_sums[(size_t)e * kNP + t];
    }
    esl[t] = acc;
  }
  __syncthreads();
  finalize_edge(esl, Twc + 8 * (size_t)rank_i[e], fin + (size_t)e * kFin);
}

// Block-sparse assembly, one 64-thread block per factor slot (then one per
// free pose for the RHS): slot s = sum over its assembly edges, in edge order,
// of +H_jj (diagonal slots) or -H_jj (off-diagonal slots); rhs_v = sum of
// +-g_j. Written to the global factor array the LLT kernel starts from.
__global__ void __launch_bounds__(64) assemble_slots_kernel(const double *__restrict__ fin,
                                                            const int32_t *__restrict__ plan, int off_asm_ptr,
                                                            int off_asm_edge, int off_g_ptr, int off_g_edge,
                                                            int m, int S, double *__restrict__ L,
                                                            double *__restrict__ rhs,
                                                            const int32_t *__restrict__ stop) {
  if (*stop) return;
  const int b = blockIdx.x, t = threadIdx.x;
  if (b < S) {
    if (t >= 49) return;
    const int32_t *asm_ptr = plan + off_asm_ptr, *asm_edge = plan + off_asm_edge;
    double v = 0.0;
    for (int q = asm_ptr[b]; q < asm_ptr[b + 1]; q++) v += fin[(size_t)asm_edge[q] * kFin + t];
    L[(size_t)b * 49 + t] = (b < m) ? v : -v;
  } else {
    const int vv = b - S;
    if (t >= 7 || vv >= m) return;
    const int32_t *g_ptr = plan + off_g_ptr, *g_edge = plan + off_g_edge;
    double v = 0.0;
    for (int q = g_ptr[vv]; q < g_ptr[vv + 1]; q++) {
      const int ent = g_edge[q];
      const double gj = fin[(size_t)(ent >> 1) * kFin + 49 + t];
      v += (ent & 1) ? gj : -gj;
    }
    rhs[(size_t)vv * 7 + t] = v;
  }
}

struct SparseDev {
  const int32_t *plan;  // flattened plan (global); copied to LDS by the IN_LDS variant
  int plan_len;
  int off[kPlanSections];  // section offsets, indexed by kSec_<name> (m3s_symbolic.h)
  int m, S, levels, n_items;
  int n_tasks, n_parts;  // OFF tasks; PART items (0: no split updates)
  int E, asm_lds;        // asm_lds: assemble in-kernel from fin staged in LDS (else assemble_slots_kernel)
  int nc;                // dense-tail columns (m3s_symbolic.h, clq); 0: none
  double *parts;         // [n_parts][56] partial update blocks (+ partial RHS)
  int64_t *dbg;  // 0: per-column DIAG completion stamps
  double *L;     // [S][49] (global variant)
  double *Dinv;  // [m][49] (global variant)
  const double *fin;
  const double *rhs;  // assembled RHS [m][7] (assemble_slots_kernel)
  float *Twc;
  int64_t N;
  float *dx_out;
  int32_t *info;
  int32_t *flags;
  float delta_thresh;
  int tail_done;  // phase 2: the dense tail was solved by tail_llt_kernel (x_tail in rhs)
  double *tail_A;  // border_kernel: also write the bordered tail blocks densely here (or null)
  int tail_ld;
  int phase;  // global factors with a dense tail: 0 whole solve, 1 up to the
              // tail border, 2 from the tail factor (border_kernel between)
};

// Broadcast lane `l` (a compile-time / wave-uniform index) of a double:
// two v_readlane_b32, no LDS round trip.
__device__ __forceinline__ double readlane_d(double v, int l) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), l);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// 1/sqrt(d) for d > 0: hardware estimate + one Newton step, no IEEE
// division/sqrt sequences on the pivot chain. Measured on gfx950
// (tools/ubench_icache.hip, 16M inputs over 2^-30..2^30): v_rsq_f64 alone
// 5.2e-8 relative, one step 4.2e-15, two steps 3.0e-16; the factor's inputs
// are fp32 sums, so the second step (4 dependent fp64 ops per pivot on the
// DIAG chain) bought nothing measurable.
__device__ __forceinline__ double rsqrt_nr(double d) {
  double x = __builtin_amdgcn_rsq(d);
  const double hd = 0.5 * d;
  x = x * (1.5 - hd * x * x);
  return x;
}

// Wait (whole wave) for a workgroup-scope completion flag. Bounded: a schedule
// bug can never hang the GPU; it shows up as a solve failure instead.
__device__ __forceinline__ void wait_flag(int32_t *flag, int *fail) {
  int it = 0;
  while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0 && it < (1 << 21)) {
    __builtin_amdgcn_s_sleep(1);
    it++;
  }
  if (it >= (1 << 21)) {
    *fail = 1;
  }
}

// Dataflow over an update list [Q0, Q1): lane l polls the completion flag(s)
// of update q = q_ + l (READY, an expression in q, with acquire loads), the
// wave takes the ready prefix [qa, qb) and runs BODY on it, then polls the
// rest. The updates are applied as their inputs arrive, in list order (the
// sums are the same as waiting for all of them first), and one LDS round trip
// checks up to 64 flags. Bounded like wait_flag. (A macro: lambdas here leave
// a private segment behind.)
__device__ __forceinline__ int ready_prefix(bool ok, int q_, int q1) {
  const uint64_t nb = ~(uint64_t)__ballot(ok);
  const int n = nb ? __builtin_ctzll(nb) : 64;
  return n < q1 - q_ ? n : q1 - q_;
}
#define M3S_POLL(Q0, Q1, READY, BODY)                              \
  {                                                                \
    int q_ = (Q0), spins_ = 0;                                     \
    const int q1_ = (Q1);                                          \
    while (q_ < q1_) {                                             \
      const int q = q_ + lane;                                     \
      const int n_ = ready_prefix(q >= q1_ || (READY), q_, q1_);   \
      if (n_ == 0) {                                               \
        __builtin_amdgcn_s_sleep(1);                               \
        if (++spins_ >= (1 << 21)) {                               \
          fail_s = 1;                                              \
          break;                                                   \
        }                                                          \
        continue;                                                  \
      }                                                            \
      const int qa = q_, qb = q_ + n_;                             \
      BODY;                                                        \
      q_ = qb;                                                     \
    }                                                              \
  }

// Wave-uniform ticket from an LDS counter: every lane adds 1 (the atomic
// optimizer folds this into one ds_add of the active-lane count) and lane 0's
// old value / 64 is the ticket (whole waves only). A lane-0-only atomic
// followed by a broadcast (readfirstlane or an LDS slot) hung the dataflow
// waits behind it on gfx950 / ROCm 7.2; this form does not.
__device__ __forceinline__ int wave_ticket(int *ctr) {
  const int o = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  return __builtin_amdgcn_readfirstlane(o) >> 6;
}

__device__ __forceinline__ bool flag_set(int32_t *flag) {
  return __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != 0;
}

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One 1024-thread workgroup: assemble -> left-looking block LLT by elimination-
// tree level (phase A: diagonal blocks + RHS; phase B: off-diagonal blocks) ->
// L^T x = y by levels in reverse -> dx, retraction, ||dx|| test.
// Layouts inside a wave: "entry" lanes 0..48 hold (r, c) = (lane / 7, lane % 7)
// of a 7x7 block (block GEMMs), "row" lanes 0..6 hold a whole row / column in
// registers (7x7 Cholesky, inverse, substitution) with v_readlane broadcasts.
// Block products of the left-looking updates. Entry layout: lane = 7r + c of
// a 7x7 block (lanes >= 49 compute discarded values on clamped indices).
// LDS-resident factors read the operand rows straight from LDS, two updates in
// flight. Global factors (large graphs) are staged: every lane loads its own
// entry of up to kStage blocks at once (one memory latency per batch), the
// wave parks them in its LDS stage area and the products run from LDS.
#ifndef M3S_STAGE
#define M3S_STAGE 8
#endif
#ifndef M3S_SPLIT_UPDATES
#define M3S_SPLIT_UPDATES 32
#endif
constexpr int kStage = M3S_STAGE;                  // updates per staged batch
constexpr int kSplitUpdates = M3S_SPLIT_UPDATES;   // updates per PART item (global factors)
constexpr int kStageDoubles = 2 * kStage * 49;  // per wave
#ifndef M3S_TAIL_TR  // dense-tail trailing update tile, in 7x7 blocks
#define M3S_TAIL_TR 2
#endif
#ifndef M3S_TAIL_TC
#define M3S_TAIL_TC 2
#endif

// Cross-workgroup hand-off of doubles (column-task kernels): write-through
// (sc1) stores drained before the flag, sc1 loads (L2 / fabric served, never a
// stale L1 line) after the flag (MI355X_MICROARCH.md, inter-workgroup
// visibility, R1 / R2 forms).
__device__ __forceinline__ double ld_sc1(const double *p) {
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(p),
                                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void st_sc1(double *p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), (unsigned long long)__double_as_longlong(v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// 16-B write-through store (global_store_dwordx4 ... sc1); the caller drains
// it with an explicit s_waitcnt vmcnt(0) before signalling
__device__ __forceinline__ void st_sc1_x4(float *p, f32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}
// Poll load of a tagged 16-B granule (write-through producer, sc1 load). The
// empty asm with a memory clobber in front of every copy of the load makes it
// a fresh read on every pass of its wait loop, whatever unrolling, peeling or
// loop-invariant motion does to the loop. The builtin alone is a read-only
// memory op that the compiler may hoist out of a loop that stores nothing:
// it did once the s_sleep was gone (round 4, profiles/r04/
// trk_ab_sleep0_INVALID.txt), and the aux "volatile" bit 31 does not stop
// that (round 5: the load still left the loop). tests/test_isa.py checks every
// poll loop of the library for its load.
#ifndef M3S_POLL_BARRIER  // 0: only for tests/test_isa.py's negative check (compile-only)
#define M3S_POLL_BARRIER 1
#endif
__device__ __forceinline__ u32x4 poll_b128(__amdgpu_buffer_rsrc_t R, int off) {
#if M3S_POLL_BARRIER
  asm volatile("" ::: "memory");
#endif
  return __builtin_amdgcn_raw_buffer_load_b128(R, off, 0, 16);
}
template <bool SC1>
__device__ __forceinline__ double ld_blk(const double *p) {
  if (SC1) return ld_sc1(p);
  return *p;
}
template <bool SC1>
__device__ __forceinline__ void st_blk(double *p, double v) {
  if (SC1) st_sc1(p, v);
  else *p = v;
}

// v -= sum_q A_q(r,:) . B_q(c,:)   (A_q = L[sa[q]], B_q = L[sb[q]], or B = A if SAME)
// Wait until flag[idx] == want on every active lane (idx per lane), with
// relaxed agent-scope (sc1) loads; bounded like wait_flags. false on timeout.
__device__ __forceinline__ bool wait_lanes(const int32_t *flag, int idx, bool active, int want) {
  int spins = 0;
  for (;;) {
    const bool ok = !active || __hip_atomic_load(flag + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == want;
    if (__ballot(!ok) == 0) return true;
    __builtin_amdgcn_s_sleep(2);
    if (++spins > (1 << 20)) return false;
  }
}

// wflag (staged sc1 path only): wait for each batch's blocks (flag[slot] ==
// want) just before loading them, so the sums of the blocks that are ready
// early run while the later ones are still being produced; *ok &= no timeout
// Slot / vector offsets of the LDS-resident update lists on the full-rate
// 24-bit multiply: the index load -> address -> block load chain of every
// update is on the factor's critical path, and v_mul_lo_u32 is quarter rate
// (slot < 2^24 / 49 for every plan this library builds)
// (inline asm: from __umul24 the compiler formed a mask and a v_mul_lo_u32
// of the 392-byte stride again)
__device__ __forceinline__ uint32_t vmul_u24(uint32_t k, uint32_t a) {
  uint32_t r;
  asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "s"(k), "v"(a));
  return r;
}
template <typename T>
__device__ __forceinline__ const T *blk49(const T *Lb, int s) {  // Lb + 49 s
  return reinterpret_cast<const T *>(reinterpret_cast<const char *>(Lb) + vmul_u24(49u * sizeof(T), (uint32_t)s));
}
template <typename T>
__device__ __forceinline__ const T *vec7(const T *y, int s) {  // y + 7 s
  return reinterpret_cast<const T *>(reinterpret_cast<const char *>(y) + vmul_u24(7u * sizeof(T), (uint32_t)s));
}
template <bool STAGE, bool SAME, bool SC1 = false>
__device__ __forceinline__ double sub_products(double v, const double *Lb, const int32_t *sa,
                                               const int32_t *sb, int q0, int q1, int r7, int c7,
                                               int lane49, int lane, double *stg, const int32_t *wflag = nullptr,
                                               int want = 0, bool *ok = nullptr) {
  if (!STAGE) {
    // four products at a time: their index and block loads in flight together
    // and four independent FMA chains; subtracted in list order (bitwise the
    // same sums as one at a time). C3's DIAG items sum ~10 products after
    // their pickup: ~250 cycles each one by one (round-4 LLT stamps)
    int q = q0;
    for (; q + 3 < q1; q += 4) {
      const double *A[4], *B[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        A[u] = blk49(Lb, sa[q + u]);
        B[u] = SAME ? A[u] : blk49(Lb, sb[q + u]);
      }
      double sx[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int mm = 0; mm < 7; mm++)
#pragma unroll
        for (int u = 0; u < 4; u++) sx[u] += A[u][r7 + mm] * B[u][c7 + mm];
#pragma unroll
      for (int u = 0; u < 4; u++) v -= sx[u];
    }
    for (; q + 1 < q1; q += 2) {
      const double *A0 = blk49(Lb, sa[q]), *A1 = blk49(Lb, sa[q + 1]);
      const double *B0 = SAME ? A0 : blk49(Lb, sb[q]), *B1 = SAME ? A1 : blk49(Lb, sb[q + 1]);
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int mm = 0; mm < 7; mm++) {
        s0 += A0[r7 + mm] * B0[c7 + mm];
        s1 += A1[r7 + mm] * B1[c7 + mm];
      }
      v -= s0;
      v -= s1;
    }
    if (q < q1) {
      const double *A0 = blk49(Lb, sa[q]), *B0 = SAME ? A0 : blk49(Lb, sb[q]);
      double s0 = 0.0;
#pragma unroll
      for (int mm = 0; mm < 7; mm++) s0 += A0[r7 + mm] * B0[c7 + mm];
      v -= s0;
    }
    return v;
  }
  double *SA = stg, *SB = SAME ? stg : stg + kStage * 49;
  // the list's slot indices, 64 at a time, one per lane (one load round
  // trip; then wave-uniform readlanes), so the block loads of a batch all
  // issue at once instead of each waiting behind its own index load
  int my_a = 0, my_b = 0;
  for (int q = q0; q < q1; q += kStage) {
    if (((q - q0) & 63) == 0) {
      my_a = q + lane < q1 ? sa[q + lane] : 0;
      if (!SAME) my_b = q + lane < q1 ? sb[q + lane] : 0;
    }
    const int nb = (q1 - q < kStage) ? q1 - q : kStage;
    if (wflag) {
      const int rel = lane - ((q - q0) & 63);
      const bool act = rel >= 0 && rel < nb;
      bool w = wait_lanes(wflag, my_a, act, want);
      if (!SAME) w &= wait_lanes(wflag, my_b, act, want);
      if (!w) *ok = false;
    }
    double va[kStage], vb[kStage];
#pragma unroll
    for (int bq = 0; bq < kStage; bq++) {
      if (bq < nb) {
        const int ia = __builtin_amdgcn_readlane(my_a, ((q - q0) & 63) + bq);
        va[bq] = ld_blk<SC1>(Lb + (size_t)ia * 49 + lane49);
        if (!SAME) {
          const int ib = __builtin_amdgcn_readlane(my_b, ((q - q0) & 63) + bq);
          vb[bq] = ld_blk<SC1>(Lb + (size_t)ib * 49 + lane49);
        }
      }
    }
    if (lane < 49) {
#pragma unroll
      for (int bq = 0; bq < kStage; bq++)
        if (bq < nb) {
          SA[bq * 49 + lane] = va[bq];
          if (!SAME) SB[bq * 49 + lane] = vb[bq];
        }
    }
    wave_lds_fence();
    for (int bq = 0; bq < nb; bq++) {
      double s0 = 0.0;
#pragma unroll
      for (int mm = 0; mm < 7; mm++) s0 += SA[bq * 49 + r7 + mm] * SB[bq * 49 + c7 + mm];
      v -= s0;
    }
    wave_lds_fence();
  }
  return v;
}

// Rows (lanes 0..6): acc -= sum_q op(A_q) y_{p_q}, op(A) = A (TRANS false:
// row l7 of A) or A^T (TRANS: column `lane` of A). y lives in LDS.
template <bool STAGE, bool TRANS, bool SC1 = false>
__device__ __forceinline__ double sub_matvec(double acc, const double *Lb, const int32_t *slot,
                                             const int32_t *vidx, int q0, int q1, const double *y,
                                             int lane7, int lane49, int lane, double *stg) {
  if (!STAGE) {
    int q = q0;
    for (; q + 3 < q1; q += 4) {  // (as sub_products: four in flight, subtracted in list order)
      const double *A[4], *yv[4];
#pragma unroll
      for (int u = 0; u < 4; u++) A[u] = blk49(Lb, slot[q + u]), yv[u] = vec7(y, vidx[q + u]);
      double tx[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int mm = 0; mm < 7; mm++)
#pragma unroll
        for (int u = 0; u < 4; u++) tx[u] += (TRANS ? A[u][mm * 7 + lane7] : A[u][lane7 * 7 + mm]) * yv[u][mm];
#pragma unroll
      for (int u = 0; u < 4; u++) acc -= tx[u];
    }
    for (; q < q1; q++) {
      const double *A = blk49(Lb, slot[q]);
      const double *yv = vec7(y, vidx[q]);
      double t0 = 0.0;
#pragma unroll
      for (int mm = 0; mm < 7; mm++) t0 += (TRANS ? A[mm * 7 + lane7] : A[lane7 * 7 + mm]) * yv[mm];
      acc -= t0;
    }
    return acc;
  }
  int my_s = 0, my_v = 0;  // list indices per lane, 64 at a time (see sub_products)
  for (int q = q0; q < q1; q += kStage) {
    if (((q - q0) & 63) == 0) {
      my_s = q + lane < q1 ? slot[q + lane] : 0;
      my_v = q + lane < q1 ? vidx[q + lane] : 0;
    }
    const int nb = (q1 - q < kStage) ? q1 - q : kStage;
    double va[kStage], vy[kStage];
#pragma unroll
    for (int bq = 0; bq < kStage; bq++)
      if (bq < nb) {
        const int is = __builtin_amdgcn_readlane(my_s, ((q - q0) & 63) + bq);
        va[bq] = ld_blk<SC1>(Lb + (size_t)is * 49 + lane49);
        if (SC1) vy[bq] = ld_sc1(y + (size_t)__builtin_amdgcn_readlane(my_v, ((q - q0) & 63) + bq) * 7 + lane7);
      }
    if (lane < 49) {
#pragma unroll
      for (int bq = 0; bq < kStage; bq++)
        if (bq < nb) stg[bq * 49 + lane] = va[bq];
    }
    if (SC1 && lane < 7) {
#pragma unroll
      for (int bq = 0; bq < kStage; bq++)
        if (bq < nb) stg[kStage * 49 + bq * 7 + lane] = vy[bq];
    }
    wave_lds_fence();
    for (int bq = 0; bq < nb; bq++) {
      const double *A = stg + bq * 49;
      const double *yv = SC1 ? stg + kStage * 49 + bq * 7 : y + (size_t)vidx[q + bq] * 7;
      double t0 = 0.0;
#pragma unroll
      for (int mm = 0; mm < 7; mm++) t0 += (TRANS ? A[mm * 7 + lane7] : A[lane7 * 7 + mm]) * yv[mm];
      acc -= t0;
    }
    wave_lds_fence();
  }
  return acc;
}

// DIAG(k)'s two update sums in one staged pass over its list (the blocks
// L_kp are loaded once for both): v -= sum_q L_q(r,:) . L_q(c,:) (entry
// layout) and bb -= sum_q L_q(l7,:) . y_{p_q} (row layout); per-block sums in
// sub_products / sub_matvec order (bitwise the same results). sc1 loads.
__device__ __forceinline__ void diag_updates_sc1(double &v, double &bb, const double *Lb, const int32_t *slot,
                                                 const int32_t *vidx, int q0, int q1, const double *y, int r7,
                                                 int c7, int lane7, int lane49, int lane, double *stg,
                                                 const int32_t *wflag, int want, bool *ok) {
  int my_s = 0, my_v = 0;  // list indices per lane, 64 at a time (see sub_products)
  for (int q = q0; q < q1; q += kStage) {
    if (((q - q0) & 63) == 0) {
      my_s = q + lane < q1 ? slot[q + lane] : 0;
      my_v = q + lane < q1 ? vidx[q + lane] : 0;
    }
    const int nb = (q1 - q < kStage) ? q1 - q : kStage;
    {  // this batch's blocks L_kp (y_p is stored before L_kp can exist)
      const int rel = lane - ((q - q0) & 63);
      if (!wait_lanes(wflag, my_s, rel >= 0 && rel < nb, want)) *ok = false;
    }
    double va[kStage], vy[kStage];
#pragma unroll
    for (int bq = 0; bq < kStage; bq++)
      if (bq < nb) {
        const int is = __builtin_amdgcn_readlane(my_s, ((q - q0) & 63) + bq);
        const int iv = __builtin_amdgcn_readlane(my_v, ((q - q0) & 63) + bq);
        va[bq] = ld_sc1(Lb + (size_t)is * 49 + lane49);
        vy[bq] = ld_sc1(y + (size_t)iv * 7 + lane7);
      }
    if (lane < 49) {
#pragma unroll
      for (int bq = 0; bq < kStage; bq++)
        if (bq < nb) stg[bq * 49 + lane] = va[bq];
    }
    if (lane < 7) {
#pragma unroll
      for (int bq = 0; bq < kStage; bq++)
        if (bq < nb) stg[kStage * 49 + bq * 7 + lane] = vy[bq];
    }
    wave_lds_fence();
    for (int bq = 0; bq < nb; bq++) {
      const double *A = stg + bq * 49;
      double s0 = 0.0;
#pragma unroll
      for (int mm = 0; mm < 7; mm++) s0 += A[r7 + mm] * A[c7 + mm];
      v -= s0;
      const double *yv = stg + kStage * 49 + bq * 7;
      double t0 = 0.0;
#pragma unroll
      for (int mm = 0; mm < 7; mm++) t0 += A[lane7 * 7 + mm] * yv[mm];
      bb -= t0;
    }
    wave_lds_fence();
  }
}

// One 1024-thread workgroup: assembly -> dataflow block LLT + forward
// substitution -> dataflow back-substitution -> dx, retraction, ||dx||.
// DIAG of one column: v (entry layout, lane = 7r + c) = D_k after all its
// updates -> L_kk (row-major, upper part 0) into Lb[k], W_k = L_kk^-1
// (row-major) into Di[k] (and Wl, if given); lane c < 7 keeps column c of W_k
// in wcol for the forward step. Returns true on a non-positive pivot.
template <bool SC1 = false, bool RL = false>
__device__ __forceinline__ bool diag_factor(double v, int k, double *Lb, double *Di, double *scr, int lane,
                                            int l7, double (&wcol)[7], double *Wl = nullptr) {
  // entry layout -> row layout through the wave's scratch
  if (lane < 49) scr[lane] = v;
  wave_lds_fence();
  double a[7];
#pragma unroll
  for (int qq = 0; qq < 7; qq++) a[qq] = scr[l7 + qq];
  wave_lds_fence();
  // One pass: right-looking Cholesky by rows (lane r holds row r) and, with
  // the same column of L (broadcast through the scratch), W = L^-1 by
  // columns (lane c holds column c): at step j, W[j][c] = s_j / L_jj is
  // final and s_r (r > j) loses L[r][j] W[j][c]. Column j is scaled on every
  // lane (lane j holds the pivot itself; the lanes above keep finite upper-
  // triangle values that are masked when L_kk is stored). No per-pair
  // readlanes, no second serial chain for W. RL: the column goes by
  // constant-lane readlanes instead (sparse_llt_kernel: its one workgroup
  // has the SIMDs to itself; in df_factor_kernel the readlanes contend with
  // the other waves' issue and the LDS broadcast measured faster).
  double sw[7];
#pragma unroll
  for (int r = 0; r < 7; r++) sw[r] = (r == lane) ? 1.0 : 0.0;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 7; j++) {
    const double d = readlane_d(a[j], j);
    bad |= !(d > 0.0);
    const double inv = rsqrt_nr(d);
    a[j] *= inv;
    wcol[j] = sw[j] * inv;
    if (RL) {
      // column j of L straight from its lanes (constant-lane readlanes): no
      // LDS round trip on the pivot chain
#pragma unroll
      for (int cc = j + 1; cc < 7; cc++) {
        const double lcj = readlane_d(a[j], cc);
        a[cc] -= a[j] * lcj;
        sw[cc] -= lcj * wcol[j];
      }
      continue;
    }
    if (lane < 7) scr[lane] = a[j];
    wave_lds_fence();
#pragma unroll
    for (int cc = j + 1; cc < 7; cc++) {
      const double lcj = scr[cc];
      a[cc] -= a[j] * lcj;
      sw[cc] -= lcj * wcol[j];
    }
    wave_lds_fence();
  }
  if (lane < 7) {
#pragma unroll
    for (int qq = 0; qq < 7; qq++) {
      st_blk<SC1>(Lb + (size_t)k * 49 + lane * 7 + qq, (qq <= lane) ? a[qq] : 0.0);  // row `lane` of L_kk
      st_blk<SC1>(Di + (size_t)k * 49 + qq * 7 + lane, wcol[qq]);                    // column `lane` of W
      if (Wl) Wl[qq * 7 + lane] = wcol[qq];
    }
  }
  return bad;
}

// y_k = W_k b (lane c < 7 holds b_c in bb and column c of W in wcol; the
// sums run over c in order), stored to yk_out[0..7)
template <bool SC1 = false>
__device__ __forceinline__ void fwd_solve_store(double bb, const double (&wcol)[7], double *scr, double *yk_out,
                                                int lane) {
  if (lane < 7) {
#pragma unroll
    for (int r = 0; r < 7; r++) scr[r * 7 + lane] = wcol[r] * bb;
  }
  wave_lds_fence();
  if (lane < 7) {
    double yo = 0.0;
#pragma unroll
    for (int c = 0; c < 7; c++) yo += scr[lane * 7 + c];
    st_blk<SC1>(yk_out + lane, yo);
  }
  wave_lds_fence();
}

// Border update of one dense-tail block (column-major task t over the nc x nc
// lower triangle): the updates from the sparse columns p < c0, and for a
// diagonal block also the tail RHS. Tasks are independent (used in
// sparse_llt_kernel and, spread over the chip, by border_kernel).
// wflag (df_factor_kernel, round 5): the update blocks are waited for batch by
// batch as sub_products loads them (slot flags == want), so the products of
// the early sparse columns run while the late ones are still being factored;
// y_p of a block L_kp is final once that block is (DIAG(p) precedes OFF(k, p))
template <bool STAGE, bool SC1 = false>
__device__ __forceinline__ void border_task(int t, int nc, int c0, const int32_t *pl, const int *off, double *Lb,
                                            double *y, int r7, int c7, int lane49, int lane, int lane7, bool act49,
                                            double *stg, double *Ad = nullptr, int ld = 0,
                                            const int32_t *wflag = nullptr, int want = 0, bool *ok = nullptr) {
  auto put = [&](double *p, double v) { *p = v; };
  const int32_t *dtr_ptr = pl + off[kSec_dtr_ptr], *dtr_slot = pl + off[kSec_dtr_slot], *dtr_p = pl + off[kSec_dtr_p],
                *task_dst = pl + off[kSec_task_dst], *task_tr_ptr = pl + off[kSec_task_tr_ptr],
                *tr_a = pl + off[kSec_tr_a], *tr_b = pl + off[kSec_tr_b];
  const int32_t *clq = pl + off[kSec_clq];
  const int32_t *ct0 = clq + 2, *bend = clq + 2 + nc;
  int ci = 0, rem = t;  // t -> (ci, ri), ci <= ri < nc, column-major
  while (rem >= nc - ci) rem -= nc - ci, ci++;
  const int ri = ci + rem, k = c0 + ci;
  if (ri == ci) {
    const int q0 = dtr_ptr[k], q1 = bend[ci * nc + ci];
    double v = Lb[(size_t)k * 49 + lane49];
    v = sub_products<STAGE, true, SC1>(v, Lb, dtr_slot, dtr_slot, q0, q1, r7, c7, lane49, lane, stg, wflag, want, ok);
    double bb = y[k * 7 + lane7];
    bb = sub_matvec<STAGE, false, SC1>(bb, Lb, dtr_slot, dtr_p, q0, q1, y, lane7, lane49, lane, stg);
    if (act49) put(Lb + (size_t)k * 49 + lane, v);
    if (lane < 7) put(y + k * 7 + lane, bb);
    if (Ad && act49) put(Ad + (size_t)(7 * ci + r7 / 7) * ld + 7 * ci + c7 / 7, v);
  } else {
    const int task = ct0[ci] + ri - ci - 1, dst = task_dst[task];
    const int q0 = task_tr_ptr[task], q1 = bend[ci * nc + ri];
    double v = Lb[(size_t)dst * 49 + lane49];
    v = sub_products<STAGE, false, SC1>(v, Lb, tr_a, tr_b, q0, q1, r7, c7, lane49, lane, stg, wflag, want, ok);
    if (act49) put(Lb + (size_t)dst * 49 + lane, v);
    if (Ad && act49) {  // the block and its transpose (tail_llt_kernel reads whole 16x16 tiles)
      put(Ad + (size_t)(7 * ri + r7 / 7) * ld + 7 * ci + c7 / 7, v);
      put(Ad + (size_t)(7 * ci + c7 / 7) * ld + 7 * ri + r7 / 7, v);
    }
  }
}

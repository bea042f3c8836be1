// gn/solve.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The solve of one GN iteration, by the plan's path (SolvePath, gn/plan.h): one
// builder per kernel argument struct (sparse_dev, col_args, df_args,
// tail_args, tail_sync, g_args), one launch function per path (solve_chip,
// solve_lds, solve_global, solve_dense: the first host mention of every
// solver kernel, in the order of the order rule), gn_solve_impl (what every
// path shares, then a switch on the path) and set_lds_attributes_once.
// Relies on every kernel part, gn/args.h, gn/knobs.h, gn/launch.h
// (launch_timed, g_slv_ext_ev), gn/plan.h and gn/iterate.h (which declares
// gn_solve_impl for gn_full).

// What the launch functions of one solve share: the call, its layout, the
// plan record and epoch copied from the registry, the stream, and the
// workspace sections most of them name (flags, column sync words, tail scratch).
struct SolveCall {
  const m3s_gn_args *a;
  const Layout &Ly;
  const PlanRecord &R;
  int epoch;
  hipStream_t st;
  void *ws;
  int32_t *flags, *cs;
  double *tail;
};
constexpr int kTailLd = 16 * kTailMaxT;  // leading dimension of the bordered dense tail

SparseDev sparse_dev(const SolveCall &V) {
  const PlanRecord &R = V.R;
  SparseDev D{};  // phase 0, no dense tail handed over
  D.plan = at<int32_t>(V.ws, V.Ly.plan);
  D.plan_len = R.plan_len;
  std::copy(R.off, R.off + kPlanSections, D.off);
  D.n_items = R.n_items;
  D.n_tasks = R.n_tasks;
  D.n_parts = R.n_parts;
  D.nc = R.nc;
  D.E = (int)V.a->E;
  D.asm_lds = R.asm_lds ? 1 : 0;
  D.parts = at<double>(V.ws, V.Ly.parts);
  D.dbg = at<int64_t>(V.ws, V.Ly.A);
  D.m = R.m;
  D.S = R.S;
  D.levels = R.levels;
  D.L = at<double>(V.ws, V.Ly.Lblk);
  D.rhs = at<double>(V.ws, V.Ly.rhs);
  D.Dinv = at<double>(V.ws, V.Ly.Dinv);
  D.fin = at<double>(V.ws, V.Ly.fin);
  D.Twc = V.a->Twc;
  D.N = V.a->N;
  D.dx_out = V.a->dx_out;
  D.info = V.a->info;
  D.flags = V.flags;
  D.delta_thresh = V.a->delta_thresh;
  return D;
}

ColArgs col_args(const SolveCall &V, const SparseDev &D) {
  const PlanRecord &R = V.R;
  ColArgs C;
  C.plan = D.plan;
  std::copy(R.off, R.off + kPlanSections, C.off);
  C.m = R.m;
  C.c0 = R.m - R.nc;
  C.ncols = C.c0;
  C.epoch = V.epoch;
  C.L = D.L;
  C.Dinv = D.Dinv;
  C.y = const_cast<double *>(D.rhs);
  C.done = V.cs;
  C.done2 = V.cs + (R.m + 1);
  C.ctr = V.cs + 2 * (R.m + 1);
  C.flags = D.flags;
  C.info = V.a->info;
  C.Twc = V.a->Twc;
  C.dx_out = V.a->dx_out;
  C.N = V.a->N;
  C.delta_thresh = V.a->delta_thresh;
  return C;
}

// every block of the sparse columns and the tail border: one wave-level dataflow
DfArgs df_args(const SolveCall &V, const ColArgs &C) {
  const PlanRecord &R = V.R;
  DfArgs F;
  F.plan = C.plan;
  std::copy(R.off, R.off + kPlanSections, F.off);
  F.items = C.plan + R.off_dfitems;
  F.n_items = R.n_dfitems;
  F.n_tasks = R.n_tasks;
  F.m = R.m;
  F.c0 = C.c0;
  F.nc = R.nc;
  F.epoch = V.epoch;
  F.L = C.L;
  F.Dinv = C.Dinv;
  F.y = C.y;
  F.sdone = V.cs + 2 * (R.m + 1) + 16;
  F.ctr = C.ctr + 3;
  F.flags = C.flags;
  F.tail_A = V.tail;
  F.tail_ld = kTailLd;
  F.Wgr = at<double>(V.ws, V.Ly.wgran);
  return F;
}

TailArgs tail_args(const SolveCall &V, const SparseDev &D) {
  TailArgs T;
  T.Ad = V.tail;
  T.ld = kTailLd;
  T.rhs = const_cast<double *>(D.rhs);
  T.Lg = V.tail + (size_t)kTailLd * kTailLd;
  T.Wg = T.Lg + (size_t)kTailMaxT * (kTailMaxT + 1) / 2 * 256;
  T.flags = D.flags;
  T.nc = V.R.nc;
  T.c0 = V.R.m - V.R.nc;
  return T;
}

TailSync tail_sync(const SolveCall &V, const TailArgs &T) {
  TailSync Y;
  Y.tflag = V.cs + 2 * (V.R.m + 1) + 16 + V.Ly.slot_cap;
  Y.epoch = V.epoch;
  Y.ypg = T.Wg + (size_t)kTailMaxT * 256;
  Y.LgT = Y.ypg + 16 * kTailMaxT;
  Y.LgG = V.tail + tail_gran_offset_doubles();
  Y.warm = tail_warm_knob() ? 1 : 0;
  return Y;
}

// the sparse back-substitution on extra workgroups of the tail's launch
// (gcol_worker); X stays null until solve_chip gives it workers
GArgs g_args(const SolveCall &V, const ColArgs &C, const TailSync &Y, int TC) {
  GArgs G{};
  G.n_pairs = (TC + 1) / 2;
  G.nx = ((1 + 7 * V.R.nc) + 7) / 8 * 8;
  G.task = C.ctr + 8, G.comb = C.ctr + 9, G.fin = C.ctr + 10, G.xt_ready = C.ctr + 11;
  G.cnt = Y.tflag + 2 * kTailMaxT;
  return G;
}

void launch_border(const SolveCall &V, const SparseDev &D) {
  const int nt0 = V.R.nc * (V.R.nc + 1) / 2;
  border_kernel<<<(nt0 + kBorderWaves - 1) / kBorderWaves, 64 * kBorderWaves,
                  kBorderWaves * kStageDoubles * sizeof(double), V.st>>>(D);
}

// column tasks over the chip -> tail border -> dense tail on the MFMA ->
// column back-substitution + step. df, tail_cyc and the non-shaping knobs
// (tail_pair, tail_warm, gcomb*) are read here, at launch.
void solve_chip(const SolveCall &V, SparseDev &D) {
  const PlanRecord &R = V.R;
  const ColArgs C = col_args(V, D);
  bool gcomb_used = false;  // the tail launch also ran the sparse back-substitution
  if (df_path()) {
    const DfArgs F = df_args(V, C);
    const int nw = std::max(1, std::min(F.n_items, 1024));
    if (F.n_items > 0) df_factor_kernel<<<(nw + kDfWaves - 1) / kDfWaves, 64 * kDfWaves, 0, V.st>>>(F);
  } else {
#ifdef M3S_TEST_PATHS
    col_factor_kernel<<<std::max(1, std::min(C.ncols, 256)), 256, 0, V.st>>>(C);
#endif
  }
  if (R.nc > 0) {
    D.tail_A = V.tail;
    D.tail_ld = kTailLd;
    if (!df_path()) launch_border(V, D);
    const TailArgs T = tail_args(V, D);
    if (tail_cyc()) {
      const TailSync Y = tail_sync(V, T);
      const int TC = (7 * R.nc + 15) / 16;
      GArgs G = g_args(V, C, Y, TC);
      int nG = 0;
      if (gcomb_knob() && R.nc >= gcomb_min_nc_knob() && tail_pair_path() && C.ncols > 0) {
        G.X = at<double>(V.ws, V.Ly.gx);
        nG = std::max(1, std::min(C.ncols, std::min(gcomb_wg_knob(), 240 - G.n_pairs)));
        gcomb_used = true;
      }
      const unsigned gt = (unsigned)(G.n_pairs + nG);
      if (tail_pair_path())
        if (((7 * R.nc + 16) / 16 + 2) / 3 <= 7)  // tile rows TR: rows per wave of waves 1..3
          tail_pair_kernel<7><<<gt, 64 * kTailNW, 0, V.st>>>(T, Y, C, G);
        else
          tail_pair_kernel<(kTailMaxT + 2) / 3><<<gt, 64 * kTailNW, 0, V.st>>>(T, Y, C, G);
      else
        tail_cyc_kernel<<<TC, 64 * kTailNW, 0, V.st>>>(T, Y);
    } else {
      tail_llt_kernel<<<1, 64 * kTailNW, 0, V.st>>>(T);
    }
  }
  if (!gcomb_used) col_backsub_kernel<<<std::max(1, std::min(C.ncols, 256)), 64, 0, V.st>>>(C);
}

// factor (and for lds_plan the plan) in the LDS: the whole solve is one
// launch, which takes the in-call timing pair when one is armed
void solve_lds(const SolveCall &V, const SparseDev &D) {
  if (V.R.path == SolvePath::lds_plan)
    launch_timed(g_slv_ext_ev, sparse_llt_kernel<1>, dim3(1), dim3(1024), V.R.lds_bytes, V.st, D);
  else
    sparse_llt_kernel<2><<<1, 1024, V.R.lds_bytes, V.st>>>(D);
}

// factor in global memory on one workgroup. global_split: phase 1 up to the
// tail border, border_kernel, the dense tail on the f64 MFMA when it fits
// (tail_llt_kernel; else phase 2 factors it), phase 2.
void solve_global(const SolveCall &V, SparseDev &D) {
  const PlanRecord &R = V.R;
  if (R.path == SolvePath::global) {
    sparse_llt_kernel<0><<<1, 1024, R.lds_bytes, V.st>>>(D);
    return;
  }
  D.tail_A = R.mfma_tail ? V.tail : nullptr;
  D.tail_ld = kTailLd;
  D.phase = 1;
  sparse_llt_kernel<0><<<1, 1024, R.lds_bytes, V.st>>>(D);
  launch_border(V, D);
  if (R.mfma_tail) {
    tail_llt_kernel<<<1, 64 * kTailNW, 0, V.st>>>(tail_args(V, D));
    D.tail_done = 1;
  }
  D.phase = 2;
  sparse_llt_kernel<0, true><<<1, 1024, R.lds_bytes, V.st>>>(D);
}

// dense fallback: RHS-augmented system, register or tiled LLT
int solve_dense(const SolveCall &V, const double *edge_sums, const float *partials, int64_t chunks) {
  const m3s_gn_args *a = V.a;
  const int64_t n = V.Ly.n, ld = V.Ly.ld;
  int32_t *flags = V.flags, *stop = flags + kFlagStop;
  hipStream_t st = V.st;
  int rc;
  if (!edge_sums && a->E > 0) {
    double *es = at<double>(V.ws, V.Ly.edge_sums);
    edge_reduce_kernel<<<dim3((unsigned)a->E), dim3(64), 0, st>>>(partials, chunks, es, stop);
    if ((rc = launch_ok())) return rc;
    edge_sums = es;
  }
  double *A = at<double>(V.ws, V.Ly.A);
  assemble_kernel<<<dim3((unsigned)a->N), dim3(256), 0, st>>>(
      edge_sums, at<int32_t>(V.ws, V.Ly.rank_i), at<int32_t>(V.ws, V.Ly.rank_j), a->E, a->Twc, n, ld, A, stop);
  if ((rc = launch_ok())) return rc;
#ifdef M3S_TEST_PATHS
  const int np = (int)n + 1;
  if (np <= kMaxSmallNp) {
#define M3S_CHOL(NB)                                                                                      \
  case NB:                                                                                                \
    chol_small_kernel<NB><<<dim3(1), dim3(kCholThreads), 0, st>>>(A, ld, (int)n, a->Twc, a->N, a->dx_out, \
                                                                 a->info, stop, a->delta_thresh);         \
    break;
    switch ((np + 31) / 32) {
      M3S_CHOL(1)
      M3S_CHOL(2)
      M3S_CHOL(3)
      M3S_CHOL(4)
      M3S_CHOL(5)
      M3S_CHOL(6)
      M3S_CHOL(7)
      default:
        return M3S_ETOOLARGE;
    }
#undef M3S_CHOL
    return launch_ok();
  }
#endif
  const int nt = (int)(ld / kTile);
  for (int kb = 0; kb < nt; kb++) {
    if ((int64_t)kb * kTile >= n) break;
    potrf_tile_kernel<<<1, 256, 0, st>>>(A, ld, n, kb, flags);
    const int mt = nt - kb - 1;
    if (mt > 0) {
      trsm_tile_kernel<<<mt, 256, 0, st>>>(A, ld, n, kb, flags);
      update_tiles_kernel<<<mt * (mt + 1) / 2, 256, 0, st>>>(A, ld, kb, flags);
    }
    if ((rc = launch_ok())) return rc;
  }
  const size_t smem = sizeof(double) * (size_t)(ld + kTile * (kTile + 1)) + sizeof(float) * (size_t)ld;
  backsolve_kernel<<<1, 1024, smem, st>>>(A, ld, (int)n, a->Twc, a->N, a->dx_out, a->info, flags, a->delta_thresh);
  return launch_ok();
}

// edge_sums: per-edge local sums (stepwise API), or NULL with `partials` of
// `chunks` chunks per edge (single-GPU call: no separate reduce launch).
// The path is the plan's (build_plan_meta): read once finish_plan has run,
// never derived here. A record that still has no plan launches nothing.
int gn_solve_impl(const m3s_gn_args *a, const double *edge_sums, const float *partials, int64_t chunks,
                  hipStream_t st, bool fin_ready) {
  const Layout Ly = gn_layout(a->N, a->HW, a->E);
  if (a->N <= 1) return M3S_OK;
  int rc = host_finish(a, st);
  if (rc) return rc;
  if ((rc = finish_plan(a, Ly, st))) return rc;
  SolveView view;
  {
    std::lock_guard<std::mutex> g(g_reg_mu);
    auto it = g_reg.find(a->workspace);
    if (it == g_reg.end()) return M3S_EINVAL;  // m3s_gn_prepare not called on this workspace
    view = solve_view(it->second);
    it->second.epoch++;
  }
  const PlanRecord &R = view.plan;
  void *ws = a->workspace;
  const SolveCall V{a, Ly, R, view.epoch, st, ws, at<int32_t>(ws, Ly.flags), at<int32_t>(ws, Ly.colsync),
                    at<double>(ws, Ly.tail)};
  if (R.path == SolvePath::pending) return M3S_EINVAL;
  if (R.path == SolvePath::dense) return solve_dense(V, edge_sums, partials, chunks);
  int32_t *stop = V.flags + kFlagStop;
  SparseDev D = sparse_dev(V);
  if (a->E > 0 && !fin_ready) {
    finalize_edges_kernel<<<dim3((unsigned)a->E), dim3(64), 0, st>>>(
        edge_sums, edge_sums ? nullptr : partials, chunks, at<int32_t>(ws, Ly.rank_i), a->Twc, at<double>(ws, Ly.fin),
        stop);
    if ((rc = launch_ok())) return rc;
  }
  if (!R.asm_lds) {  // multi-workgroup assembly into the global factor array
    assemble_slots_kernel<<<dim3((unsigned)(R.S + R.m)), dim3(64), 0, st>>>(
        D.fin, D.plan, R.off[kSec_asm_ptr], R.off[kSec_asm_edge], R.off[kSec_g_ptr], R.off[kSec_g_edge], R.m, R.S,
        D.L, at<double>(ws, Ly.rhs), stop);
    if ((rc = launch_ok())) return rc;
  }
  switch (R.path) {
    case SolvePath::lds_plan:
    case SolvePath::lds: solve_lds(V, D); break;
    case SolvePath::chip: solve_chip(V, D); break;
    case SolvePath::global_split:
    case SolvePath::global: solve_global(V, D); break;
    case SolvePath::pending:
    case SolvePath::dense: break;  // returned above
  }
  return launch_ok();
}

void set_lds_attributes_once() {
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(sparse_llt_kernel<0>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(sparse_llt_kernel<0, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(sparse_llt_kernel<1>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(sparse_llt_kernel<2>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gn_prologue_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes);
  });
}

// gn/iterate.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// One GN iteration and the whole call: gn_linearize_impl, gn_solve_impl (the
// first host mention of every solver kernel), set_lds_attributes_once, the
// in-call timing (CallTiming, call_mark) and gn_full.
// Relies on every part before it: gn/layout.h, every kernel part, gn/args.h
// and the three host parts.

int gn_linearize_impl(const m3s_gn_args *a, const ResidualParams &P, int64_t eb, int64_t ee,
                      double *edge_sums, hipStream_t st, bool fuse_fin = false, int64_t *chunks_used = nullptr) {
  const Layout Ly = gn_layout(a->N, a->HW, a->E);
  void *ws = a->workspace;
  const int64_t E_loc = ee - eb;
  if (E_loc <= 0) return M3S_OK;
  LinArgs L{};
  L.Twc = a->Twc;
  L.T_rel = nullptr;
  L.Xs = a->Xs;
  L.Cs = a->Cs;
  L.Xsrc = nullptr;
  L.idx = a->idx_ii2jj;
  L.idx32 = a->idx_i32 ? 1 : 0;
  L.valid = a->valid_match;
  L.Q = a->Q;
  L.rank_i = at<int32_t>(ws, Ly.rank_i);
  L.rank_j = at<int32_t>(ws, Ly.rank_j);
  L.stop = at<int32_t>(ws, Ly.flags) + kFlagStop;
  L.partials = at<float>(ws, Ly.partials);
  L.planes = at<float>(ws, Ly.planes);
  L.eorder = nullptr;
  L.cnt_base = 0;
  // fused finalize only over the whole edge set (single-GPU solve); fused
  // edge sums for the stepwise API (any range)
  const bool fin_tail = fuse_fin && eb == 0 && ee == a->E;
  L.edge_cnt = (fin_tail || edge_sums) ? at<uint32_t>(ws, Ly.edge_cnt) : nullptr;
  L.esum = fin_tail ? nullptr : edge_sums;
  L.fin = at<double>(ws, Ly.fin);
  L.HW = a->HW;
  L.edge_begin = eb;
  L.E_loc = E_loc;
  L.P = P;
  L.Kd = a->mode == M3S_MODE_CALIB ? a->K : nullptr;
  const bool vec = (a->HW % 4 == 0) && vec_ok(a->Xs, 16) && vec_ok(a->Cs, 16) && vec_ok(a->Q, 16) &&
                   vec_ok(a->idx_ii2jj, 16) && vec_ok(a->valid_match, 4);
  // (the packed and pipelined gathering kernels address a pointmap through
  // 32-bit buffer offsets: 12 HW bytes must fit a signed int)
  const bool can_pack = vec && a->HW * 12 < ((int64_t)1 << 31) &&
                        (a->mode != M3S_MODE_CALIB || (a->width < 65536 && a->height < 32768));
  int pack = 0;
  bool ordered = false;
  if (eb != 0 || ee != a->E) {  // a sharded rank's range: its edge order is built from the host ranks
    const int rc = host_finish(a, st);
    if (rc) return rc;
  }
  {
    std::lock_guard<std::mutex> stage_lock(g_stage_mu);  // (lock order: staging, then registry)
    std::lock_guard<std::mutex> g(g_reg_mu);
    auto it = g_reg.find(ws);
    if (it == g_reg.end()) return M3S_EINVAL;  // m3s_gn_prepare not called on this workspace
    PlanMeta &M = it->second;
    if (M.range_b != eb || M.range_e != ee) {  // a sharded rank's own edge range
      M.range_b = eb, M.range_e = ee, M.planes_ok = false, M.order_ok = false;
      if (M.cnt_arr) M.cnt_ok = false;
      if ((int64_t)M.rj.size() >= ee) {
        std::vector<int32_t> order;
        build_eorder(M.rj, eb, E_loc, order);
        // uploaded from pinned staging guarded by an event, so the registry
        // entry owns no host memory a queued copy still reads (m3s_gn_release
        // need not synchronise)
        Staging *SG = stage_for_device();
        const size_t nb = sizeof(int32_t) * order.size();
        if (!SG) return M3S_ELAUNCH;
        if (SG->tasks_pending && hipEventSynchronize(SG->tasks_ev) != hipSuccess) return M3S_ELAUNCH;
        SG->tasks_pending = false;
        if (!pinned_reserve(SG->tasks_up, SG->tasks_cap, nb)) return M3S_ELAUNCH;
        memcpy(SG->tasks_up, order.data(), nb);
        if (hipMemcpyAsync(at<int32_t>(ws, Ly.eorder), SG->tasks_up, nb, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipEventRecord(SG->tasks_ev, st) != hipSuccess)
          return M3S_ELAUNCH;
        SG->tasks_pending = true;
        M.order_ok = true;
      }
    }
    ordered = M.order_ok;
    if (can_pack) {
      pack = M.planes_ok ? 2 : 1;
      M.planes_ok = true;
    }
    // chunking: the gathering kernel's own (smaller chunks); the packed kernel
    // counts its arrivals after the first iteration's (edge_tail)
    const int64_t c_gather = chunks_for(a->HW, E_loc, kGatherBlocks);
    L.chunks = pack == 2 ? chunks_for(a->HW, E_loc) : c_gather;
    L.cnt_base = pack == 2 ? (uint32_t)c_gather : 0u;
    if (fin_tail) {
      M.cnt_ok = false;  // the drop-in call counts from its own prepare
    } else if (L.esum) {
      if (!M.cnt_ok) {  // stale arrivals: zero every counter (a few KB)
        if (hipMemsetAsync(L.edge_cnt, 0, edge_cnt_bytes(a->E), st) != hipSuccess) return M3S_ELAUNCH;
        M.cnt_arr = 0, M.cnt_ok = true;
      }
      L.cnt_base = M.cnt_arr;
      M.cnt_arr += (uint32_t)L.chunks;
    }
  }
  L.chunk_pix = chunk_pixels(a->HW, L.chunks);
  const int64_t T = E_loc * L.chunks;
  L.per = (T + 7) / 8;
  int64_t blocks = T;
  if (ordered) {
    L.eorder = at<int32_t>(ws, Ly.eorder);
    blocks = 8 * L.per;
  }
  if (chunks_used) *chunks_used = L.chunks;
  int rc = dispatch_linearize<false>(a->mode, L, blocks, vec, pack, st);
  if (rc && L.esum) {
    std::lock_guard<std::mutex> g(g_reg_mu);
    auto it = g_reg.find(ws);
    if (it != g_reg.end()) it->second.cnt_ok = false;  // arrivals unknown
  }
  return rc;  // NULL edge_sums: partials only (kernel timing)
}

// edge_sums: per-edge local sums (stepwise API), or NULL with `partials` of
// `chunks` chunks per edge (single-GPU call: no separate reduce launch).
int gn_solve_impl(const m3s_gn_args *a, const double *edge_sums, const float *partials, int64_t chunks,
                  hipStream_t st, bool fin_ready = false) {
  const Layout Ly = gn_layout(a->N, a->HW, a->E);
  void *ws = a->workspace;
  int32_t *flags = at<int32_t>(ws, Ly.flags);
  int32_t *stop = flags + kFlagStop;
  const int64_t n = Ly.n, ld = Ly.ld;
  if (a->N <= 1) return M3S_OK;
  int rc0 = host_finish(a, st);
  if (rc0) return rc0;
  rc0 = finish_plan(a, Ly, st);
  if (rc0) return rc0;
  SolveView view;
  {
    std::lock_guard<std::mutex> g(g_reg_mu);
    auto it = g_reg.find(ws);
    if (it == g_reg.end()) return M3S_EINVAL;  // m3s_gn_prepare not called on this workspace
    view = solve_view(it->second);
    it->second.epoch++;
  }
  const PlanRecord &meta = view.plan;
  int rc;
  float *dx = a->dx_out;
  if (meta.sparse) {
    double *fin = at<double>(ws, Ly.fin);
    if (a->E > 0 && !fin_ready) {
      finalize_edges_kernel<<<dim3((unsigned)a->E), dim3(64), 0, st>>>(
          edge_sums, edge_sums ? nullptr : partials, chunks, at<int32_t>(ws, Ly.rank_i), a->Twc, fin, stop);
      if ((rc = launch_ok())) return rc;
    }
    SparseDev D;
    D.phase = 0;
    D.tail_done = 0;
    D.tail_A = nullptr;
    D.tail_ld = 0;
    D.plan = at<int32_t>(ws, Ly.plan);
    D.plan_len = meta.plan_len;
    std::copy(meta.off, meta.off + kPlanSections, D.off);
    D.n_items = meta.n_items;
    D.n_tasks = meta.n_tasks;
    D.n_parts = meta.n_parts;
    D.nc = meta.nc;
    D.E = (int)a->E;
    D.asm_lds = meta.asm_lds ? 1 : 0;
    D.parts = at<double>(ws, Ly.parts);
    D.dbg = at<int64_t>(ws, Ly.A);
    D.m = meta.m;
    D.S = meta.S;
    D.levels = meta.levels;
    D.L = at<double>(ws, Ly.Lblk);
    D.rhs = at<double>(ws, Ly.rhs);
    if (!meta.asm_lds) {  // multi-workgroup assembly into the global factor array
      assemble_slots_kernel<<<dim3((unsigned)(meta.S + meta.m)), dim3(64), 0, st>>>(
          fin, D.plan, meta.off[kSec_asm_ptr], meta.off[kSec_asm_edge], meta.off[kSec_g_ptr], meta.off[kSec_g_edge],
          meta.m, meta.S, D.L, at<double>(ws, Ly.rhs), stop);
      if ((rc = launch_ok())) return rc;
    }
    D.Dinv = at<double>(ws, Ly.Dinv);
    D.fin = fin;
    D.Twc = a->Twc;
    D.N = a->N;
    D.dx_out = dx;
    D.info = a->info;
    D.flags = flags;
    D.delta_thresh = a->delta_thresh;
    if (meta.store == 0 && cols_path() && meta.m <= 512 && (meta.nc == 0 || 7 * meta.nc + 1 <= 16 * kTailMaxT)) {
      // column tasks over the chip -> tail border -> dense tail on the MFMA
      // -> column back-substitution + step
      ColArgs C;
      C.plan = D.plan;
      std::copy(meta.off, meta.off + kPlanSections, C.off);
      C.m = meta.m;
      C.c0 = meta.m - meta.nc;
      C.ncols = C.c0;
      C.epoch = view.epoch;
      C.L = D.L;
      C.Dinv = D.Dinv;
      C.y = const_cast<double *>(D.rhs);
      int32_t *cs = at<int32_t>(ws, Ly.colsync);
      C.done = cs;
      C.done2 = cs + (meta.m + 1);
      C.ctr = cs + 2 * (meta.m + 1);
      C.flags = flags;
      C.info = a->info;
      C.Twc = a->Twc;
      C.dx_out = dx;
      C.N = a->N;
      C.delta_thresh = a->delta_thresh;
      double *tail = at<double>(ws, Ly.tail);
      const int tld = 16 * kTailMaxT;
      bool gcomb_used = false;  // the tail launch also ran the sparse back-substitution
      // the factor launch (df_factor_kernel)
      if (df_path()) {
        // every block of the sparse columns and the tail border: one wave-level dataflow
        DfArgs F;
        F.plan = D.plan;
        std::copy(meta.off, meta.off + kPlanSections, F.off);
        F.items = D.plan + meta.off_dfitems;
        F.n_items = meta.n_dfitems;
        F.n_tasks = meta.n_tasks;
        F.m = meta.m;
        F.c0 = C.c0;
        F.nc = meta.nc;
        F.epoch = view.epoch;
        F.L = D.L;
        F.Dinv = D.Dinv;
        F.y = C.y;
        F.sdone = cs + 2 * (meta.m + 1) + 16;
        F.ctr = C.ctr + 3;
        F.flags = flags;
        F.tail_A = tail;
        F.tail_ld = tld;
        F.Wgr = at<double>(ws, Ly.wgran);
        const int nw = std::max(1, std::min(F.n_items, 1024));
        if (F.n_items > 0) df_factor_kernel<<<(nw + kDfWaves - 1) / kDfWaves, 64 * kDfWaves, 0, st>>>(F);
      } else {
#ifdef M3S_TEST_PATHS
        const int g1 = std::max(1, std::min(C.ncols, 256));
        col_factor_kernel<<<g1, 256, 0, st>>>(C);
#endif
      }
      // the dense tail's launch
      if (meta.nc > 0) {
        D.tail_A = tail;
        D.tail_ld = tld;
        const int nt0 = meta.nc * (meta.nc + 1) / 2;
        if (!df_path())
          border_kernel<<<(nt0 + kBorderWaves - 1) / kBorderWaves, 64 * kBorderWaves,
                          kBorderWaves * kStageDoubles * sizeof(double), st>>>(D);
        TailArgs T;
        T.Ad = tail;
        T.ld = tld;
        T.rhs = C.y;
        T.Lg = tail + (size_t)tld * tld;
        T.Wg = T.Lg + (size_t)kTailMaxT * (kTailMaxT + 1) / 2 * 256;
        T.flags = flags;
        T.nc = meta.nc;
        T.c0 = C.c0;
        if (tail_cyc()) {
          TailSync Y;
          Y.tflag = cs + 2 * (meta.m + 1) + 16 + Ly.slot_cap;
          Y.epoch = view.epoch;
          Y.ypg = T.Wg + (size_t)kTailMaxT * 256;
          Y.LgT = Y.ypg + 16 * kTailMaxT;
          Y.LgG = tail + tail_gran_offset_doubles();
          Y.warm = tail_warm_knob() ? 1 : 0;
          const int TC = (7 * meta.nc + 15) / 16;
          // the sparse back-substitution on extra workgroups of the tail's
          // launch (gcol_worker) when there are sparse columns
          GArgs G;
          G.X = nullptr;
          G.n_pairs = (TC + 1) / 2;
          G.nx = ((1 + 7 * meta.nc) + 7) / 8 * 8;
          G.task = C.ctr + 8, G.comb = C.ctr + 9, G.fin = C.ctr + 10, G.xt_ready = C.ctr + 11;
          G.cnt = Y.tflag + 2 * kTailMaxT;
          int nG = 0;
          if (gcomb_knob() && meta.nc >= gcomb_min_nc_knob() && tail_pair_path() && C.ncols > 0) {
            G.X = at<double>(ws, Ly.gx);
            nG = std::max(1, std::min(C.ncols, std::min(gcomb_wg_knob(), 240 - G.n_pairs)));
            gcomb_used = true;
          }
          const unsigned gt = (unsigned)(G.n_pairs + nG);
          if (tail_pair_path())
            if (((7 * meta.nc + 16) / 16 + 2) / 3 <= 7)  // tile rows TR: rows per wave of waves 1..3
              tail_pair_kernel<7><<<gt, 64 * kTailNW, 0, st>>>(T, Y, C, G);
            else
              tail_pair_kernel<(kTailMaxT + 2) / 3><<<gt, 64 * kTailNW, 0, st>>>(T, Y, C, G);
          else
            tail_cyc_kernel<<<TC, 64 * kTailNW, 0, st>>>(T, Y);
        } else {
          tail_llt_kernel<<<1, 64 * kTailNW, 0, st>>>(T);
        }
      }
      if (!gcomb_used) {
        const int g4 = std::max(1, std::min(C.ncols, 256));
        col_backsub_kernel<<<g4, 64, 0, st>>>(C);
      }
    } else if (meta.store == 1)
      if (g_slv_ext_ev) {
        hipExtLaunchKernelGGL(sparse_llt_kernel<1>, dim3(1), dim3(1024), meta.lds_bytes, st, g_slv_ext_ev[0],
                              g_slv_ext_ev[1], 0, D);
        g_slv_ext_ev = nullptr;
      } else {
        sparse_llt_kernel<1><<<1, 1024, meta.lds_bytes, st>>>(D);
      }
    else if (meta.store == 2)
      sparse_llt_kernel<2><<<1, 1024, meta.lds_bytes, st>>>(D);
    else if (meta.nc > 0 && border_split()) {
      // the dense tail on the f64 MFMA when it fits (tail_llt_kernel), else
      // in phase 2 of the one-workgroup kernel
      const bool mfma_tail = 7 * meta.nc + 1 <= 16 * kTailMaxT && tail_mfma();
      double *tail = at<double>(ws, Ly.tail);
      const int tld = 16 * kTailMaxT;
      D.tail_A = mfma_tail ? tail : nullptr;
      D.tail_ld = tld;
      D.phase = 1;
      sparse_llt_kernel<0><<<1, 1024, meta.lds_bytes, st>>>(D);
      const int nt0 = meta.nc * (meta.nc + 1) / 2;
      border_kernel<<<(nt0 + kBorderWaves - 1) / kBorderWaves, 64 * kBorderWaves,
                      kBorderWaves * kStageDoubles * sizeof(double), st>>>(D);
      if (mfma_tail) {
        TailArgs T;
        T.Ad = tail;
        T.ld = tld;
        T.rhs = const_cast<double *>(D.rhs);
        T.Lg = tail + (size_t)tld * tld;
        T.Wg = T.Lg + (size_t)kTailMaxT * (kTailMaxT + 1) / 2 * 256;
        T.flags = flags;
        T.nc = meta.nc;
        T.c0 = meta.m - meta.nc;
        tail_llt_kernel<<<1, 64 * kTailNW, 0, st>>>(T);
        D.tail_done = 1;
      }
      D.phase = 2;
      sparse_llt_kernel<0, true><<<1, 1024, meta.lds_bytes, st>>>(D);
    } else
      sparse_llt_kernel<0><<<1, 1024, meta.lds_bytes, st>>>(D);
    return launch_ok();
  }
  // dense fallback: RHS-augmented system, register or tiled LLT
  if (!edge_sums && a->E > 0) {
    double *es = at<double>(ws, Ly.edge_sums);
    edge_reduce_kernel<<<dim3((unsigned)a->E), dim3(64), 0, st>>>(partials, chunks, es, stop);
    if ((rc = launch_ok())) return rc;
    edge_sums = es;
  }
  double *A = at<double>(ws, Ly.A);
  assemble_kernel<<<dim3((unsigned)a->N), dim3(256), 0, st>>>(
      edge_sums, at<int32_t>(ws, Ly.rank_i), at<int32_t>(ws, Ly.rank_j), a->E, a->Twc, n, ld, A, stop);
  if ((rc = launch_ok())) return rc;
  const int np = (int)n + 1;
#ifdef M3S_TEST_PATHS
  if (np <= kMaxSmallNp) {
    const int nbc = (np + 31) / 32;
#define M3S_CHOL(NB)                                                                                   \
  case NB:                                                                                             \
    chol_small_kernel<NB><<<dim3(1), dim3(kCholThreads), 0, st>>>(A, ld, (int)n, a->Twc, a->N, dx, \
                                                                 a->info, stop, a->delta_thresh);  \
    break;
    switch (nbc) {
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
  (void)np;
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
  backsolve_kernel<<<1, 1024, smem, st>>>(A, ld, (int)n, a->Twc, a->N, dx, a->info, flags, a->delta_thresh);
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

// In-call launch timing (bench.py's roofline leg, m3s_debug_call_timing):
// when on, a drop-in call records a timing event on its stream before each
// linearize launch, after it and after the solve launches of that iteration,
// so the packed kernel is timed in the call's own launch pattern (behind the
// previous iteration's solve), not back to back. Kinds: 0 first-iteration
// (gathering) linearize, 1 packed linearize, 2 solve (every launch of it).
struct CallTiming {
  std::mutex mu;
  bool on = false;
  std::vector<hipEvent_t> ev;  // pool, reused
  std::vector<int> kind;       // kind of the span from event q to q + 1 (-1: none)
  size_t used = 0;
  std::vector<hipEvent_t> kev;  // pool: {start, stop} of each timed linearize dispatch
  std::vector<char> kev_ok;     // per pair: the dispatch took it (else the span uses ev[q], ev[q + 1])
  size_t kused = 0;
};
CallTiming &call_timing() {
  static CallTiming t;
  return t;
}
bool call_mark(hipStream_t st, int kind_next) {  // caller holds the lock
  CallTiming &T = call_timing();
  if (T.used == T.ev.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return false;
    T.ev.push_back(e);
    T.kind.push_back(-1);
  }
  T.kind[T.used] = kind_next;
  return hipEventRecord(T.ev[T.used++], st) == hipSuccess;
}

int gn_full(const m3s_gn_args *a, int mode, void *stream) {
  int rc = check_args(a);
  if (rc) return rc;
  if (a->mode != mode) return M3S_EINVAL;
  if (gn_layout(a->N, a->HW, a->E).ld > kMaxLd) return M3S_ETOOLARGE;
  hipStream_t st = S(stream);
  const ResidualParams P = make_params(a);  // calib intrinsics: read by the kernels (LinArgs::Kd)
  if ((rc = gn_prepare_async(a, st))) return rc;
  const Layout Ly = gn_layout(a->N, a->HW, a->E);
  const float *partials = at<float>(a->workspace, Ly.partials);
  bool sparse;
  {
    std::lock_guard<std::mutex> g(g_reg_mu);
    sparse = g_reg.at(a->workspace).plan.sparse;
  }
  CallTiming &CT = call_timing();
  std::unique_lock<std::mutex> tl(CT.mu, std::defer_lock);
  bool timing = false;
  {
    std::lock_guard<std::mutex> g(CT.mu);
    timing = CT.on;
  }
  if (timing) tl.lock();
  // sparse solve: the linearize kernels finalize each edge themselves
  for (int it = 0; it < a->max_iter; it++) {
    int64_t chunks = 0;  // of this iteration's linearize launch (the dense path reduces its partials)
    if (timing && !call_mark(st, it == 0 ? 0 : 1)) return M3S_ELAUNCH;
    if (timing) {  // the linearize dispatch's own begin / end (launch_lin)
      while (CT.kev.size() < CT.kused + 2) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return M3S_ELAUNCH;
        CT.kev.push_back(e);
      }
      if (CT.kev_ok.size() < CT.kev.size() / 2) CT.kev_ok.resize(CT.kev.size() / 2);
      g_lin_ext_ev = &CT.kev[CT.kused];
    }
    rc = gn_linearize_impl(a, P, 0, a->E, nullptr, st, sparse, &chunks);
    if (timing) {
      CT.kev_ok[CT.kused / 2] = g_lin_ext_ev == nullptr;  // launch_lin took the pair
      CT.kused += 2;
    }
    g_lin_ext_ev = nullptr;
    if (rc) return rc;
    if (timing && !call_mark(st, 2)) return M3S_ELAUNCH;
    if (timing) {  // the solve dispatch's own begin / end when it is one launch (sparse_llt_kernel<1>)
      while (CT.kev.size() < CT.kused + 2) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return M3S_ELAUNCH;
        CT.kev.push_back(e);
      }
      if (CT.kev_ok.size() < CT.kev.size() / 2) CT.kev_ok.resize(CT.kev.size() / 2);
      g_slv_ext_ev = &CT.kev[CT.kused];
    }
    rc = gn_solve_impl(a, nullptr, partials, chunks, st, sparse);
    if (timing) {
      CT.kev_ok[CT.kused / 2] = g_slv_ext_ev == nullptr;
      CT.kused += 2;
    }
    g_slv_ext_ev = nullptr;
    if (rc) return rc;
    if (timing && !call_mark(st, -1)) return M3S_ELAUNCH;
  }
  return M3S_OK;
}

// gn/iterate.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// One GN iteration's linearize and the whole call: gn_linearize_impl, the
// in-call timing (CallTiming, call_mark, arm_pair / close_pair) and gn_full.
// Relies on every part before it: gn/layout.h, gn/args.h and the three host
// parts; declares gn_solve_impl, which gn/solve.h defines.

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

// The solve of one iteration. Defined in gn/solve.h, behind this part: its
// launch functions name the solver kernel templates, which the order rule
// (m3s_gn.hip) keeps behind gn_linearize_impl's mention of the linearize ones.
int gn_solve_impl(const m3s_gn_args *a, const double *edge_sums, const float *partials, int64_t chunks,
                  hipStream_t st, bool fin_ready = false);

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

// The next {start, stop} pair of the kev pool, for the caller to arm a launch
// with (launch_timed takes and clears an armed pair); nullptr if an event
// cannot be created. Caller holds the lock.
hipEvent_t *arm_pair(CallTiming &T) {
  while (T.kev.size() < T.kused + 2) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    T.kev.push_back(e);
  }
  if (T.kev_ok.size() < T.kev.size() / 2) T.kev_ok.resize(T.kev.size() / 2);
  return &T.kev[T.kused];
}
// After the launches the pair was armed for: did one take it (and clear
// `armed`)? Else the span falls back to the events recorded around it.
void close_pair(CallTiming &T, hipEvent_t *&armed) {
  T.kev_ok[T.kused / 2] = armed == nullptr;
  T.kused += 2;
  armed = nullptr;
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
    // the linearize dispatch's own begin / end (launch_lin)
    if (timing && !(call_mark(st, it == 0 ? 0 : 1) && (g_lin_ext_ev = arm_pair(CT)))) return M3S_ELAUNCH;
    rc = gn_linearize_impl(a, P, 0, a->E, nullptr, st, sparse, &chunks);
    if (timing) close_pair(CT, g_lin_ext_ev);
    if (rc) return rc;
    // the solve dispatch's own begin / end when it is one launch (sparse_llt_kernel<1>)
    if (timing && !(call_mark(st, 2) && (g_slv_ext_ev = arm_pair(CT)))) return M3S_ELAUNCH;
    rc = gn_solve_impl(a, nullptr, partials, chunks, st, sparse);
    if (timing) close_pair(CT, g_slv_ext_ev);
    if (rc) return rc;
    if (timing && !call_mark(st, -1)) return M3S_ELAUNCH;
  }
  return M3S_OK;
}

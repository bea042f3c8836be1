// gn/plan.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// From edge ids to a plan on the device: SolvePath (the row list of the
// launch paths), PlanRecord (the one declaration of what a solve launch reads
// of a plan, its path included), PlanMeta and the workspace registry,
// pinned staging, the plan cache (find_cached_plan), set_knob,
// build_plan_meta (the one place that decides a plan's path: the LDS budget,
// the chip-wide condition and the shaping knobs), build_eorder, upload_plan,
// adopt_plan, gn_prepare_impl
// (host prepare), finish_plan / host_finish, gn_prepare_async (the prologue
// launch) and gn_release_impl.
// Relies on gn/layout.h (Layout / gn_layout), gn/llt_blocks.h
// (kStageDoubles, kSplitUpdates), gn/prologue.h (the call prologue), gn/args.h
// (S, launch_ok) and gn/knobs.h; declares set_lds_attributes_once, which
// gn/solve.h defines.

// The launches that solve a plan (gn/solve.h has one launch function per
// path). One row per path: the enum and the names (m3s_gn_plan_path_debug)
// are derived from the list. build_plan_meta decides the path, once, from the
// plan and the shaping knobs; nothing re-derives it at launch.
#define M3S_SOLVE_PATHS(X)                                                                                \
  X(pending)      /* no plan yet (a record whose plan is still to be built): nothing may launch */       \
  X(dense)        /* no sparse plan that fits: the tiled (test build: register) dense Cholesky */        \
  X(lds_plan)     /* sparse_llt_kernel<1>: factor and plan in the LDS */                                 \
  X(lds)          /* sparse_llt_kernel<2>: factor in the LDS */                                          \
  X(chip)         /* df_factor_kernel -> dense tail -> back-substitution, over the chip */               \
  X(global_split) /* sparse_llt_kernel<0> in two phases around border_kernel (+ tail_llt_kernel) */      \
  X(global)       /* sparse_llt_kernel<0> alone */
#define M3S_PATH_ID(name) name,
#define M3S_PATH_NAME(name) #name,
enum class SolvePath : int { M3S_SOLVE_PATHS(M3S_PATH_ID) };
constexpr const char *kSolvePathNames[] = {M3S_SOLVE_PATHS(M3S_PATH_NAME)};
#undef M3S_PATH_ID
#undef M3S_PATH_NAME

// What a solve launch reads of a plan. Built once per edge set
// (build_plan_meta), kept by the plan cache and copied whole: a field added
// here reaches the cold, the cached and the host-prepare path alike.
struct PlanRecord {
  SolvePath path = SolvePath::pending;
  bool mfma_tail = false;  // global_split: the dense tail fits tail_llt_kernel (else phase 2 factors it)
  bool sparse = false;
  int store = 0;  // sparse_llt_kernel<STORE>
  bool asm_lds = false;  // LDS factor with room for the staged fin blocks: assembly in the LLT kernel
  size_t lds_bytes = 0;
  int m = 0, S = 0, levels = 0, plan_len = 0, n_items = 0, n_tasks = 0, n_parts = 0, nc = 0;
  int nnz = 0;  // off-diagonal blocks (col_ptr[m])
  int off_dfitems = 0, n_dfitems = 0;  // df_factor_kernel dispatch list (appended to the plan image)
  int n_dfsparse = 0;                  // its sparse-column items (the border items follow)
  int off[kPlanSections] = {};         // section offsets into the image (PlanImage::off)
};
static_assert(std::is_trivially_copyable<PlanRecord>::value, "copied under the registry lock");

// The registry entry of a solve call: its plan, the plan's image, and the
// state of this call alone. Every prepare starts from a fresh one.
struct PlanMeta {
  PlanRecord plan;
  std::vector<int32_t> h_plan;  // flattened plan image (host copy of the upload)
  int epoch = 0;  // solve launches since m3s_gn_prepare (column-task flags / tickets)
  // linearize state of this solve call: edge ranks, the edge range last
  // linearized and whether that range's planes are stored
  std::vector<int32_t> rj, h_ri;   // edge ranks (host copies of the uploaded arrays)
  int64_t range_b = -1, range_e = -1;  // the edge range last linearized
  bool order_ok = false;               // its edge order is in the workspace (Layout::eorder)
  bool planes_ok = false;
  // stepwise linearize with fused edge sums: edge_cnt arrivals counted since
  // the counters were last zeroed (valid for every edge of the range); false:
  // the counters hold arrivals of another range or of a drop-in call
  uint32_t cnt_arr = 0;
  bool cnt_ok = true;
  // the symbolic plan of this call is built by its first solve (cache miss at
  // prepare): the host analysis then overlaps the first linearize kernel
  bool plan_pending = false;
  bool force_dense = false;
  // the ids of this call are still on their way to the host (device prologue,
  // gn_prepare_async): host_finish reads them from pinned slot `slot`
  bool host_pending = false;
  int slot = -1;
};

// What a solve launch reads of the registry entry: the plan record and the
// epoch, not the host vectors (ranks, plan image) that the entry keeps alive
// for queued uploads.
struct SolveView {
  PlanRecord plan;
  int epoch;
};
SolveView solve_view(const PlanMeta &M) { return {M.plan, M.epoch}; }
// Host registry of the per-call plan (keyed by workspace): the stepwise API
// calls prepare and solve separately.
std::mutex g_reg_mu;
std::unordered_map<const void *, PlanMeta> g_reg;

// Pinned host staging of the per-call transfers (gn_prepare_impl: the D2H
// reads of ii, jj and ONE H2D upload of flags | ranks | task table | plan;
// finish_plan: a deferred plan; gn_linearize_impl: a sharded rank's task
// table). Pageable copies were one staged, host-synchronous transfer each
// (~7 per call); an event per buffer guards it until the copy that reads it
// has left. The registry entries own no memory a queued copy still reads.
// Pinned slot the device prologue writes a call's ii, jj and K into (host-
// mapped); busy from the prepare until the host has read it (host_finish or
// release), its event marks the prologue's completion.
struct DownSlot {
  char *p = nullptr, *dp = nullptr;  // host / device view
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  bool busy = false, used = false;
};
struct Staging {
  char *down = nullptr, *up = nullptr, *plan_up = nullptr, *tasks_up = nullptr;
  size_t down_cap = 0, up_cap = 0, plan_cap = 0, tasks_cap = 0;
  hipEvent_t ev = nullptr, plan_ev = nullptr, tasks_ev = nullptr;
  bool pending = false, plan_pending = false, tasks_pending = false;
  hipStream_t side = nullptr;  // plan uploads that must not queue behind a running linearize
  std::vector<DownSlot> slots;
};
// One staging set per device: an event recorded on one device's stream cannot
// guard another device's copies (a process may drive GN on several GPUs).
std::mutex g_stage_mu;
std::unordered_map<int, Staging> g_stages;
bool pinned_reserve(char *&p, size_t &cap, size_t need) {
  if (need <= cap) return true;
  if (p) (void)hipHostFree(p);
  p = nullptr, cap = 0;
  const size_t n = std::max<size_t>(need + need / 2, 1 << 16);
  if (hipHostMalloc(reinterpret_cast<void **>(&p), n, hipHostMallocDefault) != hipSuccess) return false;
  cap = n;
  return true;
}
Staging *stage_for_device() {  // caller holds g_stage_mu
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  Staging &S = g_stages[dev];
  for (hipEvent_t *e : {&S.ev, &S.plan_ev, &S.tasks_ev})
    if (!*e && hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) return nullptr;
  if (!S.side && hipStreamCreateWithFlags(&S.side, hipStreamNonBlocking) != hipSuccess) return nullptr;
  return &S;
}
// A free pinned slot of at least `need` bytes (caller holds g_stage_mu).
int acquire_slot(Staging &SG, size_t need) {
  int k = -1;
  for (int q = 0; q < (int)SG.slots.size(); q++)
    if (!SG.slots[q].busy) {
      k = q;
      break;
    }
  if (k < 0) {
    SG.slots.emplace_back();
    k = (int)SG.slots.size() - 1;
  }
  DownSlot &D = SG.slots[k];
  if (D.used && hipEventSynchronize(D.ev) != hipSuccess) return -1;  // its last prologue has finished writing
  if (!D.ev && hipEventCreateWithFlags(&D.ev, hipEventDisableTiming) != hipSuccess) return -1;
  if (need > D.cap) {
    if (D.p) (void)hipHostFree(D.p);
    D.p = D.dp = nullptr, D.cap = 0;
    const size_t n = std::max<size_t>(need + need / 2, 1 << 16);
    if (hipHostMalloc(reinterpret_cast<void **>(&D.p), n, hipHostMallocDefault) != hipSuccess) return -1;
    void *dp = nullptr;
    if (hipHostGetDevicePointer(&dp, D.p, 0) != hipSuccess) return -1;
    D.dp = static_cast<char *>(dp), D.cap = n;
  }
  D.busy = true, D.used = true;
  return k;
}

// Linearize edge order of an edge range: its edges (local indices) sorted by
// KF j (block_task deals the (chunk, KF j)-sorted tasks over the XCDs).
void build_eorder(const std::vector<int32_t> &rj, int64_t eb, int64_t E_loc, std::vector<int32_t> &out) {
  out.resize((size_t)E_loc);
  for (int64_t e = 0; e < E_loc; e++) out[e] = (int32_t)e;
  std::stable_sort(out.begin(), out.end(), [&](int32_t x, int32_t y) { return rj[eb + x] < rj[eb + y]; });
}

constexpr size_t kMaxLdsBytes = 150 * 1024;
// Defined behind the launch functions of gn/solve.h: its body names the
// sparse_llt_kernel specialisations, and where a kernel template is first
// named decides its place in the device code (the order rule, m3s_gn.hip).
void set_lds_attributes_once();

// Host symbolic plans of recent edge sets (the same factor graph is usually
// solved many times: every keyframe's local/global optimisation, every bench
// step). Keyed by (N, HW, E, dense override, remapped ranks). An entry is its
// key, the plan record and the image: no part of the call that built it.
struct PlanCacheEntry {
  int64_t N = 0, HW = 0, E = 0;
  bool dense = false;
  int tail_min = 0;  // dense_tail_min() the plan was built with
  std::vector<int32_t> ri, rj;
  PlanRecord plan;
  std::vector<int32_t> image;
};
std::mutex g_cache_mu;
std::vector<PlanCacheEntry> g_cache;  // most recent first
constexpr size_t kPlanCacheSize = 4;

// The cached plan of this edge set, moved to the front of the cache.
bool find_cached_plan(const m3s_gn_args *a, bool force_dense, const std::vector<int32_t> &ri,
                      const std::vector<int32_t> &rj, PlanRecord &plan, std::vector<int32_t> &image) {
  if (!plan_cache_enabled()) return false;
  std::lock_guard<std::mutex> g(g_cache_mu);
  for (size_t q = 0; q < g_cache.size(); q++) {
    const PlanCacheEntry &C = g_cache[q];
    if (C.N == a->N && C.HW == a->HW && C.E == a->E && C.dense == force_dense &&
        C.tail_min == dense_tail_min() && C.ri == ri && C.rj == rj) {
      plan = C.plan;
      image = C.image;
      std::rotate(g_cache.begin(), g_cache.begin() + q, g_cache.begin() + q + 1);
      return true;
    }
  }
  return false;
}

// m3s_set_knob: the previous value, or -(1 << 30) for a name this build does
// not know. A plan-shaping knob set to a different value drops the plan cache.
int set_knob(const char *name, int value) {
  Knobs &K = knobs();
  for (int k = 0; k < kNumKnobs; k++)
    if (std::strcmp(kKnobDefs[k].name, name) == 0) {
      const int old = K.v[k].exchange(value);
      if (kKnobDefs[k].shaping && old != value) {
        std::lock_guard<std::mutex> g(g_cache_mu);
        g_cache.clear();
      }
      return old;
    }
  return -(1 << 30);
}

// Symbolic plan + LDS budget + full-range task table for remapped ranks.
PlanMeta build_plan_meta(const m3s_gn_args *a, const Layout &Ly, const std::vector<int32_t> &ri,
                         const std::vector<int32_t> &rj, bool force_dense) {
  PlanMeta built;
  PlanRecord &R = built.plan;
  const int64_t E = a->E;
  if (a->N > 1) {
    SparsePlan P;
    // The dispatch schedule (witems) and the split update lists (PART items)
    // serve only the one-workgroup sparse_llt_kernel; a factor in global
    // memory on the chip-wide path (df_factor / tail / column back-
    // substitution) needs neither: at 256 KFs that halves the host analysis.
    build_sparse_plan((int)a->N, ri, rj, P, 0, 0, dense_tail_min(), false);
    const bool global_factor = sizeof(double) * ((size_t)(P.S + P.m) * 49 + (size_t)P.m * 7) > kMaxLdsBytes;
    // the chip-wide launches take a factor in global memory of up to 512
    // columns whose dense tail (if any) fits tail_llt_kernel's tiles
    const bool tail_fits = 7 * P.nc + 1 <= 16 * kTailMaxT;
    const bool chip_ok = cols_path() && P.m <= 512 && (P.nc == 0 || tail_fits);
    const bool chip_path = global_factor && chip_ok;
    if (global_factor && !chip_path)  // split long update lists for the staged global-factor products
      build_sparse_plan((int)a->N, ri, rj, P, kSplitUpdates, Ly.slot_cap - 1, dense_tail_min(), true);
    else if (!chip_path)
      schedule_plan_items(P);
    PlanImage img;
    flatten_plan(P, img);
    // df_factor_kernel's dispatch list: the sparse columns in level order,
    // DIAG(k) then the OFF tasks of column k, then the dense-tail border tasks
    R.off_dfitems = (int)img.data.size();
    for (int32_t k : P.corder) {
      img.data.push_back(-1 - k);
      for (int q = 0; q < P.col_ptr[k + 1] - P.col_ptr[k]; q++) img.data.push_back(P.ctask0[k] + q);
    }
    R.n_dfsparse = (int)img.data.size() - R.off_dfitems;
    for (int b = 0; b < P.nc * (P.nc + 1) / 2; b++) img.data.push_back((int32_t)P.task_dst.size() + b);
    R.n_dfitems = (int)img.data.size() - R.off_dfitems;
    const bool fits = (int64_t)img.data.size() <= Ly.plan_cap && P.S <= Ly.slot_cap;
    if (fits && !force_dense) {
      R.sparse = true;
      R.m = P.m;
      R.S = P.S;
      R.levels = P.levels;
      R.plan_len = (int)img.data.size();
      R.n_items = (int)P.items.size();
      R.n_tasks = (int)P.task_dst.size();
      R.n_parts = (int)P.part_q0.size();
      R.nc = P.nc;
      R.nnz = P.col_ptr.empty() ? 0 : P.col_ptr[P.m];
      // LDS plan of sparse_llt_kernel<STORE>: flags always, factor + W + y if
      // they fit, the plan too if it fits as well; else global factor with
      // per-wave stage areas
      const size_t flags_bytes =
          sizeof(int32_t) * (((size_t)(P.S + 2 * P.m + P.part_q0.size()) + 1) & ~size_t(1));
      const size_t fac_bytes = sizeof(double) * ((size_t)(P.S + P.m) * 49 + (size_t)P.m * 7);
      const size_t plan_bytes = sizeof(int32_t) * ((img.data.size() + 1) & ~size_t(1));
      const size_t stage_bytes = sizeof(double) * 16 * (size_t)kStageDoubles;
      const size_t fin_bytes = sizeof(double) * kFin * (size_t)E;
      if (fac_bytes + plan_bytes + flags_bytes <= kMaxLdsBytes) {
        R.store = 1;
        R.lds_bytes = fac_bytes + plan_bytes + flags_bytes;
      } else if (fac_bytes + flags_bytes <= kMaxLdsBytes) {
        R.store = 2;
        R.lds_bytes = fac_bytes + flags_bytes;
      }
      if (R.store != 0 && R.lds_bytes + fin_bytes <= kMaxLdsBytes) {
        R.asm_lds = true;
        R.lds_bytes += fin_bytes;
      }
      if (R.store == 0) {
        R.store = 0;
        R.lds_bytes = sizeof(double) * (size_t)P.m * 7 + flags_bytes + stage_bytes;
        if (R.lds_bytes > kMaxLdsBytes) R.sparse = false;  // dense fallback
      }
      std::copy(img.off, img.off + kPlanSections, R.off);
      built.h_plan = std::move(img.data);
      // the launches of this plan: the LDS kernels by what fits beside the
      // factor, else (a factor in global memory) over the chip, else on one
      // workgroup, split around the tail border when there is a dense tail
      if (R.store != 0)
        R.path = R.store == 1 ? SolvePath::lds_plan : SolvePath::lds;
      else if (chip_ok)
        R.path = SolvePath::chip;
      else
        R.path = P.nc > 0 && border_split() ? SolvePath::global_split : SolvePath::global;
      R.mfma_tail = tail_fits && tail_mfma();
    }
    if (!R.sparse) R.path = SolvePath::dense;
  }
  (void)E;
  return built;
}

// The per-call flag state the solve kernels of a plan rely on: the column-
// task / dataflow / dense-tail epoch flags live only on the global-factor
// path (the LDS-resident factors keep theirs in LDS), and no tagged granule
// of an earlier call may match this call's epochs.
bool reset_plan_flags(const PlanRecord &R, const Layout &Ly, void *ws, hipStream_t st) {
  bool ok = true;
  if (!(R.sparse && R.store != 0))
    ok &= hipMemsetAsync(at<int32_t>(ws, Ly.colsync), 0, Ly.tail - Ly.colsync, st) == hipSuccess;
  if (R.nc > 0)
    ok &= hipMemsetAsync(at<double>(ws, Ly.tail) + tail_gran_offset_doubles(), 0,
                         sizeof(double) * (tail_scratch_doubles() - tail_gran_offset_doubles()), st) == hipSuccess;
  return ok;
}

// Upload a plan on the device's side stream and make `st` wait for it: the
// copy runs while the first linearize kernel does instead of queueing behind
// it. Callers have waited for every earlier launch on `st` (the prologue's
// event or a stream sync), so nothing still running there reads `dst`.
bool upload_plan(Staging *SG, PlanMeta &M, char *dst, hipStream_t st) {
  if (!(M.plan.sparse && !M.h_plan.empty())) return true;
  const size_t nb = sizeof(int32_t) * M.h_plan.size();
  if (SG->plan_pending && hipEventSynchronize(SG->plan_ev) != hipSuccess) return false;
  SG->plan_pending = false;
  if (!pinned_reserve(SG->plan_up, SG->plan_cap, nb)) return false;
  memcpy(SG->plan_up, M.h_plan.data(), nb);
  bool ok = hipMemcpyAsync(dst, SG->plan_up, nb, hipMemcpyHostToDevice, SG->side) == hipSuccess;
  ok &= hipEventRecord(SG->plan_ev, SG->side) == hipSuccess;
  ok &= hipStreamWaitEvent(st, SG->plan_ev, 0) == hipSuccess;
  SG->plan_pending = ok;
  return ok;
}

// Test hook for the bounded waits (tests/test_gpu_backend.py, knob
// debug_drop_item): drop one item of sparse_llt_kernel's dispatch list, so the
// items that read its blocks wait on a flag that is never set; the waits time
// out and the iteration ends as a solve failure (dx = 0) instead of hanging.
// On the chip-wide path (global factor) the item is dropped from
// df_factor_kernel's dispatch list instead.
void apply_drop_item(PlanMeta &M) {
  const int d = drop_item_knob();
  PlanRecord &R = M.plan;
  if (d < 0 || !R.sparse || M.h_plan.empty()) return;
  if (R.store == 0 && R.n_dfitems > 0) {
    int32_t *di = M.h_plan.data() + R.off_dfitems;
    if (d < R.n_dfitems) {
      for (int t = d; t + 1 < R.n_dfitems; t++) di[t] = di[t + 1];
      R.n_dfitems -= 1;
    }
    return;
  }
  if (R.off[kSec_wave_ptr] >= (int64_t)M.h_plan.size()) return;
  int32_t *wp = M.h_plan.data() + R.off[kSec_wave_ptr], *wi = M.h_plan.data() + R.off[kSec_witems];
  if (d < wp[1]) {
    for (int t = d; t + 1 < wp[1]; t++) wi[t] = wi[t + 1];
    wp[1] -= 1;
  }
}

// A plan becomes the plan of the call behind registry entry M (a deferred
// plan just built, finish_plan; a cached one, host_finish): record and image
// into the entry, the per-plan flag resets, the test hook, the upload.
// Caller holds g_stage_mu and g_reg_mu.
int adopt_plan(Staging *SG, PlanMeta &M, const PlanRecord &plan, std::vector<int32_t> &&image, const Layout &Ly,
               void *ws, hipStream_t st) {
  M.plan = plan;
  M.h_plan = std::move(image);
  M.plan_pending = false;
  if (plan.sparse && plan.lds_bytes > 64 * 1024) set_lds_attributes_once();
  bool ok = reset_plan_flags(M.plan, Ly, ws, st);
  apply_drop_item(M);
  ok &= upload_plan(SG, M, at<char>(ws, Ly.plan), st);
  return ok ? M3S_OK : M3S_ELAUNCH;
}

// The host prepare, per solve call (the reference's _unique / searchsorted
// also synchronise): read ii/jj once — the call's only host sync — rank the
// ids, fetch the plan (or defer it to the first solve) and enqueue ONE
// upload of everything the launches read (pinned staging, above).
int gn_prepare_impl(const m3s_gn_args *a, hipStream_t st) {
  const Layout Ly = gn_layout(a->N, a->HW, a->E);
  void *ws = a->workspace;
  std::lock_guard<std::mutex> stage_lock(g_stage_mu);
  Staging *SG = stage_for_device();
  if (!SG) return M3S_ELAUNCH;
  if (SG->pending && hipEventSynchronize(SG->ev) != hipSuccess) return M3S_ELAUNCH;
  SG->pending = false;
  const int64_t E = a->E;
  if (!pinned_reserve(SG->down, SG->down_cap, 2 * sizeof(int64_t) * (size_t)E)) return M3S_ELAUNCH;
  int64_t *hii = reinterpret_cast<int64_t *>(SG->down), *hjj = hii + E;
  if (a->N > 1 && a->dx_out && hipMemsetAsync(a->dx_out, 0, sizeof(float) * 7 * (a->N - 1), st) != hipSuccess)
    return M3S_ELAUNCH;
  if (E > 0 && hipMemcpyAsync(hii, a->ii, sizeof(int64_t) * E, hipMemcpyDeviceToHost, st) != hipSuccess)
    return M3S_ELAUNCH;
  if (E > 0 && hipMemcpyAsync(hjj, a->jj, sizeof(int64_t) * E, hipMemcpyDeviceToHost, st) != hipSuccess)
    return M3S_ELAUNCH;
  if (hipStreamSynchronize(st) != hipSuccess) return M3S_ELAUNCH;
  std::vector<int32_t> ri, rj;
  const int nu = host_remap(hii, hjj, E, ri, rj);
  const bool bad = nu > a->N;
  const bool force_dense = force_dense_knob();
  PlanMeta meta;
  const bool hit = !bad && find_cached_plan(a, force_dense, ri, rj, meta.plan, meta.h_plan);
  if (!hit) {
    // the symbolic plan is built by the first solve of this call, while the
    // first linearize kernel runs (finish_plan); `sparse` is the expected
    // outcome until then (the dense path reads partials either way)
    meta.plan.sparse = !bad && !force_dense && a->N > 1;
    meta.plan_pending = !bad && a->N > 1;
    if (bad) meta.plan.path = SolvePath::dense;  // a stopped call: the dense launches return at the stop flag
  }
  meta.force_dense = force_dense;
  // ranks and the full range's edge order now (the first linearize needs them)
  std::vector<int32_t> eorder;
  if (E > 0) build_eorder(rj, 0, E, eorder);
  meta.h_ri = std::move(ri), meta.rj = std::move(rj);
  int32_t h_info[8] = {0}, h_flags[64] = {0};
  h_info[M3S_INFO_N_UNIQUE] = nu;
  if (bad) h_info[M3S_INFO_BAD_EDGE] = 1, h_flags[kFlagStop] = 1;
  meta.range_b = 0, meta.range_e = E, meta.order_ok = E > 0;
  if (meta.plan.sparse && !meta.plan_pending && meta.plan.lds_bytes > 64 * 1024) set_lds_attributes_once();
  std::lock_guard<std::mutex> g(g_reg_mu);
  PlanMeta &M = g_reg[ws];
  M = std::move(meta);
  bool ok = true;
  if (!M.plan_pending) ok &= reset_plan_flags(M.plan, Ly, ws, st);
  if (!M.plan_pending) apply_drop_item(M);
  // one upload: flags | rank_i | rank_j | edge counters | edge order [| plan] (the
  // layout keeps them in this order), then info (the caller's tensor) from
  // the same buffer
  const bool with_plan = M.plan.sparse && !M.plan_pending && !M.h_plan.empty();
  const bool with_tasks = E > 0;
  size_t n_up = with_plan ? Ly.plan - Ly.flags + sizeof(int32_t) * M.h_plan.size()
                          : with_tasks ? Ly.eorder - Ly.flags + sizeof(int32_t) * eorder.size()
                                       : Ly.edge_cnt - Ly.flags + edge_cnt_bytes(E);
  n_up = align_up(n_up, 16);
  if (!pinned_reserve(SG->up, SG->up_cap, n_up + sizeof h_info)) return M3S_ELAUNCH;
  char *up = SG->up;
  memcpy(up, h_flags, sizeof h_flags);
  memset(up + (Ly.edge_cnt - Ly.flags), 0, edge_cnt_bytes(E));  // the fused finalize's counters
  if (E > 0) {
    memcpy(up + (Ly.rank_i - Ly.flags), M.h_ri.data(), sizeof(int32_t) * E);
    memcpy(up + (Ly.rank_j - Ly.flags), M.rj.data(), sizeof(int32_t) * E);
  }
  if (with_tasks) memcpy(up + (Ly.eorder - Ly.flags), eorder.data(), sizeof(int32_t) * eorder.size());
  if (with_plan) memcpy(up + (Ly.plan - Ly.flags), M.h_plan.data(), sizeof(int32_t) * M.h_plan.size());
  memcpy(up + n_up, h_info, sizeof h_info);
  ok &= hipMemcpyAsync(at<char>(ws, Ly.flags), up, n_up, hipMemcpyHostToDevice, st) == hipSuccess;
  ok &= hipMemcpyAsync(a->info, up + n_up, sizeof h_info, hipMemcpyHostToDevice, st) == hipSuccess;
  ok &= hipEventRecord(SG->ev, st) == hipSuccess;
  SG->pending = ok;
  return ok ? M3S_OK : M3S_ELAUNCH;
}

// The deferred half of a cold prepare: the symbolic plan (ordering, fill,
// update lists; build_plan_meta) on the host, its upload, and the per-plan
// flag resets. Called by a call's first solve, i.e. after its first
// linearize is on the stream: the analysis runs while that kernel does.
int finish_plan(const m3s_gn_args *a, const Layout &Ly, hipStream_t st) {
  void *ws = a->workspace;
  std::vector<int32_t> ri, rj;
  bool force_dense;
  {
    std::lock_guard<std::mutex> g(g_reg_mu);
    auto it = g_reg.find(ws);
    if (it == g_reg.end()) return M3S_EINVAL;
    if (!it->second.plan_pending) return M3S_OK;
    ri = it->second.h_ri;
    rj = it->second.rj;
    force_dense = it->second.force_dense;
  }
  PlanMeta built = build_plan_meta(a, Ly, ri, rj, force_dense);
  std::lock_guard<std::mutex> stage_lock(g_stage_mu);
  Staging *SG = stage_for_device();
  if (!SG) return M3S_ELAUNCH;
  if (SG->plan_pending && hipEventSynchronize(SG->plan_ev) != hipSuccess) return M3S_ELAUNCH;
  SG->plan_pending = false;
  std::lock_guard<std::mutex> g(g_reg_mu);
  if (plan_cache_enabled()) {
    PlanCacheEntry C;
    C.N = a->N, C.HW = a->HW, C.E = a->E, C.dense = force_dense, C.ri = ri, C.rj = rj;
    C.tail_min = dense_tail_min();
    C.plan = built.plan, C.image = built.h_plan;
    std::lock_guard<std::mutex> gc(g_cache_mu);
    g_cache.insert(g_cache.begin(), std::move(C));
    if (g_cache.size() > kPlanCacheSize) g_cache.pop_back();
  }
  return adopt_plan(SG, g_reg[ws], built.plan, std::move(built.h_plan), Ly, ws, st);
}

// The host half of an async prepare (gn_prepare_async), at the first point a
// call needs its ids on the host (its first solve, or a sharded rank's edge
// range): wait for the prologue (normally long done: the first linearize is
// queued behind it), read ii / jj from the pinned slot, rank the ids on
// the host (the plan and its cache key need them), and fetch the cached plan;
// a miss leaves the plan to finish_plan. The linearize state of the entry
// (range, task table, planes) is the prologue's and stays.
int host_finish(const m3s_gn_args *a, hipStream_t st) {
  void *ws = a->workspace;
  int slot = -1;
  {
    std::lock_guard<std::mutex> g(g_reg_mu);
    auto it = g_reg.find(ws);
    if (it == g_reg.end()) return M3S_EINVAL;
    if (!it->second.host_pending) return M3S_OK;
    slot = it->second.slot;
  }
  const int64_t E = a->E;
  std::vector<int64_t> hii((size_t)E), hjj((size_t)E);
  {
    std::lock_guard<std::mutex> stage_lock(g_stage_mu);
    Staging *SG = stage_for_device();
    if (!SG || slot < 0 || slot >= (int)SG->slots.size()) return M3S_ELAUNCH;
    DownSlot &D = SG->slots[slot];
    if (hipEventSynchronize(D.ev) != hipSuccess) return M3S_ELAUNCH;
    if (E > 0) {
      memcpy(hii.data(), D.p + 64, sizeof(int64_t) * (size_t)E);
      memcpy(hjj.data(), D.p + 64 + sizeof(int64_t) * (size_t)E, sizeof(int64_t) * (size_t)E);
    }
    D.busy = false;
  }
  std::vector<int32_t> ri, rj;
  const int nu = host_remap(hii.data(), hjj.data(), E, ri, rj);
  const bool bad = nu > a->N;  // the prologue has stopped the call (flags, info)
  const Layout Ly = gn_layout(a->N, a->HW, a->E);
  bool force_dense;
  {
    std::lock_guard<std::mutex> g(g_reg_mu);
    force_dense = g_reg.at(ws).force_dense;
  }
  PlanRecord plan;
  std::vector<int32_t> image;
  const bool hit = !bad && find_cached_plan(a, force_dense, ri, rj, plan, image);
  std::lock_guard<std::mutex> stage_lock(g_stage_mu);
  Staging *SG = stage_for_device();
  if (!SG) return M3S_ELAUNCH;
  std::lock_guard<std::mutex> g(g_reg_mu);
  PlanMeta &M = g_reg[ws];
  M.host_pending = false, M.slot = -1;
  M.h_ri = std::move(ri), M.rj = std::move(rj);
  if (bad) {
    M.plan.sparse = false, M.plan.path = SolvePath::dense, M.plan_pending = false;
    return M3S_OK;
  }
  if (!hit) return M3S_OK;  // plan_pending: finish_plan builds it
  return adopt_plan(SG, M, plan, std::move(image), Ly, ws, st);
}

// Prepare a call without a host round trip: one prologue kernel on the stream
// (ranks, task table, flags, info, dx_out; the ids to pinned memory) and the
// registry entry; the host reads the ids later (host_finish), while the first
// linearize runs. Large edge sets (> kProMaxE) take the synchronous prepare.
int gn_prepare_async(const m3s_gn_args *a, hipStream_t st) {
  const int64_t E = a->E;
  if (E > kProMaxE || a->N > (int64_t)1 << 30 || knob<K_prologue>() == 0) return gn_prepare_impl(a, st);
  const Layout Ly = gn_layout(a->N, a->HW, E);
  void *ws = a->workspace;
  std::lock_guard<std::mutex> stage_lock(g_stage_mu);
  Staging *SG = stage_for_device();
  if (!SG) return M3S_ELAUNCH;
  const int slot = acquire_slot(*SG, 64 + 2 * sizeof(int64_t) * (size_t)E);
  if (slot < 0) return M3S_ELAUNCH;
  DownSlot &D = SG->slots[slot];
  ProArgs P;
  P.ii = a->ii, P.jj = a->jj;
  P.K = a->mode == M3S_MODE_CALIB ? a->K : nullptr;
  P.down_K = reinterpret_cast<float *>(D.dp);
  P.down_ii = reinterpret_cast<int64_t *>(D.dp + 64);
  P.down_jj = P.down_ii + E;
  P.E = (int)E, P.N = (int)a->N, P.P2 = prologue_p2(E);
  P.flags = at<int32_t>(ws, Ly.flags), P.rank_i = at<int32_t>(ws, Ly.rank_i), P.rank_j = at<int32_t>(ws, Ly.rank_j);
  P.eorder = at<int32_t>(ws, Ly.eorder), P.info = a->info, P.edge_cnt = at<uint32_t>(ws, Ly.edge_cnt);
  P.dx_out = a->dx_out;
  P.n_dx = (a->N > 1 && a->dx_out) ? (int)(7 * (a->N - 1)) : 0;
  const size_t lds = prologue_lds(P.E, P.P2);
  if (lds > 64 * 1024) set_lds_attributes_once();
  gn_prologue_kernel<<<1, kProThreads, lds, st>>>(P);
  if (launch_ok() != M3S_OK || hipEventRecord(D.ev, st) != hipSuccess) {
    D.busy = false;
    return M3S_ELAUNCH;
  }
  PlanMeta meta;
  meta.host_pending = true, meta.slot = slot;
  meta.force_dense = force_dense_knob();
  meta.plan.sparse = !meta.force_dense && a->N > 1;  // the expected outcome (the dense path reads partials either way)
  meta.plan_pending = a->N > 1;
  meta.range_b = 0, meta.range_e = E, meta.order_ok = E > 0;
  std::lock_guard<std::mutex> g(g_reg_mu);
  PlanMeta &M = g_reg[ws];
  if (M.host_pending && M.slot >= 0 && M.slot < (int)SG->slots.size() && M.slot != slot)
    SG->slots[M.slot].busy = false;  // a re-prepare of a workspace whose ids were never read
  M = std::move(meta);
  return M3S_OK;
}

// m3s_gn_release: drop the registry entry of a workspace. No stream sync:
// every queued upload reads pinned staging, not the entry.
int gn_release_impl(const m3s_gn_args *a) {
  if (!a || !a->workspace) return M3S_EINVAL;
  std::lock_guard<std::mutex> stage_lock(g_stage_mu);  // (lock order: staging, then registry)
  std::lock_guard<std::mutex> g(g_reg_mu);
  auto it = g_reg.find(a->workspace);
  if (it == g_reg.end()) return M3S_OK;
  if (it->second.host_pending && it->second.slot >= 0) {  // ids never read: free the slot (its
    Staging *SG = stage_for_device();                      // event guards the reuse)
    if (SG && it->second.slot < (int)SG->slots.size()) SG->slots[it->second.slot].busy = false;
  }
  g_reg.erase(it);
  return M3S_OK;
}

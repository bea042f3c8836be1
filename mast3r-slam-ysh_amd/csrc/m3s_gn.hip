// m3s_gn.hip — MI355X (gfx950) Gauss-Newton backend and tracker for MASt3R-SLAM.
//
// One translation unit, and this file is its map, its list and its exports:
// the map of who launches what (below), the system and project includes, the
// three vector typedefs, the list of the parts inside one anonymous namespace,
// and the C exports. All device code and the host code behind the exports live
// in the parts, csrc/gn/*.h: the constants and the workspace (gn/layout.h),
// the backend's device code (gn/linearize.h, gn/gather.h, gn/assemble.h,
// gn/chol_tiled.h, gn/llt_blocks.h, gn/sparse_llt.h, gn/col_tasks.h,
// gn/dataflow.h, gn/tail_llt.h, gn/tail_cyc.h, gn/tail_pair.h,
// gn/chol_small.h, gn/prologue.h, gn/border.h), then the host side of the
// backend (gn/args.h, gn/knobs.h, gn/launch.h, gn/plan.h, gn/iterate.h,
// gn/solve.h: the launch functions of the solve, one per path of a plan), the
// tracker (gn/track.h) and the track_frame front end (gn/track_frame.h), then
// the two debug kernels (gn/debug.h). The gn/*.h files are parts of this file,
// not stand-alone headers: each is text inside the one anonymous namespace
// opened below, has no includes or guards of its own, and relies on what
// stands before it. Every launch is on the caller's stream; a call does not
// wait for the device except where noted. The rule lines (`// ---- name --`)
// that named the sections of this file now head them inside the parts.
//
// gauss_newton_{points,rays,calib} (gn_full, gn/iterate.h):
//   prepare    gn_prologue_kernel (gn/prologue.h): ranks the edge ids, writes the
//              linearize edge order, flags, info, dx; the ids go to pinned memory
//              and the host builds (or fetches from the plan cache) the symbolic
//              plan while the first linearize runs (gn/plan.h). Above 2048
//              edges: the host prepare (one stream sync, gn_prepare_impl).
//   iteration  1 linearize launch (gn/launch.h); its last chunk of an edge
//              finalizes the edge:
//                first iteration   linearize_gather_kernel (gn/gather.h, the
//                                  pipelined gathering launch), or
//                                  linearize_kernel (gn/linearize.h) where the
//                                  gathering kernel does not apply
//                later iterations  linearize_packed_kernel (gn/linearize.h)
//              then the solve (gn_solve_impl, gn/solve.h), by the path that
//              build_plan_meta (gn/plan.h) wrote into the plan (SolvePath), one
//              launch function per path:
//                factor fits the LDS (small graphs; lds_plan / lds, solve_lds):
//                  sparse_llt_kernel<1> / <2>
//                  (gn/sparse_llt.h), one workgroup: assembly, LLT,
//                  back-substitution, retraction, stop flag;
//                  assemble_slots_kernel (gn/llt_blocks.h) first when the
//                  staged edge blocks do not fit beside the factor
//                else, up to 512 columns (large graphs), over the chip (chip,
//                  solve_chip):
//                  assemble_slots_kernel,
//                  df_factor_kernel (gn/dataflow.h, the wave-level dataflow
//                  factorisation),
//                  tail_pair_kernel (gn/tail_pair.h) when the plan has a dense
//                  tail (from 32 tail columns its extra workgroups run the
//                  sparse back-substitution, gcol_worker, gn/tail_pair.h),
//                  else col_backsub_kernel (gn/dataflow.h)
//                else (global_split / global, solve_global): sparse_llt_kernel<0>,
//                  in two phases around border_kernel (gn/border.h) and
//                  tail_llt_kernel (gn/tail_llt.h, the dense tail on the f64
//                  MFMA) with a dense tail
//                no sparse plan that fits (dense, solve_dense):
//                  edge_reduce_kernel (gn/gather.h),
//                  assemble_kernel (gn/assemble.h) and the tiled dense Cholesky:
//                  potrf_tile_kernel (gn/chol_tiled.h), trsm_tile_kernel
//                  (gn/chol_tiled.h), update_tiles_kernel (gn/chol_tiled.h),
//                  backsolve_kernel (gn/chol_tiled.h)
//   The stepwise API (m3s_gn_prepare / _linearize / _solve, sharded ranks) runs
//   the same launches, with finalize_edges_kernel (gn/llt_blocks.h) ahead of a
//   sparse solve.
// track_{rays,calib}_sim3 (track_impl, gn/track.h): track_init_kernel
//   (gn/track.h), then track_persistent_kernel (gn/track.h; every iteration in
//   one launch), or per iteration one linearize_kernel<MODE, TRACK> whose last
//   chunk runs track_solve_block (gn/track.h). calib reads K back once (a
//   stream sync).
// track_frame (track_frame_impl, gn/track_frame.h): track_prep_clear_kernel
//   (gn/track_frame.h), track_prep_kernel (gn/track_frame.h),
//   track_prep_count_kernel (gn/track_frame.h), then the tracker's launches.
// The test build (-DM3S_TEST_PATHS) adds the A/B reference paths behind the
// test-only knobs (gn/knobs.h): col_factor_kernel (gn/col_tasks.h),
// chol_small_kernel (gn/chol_small.h), tail_cyc_kernel (gn/tail_cyc.h), the
// VGPR-staged gathering kernel.
// m3s_debug_copy / m3s_debug_sim3: hbm_copy_kernel (gn/debug.h),
// sim3_debug_kernel (gn/debug.h).
//
// Order rule: the include list is the order of the device code. The parts keep
// their places in the list, device functions and kernels keep their relative
// order inside a part, and the first host mention of each kernel template
// stays where it is (gn/launch.h, gn/plan.h, gn/iterate.h, gn/solve.h; it
// decides where the instantiation lands: gn/solve.h stands behind
// gn/iterate.h because the linearize templates come first, and its launch
// functions stand in the order chip, lds, global, dense, then
// set_lds_attributes_once). The code object holds real calls to
// non-inlined device functions, so a reordering changes pc-relative literals
// and the device code can no longer be compared instruction for instruction
// with the build before (tools/code_identity.py). Host code may move otherwise.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cstring>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "m3s_device.h"
#include "m3s_gn.h"
#include "m3s_symbolic.h"

using namespace m3s;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef long long i64x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace {

#include "gn/layout.h"
#include "gn/linearize.h"
#include "gn/gather.h"
#include "gn/assemble.h"
#include "gn/chol_tiled.h"
#include "gn/llt_blocks.h"
#include "gn/sparse_llt.h"
#include "gn/col_tasks.h"
#include "gn/dataflow.h"
#include "gn/tail_llt.h"
#include "gn/tail_cyc.h"
#include "gn/tail_pair.h"
#include "gn/chol_small.h"
#include "gn/prologue.h"
#include "gn/border.h"
#include "gn/args.h"
#include "gn/knobs.h"
#include "gn/launch.h"
#include "gn/plan.h"
#include "gn/iterate.h"
#include "gn/solve.h"
#include "gn/track.h"
#include "gn/track_frame.h"
#include "gn/debug.h"

}  // namespace

// ------------------------------------------------------------ C exports --
extern "C" {

size_t m3s_gn_workspace_size(int64_t N, int64_t HW, int64_t E) { return gn_layout(N, HW, E).total; }

int m3s_gauss_newton_points(const m3s_gn_args *a, void *stream) { return gn_full(a, M3S_MODE_POINTS, stream); }
int m3s_gauss_newton_rays(const m3s_gn_args *a, void *stream) { return gn_full(a, M3S_MODE_RAYS, stream); }
int m3s_gauss_newton_calib(const m3s_gn_args *a, void *stream) { return gn_full(a, M3S_MODE_CALIB, stream); }

int m3s_gn_prepare(const m3s_gn_args *a, void *stream) {
  int rc = check_args(a);
  if (rc) return rc;
  return gn_prepare_async(a, S(stream));
}

int m3s_gn_linearize(const m3s_gn_args *a, int64_t edge_begin, int64_t edge_end, double *edge_sums,
                     void *stream) {
  int rc = check_args(a);
  if (rc) return rc;
  if (edge_begin < 0 || edge_end > a->E || edge_begin > edge_end) return M3S_EINVAL;
  const ResidualParams P = make_params(a);  // calib intrinsics: read by the kernels (LinArgs::Kd)
  return gn_linearize_impl(a, P, edge_begin, edge_end, edge_sums, S(stream));
}

int m3s_gn_solve(const m3s_gn_args *a, const double *edge_sums, void *stream) {
  int rc = check_args(a);
  if (rc) return rc;
  if (!edge_sums) return M3S_EINVAL;
  if (gn_layout(a->N, a->HW, a->E).ld > kMaxLd) return M3S_ETOOLARGE;
  return gn_solve_impl(a, edge_sums, nullptr, 0, S(stream));
}

int m3s_gn_release(const m3s_gn_args *a, void *) { return gn_release_impl(a); }

size_t m3s_track_workspace_size(int64_t HW) {
  const int64_t chunks = chunks_for(HW, 1);
  const size_t parts = std::max<size_t>((size_t)(chunks + 1), 2 * (size_t)kTrkMaxBlocks);
  return track_part_off() + align_up(sizeof(float) * kNP * parts, 256);
}

int m3s_track_rays_sim3(const m3s_track_args *a, void *stream) { return track_impl(a, M3S_MODE_RAYS, stream); }
int m3s_track_calib_sim3(const m3s_track_args *a, void *stream) { return track_impl(a, M3S_MODE_CALIB, stream); }

size_t m3s_track_frame_workspace_size(int64_t HW) { return frame_layout(HW).total; }
int m3s_track_frame(const m3s_track_frame_args *a, void *stream) { return track_frame_impl(a, stream); }

const char *m3s_version(void) { return "m3s-gn 0.2 gfx950"; }

int64_t m3s_sparse_plan_debug(int32_t N, int64_t E, const int32_t *ri, const int32_t *rj, int32_t split,
                              int32_t max_parts, int32_t *out, int64_t cap, int32_t *meta) {
  std::vector<int32_t> a(ri, ri + E), b(rj, rj + E);
  SparsePlan P;
  build_sparse_plan(N, a, b, P, split, max_parts, dense_tail_min());
  PlanImage I;
  flatten_plan(P, I);
  if (meta) {
    meta[0] = P.m, meta[1] = P.S, meta[2] = P.levels;
    std::copy(I.off, I.off + kPlanSections, meta + 3);
    meta[3 + kPlanSections] = (int32_t)P.part_q0.size();
  }
  const int64_t n = (int64_t)I.data.size();
  if (out && cap >= n) std::copy(I.data.begin(), I.data.end(), out);
  return n;
}

// Instrumented builds only (tools/trk_stamps.py, tools/col_stamps.py):
// which = 0: persistent tracker phase stamps [2][16][8] (-DM3S_TRK_STAMPS);
// which = 1: column-task stamps [4][2048][4] (-DM3S_COL_STAMPS: factor
// DIAG / column tasks, back-substitution, tail_cyc_kernel columns, OFF items
// by slot). Wall-clock
// ticks (100 MHz). Returns 1, or 0 when the build has no such stamps.
int m3s_debug_stamps(int which, int64_t *out) {
  if (hipDeviceSynchronize() != hipSuccess) return M3S_ELAUNCH;
#ifdef M3S_TRK_STAMPS
  if (which == 0)
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trk_stamp), sizeof(g_trk_stamp)) == hipSuccess ? 1 : M3S_ELAUNCH;
#endif
#ifdef M3S_COL_STAMPS
  if (which == 1)
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_col_stamp), sizeof(g_col_stamp)) == hipSuccess ? 1 : M3S_ELAUNCH;
#endif
#ifdef M3S_LLT_STAMPS
  if (which == 2) {  // [2048][4] stamps, then [2048][2] items (as int64), then [8] phases
    int32_t items[2048][2];
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_llt_stamp), sizeof(g_llt_stamp)) != hipSuccess ||
        hipMemcpyFromSymbol(items, HIP_SYMBOL(g_llt_item), sizeof(items)) != hipSuccess ||
        hipMemcpyFromSymbol(out + 2048 * 4 + 2048 * 2, HIP_SYMBOL(g_llt_phase), sizeof(g_llt_phase)) != hipSuccess)
      return M3S_ELAUNCH;
    for (int q = 0; q < 2048; q++) out[2048 * 4 + 2 * q] = items[q][0], out[2048 * 4 + 2 * q + 1] = items[q][1];
    return 1;
  }
#endif
  (void)which;
  (void)out;
  return 0;
}

int m3s_set_knob(const char *name, int value) {
  if (!name) return M3S_EINVAL;
  return set_knob(name, value);
}

int m3s_debug_call_timing(int enable) {
  CallTiming &T = call_timing();
  std::lock_guard<std::mutex> g(T.mu);
  T.on = enable != 0;
  T.used = 0;
  T.kused = 0;
  return M3S_OK;
}

int m3s_debug_call_times(float *ms, int32_t *kinds, int cap) {
  CallTiming &T = call_timing();
  std::lock_guard<std::mutex> g(T.mu);
  if (T.used == 0) return 0;
  if (hipEventSynchronize(T.ev[T.used - 1]) != hipSuccess) return M3S_ELAUNCH;
  // every span (kinds 0, 1 linearize, 2 solve) has an event pair in kev: the
  // dispatch's own begin / end (hipExtLaunchKernel) when its work was one
  // launch that took the pair, else the events recorded around its launches
  int n = 0;
  size_t li = 0;
  for (size_t q = 0; q + 1 < T.used; q++) {
    if (T.kind[q] < 0) continue;
    if (n < cap) {
      float t = 0.0f;
      const bool own = li + 1 < T.kused && T.kev_ok[li / 2];
      if (hipEventElapsedTime(&t, own ? T.kev[li] : T.ev[q], own ? T.kev[li + 1] : T.ev[q + 1]) != hipSuccess)
        return M3S_ELAUNCH;
      ms[n] = t;
      kinds[n] = T.kind[q];
    }
    li += 2;
    n++;
  }
  T.used = 0;
  T.kused = 0;
  return n;
}

int m3s_debug_copy(const void *src, void *dst, int64_t nbytes, int blocks, void *stream) {
  if (!src || !dst || nbytes < 0 || (nbytes & 15) || (((uintptr_t)src | (uintptr_t)dst) & 15) || blocks <= 0)
    return M3S_EINVAL;
  if (nbytes == 0) return M3S_OK;
  hbm_copy_kernel<<<blocks, 256, 0, S(stream)>>>(reinterpret_cast<const f32x4 *>(src), reinterpret_cast<f32x4 *>(dst),
                                                 nbytes / 16);
  return hipGetLastError() == hipSuccess ? M3S_OK : M3S_ELAUNCH;
}

int m3s_debug_sim3(int op, const float *a, const float *b, float *out, int64_t n, void *stream) {
  if (op < 0 || op > 8 || n < 0 || !a || !out || (op != 0 && op != 3 && op != 7 && !b)) return M3S_EINVAL;
  if (n == 0) return M3S_OK;
  sim3_debug_kernel<<<(unsigned)((n + 255) / 256), 256, 0, S(stream)>>>(op, a, b, out, n);
  return hipGetLastError() == hipSuccess ? M3S_OK : M3S_ELAUNCH;
}

const char *m3s_gn_plan_path_debug(int64_t N, int64_t HW, int64_t E, const int32_t *ri, const int32_t *rj) {
  if (N < 1 || HW < 1 || E < 0 || (E > 0 && (!ri || !rj))) return nullptr;
  for (int64_t e = 0; e < E; e++)
    if (ri[e] < 0 || ri[e] >= N || rj[e] < 0 || rj[e] >= N) return nullptr;
  m3s_gn_args a{};
  a.N = N, a.HW = HW, a.E = E;
  const PlanMeta built = build_plan_meta(&a, gn_layout(N, HW, E), std::vector<int32_t>(ri, ri + E),
                                         std::vector<int32_t>(rj, rj + E), force_dense_knob());
  return kSolvePathNames[(int)built.plan.path];
}

size_t m3s_gn_layout_debug(int64_t N, int64_t HW, int64_t E, size_t *offs) {
  const Layout L = gn_layout(N, HW, E);
  const size_t o[15] = {L.flags, L.rank_i, L.rank_j, L.first, L.partials, L.edge_sums, L.A, L.fin,
                        L.plan,  L.Lblk,   L.Dinv,   L.tail,  L.eorder,   L.planes,    L.total};
  if (offs) std::copy(o, o + 15, offs);
  return L.total;
}

}  // extern "C"

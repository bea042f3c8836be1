// m3s_gn.hip — MI355X (gfx950) Gauss-Newton backend and tracker for MASt3R-SLAM.
//
// One translation unit: the backend's device code, section by section, below
// as far as the dense tail on the f64 MFMA and from there in parts
// (gn/tail_cyc.h, gn/tail_pair.h, gn/chol_small.h, gn/prologue.h, gn/border.h),
// then the host side of the backend (gn/args.h, gn/knobs.h, gn/launch.h,
// gn/plan.h, gn/iterate.h), the tracker (gn/track.h) and the track_frame front
// end (gn/track_frame.h), then the two debug kernels (gn/debug.h) and the C
// exports. The gn/*.h files are parts of this file, not
// stand-alone headers: each is text inside the one anonymous namespace opened
// below, has no includes or guards of its own, and relies on what stands
// before it. Every launch is on the caller's stream; a call does not wait for
// the device except where noted. Sections of this file are named by their rule
// lines (`// ---- name --`).
//
// gauss_newton_{points,rays,calib} (gn_full, gn/iterate.h):
//   prepare    gn_prologue_kernel (gn/prologue.h): ranks the edge ids, writes the
//              linearize edge order, flags, info, dx; the ids go to pinned memory
//              and the host builds (or fetches from the plan cache) the symbolic
//              plan while the first linearize runs (gn/plan.h). Above 2048
//              edges: the host prepare (one stream sync, gn_prepare_impl).
//   iteration  1 linearize launch (gn/launch.h); its last chunk of an edge
//              finalizes the edge:
//                first iteration   linearize_gather_kernel (pipelined gathering
//                                  launch), or linearize_kernel (linearize)
//                                  where the gathering kernel does not apply
//                later iterations  linearize_packed_kernel (linearize)
//              then the solve (gn_solve_impl, gn/iterate.h), by the plan:
//                factor fits the LDS (small graphs): sparse_llt_kernel<1> / <2>,
//                  one workgroup: assembly, LLT, back-substitution, retraction,
//                  stop flag (block-sparse LLT; assemble_slots_kernel first when
//                  the staged edge blocks do not fit beside the factor)
//                else, up to 512 columns (large graphs), over the chip:
//                  assemble_slots_kernel (block-sparse LLT),
//                  df_factor_kernel (wave-level dataflow factorisation),
//                  tail_pair_kernel (gn/tail_pair.h) when the plan has a dense
//                  tail (from 32 tail columns its extra workgroups run the
//                  sparse back-substitution, gcol_worker, gn/tail_pair.h),
//                  else col_backsub_kernel (dataflow)
//                else: sparse_llt_kernel<0>, in two phases around border_kernel
//                  (gn/border.h) and tail_llt_kernel (dense tail on the f64
//                  MFMA) with a dense tail
//                no sparse plan that fits: edge_reduce_kernel (gathering launch),
//                  assemble_kernel and the tiled dense Cholesky (assemble)
//   The stepwise API (m3s_gn_prepare / _linearize / _solve, sharded ranks) runs
//   the same launches, with finalize_edges_kernel ahead of a sparse solve.
// track_{rays,calib}_sim3 (track_impl, gn/track.h): track_init_kernel, then
//   track_persistent_kernel (every iteration in one launch), or per iteration
//   one linearize_kernel<MODE, TRACK> whose last chunk runs track_solve_block.
//   calib reads K back once (a stream sync).
// track_frame (track_frame_impl, gn/track_frame.h): track_prep_clear_kernel,
//   track_prep_kernel, track_prep_count_kernel, then the tracker's launches.
// The test build (-DM3S_TEST_PATHS) adds the A/B reference paths behind the
// test-only knobs (gn/knobs.h): col_factor_kernel (column tasks),
// chol_small_kernel (gn/chol_small.h), tail_cyc_kernel (gn/tail_cyc.h), the
// VGPR-staged gathering kernel.
// m3s_debug_copy / m3s_debug_sim3: hbm_copy_kernel, sim3_debug_kernel
// (gn/debug.h).
//
// Order rule: the sections below and then the include list are the order of
// the device code. The parts keep their places in the list, device functions
// and kernels keep their relative order, in this file and inside a part, and
// the first host mention of each kernel template keeps its place (gn/launch.h, gn/plan.h, gn/iterate.h; it decides
// where the instantiation lands). The code object holds real calls to
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

constexpr int kThreads = 256;        // linearize block
constexpr int kPixPerThread = 4;     // one 16-B vector group
constexpr int kBlockPix = kThreads * kPixPerThread;  // 1024 pixels per block sweep
#ifndef M3S_TARGET_BLOCKS
#define M3S_TARGET_BLOCKS 2048
#endif
constexpr int kTargetBlocks = M3S_TARGET_BLOCKS;  // linearize grid target (edges x chunks)
#ifndef M3S_GATHER_BLOCKS
#define M3S_GATHER_BLOCKS 6400
#endif
// the gathering kernel (first GN iteration) prefers ~3x smaller chunks: its
// random Xi reads then stay closer together in time per XCD (C3: 249 -> 232
// us, 128 KFs rays: 1092 -> 1004 us; profiles/r03/tb_sweep_r3f.txt)
constexpr int kGatherBlocks = M3S_GATHER_BLOCKS;
#ifndef M3S_MAX_BLOCKS
#define M3S_MAX_BLOCKS 8192
#endif
constexpr int kMaxBlocks = M3S_MAX_BLOCKS;  // workspace capacity for partials (>= both targets)
static_assert(kTargetBlocks <= kMaxBlocks && kGatherBlocks <= kMaxBlocks, "linearize grid target above capacity");
constexpr int kMaxSmallNp = 224;     // register Cholesky limit (n + 1 <= 7 * 32)
constexpr int kCholThreads = 512;    // 16 x 32 thread grid
constexpr int64_t kMaxLd = 8192;     // tiled path: back-substitution keeps x in LDS

// workspace-resident flags (int32)
constexpr int kFlagStop = 0;  // set when converged / bad input: later launches no-op
constexpr int kFlagFail = 1;  // set by the tiled Cholesky on a non-positive pivot (per iteration)
constexpr int kFlagSplitFail = 2;  // sparse LLT split launches: a pivot failure before the tail border

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline int64_t chunks_for(int64_t HW, int64_t E_loc, int64_t target = kTargetBlocks) {
  const int64_t max_chunks = (HW + kBlockPix - 1) / kBlockPix;
  int64_t c = (target + E_loc - 1) / (E_loc > 0 ? E_loc : 1);
  if (c < 1) c = 1;
  if (c > max_chunks) c = max_chunks;
  // make the chunk a multiple of kBlockPix, then recount
  int64_t ch = (HW + c - 1) / c;
  ch = (ch + kBlockPix - 1) / kBlockPix * kBlockPix;
  return (HW + ch - 1) / ch;
}
// bytes per edge of the validity nibbles (HW / 4, padded: 8-B loads stay aligned)
inline int64_t chunk_pixels(int64_t HW, int64_t chunks) {
  int64_t ch = (HW + chunks - 1) / chunks;
  return (ch + kBlockPix - 1) / kBlockPix * kBlockPix;
}

// tail_llt_kernel (dense top of the elimination tree on the f64 MFMA): tile
// rows (n + 1 <= 16 kTailMaxT) and its scratch (dense bordered tail, L tiles,
// W_k); see the kernel
constexpr int kTailMaxT = 32;
inline size_t tail_gran_offset_doubles() {  // tail scratch: dense tail, Lg, Wg, y', LgT, then the granules
  const size_t nmax = 16 * kTailMaxT;
  return nmax * nmax + (size_t)kTailMaxT * (kTailMaxT + 1) / 2 * 256 * 2 + (size_t)kTailMaxT * 256 + nmax;
}
constexpr int kGNx = 16 * kTailMaxT + 8;  // columns of X_k: a_k and one per tail dof (gcol_worker), padded
inline size_t tail_scratch_doubles() {  // dense tail, L tiles, W_k, y' (tail_cyc_kernel)
  // + the tagged-granule copy of the L tiles (tail_cyc_kernel hand-offs, 16 B per entry)
  return tail_gran_offset_doubles() + (size_t)kTailMaxT * (kTailMaxT + 1) / 2 * 256 * 2;
}

struct Layout {
  size_t flags, rank_i, rank_j, first, edge_cnt, partials, edge_sums, A, fin, plan, Lblk, Dinv, rhs, parts,
      colsync, wgran, tail, gx, eorder, planes, total;
  int64_t n, ld;          // system size 7(N-1); leading dim of the RHS-augmented matrix
  int64_t plan_cap, slot_cap;  // sparse-LLT capacities (int32 plan words, 7x7 slots)
};

constexpr int kTile = 64;  // tiled Cholesky tile (large systems)
inline int64_t aug_ld(int64_t n) { return (n + 1 + kTile - 1) / kTile * kTile; }

inline size_t edge_cnt_bytes(int64_t E) { return (sizeof(uint32_t) * (size_t)(E + 1) + 15) & ~size_t(15); }

inline Layout gn_layout(int64_t N, int64_t HW, int64_t E) {
  Layout L;
  const int64_t n = 7 * (N > 1 ? N - 1 : 0);
  const int64_t max_partials = kMaxBlocks + E + 1;
  size_t off = 0;
  L.flags = off;
  off = align_up(off + 64 * sizeof(int32_t), 256);
  L.rank_i = off;
  off = align_up(off + sizeof(int32_t) * (size_t)(E + 1), 256);
  L.rank_j = off;
  off = align_up(off + sizeof(int32_t) * (size_t)(E + 1), 256);
  // flags, ranks, edge counters, linearize task table and sparse plan are
  // contiguous: one H2D copy per call uploads them all (gn_prepare_impl)
  const int64_t m0 = N > 1 ? N - 1 : 0;
  L.edge_cnt = off;  // per-edge chunk arrival counters (fused finalize), zeroed per call (by the upload)
  off = align_up(off + edge_cnt_bytes(E), 256);
  L.eorder = off;  // linearize edge order (block -> (edge, chunk), block_task)
  off = align_up(off + sizeof(int32_t) * (size_t)(E + 16), 256);
  L.slot_cap = std::min<int64_t>(m0 * (m0 + 1) / 2, 64 * m0 + 4096) + 1;
  L.plan_cap = (int64_t(1) << 22) + 16 * E + 64 * m0;
  L.plan = off;
  off = align_up(off + sizeof(int32_t) * (size_t)L.plan_cap, 256);
  L.first = off;
  off = align_up(off + sizeof(int32_t) * (size_t)(2 * E + 1), 256);
  L.partials = off;
  off = align_up(off + sizeof(float) * kNP * (size_t)max_partials, 256);
  L.edge_sums = off;
  off = align_up(off + sizeof(double) * kNP * (size_t)(E + 1), 256);
  L.n = n;
  L.ld = aug_ld(n);
  L.A = off;
  off = align_up(off + sizeof(double) * (size_t)(L.ld * L.ld), 256);
  const int64_t m = N > 1 ? N - 1 : 0;
  L.fin = off;
  off = align_up(off + sizeof(double) * 56 * (size_t)(E + 1), 256);
  L.Lblk = off;
  off = align_up(off + sizeof(double) * 49 * (size_t)L.slot_cap, 256);
  L.Dinv = off;
  off = align_up(off + sizeof(double) * 49 * (size_t)(m + 1), 256);
  L.rhs = off;
  off = align_up(off + sizeof(double) * 7 * (size_t)(m + 1), 256);
  L.parts = off;  // split update partials, at most slot_cap of them
  off = align_up(off + sizeof(double) * 56 * (size_t)L.slot_cap, 256);
  L.colsync = off;  // column tasks: done[m+1], done2[m+1], tickets, slot flags [slot_cap], tail flags,
                    // X_k chunk counters [m+1], border task flags (epoch-tagged, zeroed per call)
  off = align_up(off + sizeof(int32_t) * (size_t)(3 * (m + 1) + 16 + L.slot_cap + 2 * kTailMaxT), 256);
  L.wgran = off;  // df_factor_kernel: W_k of every column as 16-B tagged granules (zeroed with colsync per call)
  off = align_up(off + (size_t)16 * 49 * (size_t)(m + 1), 256);
  L.tail = off;  // tail_llt_kernel scratch: dense bordered tail, L tiles, W_k
  off = align_up(off + sizeof(double) * tail_scratch_doubles(), 256);
  L.gx = off;  // the sparse columns' X_k = [a_k | B_k] (gcol_worker), [m][7][kGNx]
  off = align_up(off + sizeof(double) * 7 * kGNx * (size_t)(m + 1), 256);
  // target-side planes of every edge (4 planes = rays / points, the widest modes)
  L.planes = off;
  off = align_up(off + sizeof(float) * 4 * (size_t)E * (size_t)HW, 256);
  L.total = off;
  return L;
}

template <typename T>
inline T *at(void *base, size_t off) {
  return reinterpret_cast<T *>(static_cast<char *>(base) + off);
}

// tracker state (workspace, one per call): the relative pose being refined,
// the convergence state, and the chunk arrival counter of the fused solve
struct TrackState {
  float T_rel[8];   // T_CkCf
  float T_WCk[8];
  double old_cost;
  int32_t done;
  uint32_t arrive;  // linearize chunks arrived (all iterations of the call)
};
struct LinArgs;
__device__ void track_solve_block(const LinArgs &A);

// ------------------------------------------------------------- linearize --
struct LinArgs {
  const float *Twc;        // backend: poses (rank order)
  const float *T_rel;      // tracker: T_CkCf (single pose), else null
  const float *Xs;
  const float *Cs;
  const float *Xsrc;       // tracker: Xf (source points); backend: unused
  const int64_t *idx;
  int idx32;  // idx holds int32 (m3s_gn_args.idx_i32)
  const uint8_t *valid;
  const float *Q;
  const int32_t *rank_i;
  const int32_t *rank_j;
  const int32_t *stop;
  const int32_t *eorder;   // the launch's edges sorted by KF j (block_task); null: block = task
  int64_t per, E_loc;      // block_task: 8 runs of `per` blocks; edges of the launch
  uint32_t cnt_base;       // edge_cnt arrivals before this launch in the call (edge_tail)
  float *planes;           // per-edge target-side planes (PixIn), [E_loc][kPlanes][HW]
  float *partials;         // [task][36]
  uint32_t *edge_cnt;      // non-null: the last chunk of an edge to finish also finalizes it into fin
  double *esum;            // non-null (stepwise API): that chunk writes the edge's fp64 sums here instead
  double *fin;             // [E][kFin] per-edge blocks M L M^T, M g (fused finalize)
  TrackState *track;       // tracker: the last chunk of an iteration runs the 7x7 solve (else null)
  int32_t *info;           // tracker outputs / convergence rule
  float *T_WCf_out, *T_CkCf_out;
  float rel_error, delta_norm;
  int64_t HW, edge_begin, chunks, chunk_pix;
  ResidualParams P;
  const float *Kd;  // calib backend: the caller's 3x3 K (device), read by the kernels (P.fx.. unset)
};

// The residual parameters of a launch: the intrinsics of a calib backend
// launch come from the caller's K on the device (uniform loads), so the first
// linearize of a call can be enqueued before the host has read anything back.
__device__ __forceinline__ ResidualParams kparams(const LinArgs &A) {
  ResidualParams P = A.P;
  if (A.Kd) P.fx = A.Kd[0], P.fy = A.Kd[4], P.cx = A.Kd[2], P.cy = A.Kd[5];
  return P;
}

// one pixel's gathered inputs -> target-side inputs (shared by all paths)
template <int MODE, bool TRACK>
__device__ __forceinline__ PixIn<MODE> gather_pixel(const LinArgs &A, const float *Xs_i, const float *Cs_i,
                                                    int64_t p, bool vm, int64_t id_raw, float q, float cj) {
  const int64_t id = TRACK ? p : (vm ? id_raw : 0);
  const float Xi[3] = {Xs_i[3 * id + 0], Xs_i[3 * id + 1], Xs_i[3 * id + 2]};
  bool ok;
  if (TRACK) {
    ok = vm;
  } else {
    const float ci = Cs_i[id];
    ok = vm && (q > A.P.Q_thresh) && (ci > A.P.C_thresh) && (cj > A.P.C_thresh);
  }
  int u_t = 0, v_t = 0;
  if (MODE == M3S_MODE_CALIB) {  // ind_Xi % width, ind_Xi / width (gn_kernels.cu:1360-1361)
    const int iid = (int)id;
    int vv = (int)((float)iid * (1.0f / (float)A.P.width));
    if (vv * A.P.width > iid) vv--;
    if ((vv + 1) * A.P.width <= iid) vv++;
    v_t = vv;
    u_t = iid - vv * A.P.width;
  }
  return make_pixin<MODE>(A.P, Xi, ok, q, u_t, v_t);
}

// block -> task (e_loc * chunks + c). The E_loc x chunks tasks sorted by
// (chunk, KF j) are cut into 8 contiguous runs and run x is dealt to blocks
// x, x + 8, x + 16, ...: the edges that stream the same Xj chunk run back to
// back on one XCD (blocks b and b + 8 share an XCD under round-robin
// placement; speed only: partials are indexed by task). -1: idle padding.
__device__ __forceinline__ int64_t block_task(const LinArgs &A) {
  if (!A.eorder) return (int64_t)blockIdx.x;
  const int64_t b = blockIdx.x, t = (b & 7) * A.per + (b >> 3);
  if (t >= A.E_loc * A.chunks) return -1;
  const int64_t c = t / A.E_loc;
  return (int64_t)A.eorder[t - c * A.E_loc] * A.chunks + c;
}

// The block partial is stored write-through (sc1), so the edge's last chunk
// can read it from another XCD without a release fence (guide §6 G16 R1).
__device__ __forceinline__ void store_sc1(float *p, float v) {
  __hip_atomic_store(reinterpret_cast<uint32_t *>(p), __float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// Block reduction of the 36 per-thread sums through LDS: every thread stores
// its row (16-B stores), then 252 threads each add a 1/7 slice of one column,
// then 36 threads combine the 7 slices. ~100 instructions per thread instead
// of 36 wave-wide shuffle trees.
constexpr int kRedW = kNP / 2;  // values per pass (36 or 18)
__device__ __forceinline__ void block_reduce_store(const float *acc, float *out) {
  __shared__ __attribute__((aligned(16))) float red[kThreads * kRedW];
  __shared__ float part[kRedW][8];
  const int t = threadIdx.x;
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    if (pass) __syncthreads();
    float2 *row = reinterpret_cast<float2 *>(red + (size_t)t * kRedW);
#pragma unroll
    for (int k = 0; k < kRedW / 2; k++)
      row[k] = make_float2(acc[pass * kRedW + 2 * k], acc[pass * kRedW + 2 * k + 1]);
    __syncthreads();
    constexpr int S = (kThreads + kRedW * 7 - 1) / (kRedW * 7) * 7 > 0 ? 7 : 7;
    constexpr int per = (kThreads + S - 1) / S;
    if (t < kRedW * S) {
      const int v = t / S, s = t % S;
      const int r0 = s * per, r1 = (r0 + per < kThreads) ? r0 + per : kThreads;
      float x = 0.0f;
      for (int r = r0; r < r1; r++) x += red[r * kRedW + v];
      part[v][s] = x;
    }
    __syncthreads();
    if (t < kRedW) {
      float x = 0.0f;
#pragma unroll
      for (int s = 0; s < S; s++) x += part[t][s];
      store_sc1(out + pass * kRedW + t, x);
    }
  }
}

template <typename T>
__device__ __forceinline__ T ld_stream(const T *p) {
  return __builtin_nontemporal_load(p);
}


// Per edge: H_jj = M L M^T and g_j = M l in fp64 (M = Adj(T_i)^-T), written
// as fin[0:49] (row-major) and fin[49:56], from the edge's 36 local sums `es`
// (LDS). Threads 0..63 of the block work; every thread of the block must call
// it (block barriers). Mc: M already in LDS (the fused finalize forms it on
// its second wave while the first loads the partials); else lanes 0..48 form
// it here, one entry each.
constexpr int kFin = 56;
__device__ __forceinline__ void finalize_edge(const double *es, const float *Ti, double *fin,
                                              const double (*Mc)[7] = nullptr) {
  __shared__ double Mo[7][7], Lm[7][7], T1[7][7], l[7];
  const double(*M)[7] = Mc ? Mc : Mo;
  const int t = threadIdx.x;
  if (!Mc && t < 49) Mo[t / 7][t % 7] = adjT_inv_entry(Ti, t / 7, t % 7);
  if (t < 49) {
    const int a = t / 7, c = t % 7;
    Lm[a][c] = es[kL + tri(a < c ? a : c, a < c ? c : a)];
  }
  if (t < 7) l[t] = es[kG + t];
  __syncthreads();
  if (t < 49) {
    const int a = t / 7, c = t % 7;
    double sm = 0.0;
    for (int k = 0; k < 7; k++) sm += M[a][k] * Lm[k][c];
    T1[a][c] = sm;
  } else if (t < 56) {
    const int a = t - 49;
    double sm = 0.0;
    for (int k = 0; k < 7; k++) sm += M[a][k] * l[k];
    fin[49 + a] = sm;
  }
  __syncthreads();
  if (t < 49) {
    const int a = t / 7, c = t % 7;
    double sm = 0.0;
    for (int k = 0; k < 7; k++) sm += T1[a][k] * M[c][k];
    fin[t] = sm;
  }
}

// Each lane owns 4 consecutive pixels (one 16-B vector per stream); a wave
// sweeps 256 pixels per trip, a block 1024.
// 36 per-thread sums -> one block partial
// Transposed wave reduction of N values: each butterfly step (xor 32, 16,
// ..., 1) a lane keeps one half of its values and sends the other half to its
// partner, so the count halves every step: 18 + 9 + 5 + 3 + 2 + 1 = 38
// shuffles for 36 values instead of 36 x 6. Lane l ends with the full sum of
// value index `idx` (valid when the path never took a padding slot).
template <int N, int M, typename T>
__device__ __forceinline__ void xreduce_step(const T (&v)[N], T (&o)[(N + 1) / 2], bool hi) {
  constexpr int H = (N + 1) / 2;
#pragma unroll
  for (int i = 0; i < H; i++) {
    const T lo_v = v[i];
    const T hi_v = (i + H < N) ? v[i + H] : T(0);
    const T keep = hi ? hi_v : lo_v, send = hi ? lo_v : hi_v;
    o[i] = keep + __shfl_xor(send, M, 64);
  }
}
template <typename T>
__device__ __forceinline__ T xreduce36(const T (&v)[kNP], int lane, int &idx, bool &valid) {
  T a[18], b[9], c[5], d[3], e[2], f[1];
  xreduce_step<36, 32>(v, a, lane & 32);
  xreduce_step<18, 16>(a, b, lane & 16);
  xreduce_step<9, 8>(b, c, lane & 8);
  xreduce_step<5, 4>(c, d, lane & 4);
  xreduce_step<3, 2>(d, e, lane & 2);
  xreduce_step<2, 1>(e, f, lane & 1);
  // the value index a lane ends with: array sizes 36, 18, 9, 5, 3, 2 (the
  // halves H are compile-time); r = real (non-padding) values on the path
  int base = 0, r = kNP, sz = kNP;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int h = (sz + 1) / 2;
    if (lane & m)
      base += h, r = r > h ? r - h : 0;
    else
      r = r < h ? r : h;
    sz = h;
  }
  idx = base;
  valid = r == 1;
  return f[0];
}

// The same transposed reduction on the VALU's cross-lane paths instead of
// ds_bpermute (an LDS round trip per shuffle, ~6 dependent ones per call on
// the tracker's per-iteration critical path): xor 32 and xor 16 by the gfx950
// v_permlane32_swap / v_permlane16_swap (one swap exchanges the halves of a
// value pair: each side then adds what it keeps to what it received), xor 8
// by DPP row_ror:8, then DPP row_half_mirror (lane i of a half-row pairs with
// 7 - i: the pairs still split on lane bit 2, so the keep rule and the final
// index are xreduce36's), quad_perm [2,3,0,1] and [1,0,3,2]. Every sum is
// keep + partner as before; only the xor-4 step's partner (and so the fp
// rounding of the result) differs from xreduce36's.
template <typename T>
__device__ __forceinline__ void xr_swap(bool s32, T &x, T &y) {  // {x, y} -> {x_lo|y_lo, x_hi|y_hi}
  if constexpr (sizeof(T) == 4) {
    const auto r = s32 ? __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false)
                       : __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    x = __uint_as_float(r[0]), y = __uint_as_float(r[1]);
  } else {
    const unsigned long long xb = (unsigned long long)__double_as_longlong(x), yb = (unsigned long long)__double_as_longlong(y);
    const unsigned xl = (unsigned)xb, xh = (unsigned)(xb >> 32), yl = (unsigned)yb, yh = (unsigned)(yb >> 32);
    const auto rl = s32 ? __builtin_amdgcn_permlane32_swap(xl, yl, false, false) : __builtin_amdgcn_permlane16_swap(xl, yl, false, false);
    const auto rh = s32 ? __builtin_amdgcn_permlane32_swap(xh, yh, false, false) : __builtin_amdgcn_permlane16_swap(xh, yh, false, false);
    x = __longlong_as_double((long long)(((unsigned long long)rh[0] << 32) | rl[0]));
    y = __longlong_as_double((long long)(((unsigned long long)rh[1] << 32) | rl[1]));
  }
}
template <int CTRL, typename T>
__device__ __forceinline__ T xr_dpp(T v) {  // the DPP partner's value
  if constexpr (sizeof(T) == 4) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
  } else {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
  }
}
// u + (u of lane ^ 16), then + (that of lane ^ 32): the two butterfly steps of
// `u += __shfl_xor(u, 16); u += __shfl_xor(u, 32)` by v_permlane16/32_swap of
// u with itself (each side gets its partner's value; the sums are the same
// additions, so bitwise the same result) instead of two ds_bpermute LDS round
// trips (the dense tail's back-substitution chain, round 5)
__device__ __forceinline__ double sum_xor16_32(double u) {
  double a = u, b = u;
  xr_swap(false, a, b);
  u = a + b;
  a = u, b = u;
  xr_swap(true, a, b);
  return a + b;
}
// whole-wave sum on every lane by the same exchanges (permlane swaps of the
// value with itself for xor 32 / 16, then DPP; the xor-4 partner is 7 - i
// within a half-row): the solve tails' ||dx|| sums (round 5)
__device__ __forceinline__ float wave_sum_pl(float u) {
  float a = u, b = u;
  xr_swap(true, a, b);
  u = a + b;
  a = u, b = u;
  xr_swap(false, a, b);
  u = a + b;
  u += xr_dpp<0x128>(u);
  u += xr_dpp<0x141>(u);
  u += xr_dpp<0x4E>(u);
  u += xr_dpp<0xB1>(u);
  return u;
}
template <int N, bool S32, typename T>
__device__ __forceinline__ void xr_swap_step(const T (&v)[N], T (&o)[(N + 1) / 2]) {
  constexpr int H = (N + 1) / 2;
#pragma unroll
  for (int i = 0; i < H; i++) {
    T x = v[i], y = (i + H < N) ? v[i + H] : T(0);
    xr_swap(S32, x, y);
    o[i] = x + y;
  }
}
template <int N, int CTRL, typename T>
__device__ __forceinline__ void xr_dpp_step(const T (&v)[N], T (&o)[(N + 1) / 2], bool hi) {
  constexpr int H = (N + 1) / 2;
#pragma unroll
  for (int i = 0; i < H; i++) {
    const T lo_v = v[i];
    const T hi_v = (i + H < N) ? v[i + H] : T(0);
    const T keep = hi ? hi_v : lo_v, send = hi ? lo_v : hi_v;
    o[i] = keep + xr_dpp<CTRL>(send);
  }
}
template <typename T>
__device__ __forceinline__ T xreduce36_dpp(const T (&v)[kNP], int lane, int &idx, bool &valid) {
  T a[18], b[9], c[5], d[3], e[2], f[1];
  xr_swap_step<36, true>(v, a);
  xr_swap_step<18, false>(a, b);
  xr_dpp_step<9, 0x128>(b, c, lane & 8);  // row_ror:8
  xr_dpp_step<5, 0x141>(c, d, lane & 4);  // row_half_mirror
  xr_dpp_step<3, 0x4E>(d, e, lane & 2);   // quad_perm [2,3,0,1]
  xr_dpp_step<2, 0xB1>(e, f, lane & 1);   // quad_perm [1,0,3,2]
  int base = 0, r = kNP, sz = kNP;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int h = (sz + 1) / 2;
    if (lane & m)
      base += h, r = r > h ? r - h : 0;
    else
      r = r < h ? r : h;
    sz = h;
  }
  idx = base;
  valid = r == 1;
  return f[0];
}
// The same transposed reduction for N <= 64 values (xreduce36_dpp's steps);
// xred_index gives the value index a lane ends with and whether it is real.
template <int N>
__device__ __forceinline__ void xred_index(int lane, int &idx, bool &valid) {
  int base = 0, r = N, sz = N;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int h = (sz + 1) / 2;
    if (lane & m)
      base += h, r = r > h ? r - h : 0;
    else
      r = r < h ? r : h;
    sz = h;
  }
  idx = base;
  valid = r == 1;
}
template <int N, typename T>
__device__ __forceinline__ T xreduceN_dpp(const T (&v)[N], int lane) {
  constexpr int S1 = (N + 1) / 2, S2 = (S1 + 1) / 2, S3 = (S2 + 1) / 2, S4 = (S3 + 1) / 2, S5 = (S4 + 1) / 2;
  T a[S1], b[S2], c[S3], d[S4], e[S5], f[(S5 + 1) / 2];
  xr_swap_step<N, true>(v, a);
  xr_swap_step<S1, false>(a, b);
  xr_dpp_step<S2, 0x128>(b, c, lane & 8);
  xr_dpp_step<S3, 0x141>(c, d, lane & 4);
  xr_dpp_step<S4, 0x4E>(d, e, lane & 2);
  xr_dpp_step<S5, 0xB1>(e, f, lane & 1);
  return f[0];
}
// the linearize kernels' block partials on xreduce36_dpp (1) or xreduce36 (0):
// within noise for the packed kernel (an A/B of the first-listed library reads
// ~2-3% slow in tools/ab_linearize.py either way, profiles/r05/ab_pkw_*.txt),
// so the round-4 rounding stays
template <typename T>
__device__ __forceinline__ T xreduce36_trk(const T (&v)[kNP], int lane, int &idx, bool &valid) {
  return xreduce36_dpp(v, lane, idx, valid);
}

__device__ __forceinline__ void store_partial(const float *acc, float *out) {
  __shared__ float red[kThreads / 64][kNP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float v[kNP];
#pragma unroll
  for (int k = 0; k < kNP; k++) v[k] = acc[k];
  int idx;
  bool valid;
  const float s = xreduce36(v, lane, idx, valid);
  if (valid) red[wave][idx] = s;
  __syncthreads();
  if (threadIdx.x < kNP) {
    float t = 0.0f;
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) t += red[w][threadIdx.x];
    store_sc1(out + threadIdx.x, t);
  }
}

// Fused finalize (single-GPU solve): after its chunk partial is stored, a
// block draws a ticket from its edge's counter; the edge's last chunk
// (ticket = chunks - 1 mod chunks: the counter runs on over a call's GN
// iterations and is zeroed per call) sums the edge's chunk partials in fp64
// in chunk order with sc1 loads (the same sums as edge_reduce_kernel /
// finalize_edges_kernel) and writes fin[e] - the finalize launch disappears.
// Stepwise API (a sharded rank's range): the same chunk writes the 36 sums
// to esum[e_loc] - the edge_reduce launch disappears (bitwise the same sums).
__device__ __forceinline__ void edge_tail(const LinArgs &A, int64_t e_loc, int64_t e) {
  __shared__ double esl[kNP], Ms[7][7];
  __shared__ int last_s;
  const int t = threadIdx.x;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its sc1 stores
  __syncthreads();
  if (t == 0) {
    const uint32_t ch = (uint32_t)A.chunks;
    const uint32_t old = __hip_atomic_fetch_add(A.edge_cnt + e_loc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_s = ((old - A.cnt_base) % ch) == ch - 1;
  }
  __syncthreads();
  if (!last_s) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no loads above the ticket
  if (t < kNP) {
    const uint32_t *p = reinterpret_cast<const uint32_t *>(A.partials + (size_t)e_loc * A.chunks * kNP + t);
    double acc = 0.0;
    int64_t c = 0;
    for (; c + 8 <= A.chunks; c += 8) {
      uint32_t v[8];
#pragma unroll
      for (int k = 0; k < 8; k++)
        v[k] = __hip_atomic_load(p + (size_t)(c + k) * kNP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int k = 0; k < 8; k++) acc += (double)__uint_as_float(v[k]);
    }
    for (; c < A.chunks; c++)
      acc += (double)__uint_as_float(__hip_atomic_load(p + (size_t)c * kNP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (A.esum)
      A.esum[(size_t)e_loc * kNP + t] = acc;
    else
      esl[t] = acc;
  } else if (!A.esum && t >= 64 && t < 64 + 49) {  // the second wave forms M under the first's loads
    const int q = t - 64;
    Ms[q / 7][q % 7] = adjT_inv_entry(A.Twc + 8 * (size_t)A.rank_i[e], q / 7, q % 7);
  }
  if (A.esum) return;
  __syncthreads();
  finalize_edge(esl, A.Twc + 8 * (size_t)A.rank_i[e], A.fin + (size_t)e * kFin, Ms);
}

// Fused tracker solve: the iteration's last chunk to arrive (ticket =
// chunks - 1 mod chunks; the counter runs over the call's iterations and is
// zeroed by track_init_kernel) reduces the partials and updates the pose.
__device__ __forceinline__ void track_tail(const LinArgs &A) {
  __shared__ int last_t;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this block's sc1 partial is stored
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t ch = (uint32_t)A.chunks;
    const uint32_t old = __hip_atomic_fetch_add(&A.track->arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_t = (old % ch) == ch - 1;
  }
  __syncthreads();
  if (!last_t) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // the other chunks' partials, not stale L1 lines
  track_solve_block(A);
}

// WPACK: also store the target-side planes for the packed kernel (first GN
// iteration of a solve call).
template <int MODE, bool TRACK, bool VEC, bool WPACK>
__global__ void __launch_bounds__(kThreads) linearize_kernel(LinArgs A) {
  if (*A.stop) return;
  const int64_t b = block_task(A);
  if (b < 0) return;
  const int64_t e_loc = b / A.chunks;
  const int64_t c = b - e_loc * A.chunks;
  const int64_t e = A.edge_begin + e_loc;
  const int64_t HW = A.HW;
  const ResidualParams P = kparams(A);

  Sim3f Tij;
  const float *Xs_i, *Xs_j, *Cs_i = nullptr, *Cs_j = nullptr;
  if (TRACK) {
    Tij = load_sim3(A.T_rel);
    Xs_i = A.Xs;    // Xk (target, pixel-aligned)
    Xs_j = A.Xsrc;  // Xf (source, already gathered by idx_f2k)
  } else {
    const int ri = A.rank_i[e], rj = A.rank_j[e];
    Tij = relative(load_sim3(A.Twc + 8 * ri), load_sim3(A.Twc + 8 * rj));
    Xs_i = A.Xs + (size_t)ri * HW * 3;
    Xs_j = A.Xs + (size_t)rj * HW * 3;
    Cs_i = A.Cs + (size_t)ri * HW;
    Cs_j = A.Cs + (size_t)rj * HW;
  }
  const Sim3Mat Tm = sim3_matrix(Tij);
  // edge data (idx/valid/Q) is addressed relative to the launch's edge slice
  const size_t eoff = TRACK ? 0 : (size_t)e_loc * HW;
  const int64_t *__restrict__ idx = TRACK ? nullptr : A.idx + eoff;
  const int32_t *__restrict__ idx32 = TRACK ? nullptr : reinterpret_cast<const int32_t *>(A.idx) + eoff;
  const uint8_t *__restrict__ valid = A.valid + eoff;
  const float *__restrict__ Qe = A.Q + eoff;
  constexpr int NPL = PixIn<MODE>::kPlanes;
  float *__restrict__ pl = WPACK ? A.planes + (size_t)e_loc * NPL * HW : nullptr;

  // scalar accumulators here: 4 pixels of raw inputs stay live in this kernel
  AccumFlat acc;
  acc.zero();

  const int64_t p_begin = c * A.chunk_pix;
  const int64_t p_end = (p_begin + A.chunk_pix < HW) ? p_begin + A.chunk_pix : HW;

  if (VEC) {
    for (int64_t p0 = p_begin + kPixPerThread * threadIdx.x; p0 < p_end; p0 += kBlockPix) {
      // edge data is read once per iteration: non-temporal, so the pointmaps
      // (re-read by every edge that touches a keyframe) keep the caches
      const uint32_t vb = ld_stream(reinterpret_cast<const uint32_t *>(valid + p0));
      const f32x4 q4 = ld_stream(reinterpret_cast<const f32x4 *>(Qe + p0));
      int64_t ids[4] = {0, 0, 0, 0};
      if (!TRACK) {
        if (A.idx32) {  // uniform branch: 16 B of int32 ids
          typedef int i32x4 __attribute__((ext_vector_type(4)));
          const i32x4 i4 = ld_stream(reinterpret_cast<const i32x4 *>(idx32 + p0));
          ids[0] = i4.x, ids[1] = i4.y, ids[2] = i4.z, ids[3] = i4.w;
        } else {
          const i64x2 i01 = ld_stream(reinterpret_cast<const i64x2 *>(idx + p0));
          const i64x2 i23 = ld_stream(reinterpret_cast<const i64x2 *>(idx + p0 + 2));
          ids[0] = i01.x, ids[1] = i01.y, ids[2] = i23.x, ids[3] = i23.y;
        }
      }
      const f32x4 *xj4 = reinterpret_cast<const f32x4 *>(Xs_j + 3 * p0);
      const f32x4 xa = xj4[0], xb = xj4[1], xc = xj4[2];
      f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
      if (!TRACK) c4 = *reinterpret_cast<const f32x4 *>(Cs_j + p0);
      const float Xj[4][3] = {{xa.x, xa.y, xa.z}, {xa.w, xb.x, xb.y}, {xb.z, xb.w, xc.x}, {xc.y, xc.z, xc.w}};
      const float qs[4] = {q4.x, q4.y, q4.z, q4.w};
      const float cjs[4] = {c4.x, c4.y, c4.z, c4.w};
      PixIn<MODE> in[4];
#pragma unroll
      for (int s = 0; s < 4; s++)
        in[s] = gather_pixel<MODE, TRACK>(A, Xs_i, Cs_i, p0 + s, ((vb >> (8 * s)) & 0xffu) != 0, ids[s],
                                          qs[s], cjs[s]);
      {
#pragma unroll
        for (int s = 0; s < 4; s++) {
          float Y[3];
          act(Tm, Xj[s], Y);
          pixel_contrib<MODE>(acc, P, in[s], Y);
        }
      }
      if (WPACK) {
#pragma unroll
        for (int k = 0; k < NPL; k++) {
          const f32x4 v = {in[0].v[k], in[1].v[k], in[2].v[k], in[3].v[k]};
          // streamed past L2, where the pointmaps that other edges re-read live
          // (first call 258 -> 251 us at C3, 1172 -> 1134 us at 128 KFs rays)
          __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(pl + (size_t)k * HW + p0));
        }
      }
    }
  } else {
    for (int64_t p = p_begin + threadIdx.x; p < p_end; p += kThreads) {
      const bool vm = valid[p] != 0;
      const int64_t id = TRACK ? p : (A.idx32 ? (int64_t)idx32[p] : idx[p]);
      const float Xj[3] = {Xs_j[3 * p], Xs_j[3 * p + 1], Xs_j[3 * p + 2]};
      const float cj = TRACK ? 0.0f : Cs_j[p];
      const PixIn<MODE> in = gather_pixel<MODE, TRACK>(A, Xs_i, Cs_i, p, vm, id, Qe[p], cj);
      {
        float Y[3];
        act(Tm, Xj, Y);
        pixel_contrib<MODE>(acc, P, in, Y);
      }
      if (WPACK) {
#pragma unroll
        for (int k = 0; k < NPL; k++) pl[(size_t)k * HW + p] = in.v[k];
      }
    }
  }
  float sums[kNP];
#pragma unroll
  for (int k = 0; k < kNP; k++) sums[k] = 0.0f;
  acc.fold(sums);
  store_partial(sums, A.partials + (size_t)b * kNP);
  if (A.edge_cnt) edge_tail(A, e_loc, e);
  if (TRACK && A.track) track_tail(A);
}

// Later GN iterations of a solve call: target-side inputs from the planes the
// first iteration stored, Xj streamed (shared through L2 by the edges of one
// keyframe, which the task table places on one XCD back to back). No gathers.
// calib / points fit 128 VGPRs (4 waves per SIMD); rays keeps 84 accumulator
// VGPRs and is left unbounded (164, 3 waves)
// 16 B per lane from a buffer resource straight into LDS (lane-linear at
// m0 = lds): wave-uniform soffset, per-lane voffset (nt: streamed once)
__device__ __forceinline__ void buf_lds16_nt(__amdgpu_buffer_rsrc_t R, __attribute__((address_space(3))) void *lds,
                                             int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(R, lds, 16, voff, soff, 0, 2);
}
__device__ __forceinline__ void buf_lds16(__amdgpu_buffer_rsrc_t R, __attribute__((address_space(3))) void *lds,
                                          int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(R, lds, 16, voff, soff, 0, 0);
}
__device__ __forceinline__ void buf_lds16_sc0(__amdgpu_buffer_rsrc_t R, __attribute__((address_space(3))) void *lds,
                                              int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(R, lds, 16, voff, soff, 0, 1);
}
// A buffer offset past every resource's range (num_records < 2^31): the load
// returns zeros and makes no memory access.
constexpr int kFarOff = 0x7fff0000;
// Xj floats 6h .. 6h + 5 of a lane's 12 (its 4 pixels x y z, interleaved over
// three 16-B LDS rows 1 KB apart, from xs), one ds_read_b32 each straight
// into the half of the pair that uses it: plain loads merge into 16-B reads
// whose halves then need 5 v_mov per pair to regroup by pixel. LDS reads
// complete in order, so the compiler's own counted waits stay correct; ours
// is explicit.
__device__ __forceinline__ void lds_xj6(const float *xs, int h, float (&xf)[6]) {
  const uint32_t xa = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) const float *)xs);
#define M3S_XRD(q_, f_) \
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(xf[q_]) : "v"(xa), "i"(4 * (256 * ((f_) >> 2) + ((f_) & 3))))
  if (h == 0) {
    M3S_XRD(0, 0); M3S_XRD(1, 1); M3S_XRD(2, 2); M3S_XRD(3, 3); M3S_XRD(4, 4); M3S_XRD(5, 5);
  } else {
    M3S_XRD(0, 6); M3S_XRD(1, 7); M3S_XRD(2, 8); M3S_XRD(3, 9); M3S_XRD(4, 10); M3S_XRD(5, 11);
  }
#undef M3S_XRD
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xf[0]), "+v"(xf[1]), "+v"(xf[2]), "+v"(xf[3]), "+v"(xf[4]), "+v"(xf[5]));
}
#ifndef M3S_PK_WAVES  // packed linearize: minimum waves per SIMD (register bound 512 / w)
#define M3S_PK_WAVES 3
#endif
#ifndef M3S_PK_WAVES_RAYS
#define M3S_PK_WAVES_RAYS 2
#endif
template <int MODE>
__global__ void __launch_bounds__(kThreads, MODE == 1 ? M3S_PK_WAVES_RAYS : M3S_PK_WAVES)
    linearize_packed_kernel(LinArgs A) {
  if (*A.stop) return;
  const int64_t b = block_task(A);
  if (b < 0) return;
  const int64_t e_loc = b / A.chunks;
  const int64_t c = b - e_loc * A.chunks;
  const int64_t e = A.edge_begin + e_loc;
  const int64_t HW = A.HW;
  const int ri = A.rank_i[e], rj = A.rank_j[e];
  const Sim3f Tij = relative(load_sim3(A.Twc + 8 * ri), load_sim3(A.Twc + 8 * rj));
  const Sim3Mat Tm = sim3_matrix(Tij);
  const ResidualParams P = kparams(A);
  const float *__restrict__ Xs_j = A.Xs + (size_t)rj * HW * 3;
  constexpr int NPL = PixIn<MODE>::kPlanes;
  const float *__restrict__ pl = A.planes + (size_t)e_loc * NPL * HW;

  AccumPP acc;
  acc.zero();
  const int64_t p_begin = c * A.chunk_pix;
  const int64_t p_end = (p_begin + A.chunk_pix < HW) ? p_begin + A.chunk_pix : HW;
  float sink = 0.0f;  // the memory-floor build only (M3S_PK_FLOOR=1)
  // Prefetch one trip ahead through LDS with no VGPR cost: each wave's next
  // trip (NPL plane vectors + 3 Xj vectors, 16 B per lane each) is loaded by
  // buffer_load_dwordx4 ... lds into the wave's own LDS slot while the wave
  // computes the current trip from registers. Lane l's 16 B land at slot +
  // 16 l (lane-linear), so every lane reads back exactly what it loaded.
  // Round 3: buffer loads with wave-uniform soffsets (the trip's first pixel)
  // and per-lane voffsets fixed for the whole kernel, and the LDS slot (m0)
  // from a wave-uniform wave index: no per-load VALU address arithmetic
  // (17 VALU per trip before). One resource per plane, sized HW floats.
  // one slot per wave (a 2-deep prefetch measured slower)
  constexpr int DEPTH = 1;
  __shared__ __attribute__((aligned(16))) f32x4 stage[DEPTH][kThreads / 64][NPL + 3][64];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), ln = threadIdx.x & 63;
  __amdgpu_buffer_rsrc_t Rp[NPL];
#pragma unroll
  for (int k = 0; k < NPL; k++)
    Rp[k] = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pl + (size_t)k * HW), 0, (int)(4 * HW), 0x00020000);
  const __amdgpu_buffer_rsrc_t Rx =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Xs_j), 0, (int)(12 * HW), 0x00020000);
  const int vo_p = 16 * ln, vo_x = 48 * ln;
  const int pend = (int)p_end;
  // pw: the wave's first pixel of a trip (wave-uniform); lane pixels pw + 4 ln
  auto issue = [&](int pw, int sl_) {
#if defined(M3S_PK_FLOOR) && M3S_PK_FLOOR == 2  // compute floor (A/B only): no loads
    return;
#endif
    // A trip that runs past the chunk's end (a partial last trip only): its
    // lanes past the end take an offset beyond every resource, which reads
    // zeros with no memory access. The buffer range check covers voffset (+
    // the instruction offset), not soffset, so the wave-uniform trip base in
    // soffset alone would let them read past the last plane / pointmap.
    // Round 5: the partial trip has loads of its own with other cache bits
    // (sc0, no nt): with the same intrinsic calls on both sides the compiler
    // merged the two paths into per-lane selects of the offsets on every trip
    // (round 4: 277 -> 283 VALU per calib trip, tools/isa_loop.py).
    if (pw + kPixPerThread * 64 > pend) {  // wave-uniform: the full trips keep the fixed offsets
      const bool out = pw + kPixPerThread * ln >= pend;
      const int vp = out ? kFarOff : vo_p, vx = out ? kFarOff : vo_x;
#pragma unroll
      for (int k = 0; k < NPL; k++)
        buf_lds16_sc0(Rp[k], (__attribute__((address_space(3))) void *)(&stage[sl_][wv][k][0]), vp, 4 * pw);
#pragma unroll
      for (int k = 0; k < 3; k++)
        buf_lds16_sc0(Rx, (__attribute__((address_space(3))) void *)(&stage[sl_][wv][NPL + k][0]), vx, 12 * pw + 16 * k);
      return;
    }
#pragma unroll
    for (int k = 0; k < NPL; k++)
      buf_lds16_nt(Rp[k], (__attribute__((address_space(3))) void *)(&stage[sl_][wv][k][0]), vo_p, 4 * pw);
#pragma unroll
    for (int k = 0; k < 3; k++)
      buf_lds16(Rx, (__attribute__((address_space(3))) void *)(&stage[sl_][wv][NPL + k][0]), vo_x, 12 * pw + 16 * k);
  };
  int pw0 = (int)p_begin + kPixPerThread * 64 * wv;
  if (pw0 < pend) issue(pw0, 0);
  if (DEPTH > 1 && pw0 + kBlockPix < pend) issue(pw0 + kBlockPix, 1 % DEPTH);
  // One trip; PARTIAL: the wave's last trip runs past the chunk's end. The
  // full trips are a loop of their own and the partial one is peeled after
  // it, so the full trips carry no per-lane end test (2 VALU per trip).
  auto trip_body = [&](const int pw, const int trip, const bool PARTIAL) {  // (inlined: PARTIAL folds)
    const int cur = DEPTH > 1 ? (trip & 1) : 0;
    if (DEPTH > 1 && pw + kBlockPix < pend) {
      // this trip's loads are done once at most the next trip's NPL + 3 are in flight
      if constexpr (NPL == 3) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // lanes past the chunk's end (a partial last trip only) read back zeros
    // from the resources and take no part (their exec bit is off)
    if (PARTIAL && pw + kPixPerThread * ln >= pend) return;
    // each pixel pair's operands are read from the LDS slot just before its
    // math (8-B reads: 2 NPL + 6 VGPRs live instead of 4 (NPL + 3)); the slot
    // is refilled once the second pair's operands are in registers
    const float *sl = reinterpret_cast<const float *>(&stage[cur][wv][0][ln]);
#pragma unroll
    for (int h = 0; h < 2; h++) {
      f32x2 in[NPL], X[3];
#pragma unroll
      for (int k = 0; k < NPL; k++) in[k] = *reinterpret_cast<const f32x2 *>(sl + 256 * k + 2 * h);
      // Xj of pixels 2h, 2h + 1: floats 6h .. 6h + 5 of the lane's 12
      const float *xs = sl + 256 * NPL;
      float xf[6];
      lds_xj6(xs, h, xf);
      X[0] = f32x2{xf[0], xf[3]}, X[1] = f32x2{xf[1], xf[4]}, X[2] = f32x2{xf[2], xf[5]};
      if (h == 1) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // slot read back before it is refilled
        if (pw + DEPTH * kBlockPix < pend) issue(pw + DEPTH * kBlockPix, cur);
      }
#if defined(M3S_PK_FLOOR) && M3S_PK_FLOOR == 1  // memory floor (A/B only): no math
      sink += in[0].x + in[NPL - 1].y + X[0].x + X[2].y;
#else
      f32x2 Y[3];
      act2(Tm, X, Y);
      pixel_contrib2<MODE, NPL, false>(acc, P, in, Y);
#endif
    }
  };
  int trip = 0;
  for (; pw0 + kPixPerThread * 64 <= pend; pw0 += kBlockPix, trip++) trip_body(pw0, trip, false);
  if (pw0 < pend) trip_body(pw0, trip, true);
  float sums[kNP];
#pragma unroll
  for (int k = 0; k < kNP; k++) sums[k] = 0.0f;
  if constexpr (MODE == 2) acc.cal25_fixup();
  acc.fold(sums);
  sums[0] += sink;
  store_partial(sums, A.partials + (size_t)b * kNP);
  if (A.edge_cnt) edge_tail(A, e_loc, e);
}

// ------------------------------------------ pipelined gathering launch --
// The first GN iteration of a backend call (round 3). Per trip a lane takes 4
// pixels; the wave's streamed inputs of the NEXT trip (valid, Q, idx of the
// edge; Xj, Cj of KF j) go by buffer_load ... lds into the wave's LDS slot
// while this trip runs, so only the dependent gathers of KF i (z_i or X_i, and
// C_i, through idx) are exposed per trip, not the stream latency before them.
// Order per trip: read the slot (inline-asm LDS reads: the compiler adds no
// vmcnt wait for the DMA), issue the gathers, then the next trip's refill
// (vmcnt is in order: waiting for the gathers then leaves the refill in
// flight), the pose-only math, the rest, the plane stores. Same arithmetic per
// pixel as linearize_kernel<MODE, false, true, true> (gather_pixel +
// make_pixin + pixel_contrib): bitwise the same planes, partials and sums.
// Floor builds (A/B measurement only, wrong sums):
// M3S_GATHER_FLOOR = 1 no math, 2 no gathers (the slot's values stand in),
// 3 no plane stores, 4 streams only (no gathers, math or stores).
#ifndef M3S_GATHER_FLOOR
#define M3S_GATHER_FLOOR 0
#endif
constexpr bool kGFloorNoMath = M3S_GATHER_FLOOR == 1 || M3S_GATHER_FLOOR == 4;
constexpr bool kGFloorNoGather = M3S_GATHER_FLOOR == 2 || M3S_GATHER_FLOOR == 4;
constexpr bool kGFloorNoStore = M3S_GATHER_FLOOR == 3 || M3S_GATHER_FLOOR == 4;
// per-wave slot (bytes): valid u8x4 | Q | idx (int64: two 1-KB rows; int32: one) | Xj (3 rows) | Cj
constexpr int kGsValid = 0, kGsQ = 256, kGsIdx = 1280, kGsXj = 3328, kGsCj = 6400, kGsBytes = 7424;
__device__ __forceinline__ void buf_lds4_nt(__amdgpu_buffer_rsrc_t R, __attribute__((address_space(3))) void *lds,
                                            int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(R, lds, 4, voff, soff, 0, 2);
}
struct GSlot {
  uint32_t vb;
  f32x4 q, x0, x1, x2, c;
  u32x4 i0, i1;
};
// one lane's trip out of the slot: a = slot + 16 lane, av = slot + 4 lane
__device__ __forceinline__ void gslot_read(uint32_t a, uint32_t av, bool i64, GSlot &g) {
  asm volatile("ds_read_b32 %0, %1 offset:0" : "=v"(g.vb) : "v"(av));
  asm volatile("ds_read_b128 %0, %1 offset:256" : "=v"(g.q) : "v"(a));
  asm volatile("ds_read_b128 %0, %1 offset:1280" : "=v"(g.i0) : "v"(a));
  if (i64) asm volatile("ds_read_b128 %0, %1 offset:2304" : "=v"(g.i1) : "v"(a));
  asm volatile("ds_read_b128 %0, %1 offset:3328" : "=v"(g.x0) : "v"(a));
  asm volatile("ds_read_b128 %0, %1 offset:4352" : "=v"(g.x1) : "v"(a));
  asm volatile("ds_read_b128 %0, %1 offset:5376" : "=v"(g.x2) : "v"(a));
  asm volatile("ds_read_b128 %0, %1 offset:6400" : "=v"(g.c) : "v"(a));
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(g.vb), "+v"(g.q), "+v"(g.i0), "+v"(g.i1), "+v"(g.x0), "+v"(g.x1), "+v"(g.x2), "+v"(g.c));
}

template <int MODE>
__global__ void __launch_bounds__(kThreads) linearize_gather_kernel(LinArgs A) {
  if (*A.stop) return;
  const int64_t b = block_task(A);
  if (b < 0) return;
  const int64_t e_loc = b / A.chunks;
  const int64_t c = b - e_loc * A.chunks;
  const int64_t e = A.edge_begin + e_loc;
  const int64_t HW = A.HW;
  const ResidualParams P = kparams(A);
  const int ri = A.rank_i[e], rj = A.rank_j[e];
  const Sim3Mat Tm = sim3_matrix(relative(load_sim3(A.Twc + 8 * ri), load_sim3(A.Twc + 8 * rj)));
  const float *Xs_i = A.Xs + (size_t)ri * HW * 3, *Xs_j = A.Xs + (size_t)rj * HW * 3;
  const float *Cs_i = A.Cs + (size_t)ri * HW, *Cs_j = A.Cs + (size_t)rj * HW;
  const size_t eoff = (size_t)e_loc * HW;
  constexpr int NPL = PixIn<MODE>::kPlanes;
  float *__restrict__ pl = A.planes + (size_t)e_loc * NPL * HW;
  const bool i64 = A.idx32 == 0;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), ln = threadIdx.x & 63;
  // streams (ranges: reads past the end return zeros) and the gather sources
  const __amdgpu_buffer_rsrc_t Rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(A.valid + eoff), 0, (int)HW, 0x00020000);
  const __amdgpu_buffer_rsrc_t Rq = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(A.Q + eoff), 0, (int)(4 * HW), 0x00020000);
  const __amdgpu_buffer_rsrc_t Ri = __builtin_amdgcn_make_buffer_rsrc(
      i64 ? (void *)(A.idx + eoff) : (void *)(reinterpret_cast<const int32_t *>(A.idx) + eoff), 0,
      (int)((i64 ? 8 : 4) * HW), 0x00020000);
  const __amdgpu_buffer_rsrc_t Rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Xs_j), 0, (int)(12 * HW), 0x00020000);
  const __amdgpu_buffer_rsrc_t Rc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Cs_j), 0, (int)(4 * HW), 0x00020000);
  const __amdgpu_buffer_rsrc_t RXi = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Xs_i), 0, (int)(12 * HW), 0x00020000);
  const __amdgpu_buffer_rsrc_t RCi = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Cs_i), 0, (int)(4 * HW), 0x00020000);
  __shared__ __attribute__((aligned(16))) uint8_t gstage[kThreads / 64][kGsBytes];
  uint8_t *slot = gstage[wv];
  auto L3 = [&](int off) { return (__attribute__((address_space(3))) void *)(slot + off); };
  // per-lane offsets; kFar (past every resource's range) reads zeros without a
  // memory access: the refill is issued unconditionally (a fixed count of 8
  // loads per trip, so the compiler's counted waits for the gathers behind it
  // stay exact), with kFar when there is no next trip and for the second idx
  // row of int32 ids
  constexpr int kFar = kFarOff;
  const int v4 = 4 * ln, v16 = 16 * ln, v48 = 48 * ln, vi0 = (i64 ? 32 : 16) * ln, vi1 = i64 ? 32 * ln + 16 : kFar;
  const int64_t p_begin = c * A.chunk_pix;
  const int pend = (int)((p_begin + A.chunk_pix < HW) ? p_begin + A.chunk_pix : HW);
  auto issue = [&](int pw, bool far) {  // pw: the wave's first pixel of the trip
    // a partial last trip: its lanes past the chunk's end load from kFar too
    // (the range check covers voffset, not the trip base in soffset). (Round
    // 5: loads of their own here, as in the packed kernel, made the compiler's
    // counted waits after the refill conservative — vmcnt(3) behind the 8
    // refill loads, tests/test_isa.py — so this path stays merged.)
    if (!far && pw + kPixPerThread * 64 > pend) {
      const bool out = pw + kPixPerThread * ln >= pend;
      buf_lds4_nt(Rv, L3(kGsValid), out ? kFar : v4, pw);
      buf_lds16_nt(Rq, L3(kGsQ), out ? kFar : v16, 4 * pw);
      buf_lds16_nt(Ri, L3(kGsIdx), out ? kFar : vi0, (i64 ? 8 : 4) * pw);
      buf_lds16_nt(Ri, L3(kGsIdx + 1024), out ? kFar : vi1, 8 * pw);
#pragma unroll
      for (int k = 0; k < 3; k++) buf_lds16(Rx, L3(kGsXj + 1024 * k), out ? kFar : v48, 12 * pw + 16 * k);
      buf_lds16(Rc, L3(kGsCj), out ? kFar : v16, 4 * pw);
      return;
    }
    buf_lds4_nt(Rv, L3(kGsValid), far ? kFar : v4, pw);
    buf_lds16_nt(Rq, L3(kGsQ), far ? kFar : v16, 4 * pw);
    buf_lds16_nt(Ri, L3(kGsIdx), far ? kFar : vi0, (i64 ? 8 : 4) * pw);
    buf_lds16_nt(Ri, L3(kGsIdx + 1024), far ? kFar : vi1, 8 * pw);
#pragma unroll
    for (int k = 0; k < 3; k++) buf_lds16(Rx, L3(kGsXj + 1024 * k), far ? kFar : v48, 12 * pw + 16 * k);
    buf_lds16(Rc, L3(kGsCj), far ? kFar : v16, 4 * pw);
  };
  const uint32_t sa = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) const uint8_t *)slot);
  const uint32_t a16 = sa + 16 * ln, a4 = sa + 4 * ln;

  AccumFlat acc;
  acc.zero();
  float gsink = 0.0f;  // the floor builds only
  int pw = (int)p_begin + kPixPerThread * 64 * wv;
  if (pw < pend) issue(pw, false);
  for (int trip = 0; pw < pend; pw += kBlockPix, trip++) {
    // the slot's DMA is done once only the previous trip's NPL plane stores
    // may still be in flight behind it (stores count in vmcnt, in issue
    // order); the first trip has no stores behind its loads
    if (trip == 0 || kGFloorNoStore) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (NPL == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    const int p0 = pw + kPixPerThread * ln;
    if (p0 >= pend) continue;  // a partial last trip: lanes past the end take no part
    GSlot g;
    gslot_read(a16, a4, i64, g);
    int64_t ids[4];
    if (i64) {
      ids[0] = (int64_t)(((uint64_t)g.i0.y << 32) | g.i0.x), ids[1] = (int64_t)(((uint64_t)g.i0.w << 32) | g.i0.z);
      ids[2] = (int64_t)(((uint64_t)g.i1.y << 32) | g.i1.x), ids[3] = (int64_t)(((uint64_t)g.i1.w << 32) | g.i1.z);
    } else {
      ids[0] = (int32_t)g.i0.x, ids[1] = (int32_t)g.i0.y, ids[2] = (int32_t)g.i0.z, ids[3] = (int32_t)g.i0.w;
    }
    // the gathers of this trip (gather_pixel's: id = valid ? idx : 0)
    bool vm[4];
    int id[4];
    float gx[4][3], gc[4];
#pragma unroll
    for (int s4 = 0; s4 < 4; s4++) {
      vm[s4] = ((g.vb >> (8 * s4)) & 0xffu) != 0;
#if M3S_GATHER_IDENT  // A/B bound only (wrong sums): every gather at the pixel's own index
      id[s4] = vm[s4] ? p0 + s4 : 0;
#else
      id[s4] = vm[s4] ? (int)ids[s4] : 0;
#endif
      // 12 id on the full-rate 24-bit multiply (v_mul_lo_u32 is quarter rate;
      // the host takes this kernel only for HW <= 2^24)
      const int o12 = (int)__umul24((unsigned)id[s4], 12u);
      if constexpr (kGFloorNoGather) {  // floor build: the slot's own values stand in for the gathers
        gx[s4][0] = g.x0.x, gx[s4][1] = g.x0.y, gx[s4][2] = g.x0.z + (float)o12, gc[s4] = g.c.x;
        continue;
      }
      if (MODE == M3S_MODE_CALIB) {
        gx[s4][2] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(RXi, o12 + 8, 0, 0));
      } else {
#pragma unroll
        for (int k = 0; k < 3; k++)
          gx[s4][k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(RXi, o12 + 4 * k, 0, 0));
      }
      gc[s4] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(RCi, 4 * id[s4], 0, 0));
    }
    __builtin_amdgcn_sched_barrier(0);  // the gathers go out before the refill
    issue(pw + kBlockPix, pw + kBlockPix >= pend);
    __builtin_amdgcn_sched_barrier(0);
    const float Xj[4][3] = {{g.x0.x, g.x0.y, g.x0.z}, {g.x0.w, g.x1.x, g.x1.y}, {g.x1.z, g.x1.w, g.x2.x},
                            {g.x2.y, g.x2.z, g.x2.w}};
    const float qs[4] = {g.q.x, g.q.y, g.q.z, g.q.w};
    const float cjs[4] = {g.c.x, g.c.y, g.c.z, g.c.w};
    PixIn<MODE> in[4];
    if constexpr (kGFloorNoMath) {  // floor build: the loaded values go straight to the planes
#pragma unroll
      for (int s4 = 0; s4 < 4; s4++) {
#pragma unroll
        for (int k = 0; k < NPL; k++) in[s4].v[k] = gx[s4][k % 3] + (k == 1 ? gc[s4] + qs[s4] + cjs[s4] + Xj[s4][0] : 0.0f);
      }
      gsink += in[0].v[0] + in[3].v[NPL - 1];
    }
#pragma unroll
    for (int s4 = 0; s4 < 4 && !kGFloorNoMath; s4++) {
      const bool ok = vm[s4] && (qs[s4] > P.Q_thresh) && (gc[s4] > P.C_thresh) && (cjs[s4] > P.C_thresh);
      int u_t = 0, v_t = 0;
      if (MODE == M3S_MODE_CALIB) {  // gather_pixel's ind_Xi % width, ind_Xi / width
        // products on the full-rate 24-bit multiply (row < 2^15, width <
        // 2^16), not the quarter-rate v_mul_lo_u32
        const int iid = id[s4];
        const unsigned w = (unsigned)P.width;
        int vv = (int)((float)iid * (1.0f / (float)P.width));
        if (__umul24((unsigned)vv, w) > iid) vv--;
        if (__umul24((unsigned)vv + 1u, w) <= iid) vv++;
        v_t = vv;
        u_t = iid - __umul24((unsigned)vv, w);
      }
      in[s4] = make_pixin<MODE>(P, gx[s4], ok, qs[s4], u_t, v_t);
    }
#pragma unroll
    for (int s4 = 0; s4 < 4 && !kGFloorNoMath; s4++) {
      float Y[3];
      act(Tm, Xj[s4], Y);
      pixel_contrib<MODE>(acc, P, in[s4], Y);
    }
    if constexpr (kGFloorNoStore) {
      gsink += in[0].v[0] + in[1].v[NPL - 1] + in[2].v[0] + in[3].v[NPL - 1];
      continue;
    }
    // NPL plane stores after the refill: the loop top's counted vmcnt(NPL)
    // relies on at least NPL vector-memory operations following the refill's
    // 8 LDS-DMA loads on every path back to it (tests/test_isa.py checks the
    // disassembly of the built library)
#pragma unroll
    for (int k = 0; k < NPL; k++) {
      const f32x4 v = {in[0].v[k], in[1].v[k], in[2].v[k], in[3].v[k]};
      __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(pl + (size_t)k * HW + p0));
    }
  }
  float sums[kNP];
#pragma unroll
  for (int k = 0; k < kNP; k++) sums[k] = 0.0f;
  acc.fold(sums);
  sums[0] += gsink;  // 0 but in the floor builds
  store_partial(sums, A.partials + (size_t)b * kNP);
  if (A.edge_cnt) edge_tail(A, e_loc, e);
}

// fp64 sum of each edge's chunk partials (fixed order)
__global__ void edge_reduce_kernel(const float *__restrict__ partials, int64_t chunks,
                                   double *__restrict__ edge_sums, const int32_t *__restrict__ stop) {
  if (*stop) return;
  const int64_t e = blockIdx.x;
  const int t = threadIdx.x;
  if (t >= kNP) return;
  double s = 0.0;
  const float *p = partials + (size_t)e * chunks * kNP + t;
  for (int64_t c = 0; c < chunks; c++) s += (double)p[(size_t)c * kNP];
  edge_sums[(size_t)e * kNP + t] = s;
}

// ------------------------------------------------------------- assemble --
// RHS-augmented system in A (row-major, leading dim ld = roundup(n+1, 64)):
//   A[0:n, 0:n] = H,  A[n, 0:n] = g^T,  rows > n = identity padding.
// Block r < N-1 owns rows [7r, 7r+7) and the entries A[n, 7r:7r+7); block
// N-1 initialises row n's tail and the padding rows.
__global__ void __launch_bounds__(256) assemble_kernel(const double *__restrict__ edge_sums,
                                                       const int32_t *__restrict__ rank_i,
                                                       const int32_t *__restrict__ rank_j, int64_t E,
                                                       const float *__restrict__ Twc, int64_t n,
                                                       int64_t ld, double *__restrict__ A,
                                                       const int32_t *__restrict__ stop) {
  if (*stop) return;
  const int r = blockIdx.x;
  const int t = threadIdx.x;
  const int nb = (int)(n / 7);
  if (r == nb) {  // padding block
    for (int64_t k = n + t; k < ld; k += blockDim.x) A[(size_t)n * ld + k] = 0.0;
    for (int64_t k = t; k < (ld - n - 1) * ld; k += blockDim.x) {
      const int64_t i = n + 1 + k / ld, j = k % ld;
      A[(size_t)i * ld + j] = (i == j) ? 1.0 : 0.0;
    }
    return;
  }
  __shared__ double M[7][7], Lm[7][7], T1[7][7], Hjj[7][7], l[7], gj[7];
  for (int64_t k = t; k < 7 * ld; k += blockDim.x) A[(size_t)7 * r * ld + k] = 0.0;
  double *g = A + (size_t)n * ld;
  if (t < 7) g[7 * r + t] = 0.0;
  __syncthreads();
  for (int64_t e = 0; e < E; e++) {
    const int i = rank_i[e] - 1, j = rank_j[e] - 1;
    if (i != r && j != r) continue;  // uniform across the block
    const double *es = edge_sums + (size_t)e * kNP;
    if (t == 0) adjT_inv_matrix(Twc + 8 * (size_t)(i + 1), M);
    if (t < 49) {
      const int a = t / 7, c = t % 7;
      const int lo = a < c ? a : c, hi = a < c ? c : a;
      Lm[a][c] = es[kL + tri(lo, hi)];
    }
    if (t < 7) l[t] = es[kG + t];
    __syncthreads();
    if (t < 49) {
      const int a = t / 7, c = t % 7;
      double s = 0.0;
      for (int k = 0; k < 7; k++) s += M[a][k] * Lm[k][c];
      T1[a][c] = s;
    } else if (t < 56) {
      const int a = t - 49;
      double s = 0.0;
      for (int k = 0; k < 7; k++) s += M[a][k] * l[k];
      gj[a] = s;
    }
    __syncthreads();
    if (t < 49) {
      const int a = t / 7, c = t % 7;
      double s = 0.0;
      for (int k = 0; k < 7; k++) s += T1[a][k] * M[c][k];
      Hjj[a][c] = s;
    }
    __syncthreads();
    if (t < 49) {
      const int a = t / 7, c = t % 7;
      double *row = A + (size_t)(7 * r + a) * ld;
      const double h = Hjj[a][c];
      // edge (i -> j): Hs[0]=Hs[3]=Hjj at (i,i),(j,j); Hs[1]=Hs[2]=-Hjj off-diagonal
      if (i == r) {
        row[7 * r + c] += h;
        if (j >= 0) row[7 * j + c] -= h;
      }
      if (j == r) {
        row[7 * r + c] += h;
        if (i >= 0) row[7 * i + c] -= h;
      }
    } else if (t < 56) {
      const int a = t - 49;
      if (i == r) g[7 * r + a] -= gj[a];  // gs[0] = -M l
      if (j == r) g[7 * r + a] += gj[a];  // gs[1] = +M l
    }
    __syncthreads();
  }
}

// dx = -x, retraction of poses 1..N-1, ||dx|| test, info update. x in LDS.
// Called by one whole block (blockDim.x threads, multiple of 64).
__device__ void finish_step(const double *xs, float *dxs, float *nrm, int n, float *Twc, int64_t N,
                            float *dx_out, int32_t *info, int32_t *stop, float delta_thresh) {
  const int tid = threadIdx.x, nt = blockDim.x;
  float part = 0.0f;
  for (int k = tid; k < n; k += nt) {
    const float v = -(float)xs[k];
    dxs[k] = v;
    dx_out[k] = v;
    part += v * v;
  }
  part = wave_sum_pl(part);
  if ((tid & 63) == 0) nrm[tid >> 6] = part;
  __syncthreads();
  for (int p = tid; p < (int)(N - 1); p += nt) {
    const Sim3f T = load_sim3(Twc + 8 * (size_t)(p + 1));
    store_sim3(Twc + 8 * (size_t)(p + 1), retract_f64(dxs + 7 * p, T));
  }
  if (tid == 0) {
    float s = 0.0f;
    for (int w = 0; w < nt / 64; w++) s += nrm[w];
    info[M3S_INFO_ITERS] += 1;
    if (sqrtf(s) < delta_thresh) {
      info[M3S_INFO_CONVERGED] = 1;
      stop[0] = 1;
    }
  }
}

// LLT failure: dx = 0 (poses unchanged), ||0|| < delta stops like the reference
__device__ void fail_step(int n, float *dx_out, int32_t *info, int32_t *stop, float delta_thresh) {
  for (int k = threadIdx.x; k < n; k += blockDim.x) dx_out[k] = 0.0f;
  if (threadIdx.x == 0) {
    info[M3S_INFO_ITERS] += 1;
    info[M3S_INFO_SOLVE_FAIL] += 1;
    if (0.0f < delta_thresh) {
      info[M3S_INFO_CONVERGED] = 1;
      stop[0] = 1;
    }
  }
}

// ------------------------------------------------- tiled dense Cholesky --
// For systems beyond the register-resident kernel. Right-looking, 64x64
// fp64 tiles, three launches per tile column: factor the diagonal tile,
// triangular-solve the panel below it, update the trailing lower tiles.
// Thread (ty, tx) of a 16x16 grid owns tile entries (ty + 16a, tx + 16b).
__global__ void __launch_bounds__(256) potrf_tile_kernel(double *__restrict__ A, int64_t ld, int64_t n,
                                                         int kb, int32_t *__restrict__ flags) {
  if (flags[kFlagStop] || flags[kFlagFail]) return;
  __shared__ double cb[2][kTile];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double *T = A + (size_t)kb * kTile * ld + (size_t)kb * kTile;
  double v[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) v[a][b] = T[(size_t)(ty + 16 * a) * ld + tx + 16 * b];
  int step = 0;
#pragma unroll
  for (int cbk = 0; cbk < 4; cbk++) {
    for (int cc = 0; cc < 16; cc++) {
      const int c = 16 * cbk + cc;
      if ((int64_t)kb * kTile + c >= n) break;  // augmented row / padding: nothing to factor
      double *col = cb[step & 1];
      if (tx == cc) {
#pragma unroll
        for (int a = 0; a < 4; a++) col[ty + 16 * a] = (ty + 16 * a >= c) ? v[a][cbk] : 0.0;
      }
      __syncthreads();
      const double d = col[c];
      if (!(d > 0.0)) {
        if (threadIdx.x == 0) flags[kFlagFail] = 1;
        return;  // uniform: every thread read the same pivot
      }
      const double inv = 1.0 / sqrt(d);
      double lj[4];
#pragma unroll
      for (int b = 0; b < 4; b++) lj[b] = col[tx + 16 * b] * inv;
#pragma unroll
      for (int a = 0; a < 4; a++) {
        const double li = col[ty + 16 * a] * inv;
#pragma unroll
        for (int b = 0; b < 4; b++) v[a][b] -= li * lj[b];
        if (tx == cc) v[a][cbk] = li;
      }
      step++;
    }
  }
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) T[(size_t)(ty + 16 * a) * ld + tx + 16 * b] = v[a][b];
}

// X L_kk^T = A_ik for the row tiles i > kb (block b -> i = kb + 1 + b)
__global__ void __launch_bounds__(256) trsm_tile_kernel(double *__restrict__ A, int64_t ld, int64_t n,
                                                        int kb, int32_t *__restrict__ flags) {
  if (flags[kFlagStop] || flags[kFlagFail]) return;
  __shared__ double Lk[kTile][kTile + 1];
  __shared__ double cb[2][kTile];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i = kb + 1 + blockIdx.x;
  const double *D = A + (size_t)kb * kTile * ld + (size_t)kb * kTile;
  for (int k = threadIdx.x; k < kTile * kTile; k += 256) Lk[k / kTile][k % kTile] = D[(size_t)(k / kTile) * ld + k % kTile];
  double *T = A + (size_t)i * kTile * ld + (size_t)kb * kTile;
  double v[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) v[a][b] = T[(size_t)(ty + 16 * a) * ld + tx + 16 * b];
  __syncthreads();
  int step = 0;
#pragma unroll
  for (int cbk = 0; cbk < 4; cbk++) {
    for (int cc = 0; cc < 16; cc++) {
      const int c = 16 * cbk + cc;
      if ((int64_t)kb * kTile + c >= n) break;
      double *col = cb[step & 1];
      const double inv = 1.0 / Lk[c][c];
      if (tx == cc) {
#pragma unroll
        for (int a = 0; a < 4; a++) {
          v[a][cbk] *= inv;
          col[ty + 16 * a] = v[a][cbk];
        }
      }
      __syncthreads();
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int s = tx + 16 * b;
        if (s > c) {
          const double l = Lk[s][c];
#pragma unroll
          for (int a = 0; a < 4; a++) v[a][b] -= col[ty + 16 * a] * l;
        }
      }
      step++;
    }
  }
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) T[(size_t)(ty + 16 * a) * ld + tx + 16 * b] = v[a][b];
}

// A_ij -= L_ik L_jk^T for kb < j <= i < nt (block -> packed lower index)
__global__ void __launch_bounds__(256) update_tiles_kernel(double *__restrict__ A, int64_t ld, int kb,
                                                           const int32_t *__restrict__ flags) {
  if (flags[kFlagStop] || flags[kFlagFail]) return;
  __shared__ double Li[kTile][kTile + 1];
  __shared__ double Lj[kTile][kTile + 1];
  const int t = blockIdx.x;
  int ip = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((ip + 1) * (ip + 2) / 2 <= t) ip++;
  while (ip * (ip + 1) / 2 > t) ip--;
  const int jp = t - ip * (ip + 1) / 2;
  const int i = kb + 1 + ip, j = kb + 1 + jp;
  const double *Pi = A + (size_t)i * kTile * ld + (size_t)kb * kTile;
  const double *Pj = A + (size_t)j * kTile * ld + (size_t)kb * kTile;
  for (int k = threadIdx.x; k < kTile * kTile; k += 256) {
    Li[k / kTile][k % kTile] = Pi[(size_t)(k / kTile) * ld + k % kTile];
    Lj[k / kTile][k % kTile] = Pj[(size_t)(k / kTile) * ld + k % kTile];
  }
  __syncthreads();
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[4][4] = {};
  for (int s = 0; s < kTile; s++) {
    double li[4], lj[4];
#pragma unroll
    for (int a = 0; a < 4; a++) li[a] = Li[ty + 16 * a][s];
#pragma unroll
    for (int b = 0; b < 4; b++) lj[b] = Lj[tx + 16 * b][s];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) acc[a][b] += li[a] * lj[b];
  }
  double *T = A + (size_t)i * kTile * ld + (size_t)j * kTile;
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) T[(size_t)(ty + 16 * a) * ld + tx + 16 * b] -= acc[a][b];
}

// L^T x = y (y = row n of the factor), tiles from the bottom; then the step.
__global__ void __launch_bounds__(1024) backsolve_kernel(const double *__restrict__ A, int64_t ld, int n,
                                                         float *__restrict__ Twc, int64_t N,
                                                         float *__restrict__ dx_out, int32_t *__restrict__ info,
                                                         int32_t *__restrict__ flags, float delta_thresh) {
  if (flags[kFlagStop]) return;
  const int failed = flags[kFlagFail];
  __syncthreads();  // every wave has read the flag before thread 0 clears it
  if (failed) {
    fail_step(n, dx_out, info, flags + kFlagStop, delta_thresh);
    if (threadIdx.x == 0) flags[kFlagFail] = 0;
    return;
  }
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *rhs = smem;              // ld
  double *D = smem + ld;           // kTile x (kTile+1)
  float *dxs = reinterpret_cast<float *>(D + kTile * (kTile + 1));  // ld floats
  __shared__ float nrm[16];
  const int tid = threadIdx.x;
  for (int k = tid; k < ld; k += blockDim.x) rhs[k] = (k < n) ? A[(size_t)n * ld + k] : 0.0;
  const int nt = (n + kTile - 1) / kTile;
  for (int kb = nt - 1; kb >= 0; kb--) {
    __syncthreads();
    const double *T = A + (size_t)kb * kTile * ld + (size_t)kb * kTile;
    for (int k = tid; k < kTile * kTile; k += blockDim.x) D[(k / kTile) * (kTile + 1) + k % kTile] = T[(size_t)(k / kTile) * ld + k % kTile];
    __syncthreads();
    if (tid < 64) {  // one wave: L_kk^T x = rhs_kb
      double r = rhs[kb * kTile + tid];
      double x = 0.0;
      for (int c = kTile - 1; c >= 0; c--) {
        if (kb * kTile + c >= n) continue;  // uniform
        const double xc = __shfl(r, c, 64) / D[c * (kTile + 1) + c];
        if (tid < c) r -= D[c * (kTile + 1) + tid] * xc;
        if (tid == c) x = xc;
      }
      rhs[kb * kTile + tid] = (kb * kTile + tid < n) ? x : 0.0;  // rhs now holds x for this tile
    }
    __syncthreads();
    // rhs_j -= sum_r L[kb*64 + r][j] x_r for all j < kb*64
    for (int j = tid; j < kb * kTile; j += blockDim.x) {
      double s = 0.0;
      for (int r = 0; r < kTile; r++) s += A[(size_t)(kb * kTile + r) * ld + j] * rhs[kb * kTile + r];
      rhs[j] -= s;
    }
  }
  __syncthreads();
  finish_step(rhs, dxs, nrm, n, Twc, N, dx_out, info, flags + kFlagStop, delta_thresh);
}

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
  int off[kPlanSections];  // section offsets, order of m3s_symbolic.h
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
  const int32_t *dtr_ptr = pl + off[6], *dtr_slot = pl + off[7], *dtr_p = pl + off[8], *task_dst = pl + off[10],
                *task_tr_ptr = pl + off[12], *tr_a = pl + off[13], *tr_b = pl + off[14];
  const int32_t *clq = pl + off[28];
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
  const int32_t *perm = pl + D.off[0], *col_ptr = pl + D.off[1], *col_row = pl + D.off[2],
                *col_slot = pl + D.off[3], *lev_col = pl + D.off[5], *dtr_ptr = pl + D.off[6],
                *dtr_slot = pl + D.off[7], *dtr_p = pl + D.off[8], *task_dst = pl + D.off[10],
                *task_col = pl + D.off[11], *task_tr_ptr = pl + D.off[12], *tr_a = pl + D.off[13],
                *tr_b = pl + D.off[14], *asm_ptr = pl + D.off[15], *asm_edge = pl + D.off[16],
                *g_ptr = pl + D.off[17], *g_edge = pl + D.off[18], *wave_ptr = pl + D.off[21],
                *witems = pl + D.off[22], *part_q0 = pl + D.off[23], *part_q1 = pl + D.off[24],
                *part_tgt = pl + D.off[25], *dpart_ptr = pl + D.off[26], *opart_ptr = pl + D.off[27];
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
    const int32_t *clq = pl + D.off[28];
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
    const int32_t *lev_ptr = pl + D.off[4];
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
    const int32_t *lev_ptr = pl + D.off[4];
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
  const int32_t *col_ptr = pl + C.off[1], *dtr_ptr = pl + C.off[6], *dtr_slot = pl + C.off[7],
                *dtr_p = pl + C.off[8], *task_dst = pl + C.off[10], *task_tr_ptr = pl + C.off[12],
                *tr_a = pl + C.off[13], *tr_b = pl + C.off[14], *corder = pl + C.off[29], *ctask0 = pl + C.off[30];
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
  const int32_t *dtr_ptr = pl + D.off[6], *dtr_slot = pl + D.off[7], *dtr_p = pl + D.off[8],
                *task_dst = pl + D.off[10], *task_col = pl + D.off[11], *task_tr_ptr = pl + D.off[12],
                *tr_a = pl + D.off[13], *tr_b = pl + D.off[14];
  const int32_t *clq = pl + D.off[28];
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
  const int32_t *perm = C.plan + C.off[0];
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
  const int32_t *col_ptr = pl + C.off[1], *col_row = pl + C.off[2], *col_slot = pl + C.off[3],
                *corder = pl + C.off[29];
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

// ------------------------------------------- dense tail on the f64 MFMA --
// The top clique of the elimination tree (nc block columns, n = 7 nc scalar
// columns; SparsePlan::nc) after its border updates is a dense SPD system:
// a chain of n dependent pivots. sparse_llt_kernel factored it with 7x7 block
// products on one CU's dependent global-memory round trips (B1/B2, ~440 us at
// 256 KFs). Here one workgroup of 4 waves (one per SIMD) factors it
// left-looking over 16x16 fp64 tiles on v_mfma_f64_16x16x4f64, per tile
// column k:
//   update  A(I,k) -= sum_{j<k} L(I,j) L(k,j)^T for I >= k, accumulated in
//           registers (wave w owns the rows I = k + w (mod 4)); the finished
//           L tiles stream from L2 (written once, read by later columns);
//   diag    wave 0: A(k,k) -> L_kk (register Cholesky, readlane broadcasts),
//           W_k = L_kk^-1 into LDS (and global, for the back-substitution);
//   panel   L(I,k)^T = W_k A(I,k)^T on the MFMA, stored to L2.
// The RHS y is row n of the augmented matrix, so row n of the factor is
// y' = L^-1 y; then L^T x = y' by tile columns from the bottom. Every sum
// runs in a fixed order: bitwise reproducible (the sharded ranks rely on it).
// Replaces the dense-tail part of SimplicialLLT (gn_kernels.cu:132-153).
//
// Layouts. An accumulator tile holds A(I,k)^T in the MFMA C layout: lane l,
// register r = A(I,k)[l & 15][(l >> 4) + 4 r], which is also the operand
// order q = r of a product X . A(I,k)^T. Finished tiles are stored in that
// order, [tile][lane][4] (32 B per lane): every MFMA operand is one load.
constexpr int kTailNW = 4;     // waves (one per SIMD)
constexpr int kTailRows = (kTailMaxT + kTailNW - 1) / kTailNW;  // tile rows per wave and column

struct TailArgs {
  const double *Ad;  // bordered tail, dense symmetric [n][ld] (border_kernel writes it)
  int ld;
  double *rhs;       // y [m][7] in; x of the tail columns out (same place)
  double *Lg;        // finished L tiles, [tile (I,J) = I (I + 1) / 2 + J][64][4]
  double *Wg;        // [TC][16][16]: W_k of every tile column
  int32_t *flags;
  int nc, c0;        // tail columns, first tail column
};

// augmented tail matrix entry (i, j): padding columns are identity (and the
// unused (n, n)), padding rows zero, row n the RHS y of the tail columns
// Both loads are buffer loads, unconditional: an out-of-range offset reads 0
// (kFar), so a workgroup's initial tiles are all in flight at once (a
// guarded pointer load became one branch and one vmcnt(0) per entry).
struct TailSrc {
  __amdgpu_buffer_rsrc_t ad, rhs;
};
__device__ __forceinline__ TailSrc tail_src(const TailArgs &A, int n) {
  return {__builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(A.Ad), 0, n * A.ld * 8, 0x00020000),
          __builtin_amdgcn_make_buffer_rsrc(A.rhs + 7 * A.c0, 0, n * 8, 0x00020000)};
}
__device__ __forceinline__ double tail_entry(const TailArgs &A, const TailSrc &T, int n, int i, int j) {
  constexpr int kFar = 0x7fff0000;
  const bool pad = j >= n || i > n, rrow = i == n;
  const int ao = (!pad && !rrow) ? (i * A.ld + j) * 8 : kFar;
  const int ro = (!pad && rrow) ? j * 8 : kFar;
  const unsigned long long a = __builtin_bit_cast(unsigned long long, __builtin_amdgcn_raw_buffer_load_b64(T.ad, ao, 0, 0));
  const unsigned long long r = __builtin_bit_cast(unsigned long long, __builtin_amdgcn_raw_buffer_load_b64(T.rhs, ro, 0, 0));
  // at most one of the three is non-zero (the other loads read 0): OR, not a
  // select, so the loads stay unconditional
  const unsigned long long p = (pad && j >= n && i == j) ? 0x3ff0000000000000ull : 0ull;
  return __builtin_bit_cast(double, a | r | p);
}

// Diagonal tile (one wave, round 2): the tile stays in the MFMA C layout it
// was accumulated in (lane l, register r = A[(l >> 4) + 4 r][l & 15]) and is
// factored in four steps of 4 columns on the f64 MFMA. Step b: the 4x4 block
// D_b goes to every lane through LDS (the only LDS round trip of the step);
// every lane factors it in registers (L_D, W_D = L_D^-1); the panel
// P = A[:, 4b..4b+3] W_D^T is ONE MFMA (W_D x register b of the tile, which
// is the B operand as it stands, and the result lands in A-operand order);
// the trailing update A -= P P^T is one more. W = L^-1 is accumulated as the
// product of the elementary block-column inverses (two MFMAs per step, off
// the critical path). Round 1's by-rows form broadcast every column through
// LDS and ran ~2000 f64 instructions on one wave (~4 us per tile; this form
// is ~4x fewer). Padding columns / rows (>= jv, incl. the RHS row's own
// column) are identity; the RHS row's panel values are y' (-> yv_k). W ->
// Wk[16][17] (row-major). Returns true on a non-positive pivot (computed on
// with pivot 1; the step becomes dx = 0).
template <bool FULL>  // FULL: jv == 16 (every tile column but possibly the last): no padding masks
__device__ __forceinline__ bool tail_diag_mfma_t(f64x4 a, double (*Wk)[17], double *yv_k, int jv, int rhs_row,
                                                 int lane) {
  if (FULL) jv = 16;
  __shared__ double xd[4][16], xw[4][16];
  const int lr = lane & 15, lk = lane >> 4;
  f64x4 M;  // W accumulator, identity
#pragma unroll
  for (int r = 0; r < 4; r++) M[r] = (lk + 4 * r == lr) ? 1.0 : 0.0;
  bool bad = false;
#pragma unroll
  for (int b = 0; b < 4; b++) {
    const int c0 = 4 * b;
    // D_b[i][j] = A[c0 + i][c0 + j]: register b of the lanes with column lr in the block
    if (lr >= c0 && lr < c0 + 4) xd[b][4 * lk + lr - c0] = a[b];
    wave_lds_fence();
    bool real[4];
#pragma unroll
    for (int m = 0; m < 4; m++) real[m] = FULL || c0 + m < jv;
    double D[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j <= i; j++) {
        const double v = xd[b][4 * i + j];
        D[i][j] = (real[i] && real[j]) ? v : (i == j ? 1.0 : 0.0);
      }
    // 4x4 Cholesky and W_D = L_D^-1, on every lane
    double L[4][4], Wd[4][4], iv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      double d = D[j][j];
      bad |= real[j] && !(d > 0.0);
      d = d > 0.0 ? d : 1.0;
      iv[j] = rsqrt_nr(d);
#pragma unroll
      for (int i = j + 1; i < 4; i++) L[i][j] = D[i][j] * iv[j];
#pragma unroll
      for (int i = j + 1; i < 4; i++)
#pragma unroll
        for (int k = j + 1; k <= i; k++) D[i][k] -= L[i][j] * L[k][j];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      Wd[i][i] = iv[i];
#pragma unroll
      for (int j = 0; j < i; j++) {
        double s = 0.0;
#pragma unroll
        for (int k = j; k < i; k++) s += L[i][k] * Wd[k][j];
        Wd[i][j] = -s * iv[i];
      }
    }
    // A operands: Wpad[lr][lk] = W_D[lr][lk] (lr < 4); A1[lr][lk] = (W_D - I)[lr - c0][lk] (lr in the
    // block): W_D through LDS (every lane holds it; lane 0 writes, each lane reads its entry)
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) xw[b][4 * i + k] = k <= i ? Wd[i][k] : 0.0;
    }
    wave_lds_fence();
    const double wpad = lr < 4 ? xw[b][4 * lr + lk] : 0.0;
    const double a1 =
        (lr >= c0 && lr < c0 + 4) ? xw[b][4 * (lr - c0) + lk] - (lr - c0 == lk ? 1.0 : 0.0) : 0.0;
    // panel P[lr][lk] = L[lr][c0 + lk] (rows above the block and padding columns 0)
    double p = __builtin_amdgcn_mfma_f64_16x16x4f64(wpad, a[b], f64x4{0.0, 0.0, 0.0, 0.0}, 0, 0, 0)[0];
    p = (lr >= c0 && (FULL || c0 + lk < jv)) ? p : 0.0;
    if (!FULL && lr == rhs_row && c0 + lk < jv) yv_k[c0 + lk] = p;
    a = __builtin_amdgcn_mfma_f64_16x16x4f64(-p, p, a, 0, 0, 0);  // A -= P P^T
    // W <- (elementary inverse of block column b) W: the block rows by W_D,
    // then the real rows below lose P_below times them
    const f64x4 Y = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, M[b], M, 0, 0, 0);
    const double a2 = (lr >= c0 + 4 && (FULL || lr < jv)) ? -p : 0.0;
    M = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, Y[b], Y, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; r++) Wk[lk + 4 * r][lr] = M[r];
  return bad;
}
// Not inlined: each tail workgroup factors its diagonal tile(s) once, so the
// ~600 instructions run from a cold instruction cache (measured ~2.5 us per
// tile, ~4x the MFMA / LDS latencies it is made of). One copy of the code, run
// once on a dummy tile while the workgroup waits for its updates
// (tail_diag_warm), is then hot when the real tile arrives.
// Round 6 measured a right-looking by-columns form on DPP row broadcasts
// (v_mov_b64_dpp row_newbcast, no LDS or MFMA on the chain):
// 8.7k cycles per hot call against 5.4k for this one
// (profiles/r06/r6h_ubench_diag16.txt, tools/ubench_diag16.hip): a 64-bit
// DPP broadcast feeding an FMA costs ~30 cycles, 120 of them per tile.
__device__ __noinline__ bool tail_diag_full(f64x4 a, double (*Wk)[17], double *yv_k, int lane) {
  return tail_diag_mfma_t<true>(a, Wk, yv_k, 16, -1, lane);
}
__device__ __noinline__ bool tail_diag_part(f64x4 a, double (*Wk)[17], double *yv_k, int jv, int rhs_row, int lane) {
  return tail_diag_mfma_t<false>(a, Wk, yv_k, jv, rhs_row, lane);
}
__device__ __forceinline__ bool tail_diag_mfma(f64x4 a, double (*Wk)[17], double *yv_k, int jv, int rhs_row,
                                               int lane) {
  return jv == 16 ? tail_diag_full(a, Wk, yv_k, lane) : tail_diag_part(a, Wk, yv_k, jv, rhs_row, lane);
}
// the warm-up: an identity tile through the same call (W lands in Wk before
// the real factor overwrites it; y' goes to the dummy yv_k)
__device__ __forceinline__ void tail_diag_warm(double (*Wk)[17], double *yv_dummy, int jv, int rhs_row, int lane) {
  const int lr = lane & 15, lk = lane >> 4;
  f64x4 e;
#pragma unroll
  for (int r = 0; r < 4; r++) e[r] = (lk + 4 * r == lr) ? 1.0 : 0.0;
  (void)tail_diag_mfma(e, Wk, yv_dummy, jv, rhs_row, lane);
}

__device__ __forceinline__ int tail_tile(int I, int J) { return I * (I + 1) / 2 + J; }

// one finished tile's operand registers (32 B per lane, L2)
__device__ __forceinline__ f64x4 tail_load(const double *Lg, int t, int lane) {
  const f64x4 *p = reinterpret_cast<const f64x4 *>(Lg + (size_t)t * 256) + lane;
  return __builtin_nontemporal_load(p);
}

__global__ void __launch_bounds__(64 * kTailNW, 1) tail_llt_kernel(TailArgs A) {
  if (A.flags[kFlagStop]) return;
  __shared__ double Wk[16][17];  // W_k of the current step
  __shared__ double yv[16 * kTailMaxT], xv[16 * kTailMaxT];
  __shared__ int fail_s;
  const int n = 7 * A.nc;
  const TailSrc TS = tail_src(A, n);
  const int TC = (n + 15) / 16, TR = (n + 16) / 16;  // tile columns; tile rows incl. the RHS row n
  const int In = n / 16, rn = n - 16 * In;             // RHS row: tile row, local row
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lk = lane >> 4;
  double *Lg = A.Lg, *Wg = A.Wg;
  if (tid == 0) fail_s = 0;
  for (int q = tid; q < 16 * kTailMaxT; q += 64 * kTailNW) yv[q] = 0.0, xv[q] = 0.0;
  __syncthreads();
#ifdef M3S_TAIL_STAMPS
  int64_t *stamp = reinterpret_cast<int64_t *>(Wg + (size_t)kTailMaxT * 256);
#define M3S_STAMP(i) if (tid == 0) stamp[i] = wall_clock64();
#else
#define M3S_STAMP(i)
#endif
  M3S_STAMP(0)
  for (int k = 0; k < TC; k++) {
    // column k: wave w holds the rows I = k + w + 4u (u < kTailRows)
    f64x4 acc[kTailRows];
#pragma unroll
    for (int u = 0; u < kTailRows; u++) {
      const int I = k + wave + kTailNW * u;
      f64x4 v = {0.0, 0.0, 0.0, 0.0};
      if (I < TR) {
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = tail_entry(A, TS, n, 16 * I + lr, 16 * k + lk + 4 * r);
      }
      acc[u] = v;
    }
    // A(I,k)^T -= L(k,j) L(I,j)^T, j ascending; the operands of j + 2 are
    // in flight while j's products run (3-deep register ring)
    f64x4 rk[3], ri[3][kTailRows];
#define M3S_TAIL_ISSUE(j_, b_)                                                           \
  do {                                                                                   \
    rk[b_] = tail_load(Lg, tail_tile(k, (j_)), lane);                                    \
    for (int u = 0; u < kTailRows; u++) {                                                \
      const int I = k + wave + kTailNW * u;                                              \
      if (I < TR) ri[b_][u] = tail_load(Lg, tail_tile(I, (j_)), lane);                   \
    }                                                                                    \
  } while (0)
#define M3S_TAIL_UPD(b_)                                                                 \
  do {                                                                                   \
    for (int u = 0; u < kTailRows; u++) {                                                \
      const int I = k + wave + kTailNW * u;                                              \
      if (I < TR) {                                                                      \
        for (int q = 0; q < 4; q++)                                                      \
          acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(-rk[b_][q], ri[b_][u][q], acc[u], 0, 0, 0); \
      }                                                                                  \
    }                                                                                    \
  } while (0)
    if (k > 0) M3S_TAIL_ISSUE(0, 0);
    if (k > 1) M3S_TAIL_ISSUE(1, 1);
    for (int j = 0; j < k; j += 3) {
      if (j + 2 < k) M3S_TAIL_ISSUE(j + 2, 2);
      M3S_TAIL_UPD(0);
      if (j + 1 >= k) break;
      if (j + 3 < k) M3S_TAIL_ISSUE(j + 3, 0);
      M3S_TAIL_UPD(1);
      if (j + 2 >= k) break;
      if (j + 4 < k) M3S_TAIL_ISSUE(j + 4, 1);
      M3S_TAIL_UPD(2);
    }
#undef M3S_TAIL_ISSUE
#undef M3S_TAIL_UPD
    M3S_STAMP(1 + 3 * k)
    if (wave == 0) {  // diag: tile (k, k) is wave 0's u = 0
      if (tail_diag_mfma(acc[0], Wk, yv + 16 * k, min(16, n - 16 * k), In == k ? rn : -1, lane) && lane == 0)
        fail_s = 1;
      wave_lds_fence();
      if (lane < 16) {
#pragma unroll
        for (int r = 0; r < 16; r++) Wg[(size_t)k * 256 + r * 16 + lane] = Wk[r][lane];
      }
    }
    M3S_STAMP(2 + 3 * k)
    __syncthreads();  // W_k
    // panel: L(I,k)^T = W_k A(I,k)^T for I > k, stored in operand order
#pragma unroll
    for (int u = 0; u < kTailRows; u++) {
      const int I = k + wave + kTailNW * u;
      if (I < TR && I > k) {
        f64x4 d = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 4; q++) d = __builtin_amdgcn_mfma_f64_16x16x4f64(Wk[lr][4 * q + lk], acc[u][q], d, 0, 0, 0);
        reinterpret_cast<f64x4 *>(Lg + (size_t)tail_tile(I, k) * 256)[lane] = d;
        if (I == In && lr == rn) {  // y' of this column from the RHS row
#pragma unroll
          for (int r = 0; r < 4; r++) yv[16 * k + lk + 4 * r] = d[r];
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // L(., k) in L2 before any wave loads it
    __syncthreads();
    M3S_STAMP(3 + 3 * k)
  }
  // back-substitution L^T x = y', tile columns from the bottom; yv
  // accumulates the updates of each column in decreasing K (fixed order).
  // Thread (J, c) (two per thread: 16 (K - 1) <= 496 pairs) sums column c of
  // tile (K, J), L(K,J)[r][c] at lane 16 (c % 4) + r, register c / 4; the next
  // row's tiles and W are loaded while this row runs.
  constexpr int kBP = (16 * kTailMaxT + 64 * kTailNW - 1) / (64 * kTailNW);  // pairs per thread
  double lb[kBP][16], wb[16];
  auto bs_load = [&](int K) {
#pragma unroll
    for (int pp = 0; pp < kBP; pp++) {
      const int q = tid + 64 * kTailNW * pp, J = q >> 4, c = q & 15;
      if (J < K) {
        const double *T = Lg + (size_t)tail_tile(K, J) * 256 + (c >> 2);
#pragma unroll
        for (int r = 0; r < 16; r++) lb[pp][r] = __builtin_nontemporal_load(T + 4 * (16 * (c & 3) + r));
      }
    }
    if (wave == 0 && lane < 16) {
#pragma unroll
      for (int i = 0; i < 16; i++) wb[i] = Wg[(size_t)K * 256 + i * 16 + lane];
    }
  };
  if (TC > 0) bs_load(TC - 1);
  for (int K = TC - 1; K >= 0; K--) {
    const int jv = min(16, n - 16 * K);
    if (wave == 0 && lane < 16) {
      double x = 0.0;
#pragma unroll
      for (int i = 0; i < 16; i++) x += wb[i] * yv[16 * K + i];
      xv[16 * K + lane] = lane < jv ? x : 0.0;
    }
    __syncthreads();
    double u[kBP];
#pragma unroll
    for (int pp = 0; pp < kBP; pp++) {
      u[pp] = 0.0;
      const int q = tid + 64 * kTailNW * pp, J = q >> 4;
      if (J < K) {
#pragma unroll
        for (int r = 0; r < 16; r++) u[pp] += lb[pp][r] * xv[16 * K + r];
      }
    }
    if (K > 0) bs_load(K - 1);
#pragma unroll
    for (int pp = 0; pp < kBP; pp++) {
      const int q = tid + 64 * kTailNW * pp, J = q >> 4, c = q & 15;
      if (J < K) yv[16 * J + c] -= u[pp];
    }
    __syncthreads();
  }
  M3S_STAMP(100)
  for (int j = tid; j < n; j += 64 * kTailNW) A.rhs[7 * A.c0 + j] = xv[j];
  if (tid == 0 && fail_s) A.flags[kFlagSplitFail] = 1;
#undef M3S_STAMP
}

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

int m3s_gn_release(const m3s_gn_args *a, void *stream) {
  if (!a || !a->workspace) return M3S_EINVAL;
  (void)stream;  // no sync: every queued upload reads pinned staging, not the entry
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
  const int64_t offs[kPlanSections] = {
      I.off_perm,     I.off_col_ptr,  I.off_col_row,     I.off_col_slot, I.off_lev_ptr,
      I.off_lev_col,  I.off_dtr_ptr,  I.off_dtr_slot,    I.off_dtr_p,    I.off_task_lev_ptr,
      I.off_task_dst, I.off_task_col, I.off_task_tr_ptr, I.off_tr_a,     I.off_tr_b,
      I.off_asm_ptr,  I.off_asm_edge, I.off_g_ptr,       I.off_g_edge,   I.off_ctask_ptr,
      I.off_items,    I.off_wave_ptr, I.off_witems,    I.off_part_q0,  I.off_part_q1,
      I.off_part_tgt, I.off_dpart_ptr, I.off_opart_ptr, I.off_clq, I.off_corder, I.off_ctask0};
  if (meta) {
    meta[0] = P.m, meta[1] = P.S, meta[2] = P.levels;
    for (int k = 0; k < kPlanSections; k++) meta[3 + k] = (int32_t)offs[k];
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

size_t m3s_gn_layout_debug(int64_t N, int64_t HW, int64_t E, size_t *offs) {
  const Layout L = gn_layout(N, HW, E);
  const size_t o[15] = {L.flags, L.rank_i, L.rank_j, L.first, L.partials, L.edge_sums, L.A, L.fin,
                        L.plan,  L.Lblk,   L.Dinv,   L.tail,  L.eorder,   L.planes,    L.total};
  if (offs) std::copy(o, o + 15, offs);
  return L.total;
}

}  // extern "C"

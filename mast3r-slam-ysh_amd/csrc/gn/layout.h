// gn/layout.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The constants and the workspace: the linearize block and grid sizes
// (kThreads ... kMaxLd), the workspace flags (kFlagStop, kFlagFail,
// kFlagSplitFail), chunks_for and chunk_pixels, the dense tail's scratch
// sizes (kTailMaxT, kGNx, tail_scratch_doubles), Layout / gn_layout / at<>,
// the tracker's TrackState and the forward declaration of track_solve_block
// (defined in gn/track.h, called by linearize_kernel's last chunk).
// Host code but for that declaration. Relies on nothing but kNP
// (m3s_device.h); every later part relies on this one.

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

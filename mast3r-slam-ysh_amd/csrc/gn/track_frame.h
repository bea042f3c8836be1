// gn/track_frame.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The front end of m3s_track_frame: the three prep launches
// (track_prep_clear_kernel, track_prep_kernel, track_prep_count_kernel) and
// track_frame_impl, which then runs track_impl (gn/track.h) on the prepared rows.

// ------------------------------------------------------ track_frame prep --
// The front end of FrameTracker.track (tracker.py:41-67, 103-108, 129-154)
// ahead of the tracker launches above: three small launches per call.
//   1 track_prep_clear_kernel  zeroes the occupancy map and stats[0..3]
//   2 track_prep_kernel        one lane per keyframe pixel n, j = idx_f2k[n]:
//       Xf_g[n] = Xf_canon[j] (calib: constrained to the ray of pixel j, the
//       operation order of backproject, geometry.py:107-115: divide, then
//       multiply), Xk_g[n] likewise from Xk_canon[n], valid_opt[n], and
//       map[j] = 1 where valid_match[n]: a byte map of the frame's pixels
//       written with plain stores (every writer stores the same 1, so the
//       stores need no order). n_opt and n_kf: a wave ballot and popcount,
//       summed over the workgroup's waves in LDS, one integer atomic add per
//       workgroup and counter (integer sums have no order: deterministic).
//   3 track_prep_count_kernel  n_unique = the number of set bytes of the map,
//       16 map bytes per lane, one integer atomic add per workgroup.
// No sort and no compaction: torch.unique(idx[valid]).shape[0] is the number
// of frame pixels hit at least once. Nothing is carried between calls: launch
// 1 clears every word launches 2 and 3 read.
constexpr int kPrepThreads = 256;
constexpr int kPrepWaves = kPrepThreads / 64;
constexpr int kPrepMapPerLane = 16;  // map bytes per lane and access (one dwordx4)

struct PrepArgs {
  const float *Xf_canon, *Cf_sum, *Xk_canon, *Ck_sum, *Qk;
  const float *K;  // device 3x3; null: rays mode (rows copied as they are)
  const int32_t *idx;
  const uint8_t *valid_match;
  float *Xf_g;
  float *Xk_g;  // null: the keyframe rows are not written (rays mode reads Xk_canon itself)
  uint8_t *valid_opt;
  uint8_t *map;  // [map_bytes(HW)]
  int32_t *stats;
  int64_t HW;
  int W;
  float Nf, Nk, C_conf, Q_conf;
};

inline size_t prep_map_bytes(int64_t HW) { return align_up((size_t)HW, kPrepMapPerLane); }

__global__ void __launch_bounds__(kPrepThreads) track_prep_clear_kernel(u32x4 *map, int64_t n16, int32_t *stats) {
  const int64_t stride = (int64_t)gridDim.x * kPrepThreads;
  for (int64_t k = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x; k < n16; k += stride)
    map[k] = u32x4{0u, 0u, 0u, 0u};
  if (blockIdx.x == 0 && threadIdx.x < 4) stats[threadIdx.x] = 0;
}

// sum of one int per lane over the workgroup (every lane of every wave calls
// it); the result is valid in thread 0
__device__ __forceinline__ int prep_block_sum(int c, int *sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  int s = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kPrepWaves; w++) s += sh[w];
  return s;
}

__global__ void __launch_bounds__(kPrepThreads) track_prep_kernel(PrepArgs A) {
  __shared__ int sh[2][kPrepWaves];
  const int64_t n = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x;
  bool opt = false, kf = false;
  if (n < A.HW) {  // no early return: every lane reaches the ballots and the barrier
    int64_t j = A.idx[n];
    bool vm = A.valid_match[n] != 0;
    // idx_f2k in [0, HW) is the caller's contract; a value outside it is never
    // used as an address
    if (j < 0 || j >= A.HW) j = 0, vm = false;
    const float q = A.Qk[n];
    const float cf = A.Cf_sum[j] / A.Nf, ck = A.Ck_sum[n] / A.Nk;  // frame.py:102-103
    kf = vm && q > A.Q_conf;
    opt = kf && cf > A.C_conf && ck > A.C_conf;
    float xf = A.Xf_canon[3 * j], yf = A.Xf_canon[3 * j + 1];
    const float zf = A.Xf_canon[3 * j + 2];
    float fx = 1.0f, fy = 1.0f, cx = 0.0f, cy = 0.0f;
    if (A.K) {
      fx = A.K[0], fy = A.K[4], cx = A.K[2], cy = A.K[5];
      const int v = (int)j / A.W, u = (int)j - v * A.W;  // j < HW <= INT32_MAX
      xf = zf * (((float)u - cx) / fx);
      yf = zf * (((float)v - cy) / fy);
    }
    A.Xf_g[3 * n] = xf, A.Xf_g[3 * n + 1] = yf, A.Xf_g[3 * n + 2] = zf;
    if (A.Xk_g) {
      float xk = A.Xk_canon[3 * n], yk = A.Xk_canon[3 * n + 1];
      const float zk = A.Xk_canon[3 * n + 2];
      if (A.K) {
        const int v = (int)n / A.W, u = (int)n - v * A.W;
        xk = zk * (((float)u - cx) / fx);
        yk = zk * (((float)v - cy) / fy);
      }
      A.Xk_g[3 * n] = xk, A.Xk_g[3 * n + 1] = yk, A.Xk_g[3 * n + 2] = zk;
    }
    A.valid_opt[n] = opt ? 1 : 0;
    if (vm) A.map[j] = 1;
  }
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const uint64_t m_opt = __builtin_amdgcn_ballot_w64(opt), m_kf = __builtin_amdgcn_ballot_w64(kf);
  if (lane == 0) sh[0][wave] = (int)__builtin_popcountll(m_opt), sh[1][wave] = (int)__builtin_popcountll(m_kf);
  __syncthreads();
  if (threadIdx.x < 2) {
    int s = 0;
    for (int w = 0; w < kPrepWaves; w++) s += sh[threadIdx.x][w];
    if (s) atomicAdd(&A.stats[threadIdx.x], s);
  }
}

__global__ void __launch_bounds__(kPrepThreads) track_prep_count_kernel(const u32x4 *map, int64_t n16,
                                                                        int32_t *stats) {
  __shared__ int sh[kPrepWaves];
  const int64_t k = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x;
  int c = 0;
  if (k < n16) {
    const u32x4 w = map[k];  // bytes are 0 or 1
    c = __builtin_popcount(w.x) + __builtin_popcount(w.y) + __builtin_popcount(w.z) + __builtin_popcount(w.w);
  }
  const int s = prep_block_sum(c, sh);
  if (threadIdx.x == 0 && s) atomicAdd(&stats[2], s);
}

// workspace of m3s_track_frame: the tracker's own workspace first (handed to
// track_impl unchanged), then the map and the prepared rows
struct FrameLayout {
  size_t track, map, xf, xk, valid, total;
};
FrameLayout frame_layout(int64_t HW) {
  FrameLayout L;
  const size_t hw = (size_t)std::max<int64_t>(HW, 0);
  L.track = 0;
  L.map = align_up(m3s_track_workspace_size(HW), 256);
  L.xf = L.map + align_up(prep_map_bytes(hw), 256);
  L.xk = L.xf + align_up(12 * hw, 256);
  L.valid = L.xk + align_up(12 * hw, 256);
  L.total = L.valid + align_up(hw, 256);
  return L;
}

int track_frame_impl(const m3s_track_frame_args *a, void *stream) {
  if (!a || !a->Xf_canon || !a->Cf_sum || !a->Xk_canon || !a->Ck_sum || !a->idx_f2k || !a->valid_match ||
      !a->Qk || !a->T_WCf || !a->T_WCk || !a->T_WCf_out || !a->T_CkCf_out || !a->info || !a->stats ||
      !a->workspace)
    return M3S_EINVAL;
  if (a->HW < 1 || a->height < 1 || a->width < 1 || a->HW != (int64_t)a->height * a->width) return M3S_EINVAL;
  if (a->HW > INT32_MAX) return M3S_ETOOLARGE;  // idx_f2k is int32
  if (a->Nf < 1 || a->Nk < 1) return M3S_EINVAL;
  const FrameLayout Ly = frame_layout(a->HW);
  if (a->workspace_bytes < Ly.total) return M3S_EINVAL;
  const bool calib = a->K != nullptr;
  hipStream_t st = S(stream);
  float *Xf_g = a->Xf_out ? a->Xf_out : at<float>(a->workspace, Ly.xf);
  // rays mode: the keyframe rows are Xk_canon as it is; they are copied only
  // into a buffer the caller asks for (and not onto themselves)
  float *Xk_g = a->Xk_out ? a->Xk_out : (calib ? at<float>(a->workspace, Ly.xk) : nullptr);
  if (!calib && Xk_g == a->Xk_canon) Xk_g = nullptr;
  uint8_t *valid_opt = a->valid_opt_out ? a->valid_opt_out : at<uint8_t>(a->workspace, Ly.valid);
  uint8_t *map = at<uint8_t>(a->workspace, Ly.map);
  const int64_t n16 = (int64_t)(prep_map_bytes(a->HW) / kPrepMapPerLane);
  const int64_t count_blocks = (n16 + kPrepThreads - 1) / kPrepThreads;
  track_prep_clear_kernel<<<(unsigned)std::min<int64_t>(count_blocks, 256), kPrepThreads, 0, st>>>(
      reinterpret_cast<u32x4 *>(map), n16, a->stats);
  int rc;
  if ((rc = launch_ok())) return rc;
  PrepArgs A{};
  A.Xf_canon = a->Xf_canon, A.Cf_sum = a->Cf_sum, A.Xk_canon = a->Xk_canon, A.Ck_sum = a->Ck_sum;
  A.Qk = a->Qk, A.K = a->K, A.idx = a->idx_f2k, A.valid_match = a->valid_match;
  A.Xf_g = Xf_g, A.Xk_g = Xk_g, A.valid_opt = valid_opt, A.map = map, A.stats = a->stats;
  A.HW = a->HW, A.W = a->width;
  A.Nf = (float)a->Nf, A.Nk = (float)a->Nk, A.C_conf = a->C_conf, A.Q_conf = a->Q_conf;
  track_prep_kernel<<<(unsigned)((a->HW + kPrepThreads - 1) / kPrepThreads), kPrepThreads, 0, st>>>(A);
  if ((rc = launch_ok())) return rc;
  track_prep_count_kernel<<<(unsigned)count_blocks, kPrepThreads, 0, st>>>(reinterpret_cast<const u32x4 *>(map),
                                                                          n16, a->stats);
  if ((rc = launch_ok())) return rc;
  // the launches of m3s_track_{rays,calib}_sim3 on the prepared rows
  m3s_track_args t{};
  t.Xf = Xf_g, t.Xk = Xk_g ? Xk_g : a->Xk_canon, t.Qk = a->Qk, t.valid = valid_opt;
  t.T_WCf = a->T_WCf, t.T_WCk = a->T_WCk, t.K = a->K;
  t.HW = a->HW;
  t.height = calib ? a->height : 0, t.width = calib ? a->width : 0;
  t.pixel_border = a->pixel_border, t.z_eps = a->z_eps;
  t.sigma_a = a->sigma_a, t.sigma_b = a->sigma_b, t.huber_k = a->huber_k;
  t.max_iters = a->max_iters, t.rel_error = a->rel_error, t.delta_norm = a->delta_norm;
  t.sync_every = a->sync_every;
  t.T_WCf_out = a->T_WCf_out, t.T_CkCf_out = a->T_CkCf_out, t.info = a->info;
  t.workspace = at<void>(a->workspace, Ly.track);
  t.workspace_bytes = Ly.map;
  return track_impl(&t, calib ? M3S_MODE_CALIB : M3S_MODE_RAYS, stream);
}

// gn/track.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The tracker (m3s_track_{rays,calib}_sim3, and the back half of
// m3s_track_frame): track_init_kernel, then track_persistent_kernel, every
// iteration in one launch, or one linearize_kernel<MODE, TRACK> launch per
// iteration whose last chunk runs track_solve_block. track_impl launches them.

// --------------------------------------------------------------- tracker --

constexpr size_t kTrackStateOff = 0;

struct TrackSync;
// Zeroes the sync words and the persistent kernel's partial granules (n_part
// 16-B granules, 0 on the launch-per-iteration path) of THIS call: a granule
// is accepted once its tag equals it + 1, so a granule left with tag 1 by a
// call that stopped after its first iteration (or a reused allocation holding
// such a word) must never be read as iteration 0's partial.
__global__ void __launch_bounds__(256) track_init_kernel(const float *T_WCf, const float *T_WCk, TrackState *st,
                                                         int32_t *info, float *T_WCf_out, float *T_CkCf_out,
                                                         uint32_t *sync_words, int n_sync, u32x4 *part, int n_part) {
  for (int k = threadIdx.x; k < n_sync; k += blockDim.x) sync_words[k] = 0u;
  for (int k = threadIdx.x; k < n_part; k += blockDim.x) part[k] = u32x4{0u, 0u, 0u, 0u};
  if (threadIdx.x != 0) return;
  const Sim3f Tk = load_sim3(T_WCk), Tf = load_sim3(T_WCf);
  const Sim3f R = compose(inverse(Tk), Tf);
  store_sim3(st->T_rel, R);
  store_sim3(st->T_WCk, Tk);
  st->old_cost = __builtin_inf();
  st->done = 0;
  st->arrive = 0;
  for (int k = 0; k < 8; k++) info[k] = 0;
  store_sim3(T_CkCf_out, R);
  store_sim3(T_WCf_out, Tf);
}

// One tracker GN update from the reduced sums s (kL / kG / kCost layout):
// 7x7 fp64 Cholesky of H (one thread, fully unrolled; 1/L_kk by rsqrt_nr:
// v_rsq_f64 + one Newton step, 4.2e-15 relative, round 4 -- the tracker's
// fixture parity, 1e-5 + 1e-4 sum|tau| per pose, holds with it; no IEEE sqrt /
// division sequences on the serial chain),
// tau = -H^-1 g (tracker.py:156-171: g = sum w e J with e = pred - meas), the
// retraction T <- Exp(tau) T, and check_convergence (nonlinear_optimizer.py:
// 5-25; rel is NaN on the first step, old_cost = inf). T and old_cost are
// updated in place unless the Cholesky fails.
constexpr int kTrackContinue = 0, kTrackConverged = 1, kTrackFailed = 2;
// A/B: the tracker's 7x7 Cholesky solve in fp32 (the reference's precision,
// tracker.py:168) instead of fp64: +1% GN it/s at C2
// (profiles/r05/trk_ab_f32_solve_REJECTED.txt), not worth the precision
__device__ __forceinline__ int track_update(const double *s, Sim3f &T, double &old_cost, float rel_error,
                                            float delta_norm) {
  typedef double real;
  real H[7][7], L[7][7], g[7], y[7], x[7];
  for (int a = 0; a < 7; a++)
    for (int c = 0; c < 7; c++) H[a][c] = (real)s[kL + tri(a < c ? a : c, a < c ? c : a)];
  for (int a = 0; a < 7; a++) g[a] = (real)s[kG + a];
  const double cost = 0.5 * s[kCost];
  real dinv[7];
#pragma unroll
  for (int a = 0; a < 7; a++)
#pragma unroll
    for (int c = 0; c < 7; c++) L[a][c] = 0.0;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    real d = H[k][k];
#pragma unroll
    for (int p = 0; p < k; p++) d -= L[k][p] * L[k][p];
    if (!(d > (real)0)) return kTrackFailed;
    dinv[k] = rsqrt_nr(d);
    L[k][k] = d * dinv[k];
#pragma unroll
    for (int i = k + 1; i < 7; i++) {
      real v = H[i][k];
#pragma unroll
      for (int p = 0; p < k; p++) v -= L[i][p] * L[k][p];
      L[i][k] = v * dinv[k];
    }
  }
#pragma unroll
  for (int i = 0; i < 7; i++) {
    real v = -g[i];
#pragma unroll
    for (int p = 0; p < i; p++) v -= L[i][p] * y[p];
    y[i] = v * dinv[i];
  }
#pragma unroll
  for (int i = 6; i >= 0; i--) {
    real v = y[i];
#pragma unroll
    for (int p = i + 1; p < 7; p++) v -= L[p][i] * x[p];
    x[i] = v * dinv[i];
  }
  float tau[7];
  float n2 = 0.0f;
  for (int k = 0; k < 7; k++) {
    tau[k] = (float)x[k];
    n2 += tau[k] * tau[k];
  }
  T = retract(tau, T);
  const float cost_f = (float)cost;  // the reference's cost is a python float of an fp32 .item()
  const double rel = fabs((old_cost - (double)cost_f) / old_cost);  // NaN on the first step
  old_cost = (double)cost_f;
  return (rel < (double)rel_error || sqrtf(n2) < delta_norm) ? kTrackConverged : kTrackContinue;
}

// reduce chunk partials, 7x7 fp64 Cholesky, tau = -H^-1 g, retraction,
// convergence (nonlinear_optimizer.py:5-25), outputs.
constexpr int kTrackSolveThreads = 256;  // = the linearize block (the fused solve runs in one)
__device__ void track_solve_block(const LinArgs &A) {
  const float *__restrict__ partials = A.partials;
  const int64_t chunks = A.chunks;
  TrackState *st = A.track;
  int32_t *info = A.info;
  const float rel_error = A.rel_error, delta_norm = A.delta_norm;
  float *T_WCf_out = A.T_WCf_out, *T_CkCf_out = A.T_CkCf_out;
  // fp64 sums of the chunk partials: thread t adds chunks t, t + 256, ... (all
  // 36 values of a chunk are loaded together), then a fixed tree over the
  // threads (wave butterfly, then the 4 waves in order): deterministic, and
  // every load is in flight at once instead of one dependent chain per value
  __shared__ double s[kNP], wpart[kTrackSolveThreads / 64][kNP];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  double acc[kNP];
#pragma unroll
  for (int k = 0; k < kNP; k++) acc[k] = 0.0;
  for (int64_t c = t; c < chunks; c += kTrackSolveThreads) {
    const float4 *p4 = reinterpret_cast<const float4 *>(partials + (size_t)c * kNP);
#pragma unroll
    for (int q = 0; q < kNP / 4; q++) {
      const float4 v = p4[q];
      acc[4 * q] += (double)v.x, acc[4 * q + 1] += (double)v.y;
      acc[4 * q + 2] += (double)v.z, acc[4 * q + 3] += (double)v.w;
    }
  }
  int xi;
  bool xv;
  const double xs = xreduce36(acc, lane, xi, xv);  // transposed wave reduction (store_partial)
  if (xv) wpart[wv][xi] = xs;
  __syncthreads();
  if (t < kNP) {
    double a = 0.0;
#pragma unroll
    for (int w = 0; w < kTrackSolveThreads / 64; w++) a += wpart[w][t];
    s[t] = a;
  }
  __syncthreads();
  if (t != 0) return;
  Sim3f T = load_sim3(st->T_rel);
  double old = st->old_cost;
  const int r = track_update(s, T, old, rel_error, delta_norm);
  info[M3S_INFO_ITERS] += 1;
  if (r == kTrackFailed) {  // torch.linalg.cholesky raises -> tracking failure
    info[M3S_INFO_SOLVE_FAIL] = 1;
    st->done = 1;
    return;
  }
  store_sim3(st->T_rel, T);
  store_sim3(T_CkCf_out, T);
  store_sim3(T_WCf_out, compose(load_sim3(st->T_WCk), T));
  if (r == kTrackConverged) {
    st->done = 1;
    info[M3S_INFO_CONVERGED] = 1;
  }
  st->old_cost = old;
}

// ------------------------------------------------ persistent tracker GN --
// All iterations of one frame -> keyframe solve in ONE launch (tracker.py:
// 173-266). G <= 256 workgroups, one per CU, each owning PPL pixels per lane.
// A lane loads its pixels' inputs once (target-side PixIn from Xk / Q / valid
// and the source point Xf) and keeps them in registers across iterations, so
// iterations 2.. read nothing from HBM. Per iteration (round 4: every
// hand-off is a tagged 16-B granule, {payload | it + 1}, stored write-through
// and polled by its reader; a 16-B store lands whole, so no drain, counter or
// second load of the payload sits on the critical path):
//   1. each workgroup accumulates its pixels (the packed Accum of the backend
//      kernels) and stores its 36-float partial as 12 granules;
//   2. workgroup s < 8 polls the granules of shard s = {s, s + 8, ...} (lane j:
//      member s + 8 j), sums them across lanes in a fixed order (fp64) and
//      publishes the 36 shard sums as granules;
//   3. workgroup 0 polls the 8 shards' granules, sums them in shard order,
//      runs the 7x7 update (track_update) and publishes the record (pose,
//      status, cost) as 4 granules; every other workgroup polls those.
// Reuse of the granules is safe: a workgroup stores iteration it + 1's
// partial only after it read iteration it's record, which workgroup 0
// published after every shard reducer had read iteration it's partials.
// The reduction order is fixed (deterministic). Waits are bounded: a timed-out
// shard sum is NaN (the update then fails, info[SOLVE_FAIL] = 1), a timed-out
// record poll ends the solve with info[SOLVE_FAIL] = 2. Round 2 and 3 used
// drained sc1 stores + agent atomic counters (MI355X_MICROARCH.md
// inter-workgroup table, row 1): 95-99k GN it/s at C2 against ~112k+ now.
// workgroup size: 256 threads (one wave per SIMD: the block reduction's waves
// do not take turns; 116-121k -> 124-125k GN it/s at C2, round 4) while the
// image fits 4 pixels per lane, else 512
constexpr int kTrkThreadsLo = 256, kTrkThreadsHi = 512;
constexpr int kTrkMaxBlocks = 256;
constexpr int kTrkShards = 8;
constexpr int kTrkGran = kNP / 3;  // 16-B granules per workgroup partial (3 sums + tag)
constexpr int kTrkSpins = 1 << 22;
// The per-iteration accumulation runs on pixel pairs (AccumPP /
// pixel_contrib2, as the backend's packed kernel; round 5). Measured and
// removed (DESIGN.md §4 Tracker): every workgroup running the top level
// itself, and no shard level.
constexpr int kTrkShBufs = 1;
struct TrackSync {
  uint32_t rec[32];  // the published record: 4 tagged 16-B granules (pose 0-7, status 8, cost 9-10 | tag)
  uint32_t shard_sum[kTrkShBufs][kTrkShards][kNP][4];  // level-1 sums (fp64), tagged 16-B granules {lo, hi, tag, 0}
};
static_assert(offsetof(TrackSync, rec) % 128 == 0, "the record granules share one line");
inline size_t track_sync_off() { return 128; }  // after TrackState (<= 128 B)
inline size_t track_part_off() { return track_sync_off() + sizeof(TrackSync); }
static_assert(sizeof(TrackState) <= 128, "TrackState must fit before the sync lines");
static_assert((128 + sizeof(TrackSync)) % 16 == 0, "the partial granules are 16-B aligned");

#ifdef M3S_TRK_STAMPS  // phase stamps of workgroups 0 and G - 1 (tools/trk_stamps.py)
__device__ int64_t g_trk_stamp[2][16][8];
#define M3S_TSTAMP(ph)                                                                     \
  if (t == 0 && (b == 0 || b == G - 1) && it < 16) g_trk_stamp[b == 0 ? 0 : 1][it][ph] = wall_clock64();
#else
#define M3S_TSTAMP(ph)
#endif
// M3S_TRK_SLEEP: s_sleep(1) per failed poll pass (0: spin; correct either
// way, the poll loads are poll_b128)
#ifndef M3S_TRK_SLEEP
#define M3S_TRK_SLEEP 1
#endif
__device__ __forceinline__ void trk_pause() {
#if M3S_TRK_SLEEP
  __builtin_amdgcn_s_sleep(1);
#endif
}
template <int MODE, int PPL, int TH>
__global__ void __launch_bounds__(TH) track_persistent_kernel(LinArgs A, int max_iters, TrackSync *sync) {
  const int G = (int)gridDim.x, b = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
  constexpr int NW = TH / 64;
  __shared__ float redf[NW][kNP];
  __shared__ double s_sum[kNP];
  // the iteration's record: pose (0-7), status (8: kTrackContinue /
  // kTrackConverged / kTrackFailed / 3 = barrier timeout), cost (9-10)
  __shared__ uint32_t pub_s[12];
  __shared__ __attribute__((aligned(16))) float blk_s[kNP];
  TrackState *st = A.track;
  const int64_t HW = A.HW;
  PixIn<MODE> in[PPL];
  float Xf[PPL][3];
  bool live[PPL];
#pragma unroll
  for (int s = 0; s < PPL; s++) {
    const int64_t p = ((int64_t)b * PPL + s) * TH + t;
    live[s] = p < HW;
    const int64_t pc = live[s] ? p : 0;
    in[s] = gather_pixel<MODE, true>(A, A.Xs, nullptr, pc, A.valid[pc] != 0, 0, A.Q[pc], 0.0f);
    Xf[s][0] = A.Xsrc[3 * pc], Xf[s][1] = A.Xsrc[3 * pc + 1], Xf[s][2] = A.Xsrc[3 * pc + 2];
  }
  Sim3f T = load_sim3(st->T_rel);
  const Sim3f Tk = load_sim3(st->T_WCk);
  int it = 0, status = kTrackContinue;
  // the record granules (lanes >= 4: offsets past the range, loads read zeros
  // and stores are dropped)
  const __amdgpu_buffer_rsrc_t Rrec = __builtin_amdgcn_make_buffer_rsrc(sync->rec, 0, 64, 0x00020000);
  const __amdgpu_buffer_rsrc_t Rsh = __builtin_amdgcn_make_buffer_rsrc(sync->shard_sum, 0, (int)sizeof(sync->shard_sum), 0x00020000);
  constexpr int kShFar = (int)sizeof(TrackSync::shard_sum);  // past the range: no access
  const __amdgpu_buffer_rsrc_t Rpart =
      __builtin_amdgcn_make_buffer_rsrc(A.partials, 0, kTrkMaxBlocks * kTrkGran * 16, 0x00020000);
  constexpr int kPartFar = kTrkMaxBlocks * kTrkGran * 16;
  for (; it < max_iters; it++) {
    M3S_TSTAMP(0)
    const Sim3Mat Tm = sim3_matrix(T);
    float v[kNP];
#pragma unroll
    for (int k = 0; k < kNP; k++) v[k] = 0.0f;
    {  // pixel pairs in the halves of float2 registers (the backend's packed
       // accumulation, with the cost sum); a lane's pixel past the image takes
       // a zero weight
      constexpr int NPL = PixIn<MODE>::kPlanes, SQK = MODE == 2 ? 1 : NPL - 1;
      AccumPP acc;
      acc.zero();
#pragma unroll
      for (int s = 0; s < PPL; s += 2) {
        const int s1 = s + 1 < PPL ? s + 1 : s;
        f32x2 in2[NPL], X2[3], Y2[3];
#pragma unroll
        for (int k = 0; k < NPL; k++) {
          const float lo = (k == SQK && !live[s]) ? 0.0f : in[s].v[k];
          const float hi = (k == SQK && (!live[s1] || s1 == s)) ? 0.0f : in[s1].v[k];
          in2[k] = f32x2{lo, hi};
        }
#pragma unroll
        for (int k = 0; k < 3; k++) X2[k] = f32x2{Xf[s][k], Xf[s1][k]};
        act2(Tm, X2, Y2);
        pixel_contrib2<MODE, NPL, true>(acc, A.P, in2, Y2);
      }
      acc.fold(v);
    }
    M3S_TSTAMP(1)
    {
      int idx;
      bool ok;
      const float x = xreduce36_trk(v, lane, idx, ok);
      if (ok) redf[wv][idx] = x;
    }
    __syncthreads();
    if (wv == 0) {
      // block partial -> LDS -> 12 tagged 16-B granules {3 sums | it + 1}
      // (write-through, no drain: the shard reducer polls them)
      if (lane < kNP) {
        float x = 0.0f;
#pragma unroll
        for (int w = 0; w < NW; w++) x += redf[w][lane];
        blk_s[lane] = x;
      }
      wave_lds_fence();
      {
        const int q = lane < kTrkGran ? 3 * lane : 0;
        const u32x4 w = {__float_as_uint(blk_s[q]), __float_as_uint(blk_s[q + 1]), __float_as_uint(blk_s[q + 2]),
                         (unsigned)(it + 1)};
        __builtin_amdgcn_raw_buffer_store_b128(w, Rpart, lane < kTrkGran ? (b * kTrkGran + lane) * 16 : kPartFar, 0, 16);
      }
      M3S_TSTAMP(2)
      const int shb = 0;  // the shard-sum buffer
      // level 1: workgroup s < 8 reduces shard s = {s, s + 8, ...}: lane j
      // polls member s + 8 j's granules, then the 36 sums are reduced across
      // the lanes in a fixed order (fp64)
      const int sh = b;
      const uint32_t n_top = (uint32_t)(G < kTrkShards ? G : kTrkShards);
      bool top_last = false;
      if (b < kTrkShards) {
        const int n_sh = (G - sh + kTrkShards - 1) / kTrkShards;
        u32x4 g[kTrkGran];
        int spins = 0;
        for (;;) {
#pragma unroll
          for (int k = 0; k < kTrkGran; k++)
            g[k] = poll_b128(Rpart, lane < n_sh ? ((sh + kTrkShards * lane) * kTrkGran + k) * 16 : kPartFar);
          bool ok = true;
#pragma unroll
          for (int k = 0; k < kTrkGran; k++) ok &= lane >= n_sh || g[k].w == (unsigned)(it + 1);
          if (__ballot(!ok) == 0) break;
          trk_pause();
          if (++spins > kTrkSpins) break;
        }
        double a[kNP];
#pragma unroll
        for (int k = 0; k < kTrkGran; k++) {
          a[3 * k] = (double)__uint_as_float(g[k].x);
          a[3 * k + 1] = (double)__uint_as_float(g[k].y);
          a[3 * k + 2] = (double)__uint_as_float(g[k].z);
        }
        // a timed-out shard publishes a NaN sum: the update fails (status 2)
        if (spins > kTrkSpins) a[0] = __builtin_nan("");
        int idx;
        bool ok;
        const double x = xreduce36_trk(a, lane, idx, ok);
        {
          const unsigned long long xb = (unsigned long long)__double_as_longlong(x);
          const u32x4 w = {(unsigned)(xb & 0xffffffffull), (unsigned)(xb >> 32), (unsigned)(it + 1), 0u};
          __builtin_amdgcn_raw_buffer_store_b128(w, Rsh, ok ? ((shb * kTrkShards + sh) * kNP + idx) * 16 : kShFar, 0, 16);
        }
        // level 2: workgroup 0 sums the shard sums in shard order as their
        // granules land
        top_last = sh == 0;
      }
      if (top_last) {
        M3S_TSTAMP(3)
        u32x4 g[kTrkShards];
        int spins = 0;
        for (;;) {
#pragma unroll
          for (int j = 0; j < kTrkShards; j++)
            g[j] = poll_b128(Rsh, (lane < kNP && j < (int)n_top) ? (j * kNP + lane) * 16 : kShFar);
          bool ok = true;
#pragma unroll
          for (int j = 0; j < kTrkShards; j++) ok &= lane >= kNP || j >= (int)n_top || g[j].z == (unsigned)(it + 1);
          if (__ballot(!ok) == 0) break;
          trk_pause();
          if (++spins > kTrkSpins) break;
        }
        if (lane < kNP) {
          double x = 0.0;
#pragma unroll
          for (int j = 0; j < kTrkShards; j++)
            x += j < (int)n_top ? __longlong_as_double((long long)(((unsigned long long)g[j].y << 32) | g[j].x)) : 0.0;
          s_sum[lane] = x;
        }
        const bool timed_out = spins > kTrkSpins;  // bounded wait: published as status 3
        wave_lds_fence();
        M3S_TSTAMP(4)
        if (lane == 0) {
          // the previous record's cost (inf first)
          double oc = it == 0 ? __builtin_inf()
                              : __longlong_as_double((long long)(((unsigned long long)pub_s[10] << 32) | pub_s[9]));
          Sim3f Tn = T;
          const int r = timed_out ? 3 : track_update(s_sum, Tn, oc, A.rel_error, A.delta_norm);
          M3S_TSTAMP(6)
          if (r != kTrackContinue && r != kTrackConverged) Tn = T;
          float rec[8];
          store_sim3(rec, Tn);
#pragma unroll
          for (int k = 0; k < 8; k++) pub_s[k] = __float_as_uint(rec[k]);
          const unsigned long long ob = (unsigned long long)__double_as_longlong(oc);
          pub_s[8] = (uint32_t)r, pub_s[9] = (uint32_t)(ob & 0xffffffffull), pub_s[10] = (uint32_t)(ob >> 32);
          pub_s[11] = 0;
        }
        wave_lds_fence();
        const int q = lane < 4 ? 3 * lane : 0;
        const u32x4 w = {pub_s[q], pub_s[q + 1], pub_s[q + 2], (unsigned)(it + 1)};
        __builtin_amdgcn_raw_buffer_store_b128(w, Rrec, lane * 16, 0, 16);
      } else {
        int spins = 0;
        u32x4 g;
        for (;;) {
          g = poll_b128(Rrec, lane * 16);
          if (__ballot(lane < 4 && g.w != (unsigned)(it + 1)) == 0) break;
          trk_pause();
          if (++spins > kTrkSpins) break;
        }
        M3S_TSTAMP(4)
        if (spins > kTrkSpins) {
          if (lane == 0) pub_s[8] = 3;
        } else if (lane < 4) {
          pub_s[3 * lane] = g.x, pub_s[3 * lane + 1] = g.y, pub_s[3 * lane + 2] = g.z;
        }
      }
    }
    M3S_TSTAMP(5)
    __syncthreads();
    status = (int)pub_s[8];
    if (status == 3 || status == kTrackFailed) break;
    T = load_sim3(reinterpret_cast<const float *>(pub_s));
    if (status == kTrackConverged) break;
  }
  if (b == 0 && t == 0) {  // outputs: the last successful pose, the iteration count, the status
    A.info[M3S_INFO_ITERS] = it < max_iters ? it + 1 : max_iters;
    if (status == kTrackFailed) A.info[M3S_INFO_SOLVE_FAIL] = 1;
    if (status == 3) A.info[M3S_INFO_SOLVE_FAIL] = 2;
    if (status == kTrackConverged) A.info[M3S_INFO_CONVERGED] = 1;
    store_sim3(st->T_rel, T);
    store_sim3(A.T_CkCf_out, T);
    store_sim3(A.T_WCf_out, compose(Tk, T));
  }
}

// pixels per lane of the persistent tracker (1, 2, 4) and its workgroup size
// (threads) so that the grid fits one workgroup per CU; 0: too large (one
// launch per iteration instead)
int track_ppl(int64_t HW, int &threads) {
  static int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return 0;
    return n;
  }();
  const int64_t G = std::min<int64_t>(cus, kTrkMaxBlocks);
  threads = kTrkThreadsLo;
  for (int ppl : {1, 2, 4})
    if (HW <= G * kTrkThreadsLo * ppl) return ppl;
  threads = kTrkThreadsHi;
  return HW <= G * kTrkThreadsHi * 4 ? 4 : 0;
}
// M3S_TRACK_PERSISTENT=0: one launch per iteration (A/B of the persistent kernel)
bool track_persistent_enabled() { return knob<K_track_persistent>() != 0; }

int track_impl(const m3s_track_args *a, int mode, void *stream) {
  if (!a || !a->Xf || !a->Xk || !a->Qk || !a->valid || !a->T_WCf || !a->T_WCk || !a->T_WCf_out ||
      !a->T_CkCf_out || !a->info || !a->workspace || a->HW < 1)
    return M3S_EINVAL;
  if (mode == M3S_MODE_CALIB && (!a->K || a->width < 1 || a->height < 1)) return M3S_EINVAL;
  if (a->workspace_bytes < m3s_track_workspace_size(a->HW)) return M3S_EINVAL;
  hipStream_t st = S(stream);
  ResidualParams P;
  P.inv_sig_a = (float)(1.0 / (double)a->sigma_a);
  P.inv_sig_b = (float)(1.0 / (double)a->sigma_b);
  P.C_thresh = P.Q_thresh = 0.0f;
  P.fx = P.fy = P.cx = P.cy = 0.0f;
  P.width = a->width;
  P.height = a->height;
  P.border = (float)a->pixel_border;
  P.z_eps = a->z_eps;
  P.huber_k = a->huber_k;
  int rc;
  if (mode == M3S_MODE_CALIB && (rc = read_K(a->K, P, st))) return rc;
  TrackState *ts = at<TrackState>(a->workspace, kTrackStateOff);
  TrackSync *sync = at<TrackSync>(a->workspace, track_sync_off());
  float *partials = at<float>(a->workspace, track_part_off());
  int th = kTrkThreadsLo;
  const int ppl = track_ppl(a->HW, th);
  const bool persistent = ppl > 0 && track_persistent_enabled();
  const int G = persistent ? (int)((a->HW + (int64_t)th * ppl - 1) / ((int64_t)th * ppl)) : 0;
  track_init_kernel<<<1, 256, 0, st>>>(a->T_WCf, a->T_WCk, ts, a->info, a->T_WCf_out, a->T_CkCf_out,
                                       reinterpret_cast<uint32_t *>(sync), (int)(sizeof(TrackSync) / 4),
                                       reinterpret_cast<u32x4 *>(partials), G * kTrkGran);
  if ((rc = launch_ok())) return rc;
  LinArgs L{};
  memset(&L, 0, sizeof L);
  L.T_rel = ts->T_rel;
  L.Xs = a->Xk;
  L.Xsrc = a->Xf;
  L.valid = a->valid;
  L.Q = a->Qk;
  L.stop = &ts->done;
  L.partials = partials;
  L.HW = a->HW;
  L.edge_begin = 0;
  L.chunks = chunks_for(a->HW, 1);
  L.chunk_pix = chunk_pixels(a->HW, L.chunks);
  L.P = P;
  L.Kd = nullptr;  // the tracker passes its intrinsics in P
  L.track = ts;  // one launch per iteration: the last chunk runs the solve
  L.info = a->info;
  L.T_WCf_out = a->T_WCf_out, L.T_CkCf_out = a->T_CkCf_out;
  L.rel_error = a->rel_error, L.delta_norm = a->delta_norm;
  const bool vec = (a->HW % 4 == 0) && vec_ok(a->Xf, 16) && vec_ok(a->Xk, 16) && vec_ok(a->Qk, 16) &&
                   vec_ok(a->valid, 4);
  // persistent: every iteration in one launch (one workgroup per CU)
  if (persistent) {
    if (a->max_iters < 1) return M3S_OK;
    if (mode == M3S_MODE_RAYS) {
      if (th == kTrkThreadsHi) track_persistent_kernel<M3S_MODE_RAYS, 4, kTrkThreadsHi><<<G, th, 0, st>>>(L, a->max_iters, sync);
      else if (ppl == 1) track_persistent_kernel<M3S_MODE_RAYS, 1, kTrkThreadsLo><<<G, th, 0, st>>>(L, a->max_iters, sync);
      else if (ppl == 2) track_persistent_kernel<M3S_MODE_RAYS, 2, kTrkThreadsLo><<<G, th, 0, st>>>(L, a->max_iters, sync);
      else track_persistent_kernel<M3S_MODE_RAYS, 4, kTrkThreadsLo><<<G, th, 0, st>>>(L, a->max_iters, sync);
    } else {
      if (th == kTrkThreadsHi) track_persistent_kernel<M3S_MODE_CALIB, 4, kTrkThreadsHi><<<G, th, 0, st>>>(L, a->max_iters, sync);
      else if (ppl == 1) track_persistent_kernel<M3S_MODE_CALIB, 1, kTrkThreadsLo><<<G, th, 0, st>>>(L, a->max_iters, sync);
      else if (ppl == 2) track_persistent_kernel<M3S_MODE_CALIB, 2, kTrkThreadsLo><<<G, th, 0, st>>>(L, a->max_iters, sync);
      else track_persistent_kernel<M3S_MODE_CALIB, 4, kTrkThreadsLo><<<G, th, 0, st>>>(L, a->max_iters, sync);
    }
    return launch_ok();
  }
  for (int it = 0; it < a->max_iters; it++) {
    if ((rc = dispatch_linearize<true>(mode, L, L.chunks, vec, 0, st))) return rc;
    if (a->sync_every > 0 && (it + 1) % a->sync_every == 0 && it + 1 < a->max_iters) {
      int32_t done = 0;
      if (hipMemcpyAsync(&done, &ts->done, sizeof done, hipMemcpyDeviceToHost, st) != hipSuccess)
        return M3S_ELAUNCH;
      if (hipStreamSynchronize(st) != hipSuccess) return M3S_ELAUNCH;
      if (done) break;
    }
  }
  return M3S_OK;
}

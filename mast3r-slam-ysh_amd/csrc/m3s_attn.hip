// m3s_attn.hip — MI355X (gfx950) fused attention core of MASt3R's blocks
// (include/m3s_attn.h): RoPE2D of q and k, scores, softmax and the product
// with v in one launch, flash style, on the exact fp32-input MFMA
// (v_mfma_f32_32x32x2_f32). The score matrix never leaves the registers.
//
// A workgroup owns 64 q rows of one (batch, head) and splits the kv range into
// G parts, two waves each: wave w takes the q rows 32 (w & 1) .. + 31 and part
// w >> 1; the parts of a q row are joined through LDS at the end. G = 4 (eight
// waves, two per SIMD, 140 KB of LDS) while the grid has at most one workgroup
// per compute unit, G = 2 (four waves, 74 KB: two workgroups per compute unit)
// beyond. Either way a SIMD holds two waves, and one wave's softmax and staging
// run under the other's products. Per kv tile of 32 rows:
//
//   S^T = K' Q'^T   A = K' from LDS (row = kv), B = Q' from registers (column =
//                   q row = lane & 31), 32 k-steps over D = 64. A lane then
//                   holds 16 of the 32 scores of ONE q row: register r of lane
//                   half h is kv row (r & 3) + 8 (r >> 2) + 4 h of the tile.
//   softmax         running maximum m and sum l per lane; the row maximum is 15
//                   in-lane fmaxf and one exchange with lane ^ 32. The two
//                   lane halves' partial sums meet once, after the last tile.
//   O^T = V^T P^T   sums over S^T's row index, so P goes from the score
//                   registers straight in as the B operand: k-step r pairs kv
//                   rows rho(r) and rho(r) + 4, and the A operand V^T[d = lane
//                   & 31 (+ 32)][kv] is read from exactly those rows of the V
//                   image (d on the lane: 32 consecutive banks per lane half).
//
// The k order of the first product is free as long as both operands agree:
// k-step 4 j + e of lane half h is channel 8 j + 4 h + e, so a lane's Q' and
// its K' fragments are whole 16-byte vectors, and the (u, v) channels of every
// RoPE pair (16 apart) sit in the same lane. Q' is rotated and multiplied by
// `scale` once, in registers. K is rotated as it is staged (four threads per kv
// row, eight pairs each), with (cos, sin) from a per-workgroup LDS table over
// (position 0 .. 63, frequency), filled by the same rope_angle that serves a
// position outside it; K and V tiles are double buffered in LDS and shared
// by the two waves of a part; the next tile's rows are fetched into registers
// under the current tile's products: one barrier per tile.
//
// The K image has 68-dword rows: the 16 lanes that a ds_read_b128 serves
// together then hit 16 different 16-byte slots. Rows past Nk are never read
// from memory: their K and V images are zero and their scores -inf. q rows past
// Nq are computed on zeros and not stored.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "m3s_attn.h"
#include "m3s_gn.h"
#include "m3s_rope_device.h"

namespace {

using m3s_rope::CosSin;
using m3s_rope::rope_angle;
using m3s_rope::rope_freq;
using m3s_rope::rope_rotate;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kD = 64;            // head dimension
constexpr int kQf = kD / 4;       // frequencies per axis
constexpr int kTile = 32;         // kv rows per MFMA tile
constexpr int kQRows = 64;        // q rows per workgroup
constexpr int kCUs = 256;         // compute units of an MI355X
constexpr int kKStride = kD + 4;  // dwords per row of the K image
constexpr int kVStride = kD;
constexpr int kTabPos = 64;       // positions 0 .. 63 take (cos, sin) from the workgroup's table

inline int launch_status() { return hipGetLastError() == hipSuccess ? M3S_OK : M3S_ELAUNCH; }

// four consecutive floats; `vec`: the address is 16-byte aligned
__device__ __forceinline__ float4 load4(const float *p, bool vec) {
  if (vec) return *reinterpret_cast<const float4 *>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ void store4(float *p, float4 x, bool vec) {
  if (vec) {
    *reinterpret_cast<float4 *>(p) = x;
  } else {
    p[0] = x.x, p[1] = x.y, p[2] = x.z, p[3] = x.w;
  }
}

// kv row of score register r in lane half h
__device__ __forceinline__ constexpr int score_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// kGroups: parts of the kv range, two waves (the 64 q rows) each
template <int kGroups>
__global__ void __launch_bounds__(128 * kGroups) attn_rope_kernel(m3s_attn_args A, int q_tiles, int vec_i) {
  constexpr int kThreads = 128 * kGroups;
  constexpr int kStageRows = kTile * kGroups;  // one kv tile per part
  __shared__ __attribute__((aligned(16))) float Ks[2][kStageRows * kKStride];
  __shared__ __attribute__((aligned(16))) float Vs[2][kStageRows * kVStride];
  __shared__ __attribute__((aligned(16))) float2 Tab[kTabPos * kQf];  // (cos, sin) of (position, frequency)
  const bool vec = vec_i != 0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5, qh = wave & 1, g = wave >> 1;
  int64_t blk = blockIdx.x;
  const int qt = (int)(blk % q_tiles);
  blk /= q_tiles;
  const int64_t h = blk % A.H, b = blk / A.H;
  const bool rot = A.qpos != nullptr;
  const int64_t T = (A.Nk + kTile - 1) / kTile;  // kv tiles
  const int64_t T0 = (T + kGroups - 1) / kGroups;  // part g takes the tiles [g T0, (g + 1) T0) below T

  // ---- the angle depends on (position, frequency index) only, not on the axis, the
  // token or the head: the workgroup evaluates rope_angle once per pair for the
  // positions 0 .. kTabPos - 1 (a few per thread) instead of 32 times per kv token.
  // A position outside the table goes through the same two functions directly, so
  // the values are the same bits either way.
  if (rot) {
    const int i = tid & (kQf - 1);
    const float fr = rope_freq(i, kQf, A.base, A.f0);
#pragma unroll
    for (int n = 0; n < kTabPos * kQf / kThreads; n++) {
      const int p = (tid >> 4) + (kThreads / kQf) * n;
      const CosSin cs = rope_angle(p, fr);
      Tab[p * kQf + i] = make_float2(cs.c, cs.s);
    }
  }
  __syncthreads();
  auto angle = [&](int64_t p, int i) -> CosSin {
    if ((uint64_t)p < (uint64_t)kTabPos) {
      const float2 t = Tab[(int)p * kQf + i];
      return CosSin{t.x, t.y};
    }
    return rope_angle(p, rope_freq(i, kQf, A.base, A.f0));
  };

  // ---- Q': this lane's q row, channels 8 j + 4 lh + e in qf[4 j + e]
  float qf[32];
  const int64_t qi = (int64_t)qt * kQRows + qh * 32 + li;
  const bool q_ok = qi < A.Nq;
#pragma unroll
  for (int i = 0; i < 32; i++) qf[i] = 0.f;
  if (q_ok) {
    const float *qp = static_cast<const float *>(A.q) + b * A.q_sb + qi * A.q_sn + h * kD + 4 * lh;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float4 x = load4(qp + 8 * j, vec);
      qf[4 * j] = x.x, qf[4 * j + 1] = x.y, qf[4 * j + 2] = x.z, qf[4 * j + 3] = x.w;
    }
    if (rot) {
      // j = 4 axis + jj holds u, j + 2 holds v, frequency index 8 jj + 4 lh + e
#pragma unroll
      for (int axis = 0; axis < 2; axis++) {
        const int64_t p = A.qpos[2 * (b * A.Nq + qi) + axis];
#pragma unroll
        for (int f = 0; f < 8; f++) {
          const int i = 8 * (f >> 2) + 4 * lh + (f & 3);
          rope_rotate(qf[16 * axis + f], qf[16 * axis + 8 + f], angle(p, i));
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 32; i++) qf[i] *= A.scale;

  // ---- staging: four threads per kv row. Thread part sc rotates the pairs
  // (axis = sc >> 1, i = 8 (sc & 1) .. + 7) of K and copies channels 16 sc .. + 15 of V
  const int srow = tid >> 2, sc = tid & 3, sg = srow >> 5, sr = srow & 31;
  const int saxis = sc >> 1, sd = 32 * saxis + 8 * (sc & 1);
  float4 rk[4], rv[4];  // rk[0..1]: u, rk[2..3]: v
  int64_t spos = 0;
  bool sok = false;

  auto fetch = [&](int64_t t) {
    const int64_t kv = (sg * T0 + t) * kTile + sr;
    sok = kv < A.Nk;
    if (sok) {
      const float *kp = static_cast<const float *>(A.k) + b * A.k_sb + kv * A.k_sn + h * kD + sd;
      const float *vp = static_cast<const float *>(A.v) + b * A.v_sb + kv * A.v_sn + h * kD + 16 * sc;
      rk[0] = load4(kp, vec), rk[1] = load4(kp + 4, vec);
      rk[2] = load4(kp + kQf, vec), rk[3] = load4(kp + kQf + 4, vec);
#pragma unroll
      for (int i = 0; i < 4; i++) rv[i] = load4(vp + 4 * i, vec);
      if (rot) spos = A.kpos[2 * (b * A.Nk + kv) + saxis];
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) rk[i] = rv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };

  auto stage = [&](int buf) {
    if (rot && sok) {
      float u[8] = {rk[0].x, rk[0].y, rk[0].z, rk[0].w, rk[1].x, rk[1].y, rk[1].z, rk[1].w};
      float v[8] = {rk[2].x, rk[2].y, rk[2].z, rk[2].w, rk[3].x, rk[3].y, rk[3].z, rk[3].w};
#pragma unroll
      for (int f = 0; f < 8; f++) rope_rotate(u[f], v[f], angle(spos, 8 * (sc & 1) + f));
      rk[0] = make_float4(u[0], u[1], u[2], u[3]), rk[1] = make_float4(u[4], u[5], u[6], u[7]);
      rk[2] = make_float4(v[0], v[1], v[2], v[3]), rk[3] = make_float4(v[4], v[5], v[6], v[7]);
    }
    float *kd = &Ks[buf][srow * kKStride + sd];
    *reinterpret_cast<float4 *>(kd) = rk[0];
    *reinterpret_cast<float4 *>(kd + 4) = rk[1];
    *reinterpret_cast<float4 *>(kd + kQf) = rk[2];
    *reinterpret_cast<float4 *>(kd + kQf + 4) = rk[3];
    float *vd = &Vs[buf][srow * kVStride + 16 * sc];
#pragma unroll
    for (int i = 0; i < 4; i++) *reinterpret_cast<float4 *>(vd + 4 * i) = rv[i];
  };

  // ---- the running softmax state of this lane's q row over this wave's part of kv
  f32x16 o0, o1;  // O^T: register r is channel score_row(r, lh) (+ 32 for o1)
#pragma unroll
  for (int r = 0; r < 16; r++) o0[r] = 0.f, o1[r] = 0.f;
  float m = -INFINITY, l = 0.f;  // l: this lane half's part of the sum

  fetch(0);
  stage(0);
  if (T0 > 1) fetch(1);
  __syncthreads();
  for (int64_t t = 0; t < T0; t++) {
    const int buf = (int)(t & 1);
    if (t + 1 < T0) {
      stage(buf ^ 1);  // last read in iteration t - 1, before its barrier
      if (t + 2 < T0) fetch(t + 2);
    }
    const int64_t nv = A.Nk - (g * T0 + t) * kTile;  // valid kv rows of this wave's tile
    if (nv > 0) {
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; r++) s[r] = 0.f;
      const float *kb = &Ks[buf][(g * 32 + li) * kKStride + 4 * lh];
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float4 kf = *reinterpret_cast<const float4 *>(kb + 8 * j);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[4 * j], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[4 * j + 1], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[4 * j + 2], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[4 * j + 3], s, 0, 0, 0);
      }
      if (nv < kTile) {
#pragma unroll
        for (int r = 0; r < 16; r++)
          if (score_row(r, lh) >= nv) s[r] = -INFINITY;
      }
      float mx = s[0];
#pragma unroll
      for (int r = 1; r < 16; r++) mx = fmaxf(mx, s[r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m, mx);  // finite: the tile has a valid row
      const float alpha = expf(m - m_new);
      m = m_new;
      l *= alpha;
#pragma unroll
      for (int r = 0; r < 16; r++) o0[r] *= alpha, o1[r] *= alpha;
      const float *vb = &Vs[buf][(g * 32 + 4 * lh) * kVStride + li];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const float p = expf(s[r] - m_new);
        l += p;
        const float *vr = vb + score_row(r, 0) * kVStride;
        o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[0], p, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32], p, o1, 0, 0, 0);
      }
    }
    __syncthreads();
  }
  l += __shfl_xor(l, 32, 64);

  // ---- join the kv parts (every K / V read is behind the loop's last barrier)
  float *join = &Ks[0][0];  // [part 1 ..][q half][34][64 lanes]: o0, o1, m, l
  static_assert((kGroups - 1) * 2 * 34 * 64 <= 2 * kStageRows * kKStride, "the join fits the K images");
  if (g > 0) {
    float *jp = join + ((g - 1) * 2 + qh) * 34 * 64 + lane;
#pragma unroll
    for (int r = 0; r < 16; r++) jp[r * 64] = o0[r], jp[(16 + r) * 64] = o1[r];
    jp[32 * 64] = m, jp[33 * 64] = l;
  }
  __syncthreads();
  if (g == 0 && q_ok) {
    // part 0 is never empty, so mm is finite; an empty part has m = -inf, l = 0, O = 0
    const float *jp = join + qh * 34 * 64 + lane;
    float mm = m;
#pragma unroll
    for (int p = 0; p < kGroups - 1; p++) mm = fmaxf(mm, jp[(p * 2 * 34 + 32) * 64]);
    float an[kGroups - 1];
    const float a0 = expf(m - mm);
    float L = l * a0;
#pragma unroll
    for (int p = 0; p < kGroups - 1; p++) {
      an[p] = expf(jp[(p * 2 * 34 + 32) * 64] - mm);
      L += jp[(p * 2 * 34 + 33) * 64] * an[p];
    }
    float *op = static_cast<float *>(A.out) + b * A.o_sb + qi * A.o_sn + h * kD + 4 * lh;
#pragma unroll
    for (int q4 = 0; q4 < 4; q4++) {
      float x0[4], x1[4];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int r = 4 * q4 + e;
        x0[e] = o0[r] * a0, x1[e] = o1[r] * a0;
#pragma unroll
        for (int p = 0; p < kGroups - 1; p++) {
          x0[e] += jp[(p * 2 * 34 + r) * 64] * an[p];
          x1[e] += jp[(p * 2 * 34 + 16 + r) * 64] * an[p];
        }
        x0[e] /= L, x1[e] /= L;
      }
      store4(op + 8 * q4, make_float4(x0[0], x0[1], x0[2], x0[3]), vec);
      store4(op + 32 + 8 * q4, make_float4(x1[0], x1[1], x1[2], x1[3]), vec);
    }
  }
}

inline bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" {

int m3s_attn_rope(const m3s_attn_args *a, void *stream) {
  if (!a || !a->q || !a->k || !a->v || !a->out) return M3S_EINVAL;
  if ((a->qpos == nullptr) != (a->kpos == nullptr)) return M3S_EINVAL;
  if (a->B <= 0 || a->Nq <= 0 || a->Nk <= 0 || a->H <= 0 || a->D != kD) return M3S_EINVAL;
  if (a->dtype != M3S_ROPE_F32) return M3S_EINVAL;
  // in 128 bits: any int64 sizes compare without overflow
  const __int128 row = (__int128)a->H * a->D;
  const struct {
    int64_t sb, sn, n;
  } views[4] = {{a->q_sb, a->q_sn, a->Nq}, {a->k_sb, a->k_sn, a->Nk}, {a->v_sb, a->v_sn, a->Nk}, {a->o_sb, a->o_sn, a->Nq}};
  for (const auto &v : views) {
    if (v.sn < row) return M3S_EINVAL;
    if (v.sb < (__int128)(v.n - 1) * v.sn + row) return M3S_EINVAL;
  }
  if ((__int128)a->B * a->H * a->Nq > INT32_MAX || (__int128)a->B * a->Nk > INT32_MAX) return M3S_EINVAL;
  if (!isfinite(a->base) || !(a->base > 0.0f) || !isfinite(a->f0) || !isfinite(a->scale)) return M3S_EINVAL;
  const int64_t q_tiles = (a->Nq + kQRows - 1) / kQRows;
  const int64_t blocks = a->B * a->H * q_tiles;  // <= B H Nq <= 2^31 - 1
  bool vec = aligned16(a->q) && aligned16(a->k) && aligned16(a->v) && aligned16(a->out);
  for (const auto &v : views) vec = vec && v.sb % 4 == 0 && v.sn % 4 == 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // Up to one workgroup per compute unit: eight waves, two per SIMD, so that one
  // wave's softmax and staging run under the other's products. Beyond that the
  // four-wave workgroups, whose LDS lets two share a compute unit, do the same
  // across workgroups and leave no second round of half-empty compute units.
  if (blocks <= kCUs)
    attn_rope_kernel<4><<<(unsigned)blocks, 128 * 4, 0, st>>>(*a, (int)q_tiles, vec ? 1 : 0);
  else
    attn_rope_kernel<2><<<(unsigned)blocks, 128 * 2, 0, st>>>(*a, (int)q_tiles, vec ? 1 : 0);
  return launch_status();
}

}  // extern "C"

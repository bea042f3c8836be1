// m3s_head.hip — MI355X (gfx950) tail of MASt3R's catmlp+dpt head
// (include/m3s_head.h): pixel_shuffle of the local-feature MLP, the cat with the
// DPT map, the channel-last permute, the 'exp' point and confidence maps, the
// descriptor normalisation, the downsample and the fp16 cast of the descriptors,
// in one launch from the two network outputs to the caller's X, C, D, Q slots.
//
// Two kernels, chosen on the host, that give bitwise the same values; both
// evaluate a pixel with the same three functions below, FMA contraction off.
//
// head_patch_kernel (P == 16, F == 24, ds == 1, aligned X and D). One workgroup
// of 256 threads owns one token, thread t its pixel (i, j) = (t / 16, t % 16). A
// token's feature row is (F + 1) * 256 contiguous floats and thread t reads
// row[c * 256 + t]: every wave load is 256 contiguous bytes with no staging; the
// four DPT channels are four 64-byte runs per wave load. The write side is what
// needs care: a pixel owns 24 contiguous descriptor channels, so a store from
// the lane that computed them is 96-byte-strided across the lanes (48-byte in
// fp16) and every store instruction touches 48 or more cache lines for 1 KiB of
// payload. Instead the workgroup lays D out in LDS as it lies in memory and
// stores 16 bytes per lane over contiguous bytes: an image row of the patch is
// 16 * 24 * 4 = 1,536 contiguous bytes, so a wave store is one 1-KiB run (or two
// runs where it crosses to the next image row). X goes the same way (192
// contiguous bytes per patch row); C and Q are one dword per lane in 64-byte
// runs and are stored directly. LDS image: a pixel's 24 floats at a stride of
// 28 dwords, so that the six 16-byte writes of the 8 lanes a ds_write_b128
// services together fall on 8 different 4-bank slots (28 l mod 32 = 0, 28, 24,
// 20, 16, 12, 8, 4); at the dense stride of 24 they would collide two by two.
// The image is fp32 for both output types: an fp16 D is rounded once, on the way
// out, from the same fp32 values. 31,744 bytes of LDS per workgroup.
//
// head_pixel_kernel: one thread per output pixel, element by element, any P, F,
// ds and alignment; it reads a pixel's descriptor twice (sum of squares, then the
// quotients) instead of holding F values in registers.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "m3s_gn.h"
#include "m3s_head.h"

#ifdef M3S_TEST_PATHS
// test build only: the patch kernel with every lane storing its own pixel's X and
// D straight from registers (the variant the LDS transpose is measured against,
// tools/head_time.py)
#define M3S_HEAD_DIRECT 2
#define M3S_HEAD_FLAGS (M3S_HEAD_GENERIC | M3S_HEAD_DIRECT)
#else
#define M3S_HEAD_FLAGS M3S_HEAD_GENERIC
#endif

namespace {

constexpr int kHeadThreads = 256;
constexpr int kPatch = 16;                // the patch kernel's P
constexpr int kDesc = 24;                 // and its F
constexpr int kDescStride = 28;           // dwords between two pixels of the LDS image of D
constexpr int64_t kMaxBlocks = 1 << 20;   // the blocks stride over the work beyond that

inline int launch_status() { return hipGetLastError() == hipSuccess ? M3S_OK : M3S_ELAUNCH; }

#pragma clang fp contract(off)

struct Xyz {
  float x, y, z;
};

// xyz / max(d, 1e-8) * expm1(d); a NaN d stays NaN through the max
__device__ __forceinline__ Xyz head_point(float px, float py, float pz) {
  const float d = sqrtf((px * px + py * py) + pz * pz);
  const float m = d < 1e-8f ? 1e-8f : d;
  const float e = expm1f(d);
  Xyz r;
  r.x = px / m * e;
  r.y = py / m * e;
  r.z = pz / m * e;
  return r;
}

// vmin + min(exp(raw), vmax - vmin); a NaN exp stays NaN through the min
__device__ __forceinline__ float head_conf(float raw, float vmin, float vmax) {
  const float e = expf(raw);
  const float cap = vmax - vmin;
  return vmin + (e > cap ? cap : e);
}

// the running sum of squares, in the order of the channels
__device__ __forceinline__ float head_sq_add(float s, float v) { return s + v * v; }

struct alignas(16) F32x4 {
  float e[4];
};
struct alignas(16) F16x8 {
  _Float16 e[8];
};

template <typename TD, bool kDirect>
__global__ void __launch_bounds__(kHeadThreads) head_patch_kernel(m3s_head_args A, int64_t n_tokens, int64_t S, int Wp) {
  __shared__ F32x4 sD[kHeadThreads * kDescStride / 4];
  __shared__ F32x4 sX[kHeadThreads * 3 / 4];
  float *const sXf = reinterpret_cast<float *>(sX);
  const int t = threadIdx.x;
  const int i = t >> 4, j = t & 15;
  const int64_t HW = A.H * A.W;
  TD *const Dout = static_cast<TD *>(A.D);
  for (int64_t tok = blockIdx.x; tok < n_tokens; tok += gridDim.x) {
    const int64_t b = tok / S;
    const int s = (int)(tok - b * S);
    const int ty = s / Wp, tx = s - ty * Wp;
    const int64_t pix0 = (int64_t)(ty * kPatch) * A.W + tx * kPatch;  // the patch's first pixel
    const int64_t pix = pix0 + (int64_t)i * A.W + j;
    const float *const row = A.feat + tok * ((kDesc + 1) * kPatch * kPatch) + t;
    float lf[kDesc];
#pragma unroll
    for (int c = 0; c < kDesc; c++) lf[c] = row[c * kPatch * kPatch];
    const float lq = row[kDesc * kPatch * kPatch];
    const float *const p = A.pts + b * 4 * HW + pix;
    const float px = p[0], py = p[HW], pz = p[2 * HW], pc = p[3 * HW];

    const Xyz xyz = head_point(px, py, pz);
    A.C[b * A.sbC + pix] = head_conf(pc, A.conf_vmin, A.conf_vmax);
    A.Q[b * A.sbQ + pix] = head_conf(lq, A.dconf_vmin, A.dconf_vmax);
    float sq = 0.0f;
#pragma unroll
    for (int c = 0; c < kDesc; c++) sq = head_sq_add(sq, lf[c]);
    const float n = sqrtf(sq);
#pragma unroll
    for (int c = 0; c < kDesc; c++) lf[c] = lf[c] / n;

    if constexpr (kDirect) {
      float *const xo = A.X + b * A.sbX + pix * 3;
      xo[0] = xyz.x, xo[1] = xyz.y, xo[2] = xyz.z;
      TD *const d = Dout + b * A.sbD + pix * kDesc;
      if (sizeof(TD) == 4) {
#pragma unroll
        for (int m = 0; m < kDesc / 4; m++) {
          F32x4 v;
#pragma unroll
          for (int k = 0; k < 4; k++) v.e[k] = lf[4 * m + k];
          reinterpret_cast<F32x4 *>(d)[m] = v;
        }
      } else {
#pragma unroll
        for (int m = 0; m < kDesc / 8; m++) {
          F16x8 v;
#pragma unroll
          for (int k = 0; k < 8; k++) v.e[k] = (_Float16)lf[8 * m + k];
          reinterpret_cast<F16x8 *>(d)[m] = v;
        }
      }
      continue;
    }

    sXf[t * 3 + 0] = xyz.x, sXf[t * 3 + 1] = xyz.y, sXf[t * 3 + 2] = xyz.z;
#pragma unroll
    for (int m = 0; m < kDesc / 4; m++) {
      F32x4 v;
#pragma unroll
      for (int k = 0; k < 4; k++) v.e[k] = lf[4 * m + k];
      sD[t * (kDescStride / 4) + m] = v;
    }
    __syncthreads();
    // X: a patch row is 16 * 3 floats = 12 vectors, 192 vectors in all
    if (t < kPatch * 12) {
      const int r = t / 12, q = t - r * 12;
      float *const xo = A.X + b * A.sbX + (pix0 + (int64_t)r * A.W) * 3;
      reinterpret_cast<F32x4 *>(xo)[q] = sX[t];
    }
    if (sizeof(TD) == 4) {
      // D f32: a pixel is 6 vectors, 1,536 in all, 6 per thread
#pragma unroll
      for (int m = 0; m < kDesc / 4; m++) {
        const int k = m * kHeadThreads + t;
        const int pp = k / 6, q = k - pp * 6;
        TD *const d = Dout + b * A.sbD + (pix0 + (int64_t)(pp >> 4) * A.W + (pp & 15)) * kDesc;
        reinterpret_cast<F32x4 *>(d)[q] = sD[pp * (kDescStride / 4) + q];
      }
    } else {
      // D f16: a pixel is 3 vectors of 8, 768 in all, 3 per thread
#pragma unroll
      for (int m = 0; m < kDesc / 8; m++) {
        const int k = m * kHeadThreads + t;
        const int pp = k / 3, q = k - pp * 3;
        const F32x4 lo = sD[pp * (kDescStride / 4) + 2 * q], hi = sD[pp * (kDescStride / 4) + 2 * q + 1];
        F16x8 v;
#pragma unroll
        for (int e = 0; e < 4; e++) v.e[e] = (_Float16)lo.e[e], v.e[4 + e] = (_Float16)hi.e[e];
        TD *const d = Dout + b * A.sbD + (pix0 + (int64_t)(pp >> 4) * A.W + (pp & 15)) * kDesc;
        reinterpret_cast<F16x8 *>(d)[q] = v;
      }
    }
    __syncthreads();  // the image is free for the next token
  }
}

template <typename TD>
__global__ void __launch_bounds__(kHeadThreads)
    head_pixel_kernel(m3s_head_args A, int64_t n_out, int64_t Ho, int64_t Wo) {
  const int64_t HW = A.H * A.W;
  const int P = (int)A.P, PP = P * P, F = (int)A.F;
  const int64_t Wp = A.W / A.P, S = (A.H / A.P) * Wp;
  TD *const Dout = static_cast<TD *>(A.D);
  for (int64_t o = (int64_t)blockIdx.x * kHeadThreads + threadIdx.x; o < n_out;
       o += (int64_t)gridDim.x * kHeadThreads) {
    const int64_t b = o / (Ho * Wo), po = o - b * (Ho * Wo);
    const int64_t yo = po / Wo, xo = po - yo * Wo;
    const int64_t y = yo * A.ds, x = xo * A.ds;
    const int64_t ty = y / P, tx = x / P;
    const int ij = (int)(y - ty * P) * P + (int)(x - tx * P);
    const float *const row = A.feat + (b * S + ty * Wp + tx) * ((int64_t)(F + 1) * PP) + ij;
    const float *const p = A.pts + b * 4 * HW + y * A.W + x;

    const Xyz xyz = head_point(p[0], p[HW], p[2 * HW]);
    float *const xout = A.X + b * A.sbX + po * 3;
    xout[0] = xyz.x, xout[1] = xyz.y, xout[2] = xyz.z;
    A.C[b * A.sbC + po] = head_conf(p[3 * HW], A.conf_vmin, A.conf_vmax);
    A.Q[b * A.sbQ + po] = head_conf(row[F * PP], A.dconf_vmin, A.dconf_vmax);
    float sq = 0.0f;
    for (int c = 0; c < F; c++) sq = head_sq_add(sq, row[c * PP]);
    const float n = sqrtf(sq);
    TD *const d = Dout + b * A.sbD + po * F;
    for (int c = 0; c < F; c++) d[c] = (TD)(row[c * PP] / n);
  }
}

#pragma clang fp contract(on)

template <typename TD>
int head_launch(const m3s_head_args &a, hipStream_t stream) {
  const int64_t Ho = (a.H + a.ds - 1) / a.ds, Wo = (a.W + a.ds - 1) / a.ds;
  const int64_t vec = 16 / (int64_t)sizeof(TD);
  const bool aligned = reinterpret_cast<uintptr_t>(a.X) % 16 == 0 && reinterpret_cast<uintptr_t>(a.D) % 16 == 0 &&
                       a.sbX % 4 == 0 && a.sbD % vec == 0;
  if (!(a.flags & M3S_HEAD_GENERIC) && a.P == kPatch && a.F == kDesc && a.ds == 1 && aligned) {
    const int64_t S = (a.H / kPatch) * (a.W / kPatch), n_tokens = a.B * S;
    const unsigned blocks = (unsigned)(n_tokens < kMaxBlocks ? n_tokens : kMaxBlocks);
#ifdef M3S_TEST_PATHS
    if (a.flags & M3S_HEAD_DIRECT)
      head_patch_kernel<TD, true><<<blocks, kHeadThreads, 0, stream>>>(a, n_tokens, S, (int)(a.W / kPatch));
    else
#endif
      head_patch_kernel<TD, false><<<blocks, kHeadThreads, 0, stream>>>(a, n_tokens, S, (int)(a.W / kPatch));
  } else {
    const int64_t n_out = a.B * Ho * Wo;
    const int64_t want = (n_out + kHeadThreads - 1) / kHeadThreads;
    const unsigned blocks = (unsigned)(want < kMaxBlocks ? want : kMaxBlocks);
    head_pixel_kernel<TD><<<blocks, kHeadThreads, 0, stream>>>(a, n_out, Ho, Wo);
  }
  return launch_status();
}

// vmin finite, vmax >= vmin (which a NaN vmax is not)
inline bool head_mode_ok(float vmin, float vmax) { return isfinite(vmin) && vmax >= vmin; }

}  // namespace

extern "C" {

int m3s_head_postprocess(const m3s_head_args *a, void *stream) {
  if (!a || !a->pts || !a->feat || !a->X || !a->C || !a->D || !a->Q) return M3S_EINVAL;
  if (a->B <= 0 || a->H <= 0 || a->W <= 0 || a->P <= 0 || a->F <= 0 || a->ds <= 0) return M3S_EINVAL;
  if (a->H % a->P != 0 || a->W % a->P != 0) return M3S_EINVAL;
  // in 128 bits: any int64 sizes compare without overflow
  if ((__int128)a->B * a->H > INT32_MAX || (__int128)a->B * a->H * a->W > INT32_MAX) return M3S_EINVAL;
  if (a->F >= INT32_MAX || ((__int128)a->F + 1) * a->P * a->P > INT32_MAX) return M3S_EINVAL;
  const int64_t Ho = (a->H + a->ds - 1) / a->ds, Wo = (a->W + a->ds - 1) / a->ds;
  const __int128 img = (__int128)Ho * Wo;
  if (a->sbX < img * 3 || a->sbC < img || a->sbD < img * a->F || a->sbQ < img) return M3S_EINVAL;
  if (!head_mode_ok(a->conf_vmin, a->conf_vmax) || !head_mode_ok(a->dconf_vmin, a->dconf_vmax)) return M3S_EINVAL;
  if (a->flags & ~M3S_HEAD_FLAGS) return M3S_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (a->desc_dtype) {
    case M3S_HEAD_F32: return head_launch<float>(*a, st);
    case M3S_HEAD_F16: return head_launch<_Float16>(*a, st);
    default: return M3S_EINVAL;
  }
}

}  // extern "C"

// m3s_dpt.hip — MI355X (gfx950) tail of MASt3R's DPT head (include/m3s_dpt.h):
// bilinear x2 upsampling (align_corners), the 3x3 convolution 128 -> 128, ReLU
// and the 1x1 convolution 128 -> Cout in one launch, as an implicit GEMM on
// the exact fp32-input MFMA (v_mfma_f32_32x32x2_f32). Neither the upsampled
// image nor the 128-channel map reaches memory.
//
// A workgroup of four waves owns kTileH x kTileW = 8 x 32 output pixels of one
// image and first copies the low-resolution source pixels they interpolate
// from, halo included (at most 7 x 19 pixels x 128 channels, 68 KB), into LDS;
// two workgroups share a compute unit, so a SIMD holds two waves and one wave's
// operand forming runs under the other's products. Wave w takes the tile's rows
// 2 w and 2 w + 1: two pixel blocks of 32 (one row each) x four channel blocks
// of 32, eight 32 x 32 accumulators.
//
// The product is the swapped one, mid^T = W1 U^T (DESIGN §4 'Attention'): A is
// the weight (row = mid channel = lane & 31 of a channel block), B the
// upsampled pixel (column = pixel = lane & 31). A lane then holds 64 of the 128
// mid channels of ONE pixel per pixel block: register r of channel block cb in
// lane half h is channel 32 cb + (r & 3) + 8 (r >> 2) + 4 h, so bias, ReLU and
// the 1x1 convolution are an fmaf chain in the lane and one exchange with lane
// ^ 32.
//
// K = 9 taps x 128 channels runs tap by tap, and within a tap in k-steps of two
// channels, channel 2 s + h in lane half h. The interpolation's four LDS
// offsets and four lambdas of a (pixel, tap) are formed once per tap; per
// k-step a B value is four LDS reads and seven rounded operations (contraction
// off) and a select for the zero padding. The A values of a k-step are one
// 16-byte LDS read: m3s_dpt_tail_pack lays w1 out as [tap][s][lane][cb], a
// chunk of four k-steps is 4 KB, one 16-byte global load per thread, double
// buffered in LDS under the products: one barrier per chunk of 32 MFMAs a wave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "m3s_dpt.h"
#include "m3s_gn.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kC = M3S_DPT_CH;         // Cin = Cmid
constexpr int kTileH = M3S_DPT_TILE_H;
constexpr int kTileW = M3S_DPT_TILE_W;
constexpr int kThreads = 256;          // four waves, two tile rows each
// source pixels under kTileH + 2 rows / kTileW + 2 columns of the upsampled image:
// the ratio is below 1/2, so floor(r b) - floor(r a) <= (b - a) / 2 rounded up to
// the next integer (fp32 rounding of r y is far below 1/2 up to M3S_DPT_MAX_SIDE),
// plus the row / column of y1 / x1
constexpr int kSrcH = (kTileH + 1) / 2 + 1 + 1 + 1;  // 7
constexpr int kSrcW = (kTileW + 1) / 2 + 1 + 1 + 1;  // 19
constexpr int kChStride = kSrcH * kSrcW;              // 133 dwords: odd
constexpr int kSteps = kC / 2;                        // k-steps per tap
constexpr int kChunkSteps = 4;                        // k-steps per staged weight chunk
constexpr int kChunks = 9 * kSteps / kChunkSteps;     // 144
constexpr int kChunksPerTap = kSteps / kChunkSteps;   // 16
constexpr int kW1Floats = 9 * kSteps * 64 * 4;        // [tap][s][lane][cb]
constexpr int kOffB1 = kW1Floats, kOffW2 = kOffB1 + kC, kOffB2 = kOffW2 + M3S_DPT_MAX_COUT * kC;
constexpr int kPackedFloats = kOffB2 + M3S_DPT_MAX_COUT;
static_assert(kThreads == kChunkSteps * 64, "one 16-byte load per thread stages a chunk");
static_assert(kTileH == 2 * (kThreads / 64) && kTileW == 32, "a wave owns two rows of 32 pixels");
static_assert(kPackedFloats % 4 == 0, "the packed size is a multiple of 16 bytes");

inline int launch_status() { return hipGetLastError() == hipSuccess ? M3S_OK : M3S_ELAUNCH; }

// mid channel of accumulator register r in lane half h (within a channel block)
__device__ __forceinline__ constexpr int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

struct Lerp {  // source index and lambdas of one coordinate (m3s_dpt.h)
  int i0, i1;
  float l0, l1;
};

#pragma clang fp contract(off)
__device__ __forceinline__ Lerp lerp_of(int y, float ratio, int n) {
  const float r = ratio * (float)y;
  int i0 = (int)r;
  i0 = i0 < n - 1 ? i0 : n - 1;  // never taken for y < 2 n: keeps every index in the image
  const float l1 = r - (float)i0;
  return Lerp{i0, i0 + (i0 < n - 1 ? 1 : 0), 1.0f - l1, l1};
}

__device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, float lh0, float lh1, float lw0,
                                        float lw1) {
  const float a = lw0 * v00, b = lw1 * v01, c = lw0 * v10, d = lw1 * v11;
  const float top = a + b, bot = c + d;
  const float t = lh0 * top, s = lh1 * bot;
  return t + s;
}
#pragma clang fp contract(on)

struct TailArgs {
  const float *x;
  const float *packed;
  float *out;
  int64_t x_sb, out_sb;
  int Hi, Wi, Cout, tiles_x, tiles_y;
  float rh, rw;
};

__global__ void __launch_bounds__(kThreads, 2) dpt_tail_kernel(TailArgs A) {
  __shared__ __attribute__((aligned(16))) float Src[kC * kChStride];        // [ci][row][column]
  __shared__ __attribute__((aligned(16))) float4 Ws[2][kChunkSteps * 64];  // [buffer][k-step][lane] -> cb 0..3
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int Hi = A.Hi, Wi = A.Wi, Ho = 2 * Hi, Wo = 2 * Wi;
  int blk = blockIdx.x;
  const int tx = blk % A.tiles_x;
  blk /= A.tiles_x;
  const int ty = blk % A.tiles_y, b = blk / A.tiles_y;
  const int oy0 = ty * kTileH, ox0 = tx * kTileW;

  // ---- the source tile: rows sy_lo .. + kSrcH - 1, columns sx_lo .. + kSrcW - 1
  const int sy_lo = lerp_of(oy0 > 0 ? oy0 - 1 : 0, A.rh, Hi).i0;
  const int sx_lo = lerp_of(ox0 > 0 ? ox0 - 1 : 0, A.rw, Wi).i0;
  {
    // kBatch independent loads in flight per thread. The addresses are clamped into the
    // image (and into the tile for the last, partial batch): a cell past the image holds a
    // copy of the edge pixel, and no pixel interpolates from it (y1 <= Hi - 1, x1 <= Wi - 1)
    const float *xb = A.x + (int64_t)b * A.x_sb;
    constexpr int kN = kC * kChStride, kBatch = 16;
    for (int base = 0; base < kN; base += kBatch * kThreads) {
      float v[kBatch];
#pragma unroll
      for (int i = 0; i < kBatch; i++) {
        const int e = min(base + i * kThreads + tid, kN - 1);
        const int ci = e / kChStride, rem = e - ci * kChStride;
        const int r = rem / kSrcW, c = rem - r * kSrcW;
        const int gy = sy_lo + r, gx = sx_lo + c;
        v[i] = xb[(ci * Hi + min(gy, Hi - 1)) * Wi + min(gx, Wi - 1)];  // < 128 Hi Wi <= 2^31 - 1
      }
#pragma unroll
      for (int i = 0; i < kBatch; i++) {
        const int e = base + i * kThreads + tid;
        if (e < kN) Src[e] = v[i];
      }
    }
  }

  // ---- weight chunks: thread tid moves the 16 bytes of (k-step tid >> 6, lane tid & 63)
  const float4 *wp = reinterpret_cast<const float4 *>(A.packed) + tid;
  float4 rw4 = wp[0];
  Ws[0][tid] = rw4;
  rw4 = wp[kThreads];
  __syncthreads();

  f32x16 acc[2][4];
#pragma unroll
  for (int p = 0; p < 2; p++)
#pragma unroll
    for (int cb = 0; cb < 4; cb++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[p][cb][r] = 0.f;

  const int oy[2] = {oy0 + 2 * wave, oy0 + 2 * wave + 1};
  const int ox = ox0 + li;
  int q = 0;  // chunk
  for (int tap = 0; tap < 9; tap++) {
    const int dy = tap / 3 - 1, dx = tap - 3 * (tap / 3) - 1;
    // the column is the same for both pixel blocks
    const int ux = ox + dx;
    const bool okx = ux >= 0 && ux < Wo;
    const Lerp X = lerp_of(ux < 0 ? 0 : (ux < Wo ? ux : Wo - 1), A.rw, Wi);
    const int c0 = min(max(X.i0 - sx_lo, 0), kSrcW - 1), c1 = min(max(X.i1 - sx_lo, 0), kSrcW - 1);
    int o0[2], o1[2];  // dword offsets of the rows y0, y1 in channel 0 (+ this lane half's channel)
    float lh0[2], lh1[2];
    bool ok[2];
#pragma unroll
    for (int p = 0; p < 2; p++) {
      const int uy = oy[p] + dy;
      ok[p] = okx && uy >= 0 && uy < Ho;
      const Lerp Y = lerp_of(uy < 0 ? 0 : (uy < Ho ? uy : Ho - 1), A.rh, Hi);
      const int r0 = min(max(Y.i0 - sy_lo, 0), kSrcH - 1), r1 = min(max(Y.i1 - sy_lo, 0), kSrcH - 1);
      o0[p] = r0 * kSrcW + lh * kChStride, o1[p] = r1 * kSrcW + lh * kChStride;
      lh0[p] = Y.l0, lh1[p] = Y.l1;
    }
    for (int j = 0; j < kChunksPerTap; j++, q++) {
      const int buf = q & 1;
      if (q + 1 < kChunks) {
        Ws[buf ^ 1][tid] = rw4;  // last read in iteration q - 1, before its barrier
        if (q + 2 < kChunks) rw4 = wp[(q + 2) * kThreads];
      }
      const float *sc = Src + (j * kChunkSteps * 2) * kChStride;
#pragma unroll
      for (int kk = 0; kk < kChunkSteps; kk++) {
        const float4 w = Ws[buf][kk * 64 + lane];
        const float *s = sc + kk * 2 * kChStride;
        float u[2];
#pragma unroll
        for (int p = 0; p < 2; p++) {
          const float v = bilerp(s[o0[p] + c0], s[o0[p] + c1], s[o1[p] + c0], s[o1[p] + c1], lh0[p], lh1[p], X.l0, X.l1);
          u[p] = ok[p] ? v : 0.f;
        }
#pragma unroll
        for (int p = 0; p < 2; p++) {
          acc[p][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, u[p], acc[p][0], 0, 0, 0);
          acc[p][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, u[p], acc[p][1], 0, 0, 0);
          acc[p][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, u[p], acc[p][2], 0, 0, 0);
          acc[p][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, u[p], acc[p][3], 0, 0, 0);
        }
      }
      __syncthreads();
    }
  }

  // ---- bias, ReLU and the 1x1 convolution on the accumulators: this lane's 64
  // channels in the order (cb, r), then the other lane half's sum
  const float *b1 = A.packed + kOffB1, *w2 = A.packed + kOffW2, *b2 = A.packed + kOffB2;
#pragma unroll
  for (int p = 0; p < 2; p++) {
    float sum[M3S_DPT_MAX_COUT] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cb = 0; cb < 4; cb++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int c = 32 * cb + acc_row(r, 0) + 4 * lh;
        const float v = acc[p][cb][r] + b1[c];
        const float m = v < 0.f ? 0.f : v;  // a NaN stays
#pragma unroll
        for (int o = 0; o < M3S_DPT_MAX_COUT; o++) sum[o] = fmaf(w2[o * kC + c], m, sum[o]);
      }
#pragma unroll
    for (int o = 0; o < M3S_DPT_MAX_COUT; o++) {
      const float other = __shfl_xor(sum[o], 32, 64);
      const float lo = lh ? other : sum[o], hi = lh ? sum[o] : other;
      sum[o] = b2[o] + (lo + hi);
    }
    if (lh == 0 && oy[p] < Ho && ox < Wo) {
      float *op = A.out + (int64_t)b * A.out_sb + (int64_t)oy[p] * Wo + ox;
      for (int o = 0; o < A.Cout; o++) op[(int64_t)o * Ho * Wo] = sum[o];
    }
  }
}

struct PackArgs {
  const float *w1, *b1, *w2, *b2;
  float *packed;
  int Cout;
};

__global__ void __launch_bounds__(256) dpt_pack_kernel(PackArgs P) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= kPackedFloats) return;
  float v;
  if (e < kW1Floats) {  // [tap][s][lane][cb] <- w1[c = 32 cb + (lane & 31)][ci = 2 s + (lane >> 5)][tap]
    const int cb = e & 3, lane = (e >> 2) & 63, s = (e >> 8) & (kSteps - 1), tap = e >> 14;
    const int c = 32 * cb + (lane & 31), ci = 2 * s + (lane >> 5);
    v = P.w1[(c * kC + ci) * 9 + tap];
  } else if (e < kOffW2) {
    v = P.b1[e - kOffB1];
  } else if (e < kOffB2) {  // rows past Cout are zero
    const int o = (e - kOffW2) / kC;
    v = o < P.Cout ? P.w2[e - kOffW2] : 0.f;
  } else {
    v = e - kOffB2 < P.Cout ? P.b2[e - kOffB2] : 0.f;
  }
  P.packed[e] = v;
}
static_assert(kSteps == 64 && kW1Floats == 9 << 14, "the pack kernel's shifts");

inline bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" {

size_t m3s_dpt_tail_packed_size(int64_t Cout) {
  return Cout >= 1 && Cout <= M3S_DPT_MAX_COUT ? sizeof(float) * kPackedFloats : 0;
}

int m3s_dpt_tail_pack(const float *w1, const float *b1, const float *w2, const float *b2, int64_t Cout, void *packed,
                      void *stream) {
  if (!w1 || !b1 || !w2 || !b2 || !packed) return M3S_EINVAL;
  if (Cout < 1 || Cout > M3S_DPT_MAX_COUT || !aligned16(packed)) return M3S_EINVAL;
  const PackArgs P{w1, b1, w2, b2, static_cast<float *>(packed), (int)Cout};
  dpt_pack_kernel<<<(kPackedFloats + 255) / 256, 256, 0, static_cast<hipStream_t>(stream)>>>(P);
  return launch_status();
}

int m3s_dpt_tail(const m3s_dpt_tail_args *a, void *stream) {
  if (!a || !a->x || !a->packed || !a->out) return M3S_EINVAL;
  if (a->B <= 0 || a->Hi <= 0 || a->Wi <= 0 || a->Cout <= 0 || a->Cout > M3S_DPT_MAX_COUT) return M3S_EINVAL;
  if (a->Hi > M3S_DPT_MAX_SIDE || a->Wi > M3S_DPT_MAX_SIDE) return M3S_EINVAL;
  if (a->flags != 0 || !aligned16(a->packed)) return M3S_EINVAL;
  // in 128 bits: any int64 sizes compare without overflow
  const __int128 in_img = (__int128)kC * a->Hi * a->Wi, out_img = (__int128)a->Cout * 4 * a->Hi * a->Wi;
  if (a->x_sb < in_img || a->out_sb < out_img) return M3S_EINVAL;
  if (a->B * in_img > INT32_MAX || a->B * out_img > INT32_MAX) return M3S_EINVAL;
  const int Hi = (int)a->Hi, Wi = (int)a->Wi, Ho = 2 * Hi, Wo = 2 * Wi;
  TailArgs A;
  A.x = a->x, A.packed = static_cast<const float *>(a->packed), A.out = a->out;
  A.x_sb = a->x_sb, A.out_sb = a->out_sb;
  A.Hi = Hi, A.Wi = Wi, A.Cout = (int)a->Cout;
  A.tiles_x = (Wo + kTileW - 1) / kTileW, A.tiles_y = (Ho + kTileH - 1) / kTileH;
  A.rh = (float)(Hi - 1) / (float)(Ho - 1), A.rw = (float)(Wi - 1) / (float)(Wo - 1);  // Ho, Wo >= 2
  const int64_t blocks = a->B * A.tiles_x * A.tiles_y;  // <= B Ho Wo <= 2^31 - 1
  dpt_tail_kernel<<<(unsigned)blocks, kThreads, 0, static_cast<hipStream_t>(stream)>>>(A);
  return launch_status();
}

}  // extern "C"

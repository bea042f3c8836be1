// m3s_rope.hip — MI355X (gfx950) 2-D rotary position embedding of MASt3R's
// attention (include/m3s_rope.h), in place on the q or k slice of a qkv buffer.
//
// One wave owns one token. The angles of a token depend on its (y, x) and the
// frequency index only, not on the head, so a lane evaluates its few (cos, sin)
// pairs once per token and then walks the heads: 2 Q sincosf per token against
// H * D rotated elements (32 against 1024 at MASt3R's shapes). No table, so no
// maximum position and no host read to size one. No LDS, no workspace.
//
// Two kernels, chosen on the host, that give bitwise the same values: rows as
// 16-byte vectors (a lane owns one axis and k = 16 / sizeof(T) consecutive
// frequencies: two loads, 2k rotations, two stores per head) and an
// element-wise one for everything the vector kernel cannot take (k does not
// divide Q, a head wider than a wave's 64 lanes, a misaligned base or stride).
// Both evaluate theta and the rotation by the two functions of
// m3s_rope_device.h (shared with m3s_attn.hip), with FMA contraction off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "m3s_gn.h"
#include "m3s_rope.h"
#include "m3s_rope_device.h"

namespace {

using m3s_rope::CosSin;
using m3s_rope::rope_angle;
using m3s_rope::rope_freq;
using m3s_rope::rope_rotate;

constexpr int kWave = 64;
constexpr int kRopeThreads = 256;
constexpr int kWavesPerBlock = kRopeThreads / kWave;
constexpr int64_t kMaxBlocks = 1 << 20;  // the waves stride over the tokens beyond that

inline int launch_status() { return hipGetLastError() == hipSuccess ? M3S_OK : M3S_ELAUNCH; }

#pragma clang fp contract(off)

// lanes_per_head = 2 Q / k <= 64; heads_per_pass = 64 / lanes_per_head; the
// lanes beyond heads_per_pass * lanes_per_head have nothing to do.
template <typename T>
__global__ void __launch_bounds__(kRopeThreads)
    rope_vec_kernel(m3s_rope_args A, int64_t n_tokens, int Q, int lanes_per_head, int heads_per_pass) {
  constexpr int K = 16 / (int)sizeof(T);
  struct alignas(16) Vec {
    T e[K];
  };
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int head0 = lane / lanes_per_head;
  if (head0 >= heads_per_pass) return;
  const int slot = lane - head0 * lanes_per_head;
  const int per_axis = lanes_per_head >> 1;  // Q / K
  const int axis = slot >= per_axis ? 1 : 0;
  const int i0 = (slot - axis * per_axis) * K;
  float freq[K];
#pragma unroll
  for (int k = 0; k < K; k++) freq[k] = rope_freq(i0 + k, Q, A.base, A.f0);
  T *const tokens = static_cast<T *>(A.tokens) + (axis * 2 * Q + i0);
  for (int64_t t = (int64_t)blockIdx.x * kWavesPerBlock + wave; t < n_tokens;
       t += (int64_t)gridDim.x * kWavesPerBlock) {
    const int64_t b = t / A.N, n = t - b * A.N;
    const int64_t p = A.pos[2 * t + axis];
    CosSin cs[K];
#pragma unroll
    for (int k = 0; k < K; k++) cs[k] = rope_angle(p, freq[k]);
    T *const row = tokens + b * A.stride_b + n * A.stride_n;
    for (int64_t h = head0; h < A.H; h += heads_per_pass) {
      Vec *const pu = reinterpret_cast<Vec *>(row + h * A.D);
      Vec *const pv = reinterpret_cast<Vec *>(row + h * A.D + Q);
      Vec u = *pu, v = *pv;
#pragma unroll
      for (int k = 0; k < K; k++) rope_rotate(u.e[k], v.e[k], cs[k]);
      *pu = u;
      *pv = v;
    }
  }
}

// Any D % 4 == 0, any alignment. A lane owns (axis, frequency) pairs j = axis *
// Q + i; with fewer than 64 pairs the wave's lanes form 64 / (2 Q) groups that
// share out the heads.
template <typename T>
__global__ void __launch_bounds__(kRopeThreads) rope_elem_kernel(m3s_rope_args A, int64_t n_tokens, int Q) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int pairs = 2 * Q;
  const int width = pairs < kWave ? pairs : kWave;
  const int groups = kWave / width;
  const int group = lane / width;
  if (group >= groups) return;
  T *const tokens = static_cast<T *>(A.tokens);
  for (int64_t t = (int64_t)blockIdx.x * kWavesPerBlock + wave; t < n_tokens;
       t += (int64_t)gridDim.x * kWavesPerBlock) {
    const int64_t b = t / A.N, n = t - b * A.N;
    T *const row = tokens + b * A.stride_b + n * A.stride_n;
    for (int j = lane - group * width; j < pairs; j += width) {
      const int axis = j >= Q ? 1 : 0;
      const int i = j - axis * Q;
      const CosSin cs = rope_angle(A.pos[2 * t + axis], rope_freq(i, Q, A.base, A.f0));
      T *const col = row + (axis * 2 * Q + i);
      for (int64_t h = group; h < A.H; h += groups) {
        T u = col[h * A.D], v = col[h * A.D + Q];
        rope_rotate(u, v, cs);
        col[h * A.D] = u;
        col[h * A.D + Q] = v;
      }
    }
  }
}

#pragma clang fp contract(on)

template <typename T>
int rope_launch(const m3s_rope_args &a, hipStream_t stream) {
  constexpr int64_t K = 16 / (int64_t)sizeof(T);
  const int64_t Q = a.D / 4;
  const int64_t n_tokens = a.B * a.N;
  const int64_t want = (n_tokens + kWavesPerBlock - 1) / kWavesPerBlock;
  const unsigned blocks = (unsigned)(want < kMaxBlocks ? want : kMaxBlocks);
  const int64_t lanes_per_head = 2 * Q / K;
  const bool aligned = reinterpret_cast<uintptr_t>(a.tokens) % 16 == 0 && a.stride_b % K == 0 && a.stride_n % K == 0;
  if (Q % K == 0 && lanes_per_head <= kWave && aligned)
    rope_vec_kernel<T><<<blocks, kRopeThreads, 0, stream>>>(a, n_tokens, (int)Q, (int)lanes_per_head,
                                                            (int)(kWave / lanes_per_head));
  else
    rope_elem_kernel<T><<<blocks, kRopeThreads, 0, stream>>>(a, n_tokens, (int)Q);
  return launch_status();
}

}  // namespace

extern "C" {

int m3s_rope_2d(const m3s_rope_args *a, void *stream) {
  if (!a || !a->tokens || !a->pos) return M3S_EINVAL;
  if (a->B <= 0 || a->N <= 0 || a->H <= 0 || a->D <= 0 || a->D % 4 != 0) return M3S_EINVAL;
  // in 128 bits: any int64 sizes compare without overflow
  const __int128 row = (__int128)a->H * a->D;
  if (a->stride_n < row) return M3S_EINVAL;
  if (a->stride_b < (__int128)(a->N - 1) * a->stride_n + row) return M3S_EINVAL;
  if ((__int128)a->B * a->N > INT32_MAX) return M3S_EINVAL;
  // the kernels index a head row with int: 4 Q = D has to fit
  if (a->D > INT32_MAX / 2) return M3S_EINVAL;
  if (!isfinite(a->base) || !(a->base > 0.0f) || !isfinite(a->f0)) return M3S_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (a->dtype) {
    case M3S_ROPE_F32: return rope_launch<float>(*a, st);
    case M3S_ROPE_F16: return rope_launch<_Float16>(*a, st);
    case M3S_ROPE_BF16: return rope_launch<__bf16>(*a, st);
    default: return M3S_EINVAL;
  }
}

}  // extern "C"

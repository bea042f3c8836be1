// m3s_rope_device.h — the two device functions every RoPE2D evaluation of this
// library goes through (include/m3s_rope.h states the function): theta and the
// rotation. m3s_rope.hip (in place on q or k) and m3s_attn.hip (fused into the
// attention) include this header, so the rotation is bitwise the same in both.
// FMA contraction is off inside each body: the products and the sum round
// separately, whatever the including file's setting.
#ifndef M3S_ROPE_DEVICE_H
#define M3S_ROPE_DEVICE_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace m3s_rope {

// f0 / base^(i/Q): a rounded i/Q, powf, one division
__device__ __forceinline__ float rope_freq(int i, int Q, float base, float f0) {
#pragma clang fp contract(off)
  const float x = (float)i / (float)Q;
  return f0 / powf(base, x);
}

struct CosSin {
  float c, s;
};

// one product, then the accurate sincosf (full argument reduction)
__device__ __forceinline__ CosSin rope_angle(int64_t p, float freq) {
#pragma clang fp contract(off)
  const float theta = (float)p * freq;
  CosSin r;
  sincosf(theta, &r.s, &r.c);
  return r;
}

template <typename T>
__device__ __forceinline__ void rope_rotate(T &u, T &v, CosSin t) {
#pragma clang fp contract(off)
  const float uf = (float)u, vf = (float)v;
  u = (T)((uf * t.c) - (vf * t.s));
  v = (T)((vf * t.c) + (uf * t.s));
}

}  // namespace m3s_rope

#endif  // M3S_ROPE_DEVICE_H

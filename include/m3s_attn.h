/*
 * m3s_attn.h — C ABI of the MI355X fused attention core of MASt3R's blocks
 * (croco models/blocks.py:94-112, 149-169): RoPE2D of q and k, the scaled
 * scores, the softmax over the keys and the product with v, in one launch.
 *
 *   out[b,i,h,:] = sum_j softmax_j(scale * <R(q[b,i,h], qpos[b,i]),
 *                                           R(k[b,j,h], kpos[b,j])>) * v[b,j,h,:]
 *
 * R is exactly the rotation m3s_rope.h specifies (the same two device functions
 * evaluate it in both kernels, so it is bitwise the same); with both position
 * pointers null there is no rotation. q, k and v are read only; the score
 * matrix never reaches memory. Everything is fp32: the products are fp32-input
 * MFMA (a D-term fmaf chain per score), the softmax is the running-maximum
 * form with an accurate expf, the summation order is fixed and there are no
 * atomics, so two runs agree bitwise.
 *
 * The head dimension is 64, the head dimension of both of MASt3R's attentions
 * (encoder 1024 / 16, decoder 768 / 12); nothing else is built.
 *
 * Plain C: device pointers, sizes, the caller's hipStream_t as `void *`, an int
 * status (M3S_OK / M3S_EINVAL / M3S_ELAUNCH of m3s_gn.h). One launch, no
 * allocation, no host synchronisation, no workspace.
 */
#ifndef M3S_ATTN_H
#define M3S_ATTN_H

#include <stddef.h>
#include <stdint.h>

#include "m3s_rope.h" /* M3S_ROPE_F32 */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct m3s_attn_args {
  const void *q, *k, *v;      /* q [B,Nq,H,D]; k, v [B,Nk,H,D]; head rows contiguous, stride(H) == D */
  void *out;                  /* [B,Nq,H*D]: the layout `proj` takes */
  const int64_t *qpos, *kpos; /* [B,Nq,2], [B,Nk,2] contiguous (y, x); both null = no rotation */
  int64_t B, Nq, Nk, H, D;
  int64_t q_sb, q_sn, k_sb, k_sn, v_sb, v_sn, o_sb, o_sn; /* element strides */
  float base, f0, scale;
  int dtype;                  /* M3S_ROPE_F32 only, for now */
} m3s_attn_args;

/*
 * M3S_EINVAL, before any launch: a null record, null q, k, v or out; exactly
 * one of qpos / kpos null; B, Nq, Nk, H or D <= 0; D != 64; a dtype other than
 * M3S_ROPE_F32; for each of q, out (N = Nq) and k, v (N = Nk): x_sn < H * D or
 * x_sb < (N - 1) * x_sn + H * D; B * H * Nq or B * Nk above 2^31 - 1; `base`
 * not finite or <= 0; `f0` or `scale` not finite.
 *
 * The strides cover the three slices of an attention's [B,N,3,H,D] qkv buffer
 * seen as [B,N,H,D], (3 N H D, 3 H D, D, 1), and the dense projections of a
 * cross attention. When all four base addresses are multiples of 16 bytes and
 * all eight strides multiples of 4 elements, rows move as 16-byte vectors;
 * otherwise element by element. Both ways give bitwise the same values.
 */
int m3s_attn_rope(const m3s_attn_args *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* M3S_ATTN_H */

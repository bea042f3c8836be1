/*
 * m3s_rope.h — C ABI of the MI355X 2-D rotary position embedding of MASt3R's
 * attention (RoPE2D of croco's models/pos_embed.py; the reference reaches it
 * through a CUDA-only extension, curope).
 *
 * One head row of D = 4 Q channels is [u_Y(Q) | v_Y(Q) | u_X(Q) | v_X(Q)]. For
 * the axis a in {Y, X} and the frequency index i in [0, Q), in place:
 *
 *   theta = pos[b, n, a] * (f0 / base^(i/Q))
 *   u'    = u cos(theta) - v sin(theta)
 *   v'    = v cos(theta) + u sin(theta)
 *
 * theta, cos and sin in fp32 (powf, one division, one product, an accurate
 * sincosf with full argument reduction: arguments reach tens of radians), the
 * two results rounded once to the token type. f0 -> -f0 is the inverse
 * rotation, which is also the backward pass. Positions may be negative.
 *
 * Plain C: device pointers, sizes, the caller's hipStream_t as `void *`, an int
 * status (M3S_OK / M3S_EINVAL / M3S_ELAUNCH of m3s_gn.h). One launch, no
 * allocation, no host synchronisation, no workspace.
 */
#ifndef M3S_ROPE_H
#define M3S_ROPE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M3S_ROPE_F32 0
#define M3S_ROPE_F16 1
#define M3S_ROPE_BF16 2

typedef struct m3s_rope_args {
  void *tokens;              /* [B,N,H,D], rotated in place; stride(H) == D, stride(D) == 1 */
  const int64_t *pos;        /* [B,N,2] contiguous, (y, x) */
  int64_t B, N, H, D;
  int64_t stride_b, stride_n;/* in elements */
  float base, f0;
  int dtype;                 /* M3S_ROPE_* */
} m3s_rope_args;

/*
 * M3S_EINVAL, before any launch: a null record, null `tokens` or `pos`; B, N, H
 * or D <= 0; D % 4 != 0; stride_n < H * D; stride_b < (N - 1) * stride_n + H * D;
 * B * N > 2^31 - 1; `base` not finite or <= 0; `f0` not finite; an unknown dtype.
 *
 * The strides are those of the q or k slice of an attention's qkv buffer seen
 * as [B, N, H, D]: (3 N H D, 3 H D, D, 1). When the base address and both
 * strides are multiples of 16 bytes, k = 16 / sizeof(element) divides Q and
 * 2 Q / k <= 64 (a head fits one wave), rows move as 16-byte vectors; otherwise
 * element by element. Both ways give bitwise the same values.
 */
int m3s_rope_2d(const m3s_rope_args *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* M3S_ROPE_H */

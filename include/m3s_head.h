/*
 * m3s_head.h — C ABI of the MI355X tail of MASt3R's catmlp+dpt head: everything
 * between the head's two network outputs (the DPT map and the local-feature
 * MLP) and the tensors the SLAM kernels consume (mast3r catmlp_dpt_head.py:25-39,
 * 82-96 and dust3r heads/postprocess.py:22-58; the restacking, downsampling and
 * fp16 cast of the SLAM side). One read of the two inputs, one write of X, C, D
 * and Q into the caller's slots and dtypes.
 *
 * Per output pixel (b, yo, xo), with y = yo ds, x = xo ds, all in fp32:
 *
 *   s = (y / P) (W / P) + x / P,  i = y % P,  j = x % P
 *   lf(c) = feat[b, s, c P^2 + i P + j],  c in [0, F]      (pixel_shuffle of the
 *                                                           transposed MLP output)
 *   d = sqrt(px^2 + py^2 + pz^2),  (px, py, pz, pc) = pts[b, 0..3, y, x]
 *   X = (px, py, pz) / max(d, 1e-8) * expm1(d)
 *   C = conf_vmin  + min(exp(pc),    conf_vmax  - conf_vmin)
 *   D = lf(0..F-1) / sqrt(sum_c lf(c)^2)        (no epsilon: a zero descriptor is NaN)
 *   Q = dconf_vmin + min(exp(lf(F)), dconf_vmax - dconf_vmin)
 *
 * The squares are summed in the order of c with every product and sum rounded
 * (no FMA); sqrt and the divisions are correctly rounded; an fp16 D is the fp32
 * value rounded once. NaN passes through both min and max as through torch.clip.
 * These are the modes of the released checkpoint: depth ('exp', -inf, inf), conf
 * ('exp', vmin, vmax), two_confs, desc_conf ('exp', vmin, vmax), desc 'norm'.
 *
 * Plain C: device pointers, sizes, the caller's hipStream_t as `void *`, an int
 * status (M3S_OK / M3S_EINVAL / M3S_ELAUNCH of m3s_gn.h). One launch, no
 * allocation, no host synchronisation, no workspace.
 */
#ifndef M3S_HEAD_H
#define M3S_HEAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M3S_HEAD_F32 0
#define M3S_HEAD_F16 1

#define M3S_HEAD_GENERIC 1 /* flags: take the generic path whatever the shape */

typedef struct m3s_head_args {
  const float *pts;    /* [B,4,H,W] contiguous: DPT output, channels x,y,z,conf (raw) */
  const float *feat;   /* [B,S,(F+1)*P*P] contiguous: head_local_features output, S=(H/P)*(W/P) */
  float *X;            /* [B,Ho,Wo,3] */
  float *C;            /* [B,Ho,Wo]   */
  void  *D;            /* [B,Ho,Wo,F] f32 or f16 (desc_dtype) */
  float *Q;            /* [B,Ho,Wo]   */
  int64_t B, H, W, P, F, ds;                 /* Ho=ceil(H/ds), Wo=ceil(W/ds) */
  int64_t sbX, sbC, sbD, sbQ;                /* batch strides of the outputs, in elements */
  float conf_vmin, conf_vmax, dconf_vmin, dconf_vmax;  /* 'exp' modes; vmax may be +inf */
  int desc_dtype;      /* M3S_HEAD_F32 / M3S_HEAD_F16 */
  int flags;           /* M3S_HEAD_GENERIC: take the generic path whatever the shape */
} m3s_head_args;

/*
 * M3S_EINVAL, before any launch: a null record or a null pointer; B, H, W, P, F
 * or ds <= 0; H % P or W % P != 0; an output batch stride smaller than one image
 * of that output (Ho Wo 3, Ho Wo, Ho Wo F, Ho Wo); B H W > 2^31 - 1; (F + 1) P^2 >
 * 2^31 - 1 (a token's feature row is indexed with int); conf_vmin or dconf_vmin
 * not finite; a vmax below its vmin, or NaN; an unknown desc_dtype; unknown flag
 * bits.
 *
 * Two kernels that give bitwise the same values. With P == 16, F == 24, ds == 1,
 * X and D 16-byte aligned and sbX, sbD multiples of 16 bytes, one workgroup owns
 * one token's 16 x 16 patch: every read is coalesced as it stands, X and D are
 * transposed through LDS and leave as 16-byte vectors over contiguous bytes.
 * Everything else (and M3S_HEAD_GENERIC) goes pixel by pixel, element by
 * element, for any P, F, ds >= 1 and any alignment.
 */
int m3s_head_postprocess(const m3s_head_args *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* M3S_HEAD_H */

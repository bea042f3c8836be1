/*
 * m3s_dpt.h — C ABI of the MI355X tail of MASt3R's DPT regression head: its
 * last four modules (croco models/dpt_block.py:318-324, run at dust3r
 * heads/dpt_head.py:63 as self.head(path_1)),
 *
 *   Interpolate(scale_factor=2, bilinear, align_corners=True)  [B,128,Hi,Wi] -> [B,128,Ho,Wo]
 *   Conv2d(128 -> 128, 3x3, padding 1), ReLU, Conv2d(128 -> Cout, 1x1)   -> [B,Cout,Ho,Wo]
 *
 * in one launch: the upsampled image and the 128-channel map never reach
 * memory. The result is the `pts` that m3s_head_postprocess reads.
 *
 * With Ho = 2 Hi, Wo = 2 Wi, all in fp32:
 *
 *   rh  = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0     (one fp32 division; likewise rw)
 *   h1r = rh * (float)y,  y0 = (int)h1r,  y1 = y0 + (y0 < Hi - 1),
 *   lh1 = h1r - (float)y0,  lh0 = 1 - lh1                    (likewise x0, x1, lw1, lw0 of x)
 *   u[ci,y,x]  = lh0 * (lw0 * x[ci,y0,x0] + lw1 * x[ci,y0,x1])
 *              + lh1 * (lw0 * x[ci,y1,x0] + lw1 * x[ci,y1,x1])
 *                every product and sum rounded, no FMA contraction (as m3s_head.h
 *                states for its squares); u = 0 outside [0,Ho) x [0,Wo): the
 *                convolution's zero padding is of the upsampled image
 *   mid[c,y,x] = max(0, b1[c] + sum_{ci,dy,dx} w1[c,ci,dy,dx] * u[ci, y+dy-1, x+dx-1])
 *   out[o,y,x] = b2[o] + sum_c w2[o,c] * mid[c,y,x]
 *
 * This is ATen's upsample_bilinear2d with align_corners=True, whose source
 * index is formed in fp32: the lambdas are part of the function, not of the
 * error. The two sums are fp32-input MFMA and fmaf chains in an order of the
 * kernel's own, which is fixed; there are no atomics, so two runs agree bitwise.
 * A NaN in `mid` stays a NaN (as through torch's ReLU).
 *
 * Fixed: Cin = Cmid = 128 (the `features` of the released checkpoint's DPT
 * head), 1 <= Cout <= 4, fp32, NCHW, forward only; nothing else is built.
 *
 * Plain C: device pointers, sizes, the caller's hipStream_t as `void *`, an int
 * status (M3S_OK / M3S_EINVAL / M3S_ELAUNCH of m3s_gn.h). One launch per call,
 * no allocation, no host synchronisation, no workspace.
 */
#ifndef M3S_DPT_H
#define M3S_DPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M3S_DPT_CH 128       /* Cin = Cmid */
#define M3S_DPT_MAX_COUT 4
#define M3S_DPT_TILE_H 8     /* output pixels of one workgroup: rows ... */
#define M3S_DPT_TILE_W 32    /* ... and columns */
#define M3S_DPT_MAX_SIDE (1 << 20) /* largest Hi or Wi */

/* Bytes of the packed weights for `Cout` outputs; 0 unless 1 <= Cout <= 4. */
size_t m3s_dpt_tail_packed_size(int64_t Cout);

/*
 * w1 [128,128,3,3], b1 [128], w2 [Cout,128], b2 [Cout], all f32 contiguous, into
 * `packed` (>= m3s_dpt_tail_packed_size(Cout) bytes, 16-byte aligned): w1 in the
 * order the kernel's MFMA operands take it, then b1, w2 and b2. One launch;
 * once per model, not per call. M3S_EINVAL, before any launch: a null pointer,
 * Cout outside 1..4, `packed` not 16-byte aligned.
 */
int m3s_dpt_tail_pack(const float *w1, const float *b1, const float *w2, const float *b2, int64_t Cout,
                      void *packed, void *stream);

typedef struct m3s_dpt_tail_args {
  const float *x;      /* [B,128,Hi,Wi] f32, every image contiguous (NCHW) */
  const void *packed;  /* m3s_dpt_tail_pack's output for the same Cout */
  float *out;          /* [B,Cout,2Hi,2Wi] f32, every image contiguous (NCHW) */
  int64_t B, Hi, Wi, Cout;
  int64_t x_sb, out_sb; /* batch strides, in elements */
  int flags;            /* none defined: must be 0 */
} m3s_dpt_tail_args;

/*
 * M3S_EINVAL, before any launch: a null record or a null x, packed or out; B,
 * Hi, Wi or Cout <= 0; Cout > 4; Hi or Wi > M3S_DPT_MAX_SIDE (the source index
 * is an fp32 product; up to there the source tile of a workgroup provably
 * holds every pixel it interpolates from); x_sb < 128 Hi Wi or out_sb < Cout Ho
 * Wo; B 128 Hi Wi or B Cout Ho Wo above 2^31 - 1; `packed` not 16-byte aligned;
 * any flag bit.
 */
int m3s_dpt_tail(const m3s_dpt_tail_args *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* M3S_DPT_H */

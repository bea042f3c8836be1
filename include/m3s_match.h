/*
 * m3s_match.h — C ABI of the MI355X matching kernels of MASt3R-SLAM.
 *
 * Drop-in for the two non-GN entry points of the reference's
 * `mast3r_slam_backends` module (gn.cpp:84-114, declared gn.h:89-116; kernels
 * matching_kernels.cu), called by matching.py:60-85:
 *
 *   iter_proj       per-pixel Levenberg-Marquardt projection of a 3D ray onto
 *                   a ray image with gradients (matching_kernels.cu:119-296)
 *   refine_matches  dilated local search maximising the descriptor dot
 *                   product (matching_kernels.cu:25-116)
 *
 * and one entry point the reference has no counterpart of:
 *
 *   match_dense     the whole of matching.py:52-90 around those two, plus the
 *                   caller's quality combine and match count, in three
 *                   launches (described at m3s_match_dense_args below)
 *
 * Plain C: device pointers, sizes, the caller's hipStream_t as `void *`, an
 * int status (M3S_OK / M3S_EINVAL / M3S_ELAUNCH of m3s_gn.h). All tensors are
 * the reference's layouts, contiguous, on the device. One launch each
 * (match_dense: three), no host synchronisation, no allocation.
 */
#ifndef M3S_MATCH_H
#define M3S_MATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct m3s_iter_proj_args {
  const float *rays_img;    /* [B, H, W, 9]: unit ray (3), d/du (3), d/dv (3) */
  const float *pts_3d_norm; /* [B, N, 3]: unit rays to project               */
  const float *p_init;      /* [B, N, 2]: initial pixel (u, v)               */
  int64_t B, H, W, N;
  int max_iter;
  float lambda_init;
  float cost_thresh;
  float *p_new;       /* [B, N, 2] out                                       */
  uint8_t *converged; /* [B, N] out (torch.bool)                             */
} m3s_iter_proj_args;

/* Replaces iter_proj (gn.cpp:84-99 -> matching_kernels.cu:119-296). */
int m3s_iter_proj(const m3s_iter_proj_args *a, void *stream);

#define M3S_DESC_F16 0 /* D11/D21 are float16 (the reference's .half() call) */
#define M3S_DESC_F32 1

typedef struct m3s_refine_args {
  const void *D11;   /* [B, H, W, F] descriptors of image 1             */
  const void *D21;   /* [B, N, F] descriptors of the pixels to refine   */
  const int64_t *p1; /* [B, N, 2] current match (u, v) in image 1       */
  int64_t B, H, W, N, F;
  int dtype;        /* M3S_DESC_F16 or M3S_DESC_F32                      */
  int radius;       /* matching.radius (3)                               */
  int dilation_max; /* matching.dilation_max (5)                         */
  int64_t *p1_new;  /* [B, N, 2] out                                     */
} m3s_refine_args;

/* Replaces refine_matches (gn.cpp:101-114 -> matching_kernels.cu:25-116). */
int m3s_refine_matches(const m3s_refine_args *a, void *stream);

/*
 * match_dense: from what the network emits for B view pairs (pointmaps,
 * descriptors, descriptor confidences) to the rows the Gauss-Newton entry
 * points, the edge store and the trackers consume. It is matching.py:52-90
 * (prep_for_iter_proj, iter_proj, the occlusion test, refine_matches,
 * pixel_to_lin) followed by the caller's quality combine
 * Q = sqrt(Q11[b, idx] * Q21) (global_opt.py:53-57, tracker.py:41) and the
 * per-pair count of valid && Q > Q_conf that the edge filter turns into its
 * match fraction (global_opt.py:59-66).
 *
 * Three launches on the caller's stream: the ray-image prep (m3s_prep_rays),
 * projection + occlusion test (which also zeroes n_valid), refinement +
 * finalize. No allocation, no host synchronisation; no float pixel and no
 * int64 tensor is written. With idx_init it yields the tracker's idx_f2k,
 * valid_match_k and Qk (tracker.py:31-41).
 *
 * Outputs go to the caller's rows: batch element b of idx / valid / Q starts
 * b * <name>_stride elements after the pointer (stride >= H*W), so every other
 * row of a two-way edge store is a legal destination. `valid` is the match
 * validity alone (converged and not occluded), as the reference stores it; the
 * GN applies Q_conf itself.
 */
typedef struct m3s_match_dense_args {
  const float *X11;        /* [B, H, W, 3] pointmap of view 1                     */
  const float *X21;        /* [B, H*W, 3] points of view 2 in view 1's frame      */
  const void *D11;         /* [B, H, W, F] descriptors of view 1                  */
  const void *D21;         /* [B, H*W, F] descriptors of view 2                   */
  const float *Q11;        /* [B, H*W] descriptor confidence of view 1            */
  const float *Q21;        /* [B, H*W] descriptor confidence of view 2            */
  const int64_t *idx_init; /* [B, H*W] initial linear index into view 1, or NULL:
                              pixel n starts at itself (matching.py:32-41)        */
  int64_t B, H, W, F;
  int dtype;               /* M3S_DESC_F16 or M3S_DESC_F32                        */
  int max_iter;            /* matching.max_iter (10)                              */
  float lambda_init;       /* matching.lambda_init (1e-8)                         */
  float cost_thresh;       /* matching.convergence_thresh (1e-6)                  */
  float dist_thresh;       /* matching.dist_thresh (1e-1)                         */
  int radius;              /* matching.radius (3); 0: no refinement               */
  int dilation_max;        /* matching.dilation_max (5)                           */
  float Q_conf;            /* local_opt.Q_conf (1.5): the count's threshold       */
  int32_t *idx;            /* out: u + W * v of the match in view 1               */
  uint8_t *valid;          /* out (torch.bool)                                    */
  float *Q;                /* out: sqrt(Q11[b, idx] * Q21[b, n])                  */
  int64_t idx_stride, valid_stride, Q_stride; /* elements between batch rows      */
  int32_t *n_valid;        /* [B] out: pixels with valid && Q > Q_conf            */
  void *workspace;         /* >= m3s_match_dense_workspace_size(B, H, W) bytes:
                              ray image, unit rays, integer pixels, flags         */
  size_t workspace_bytes;
} m3s_match_dense_args;

size_t m3s_match_dense_workspace_size(int64_t B, int64_t H, int64_t W);
int m3s_match_dense(const m3s_match_dense_args *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* M3S_MATCH_H */

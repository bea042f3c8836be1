// gn/args.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The small host helpers every host part uses: S() (the caller's stream),
// launch_ok, make_params, check_args.
// Host code only; relies on gn_layout (gn/layout.h) and m3s_gn.h.

// ---------------------------------------------------------------- host --
inline hipStream_t S(void *s) { return reinterpret_cast<hipStream_t>(s); }

int launch_ok() { return hipGetLastError() == hipSuccess ? M3S_OK : M3S_ELAUNCH; }

ResidualParams make_params(const m3s_gn_args *a) {
  ResidualParams P;
  P.inv_sig_a = a->sigma_a != 0.0f ? (float)(1.0 / (double)a->sigma_a) : 0.0f;
  P.inv_sig_b = a->sigma_b != 0.0f ? (float)(1.0 / (double)a->sigma_b) : 0.0f;
  P.C_thresh = a->C_thresh;
  P.Q_thresh = a->Q_thresh;
  P.fx = P.fy = P.cx = P.cy = 0.0f;
  P.width = a->width;
  P.height = a->height;
  P.border = (float)a->pixel_border;
  P.z_eps = a->z_eps;
  P.huber_k = 1.345f;  // hard-coded in the reference kernels (gn_kernels.cu:172-175)
  return P;
}

int check_args(const m3s_gn_args *a) {
  if (!a || !a->Twc || !a->Xs || !a->Cs || !a->ii || !a->jj || !a->idx_ii2jj || !a->valid_match ||
      !a->Q || !a->info || !a->workspace)
    return M3S_EINVAL;
  if (a->N < 1 || a->HW < 1 || a->E < 0) return M3S_EINVAL;
  if (a->mode == M3S_MODE_CALIB && (!a->K || a->width < 1 || a->height < 1)) return M3S_EINVAL;
  if (a->workspace_bytes < gn_layout(a->N, a->HW, a->E).total) return M3S_EINVAL;
  if (a->HW * 3 >= ((int64_t)1 << 40)) return M3S_ETOOLARGE;
  if (a->mode < 0 || a->mode > 2) return M3S_EINVAL;
  return M3S_OK;
}

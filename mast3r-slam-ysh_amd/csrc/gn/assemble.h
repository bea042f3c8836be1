// gn/assemble.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The dense system and the end of a step: assemble_kernel (the RHS-augmented
// matrix from the edge sums), finish_step (retraction, dx, info, stop flag)
// and fail_step (the same after a failed factorisation).
// Relies on wave_sum_pl (gn/linearize.h) and the Sim(3) functions of
// m3s_device.h.

// ------------------------------------------------------------- assemble --
// RHS-augmented system in A (row-major, leading dim ld = roundup(n+1, 64)):
//   A[0:n, 0:n] = H,  A[n, 0:n] = g^T,  rows > n = identity padding.
// Block r < N-1 owns rows [7r, 7r+7) and the entries A[n, 7r:7r+7); block
// N-1 initialises row n's tail and the padding rows.
__global__ void __launch_bounds__(256) assemble_kernel(const double *__restrict__ edge_sums,
                                                       const int32_t *__restrict__ rank_i,
                                                       const int32_t *__restrict__ rank_j, int64_t E,
                                                       const float *__restrict__ Twc, int64_t n,
                                                       int64_t ld, double *__restrict__ A,
                                                       const int32_t *__restrict__ stop) {
  if (*stop) return;
  const int r = blockIdx.x;
  const int t = threadIdx.x;
  const int nb = (int)(n / 7);
  if (r == nb) {  // padding block
    for (int64_t k = n + t; k < ld; k += blockDim.x) A[(size_t)n * ld + k] = 0.0;
    for (int64_t k = t; k < (ld - n - 1) * ld; k += blockDim.x) {
      const int64_t i = n + 1 + k / ld, j = k % ld;
      A[(size_t)i * ld + j] = (i == j) ? 1.0 : 0.0;
    }
    return;
  }
  __shared__ double M[7][7], Lm[7][7], T1[7][7], Hjj[7][7], l[7], gj[7];
  for (int64_t k = t; k < 7 * ld; k += blockDim.x) A[(size_t)7 * r * ld + k] = 0.0;
  double *g = A + (size_t)n * ld;
  if (t < 7) g[7 * r + t] = 0.0;
  __syncthreads();
  for (int64_t e = 0; e < E; e++) {
    const int i = rank_i[e] - 1, j = rank_j[e] - 1;
    if (i != r && j != r) continue;  // uniform across the block
    const double *es = edge_sums + (size_t)e * kNP;
    if (t == 0) adjT_inv_matrix(Twc + 8 * (size_t)(i + 1), M);
    if (t < 49) {
      const int a = t / 7, c = t % 7;
      const int lo = a < c ? a : c, hi = a < c ? c : a;
      Lm[a][c] = es[kL + tri(lo, hi)];
    }
    if (t < 7) l[t] = es[kG + t];
    __syncthreads();
    if (t < 49) {
      const int a = t / 7, c = t % 7;
      double s = 0.0;
      for (int k = 0; k < 7; k++) s += M[a][k] * Lm[k][c];
      T1[a][c] = s;
    } else if (t < 56) {
      const int a = t - 49;
      double s = 0.0;
      for (int k = 0; k < 7; k++) s += M[a][k] * l[k];
      gj[a] = s;
    }
    __syncthreads();
    if (t < 49) {
      const int a = t / 7, c = t % 7;
      double s = 0.0;
      for (int k = 0; k < 7; k++) s += T1[a][k] * M[c][k];
      Hjj[a][c] = s;
    }
    __syncthreads();
    if (t < 49) {
      const int a = t / 7, c = t % 7;
      double *row = A + (size_t)(7 * r + a) * ld;
      const double h = Hjj[a][c];
      // edge (i -> j): Hs[0]=Hs[3]=Hjj at (i,i),(j,j); Hs[1]=Hs[2]=-Hjj off-diagonal
      if (i == r) {
        row[7 * r + c] += h;
        if (j >= 0) row[7 * j + c] -= h;
      }
      if (j == r) {
        row[7 * r + c] += h;
        if (i >= 0) row[7 * i + c] -= h;
      }
    } else if (t < 56) {
      const int a = t - 49;
      if (i == r) g[7 * r + a] -= gj[a];  // gs[0] = -M l
      if (j == r) g[7 * r + a] += gj[a];  // gs[1] = +M l
    }
    __syncthreads();
  }
}

// dx = -x, retraction of poses 1..N-1, ||dx|| test, info update. x in LDS.
// Called by one whole block (blockDim.x threads, multiple of 64).
__device__ void finish_step(const double *xs, float *dxs, float *nrm, int n, float *Twc, int64_t N,
                            float *dx_out, int32_t *info, int32_t *stop, float delta_thresh) {
  const int tid = threadIdx.x, nt = blockDim.x;
  float part = 0.0f;
  for (int k = tid; k < n; k += nt) {
    const float v = -(float)xs[k];
    dxs[k] = v;
    dx_out[k] = v;
    part += v * v;
  }
  part = wave_sum_pl(part);
  if ((tid & 63) == 0) nrm[tid >> 6] = part;
  __syncthreads();
  for (int p = tid; p < (int)(N - 1); p += nt) {
    const Sim3f T = load_sim3(Twc + 8 * (size_t)(p + 1));
    store_sim3(Twc + 8 * (size_t)(p + 1), retract_f64(dxs + 7 * p, T));
  }
  if (tid == 0) {
    float s = 0.0f;
    for (int w = 0; w < nt / 64; w++) s += nrm[w];
    info[M3S_INFO_ITERS] += 1;
    if (sqrtf(s) < delta_thresh) {
      info[M3S_INFO_CONVERGED] = 1;
      stop[0] = 1;
    }
  }
}

// LLT failure: dx = 0 (poses unchanged), ||0|| < delta stops like the reference
__device__ void fail_step(int n, float *dx_out, int32_t *info, int32_t *stop, float delta_thresh) {
  for (int k = threadIdx.x; k < n; k += blockDim.x) dx_out[k] = 0.0f;
  if (threadIdx.x == 0) {
    info[M3S_INFO_ITERS] += 1;
    info[M3S_INFO_SOLVE_FAIL] += 1;
    if (0.0f < delta_thresh) {
      info[M3S_INFO_CONVERGED] = 1;
      stop[0] = 1;
    }
  }
}

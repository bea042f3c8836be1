// gn/chol_small.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// Test build only (the whole part is inside #ifdef M3S_TEST_PATHS):
// chol_small_kernel<NBC>, the register-resident dense Cholesky of one
// workgroup, an A/B reference behind the dense knob.
// Relies on kCholThreads (gn/layout.h) and on finish_step and fail_step
// (gn/assemble.h).

#ifdef M3S_TEST_PATHS  // reached only through the dense knob: every graph it fits (m <= 31) has a sparse plan
// ------------------------------------------------- small dense Cholesky --
// Thread (tr, tc) of a 16 x 32 grid owns A[lr*16 + tr][lc*32 + tc]. The RHS g
// is appended as row n, so the factor's row n is y = L^-1 g. After the loop
// the registers hold L (lower triangle). NBC = column blocks of 32.
template <int NBC>
__global__ void __launch_bounds__(kCholThreads) chol_small_kernel(
    const double *__restrict__ Aug, int64_t ld, int n, float *__restrict__ Twc, int64_t N,
    float *__restrict__ dx_out, int32_t *__restrict__ info, int32_t *__restrict__ stop,
    float delta_thresh) {
  constexpr int NBR = 2 * NBC;
  if (*stop) return;
  const int tid = threadIdx.x;
  const int tr = tid >> 5, tc = tid & 31;
  __shared__ double colbuf[2][32 * NBC];
  __shared__ double xbuf[32 * NBC];
  __shared__ double ybuf[32 * NBC];
  __shared__ double red[16][33];
  __shared__ double dblk[32][33];
  __shared__ float dxs[32 * NBC];
  __shared__ float nrm[kCholThreads / 64];

  double A[NBR][NBC];
#pragma unroll
  for (int lr = 0; lr < NBR; lr++)
#pragma unroll
    for (int lc = 0; lc < NBC; lc++) {
      const int i = lr * 16 + tr, j = lc * 32 + tc;
      A[lr][lc] = (i <= n && j < n) ? Aug[(size_t)i * ld + j] : ((i == j) ? 1.0 : 0.0);
    }
  for (int k = tid; k < 32 * NBC; k += kCholThreads) xbuf[k] = 0.0, ybuf[k] = 0.0;
  bool failed = false;
  int step = 0;

#pragma unroll
  for (int kb = 0; kb < NBC; kb++) {
    for (int c = 0; c < 32; c++) {
      const int k = kb * 32 + c;
      if (k >= n || failed) break;
      double *cb = colbuf[step & 1];
      // owners of column k publish it (rows < k as 0)
      if (tc == c) {
#pragma unroll
        for (int lr = 0; lr < NBR; lr++) {
          const int i = lr * 16 + tr;
          cb[i] = (i >= k) ? A[lr][kb] : 0.0;
        }
      }
      __syncthreads();
      const double d = cb[k];
      if (!(d > 0.0)) {  // Eigen LLT: non-positive pivot -> failure (dx = 0)
        failed = true;
        break;
      }
      const double inv = 1.0 / sqrt(d);
      double lj[NBC];
#pragma unroll
      for (int lc = 0; lc < NBC; lc++) lj[lc] = (lc >= kb) ? cb[lc * 32 + tc] * inv : 0.0;
#pragma unroll
      for (int lr = 2 * kb; lr < NBR; lr++) {
        const double li = cb[lr * 16 + tr] * inv;
#pragma unroll
        for (int lc = kb; lc < NBC; lc++)
          if (lc * 32 <= lr * 16 + 15) A[lr][lc] -= li * lj[lc];
        if (tc == c) A[lr][kb] = li;  // column k of L
      }
      step++;
    }
  }

  if (failed) {  // every thread saw the same pivot
    fail_step(n, dx_out, info, stop, delta_thresh);
    return;
  }

  // y = row n of the factor
#pragma unroll
  for (int lr = 0; lr < NBR; lr++)
    if (lr * 16 + tr == n)
#pragma unroll
      for (int lc = 0; lc < NBC; lc++) {
        const int j = lc * 32 + tc;
        if (j < n) ybuf[j] = A[lr][lc];
      }
  __syncthreads();

  // back-substitution L^T x = y, 32-column blocks from the bottom
#pragma unroll
  for (int kb = NBC - 1; kb >= 0; kb--) {
    double s = 0.0;
#pragma unroll
    for (int lr = 0; lr < NBR; lr++)
      if (lr * 16 >= (kb + 1) * 32) s += A[lr][kb] * xbuf[lr * 16 + tr];
    red[tr][tc] = s;
#pragma unroll
    for (int lr = 2 * kb; lr < 2 * kb + 2; lr++) dblk[lr * 16 + tr - kb * 32][tc] = A[lr][kb];
    __syncthreads();
    if (tid < 64) {
      const int cc = tid & 31;
      double rhs = 0.0;
      if (tid < 32) {
        const int j = kb * 32 + cc;
        double acc = 0.0;
        for (int q = 0; q < 16; q++) acc += red[q][cc];
        rhs = (j < n) ? ybuf[j] - acc : 0.0;
      }
      double x = 0.0;
      for (int cp = 31; cp >= 0; cp--) {
        const double xc = __shfl(rhs, cp, 64) / dblk[cp][cp];
        if (kb * 32 + cp >= n) continue;  // uniform
        if (cc < cp) rhs -= dblk[cp][cc] * xc;
        if (cc == cp) x = xc;
      }
      if (tid < 32) {
        const int j = kb * 32 + cc;
        xbuf[j] = (j < n) ? x : 0.0;
      }
    }
    __syncthreads();
  }
  finish_step(xbuf, dxs, nrm, n, Twc, N, dx_out, info, stop, delta_thresh);
}
#endif  // M3S_TEST_PATHS (chol_small_kernel)

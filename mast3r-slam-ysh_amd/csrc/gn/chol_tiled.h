// gn/chol_tiled.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The dense solve of systems beyond the register-resident kernel:
// potrf_tile_kernel, trsm_tile_kernel, update_tiles_kernel, backsolve_kernel.
// Relies on gn/layout.h (kTile, kFlagStop, kFlagFail) and on finish_step and
// fail_step (gn/assemble.h).

// ------------------------------------------------- tiled dense Cholesky --
// For systems beyond the register-resident kernel. Right-looking, 64x64
// fp64 tiles, three launches per tile column: factor the diagonal tile,
// triangular-solve the panel below it, update the trailing lower tiles.
// Thread (ty, tx) of a 16x16 grid owns tile entries (ty + 16a, tx + 16b).
__global__ void __launch_bounds__(256) potrf_tile_kernel(double *__restrict__ A, int64_t ld, int64_t n,
                                                         int kb, int32_t *__restrict__ flags) {
  if (flags[kFlagStop] || flags[kFlagFail]) return;
  __shared__ double cb[2][kTile];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double *T = A + (size_t)kb * kTile * ld + (size_t)kb * kTile;
  double v[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) v[a][b] = T[(size_t)(ty + 16 * a) * ld + tx + 16 * b];
  int step = 0;
#pragma unroll
  for (int cbk = 0; cbk < 4; cbk++) {
    for (int cc = 0; cc < 16; cc++) {
      const int c = 16 * cbk + cc;
      if ((int64_t)kb * kTile + c >= n) break;  // augmented row / padding: nothing to factor
      double *col = cb[step & 1];
      if (tx == cc) {
#pragma unroll
        for (int a = 0; a < 4; a++) col[ty + 16 * a] = (ty + 16 * a >= c) ? v[a][cbk] : 0.0;
      }
      __syncthreads();
      const double d = col[c];
      if (!(d > 0.0)) {
        if (threadIdx.x == 0) flags[kFlagFail] = 1;
        return;  // uniform: every thread read the same pivot
      }
      const double inv = 1.0 / sqrt(d);
      double lj[4];
#pragma unroll
      for (int b = 0; b < 4; b++) lj[b] = col[tx + 16 * b] * inv;
#pragma unroll
      for (int a = 0; a < 4; a++) {
        const double li = col[ty + 16 * a] * inv;
#pragma unroll
        for (int b = 0; b < 4; b++) v[a][b] -= li * lj[b];
        if (tx == cc) v[a][cbk] = li;
      }
      step++;
    }
  }
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) T[(size_t)(ty + 16 * a) * ld + tx + 16 * b] = v[a][b];
}

// X L_kk^T = A_ik for the row tiles i > kb (block b -> i = kb + 1 + b)
__global__ void __launch_bounds__(256) trsm_tile_kernel(double *__restrict__ A, int64_t ld, int64_t n,
                                                        int kb, int32_t *__restrict__ flags) {
  if (flags[kFlagStop] || flags[kFlagFail]) return;
  __shared__ double Lk[kTile][kTile + 1];
  __shared__ double cb[2][kTile];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i = kb + 1 + blockIdx.x;
  const double *D = A + (size_t)kb * kTile * ld + (size_t)kb * kTile;
  for (int k = threadIdx.x; k < kTile * kTile; k += 256) Lk[k / kTile][k % kTile] = D[(size_t)(k / kTile) * ld + k % kTile];
  double *T = A + (size_t)i * kTile * ld + (size_t)kb * kTile;
  double v[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) v[a][b] = T[(size_t)(ty + 16 * a) * ld + tx + 16 * b];
  __syncthreads();
  int step = 0;
#pragma unroll
  for (int cbk = 0; cbk < 4; cbk++) {
    for (int cc = 0; cc < 16; cc++) {
      const int c = 16 * cbk + cc;
      if ((int64_t)kb * kTile + c >= n) break;
      double *col = cb[step & 1];
      const double inv = 1.0 / Lk[c][c];
      if (tx == cc) {
#pragma unroll
        for (int a = 0; a < 4; a++) {
          v[a][cbk] *= inv;
          col[ty + 16 * a] = v[a][cbk];
        }
      }
      __syncthreads();
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int s = tx + 16 * b;
        if (s > c) {
          const double l = Lk[s][c];
#pragma unroll
          for (int a = 0; a < 4; a++) v[a][b] -= col[ty + 16 * a] * l;
        }
      }
      step++;
    }
  }
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) T[(size_t)(ty + 16 * a) * ld + tx + 16 * b] = v[a][b];
}

// A_ij -= L_ik L_jk^T for kb < j <= i < nt (block -> packed lower index)
__global__ void __launch_bounds__(256) update_tiles_kernel(double *__restrict__ A, int64_t ld, int kb,
                                                           const int32_t *__restrict__ flags) {
  if (flags[kFlagStop] || flags[kFlagFail]) return;
  __shared__ double Li[kTile][kTile + 1];
  __shared__ double Lj[kTile][kTile + 1];
  const int t = blockIdx.x;
  int ip = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((ip + 1) * (ip + 2) / 2 <= t) ip++;
  while (ip * (ip + 1) / 2 > t) ip--;
  const int jp = t - ip * (ip + 1) / 2;
  const int i = kb + 1 + ip, j = kb + 1 + jp;
  const double *Pi = A + (size_t)i * kTile * ld + (size_t)kb * kTile;
  const double *Pj = A + (size_t)j * kTile * ld + (size_t)kb * kTile;
  for (int k = threadIdx.x; k < kTile * kTile; k += 256) {
    Li[k / kTile][k % kTile] = Pi[(size_t)(k / kTile) * ld + k % kTile];
    Lj[k / kTile][k % kTile] = Pj[(size_t)(k / kTile) * ld + k % kTile];
  }
  __syncthreads();
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[4][4] = {};
  for (int s = 0; s < kTile; s++) {
    double li[4], lj[4];
#pragma unroll
    for (int a = 0; a < 4; a++) li[a] = Li[ty + 16 * a][s];
#pragma unroll
    for (int b = 0; b < 4; b++) lj[b] = Lj[tx + 16 * b][s];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) acc[a][b] += li[a] * lj[b];
  }
  double *T = A + (size_t)i * kTile * ld + (size_t)j * kTile;
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) T[(size_t)(ty + 16 * a) * ld + tx + 16 * b] -= acc[a][b];
}

// L^T x = y (y = row n of the factor), tiles from the bottom; then the step.
__global__ void __launch_bounds__(1024) backsolve_kernel(const double *__restrict__ A, int64_t ld, int n,
                                                         float *__restrict__ Twc, int64_t N,
                                                         float *__restrict__ dx_out, int32_t *__restrict__ info,
                                                         int32_t *__restrict__ flags, float delta_thresh) {
  if (flags[kFlagStop]) return;
  const int failed = flags[kFlagFail];
  __syncthreads();  // every wave has read the flag before thread 0 clears it
  if (failed) {
    fail_step(n, dx_out, info, flags + kFlagStop, delta_thresh);
    if (threadIdx.x == 0) flags[kFlagFail] = 0;
    return;
  }
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *rhs = smem;              // ld
  double *D = smem + ld;           // kTile x (kTile+1)
  float *dxs = reinterpret_cast<float *>(D + kTile * (kTile + 1));  // ld floats
  __shared__ float nrm[16];
  const int tid = threadIdx.x;
  for (int k = tid; k < ld; k += blockDim.x) rhs[k] = (k < n) ? A[(size_t)n * ld + k] : 0.0;
  const int nt = (n + kTile - 1) / kTile;
  for (int kb = nt - 1; kb >= 0; kb--) {
    __syncthreads();
    const double *T = A + (size_t)kb * kTile * ld + (size_t)kb * kTile;
    for (int k = tid; k < kTile * kTile; k += blockDim.x) D[(k / kTile) * (kTile + 1) + k % kTile] = T[(size_t)(k / kTile) * ld + k % kTile];
    __syncthreads();
    if (tid < 64) {  // one wave: L_kk^T x = rhs_kb
      double r = rhs[kb * kTile + tid];
      double x = 0.0;
      for (int c = kTile - 1; c >= 0; c--) {
        if (kb * kTile + c >= n) continue;  // uniform
        const double xc = __shfl(r, c, 64) / D[c * (kTile + 1) + c];
        if (tid < c) r -= D[c * (kTile + 1) + tid] * xc;
        if (tid == c) x = xc;
      }
      rhs[kb * kTile + tid] = (kb * kTile + tid < n) ? x : 0.0;  // rhs now holds x for this tile
    }
    __syncthreads();
    // rhs_j -= sum_r L[kb*64 + r][j] x_r for all j < kb*64
    for (int j = tid; j < kb * kTile; j += blockDim.x) {
      double s = 0.0;
      for (int r = 0; r < kTile; r++) s += A[(size_t)(kb * kTile + r) * ld + j] * rhs[kb * kTile + r];
      rhs[j] -= s;
    }
  }
  __syncthreads();
  finish_step(rhs, dxs, nrm, n, Twc, N, dx_out, info, flags + kFlagStop, delta_thresh);
}

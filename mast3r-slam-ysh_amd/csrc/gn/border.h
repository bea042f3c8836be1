// gn/border.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// border_kernel: the dense tail's border updates over the chip, between the
// two phases of sparse_llt_kernel<0>.
// Relies on kFlagStop (gn/layout.h) and on SparseDev, border_task and
// kStageDoubles (gn/llt_blocks.h).

// ------------------------------------------------------- border kernel --
// Dense-tail border updates spread over the chip (global factors, between
// sparse_llt_kernel phases 1 and 2): one task per wave, 4 waves per
// workgroup, y in global memory (D.rhs, written by phase 1). The tasks are
// independent; in the single-workgroup kernel they took ~290 us at N = 256.
// The kernel stays at this position, behind the prologue, to keep the device
// code's order (top of the file); a later change may move it next to the tail.
constexpr int kBorderWaves = 4;
__global__ void __launch_bounds__(64 * kBorderWaves) border_kernel(SparseDev D) {
  if (D.flags[kFlagStop]) return;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int32_t *pl = D.plan;
  const int32_t *clq = pl + D.off[kSec_clq];
  const int nc = clq[0], c0 = clq[1], nt0 = nc * (nc + 1) / 2;
  const int r = lane / 7, c = lane % 7;
  const bool act49 = lane < 49;
  const int lane49 = act49 ? lane : 0, r7 = act49 ? r * 7 : 0, c7 = act49 ? c * 7 : 0;
  const int lane7 = lane < 7 ? lane : 0;
  double *stg = smem + (size_t)wave * kStageDoubles;
  double *y = const_cast<double *>(D.rhs);
  for (int t = blockIdx.x * kBorderWaves + wave; t < nt0; t += gridDim.x * kBorderWaves)
    border_task<true>(t, nc, c0, pl, D.off, D.L, y, r7, c7, lane49, lane, lane7, act49, stg, D.tail_A, D.tail_ld);
}

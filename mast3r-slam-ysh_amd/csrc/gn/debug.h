// gn/debug.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The two debug kernels behind m3s_debug_copy and m3s_debug_sim3:
// hbm_copy_kernel and sim3_debug_kernel. They stand after the tracker: the
// include list is part of the order of the device code.
// Relies on the f32x4 typedef (m3s_gn.hip) and the Sim(3) functions of
// m3s_device.h.

// Streaming copy (m3s_debug_copy): the measured HBM ceiling bench.py reports
// beside the 8 TB/s spec. 16 B per lane per access (dwordx4), 4 accesses in
// flight per lane, non-temporal loads and stores, grid-stride over the buffer.
__global__ void __launch_bounds__(256) hbm_copy_kernel(const f32x4 *__restrict__ src, f32x4 *__restrict__ dst,
                                                       int64_t n4) {
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  for (int64_t base = (int64_t)blockIdx.x * 256 * 4 + threadIdx.x; base < n4; base += stride) {
    f32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (base + 256 * k < n4) v[k] = __builtin_nontemporal_load(src + base + 256 * k);
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (base + 256 * k < n4) __builtin_nontemporal_store(v[k], dst + base + 256 * k);
  }
}

// Sim(3) device helpers on arrays (m3s_debug_sim3): the functions the hot path
// applies, run as-is for the property tests of tests/test_gpu_sim3.py
__global__ void sim3_debug_kernel(int op, const float *__restrict__ a, const float *__restrict__ b,
                                  float *__restrict__ out, int64_t n) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  switch (op) {
    case 0: store_sim3(out + 8 * k, exp_sim3(a + 7 * k)); break;
    case 1: store_sim3(out + 8 * k, retract_f64(a + 7 * k, load_sim3(b + 8 * k))); break;
    case 2: store_sim3(out + 8 * k, compose(load_sim3(a + 8 * k), load_sim3(b + 8 * k))); break;
    case 3: store_sim3(out + 8 * k, inverse(load_sim3(a + 8 * k))); break;
    case 4: store_sim3(out + 8 * k, relative(load_sim3(a + 8 * k), load_sim3(b + 8 * k))); break;
    case 5: act(load_sim3(a + 8 * k), b + 3 * k, out + 3 * k); break;
    case 6: act(sim3_matrix(load_sim3(a + 8 * k)), b + 3 * k, out + 3 * k); break;
    case 7: {
      double M[7][7];
      adjT_inv_matrix(a + 8 * k, M);
      for (int r = 0; r < 7; r++)
        for (int c = 0; c < 7; c++) out[49 * k + 7 * r + c] = (float)M[r][c];
      break;
    }
    case 8: store_sim3(out + 8 * k, retract(a + 7 * k, load_sim3(b + 8 * k))); break;
    default: break;
  }
}

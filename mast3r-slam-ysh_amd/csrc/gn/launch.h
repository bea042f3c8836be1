// gn/launch.h — part of the m3s_gn.hip translation unit (not a stand-alone header).
// The linearize launches of the host: the in-call timing event slots and
// launch_timed (the one launch that takes an armed event pair; gn/solve.h
// uses it for sparse_llt_kernel<1>), launch_lin, launch_linearize,
// dispatch_linearize (the first host mention of the linearize kernel
// templates), vec_ok and read_K.
// Relies on the linearize and gathering kernels (gn/linearize.h,
// gn/gather.h), launch_ok (gn/args.h) and gn/knobs.h (gather_lds_path).

// In-call timing (m3s_debug_call_timing): the drop-in call sets a start /
// stop event pair for its next linearize launch, which then goes through
// hipExtLaunchKernel: the events take the dispatch's own begin / end
// timestamps (the kernel's span, as a kernel trace records it; events
// recorded around the launch read 8-12% more, profiles/r04/prof_split_*.txt)
// {start, stop}; thread_local: set and consumed by one gn_full call on its own
// thread (a call on another thread without timing never sees it).
// launch_timed clears it when it used the pair, so the caller can tell a span
// whose linearize went through another launch (the pack == 0 path) and fall
// back to the events recorded around it.
thread_local hipEvent_t *g_lin_ext_ev = nullptr;
// the same for the one-workgroup solve's launch (sparse_llt_kernel<1>, small
// graphs: the whole solve of an iteration is that one dispatch)
thread_local hipEvent_t *g_slv_ext_ev = nullptr;
// One launch that takes the armed pair `ev` (and clears it), or a plain one.
template <typename K, typename A>
void launch_timed(hipEvent_t *&ev, K kernel, dim3 g, dim3 b, size_t lds, hipStream_t st, const A &args) {
  if (ev) {
    hipExtLaunchKernelGGL(kernel, g, b, lds, st, ev[0], ev[1], 0, args);
    ev = nullptr;
  } else {
    kernel<<<g, b, lds, st>>>(args);
  }
}
template <typename K>
void launch_lin(K kernel, dim3 g, dim3 b, hipStream_t st, const LinArgs &L) {
  launch_timed(g_lin_ext_ev, kernel, g, b, 0, st, L);
}

// pack: 0 gathering kernel, 1 gathering kernel that stores the planes,
// 2 packed kernel (reads the planes; VEC layout only)
template <int MODE, bool TRACK>
int launch_linearize(const LinArgs &L, int64_t blocks, bool vec, int pack, hipStream_t st) {
  if (blocks <= 0) return M3S_OK;
  const dim3 g((unsigned)blocks), b(kThreads);
  if (TRACK || pack == 0) {
    if (vec)
      linearize_kernel<MODE, TRACK, true, false><<<g, b, 0, st>>>(L);
    else
      linearize_kernel<MODE, TRACK, false, false><<<g, b, 0, st>>>(L);
  } else if (pack == 1) {
    if (vec && gather_lds_path() && L.HW <= (int64_t(1) << 24))  // (24-bit index products)
      launch_lin(linearize_gather_kernel<MODE>, g, b, st, L);
    else if (vec)
      launch_lin(linearize_kernel<MODE, false, true, true>, g, b, st, L);
    else
      launch_lin(linearize_kernel<MODE, false, false, true>, g, b, st, L);
  } else {
    launch_lin(linearize_packed_kernel<MODE>, g, b, st, L);
  }
  return launch_ok();
}

template <bool TRACK>
int dispatch_linearize(int mode, const LinArgs &L, int64_t blocks, bool vec, int pack, hipStream_t st) {
  switch (mode) {
    case M3S_MODE_POINTS: return launch_linearize<M3S_MODE_POINTS, TRACK>(L, blocks, vec, pack, st);
    case M3S_MODE_RAYS: return launch_linearize<M3S_MODE_RAYS, TRACK>(L, blocks, vec, pack, st);
    case M3S_MODE_CALIB: return launch_linearize<M3S_MODE_CALIB, TRACK>(L, blocks, vec, pack, st);
  }
  return M3S_EINVAL;
}

bool vec_ok(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// K is a device pointer; read it once per call (tiny D2H copy, not on the
// iteration path). For graph capture the caller can pass params instead.
int read_K(const float *K, ResidualParams &P, hipStream_t st) {
  float k[9];
  if (hipMemcpyAsync(k, K, sizeof k, hipMemcpyDeviceToHost, st) != hipSuccess) return M3S_ELAUNCH;
  if (hipStreamSynchronize(st) != hipSuccess) return M3S_ELAUNCH;
  P.fx = k[0], P.fy = k[4], P.cx = k[2], P.cy = k[5];
  return M3S_OK;
}

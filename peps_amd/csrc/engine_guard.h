// The base of a step on the device-resident optimizer buffers: what the spike rollback and the step selectors of the reference do
// with host copies of the SplitIndexTPS (optimizer/optimizer_impl.h: prev_accepted_state_ :838-841, the selector trials :320-542,
// SGDPreviewUpdate_ :1001) without moving a tensor over PCIe.  One more vector in the layout of opt_theta_:
//   save      base <- theta (device to device; the padding of theta is zero, so that of base is)
//   restore   theta <- base, sitps_ = T(base) in one pass.  g is not an operand: after a spike it may hold Inf / NaN
//   clear     forget that a base is saved; the buffer stays
//   preview   theta <- SGD rule on (base, g, velocity), sitps_ = T(theta); the velocity is read and not written
// The preview evaluates opt_sgd_elem of engine_opt.h, the function opt_step_kernel<T, OPT_SGD> evaluates: on the same base the two
// leave the same bytes in theta and sitps_.  With rule parameters (0, 0, 0) it is theta_base - lr g, the trial along an SR / MinSR
// direction left in g.
// Kernels as in engine_lbfgs.h: memory bound, live elements only, 16-byte accesses where the rows allow it, at most 2048 blocks with
// grid strides, no atomics.  Fermionic decoration: base, theta, g and the velocity are in the range of E and both passes are
// element-wise and odd in their operands, so they run unchanged.
#pragma once
#include "engine_lbfgs.h"

namespace pepsgpu {

// rows q = (site, component) of rowlen = slot * Z doubles, the first ne[site] * Z of them live; o = offset of the thread's V doubles
// kPreview: theta = opt_sgd_elem(base, g, vel); else theta = base.  sitps = T(theta).
template <typename T, int V, bool kPreview>
__global__ __launch_bounds__(256) void opt_guard_kernel(OptStepArgs a, const double *__restrict__ base, const double *__restrict__ g,
                                                        const double *__restrict__ vel, double *__restrict__ theta,
                                                        T *__restrict__ sitps, const int *__restrict__ ne, int nrows, long rowlen,
                                                        int dp) {
#pragma clang fp contract(off)
  constexpr int z = is_cplx<T>::value ? 2 : 1;
  static_assert(V % z == 0, "a complex element is never split between two threads");
  const long stride = (long)gridDim.x * 256 * V;
  for (int q = blockIdx.y; q < nrows; q += gridDim.y) {
    const long nlive = (long)ne[q / dp] * z;
    for (long e = ((long)blockIdx.x * 256 + threadIdx.x) * V; e < nlive; e += stride) {      // the padding is not even read
      const long o = (long)q * rowlen + e, live = nlive - e;
      double th[V];
      lb_load<V>(base + o, th);
      if constexpr (kPreview) {
        double gv[V], vv[V];
        lb_load<V>(g + o, gv);
        for (int i = 0; i < V; ++i) vv[i] = 0.0;
        if (a.mu > 0.0) lb_load<V>(vel + o, vv);
        for (int i = 0; i < V; ++i) {
          double dropped;
          th[i] = opt_sgd_elem(a, th[i], gv[i], vv[i], &dropped);
        }
      }
      lb_store<V>(theta + o, th, live);
      for (int i = 0; i < V; i += z)
        if (i < live) opt_store_state<T>(sitps, (o + i) / z, th + i);
    }
  }
}

template <typename T>
void Engine<T>::opt_base_save() {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "opt_base_save: call pepsgpu_opt_begin first");
  const size_t bytes = sizeof(double) * (size_t)Ly_ * Lx_ * dp_ * slot_ * kOut;
  if (opt_base_ == nullptr) opt_base_ = (double *)arena_.alloc(bytes);
  PG_CHECK_HIP(hipMemcpyAsync(opt_base_, opt_theta_, bytes, hipMemcpyDeviceToDevice, stream_));
  opt_base_saved_ = true;
}

template <typename T>
void Engine<T>::opt_base_clear() {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "opt_base_clear: call pepsgpu_opt_begin first");
  opt_base_saved_ = false;
}

#define OPT_GUARD_LAUNCH(PREVIEW, ARGS)                                                                                             \
  do {                                                                                                                              \
    const dim3 grid = lbfgs_grid();                                                                                                 \
    if (lbfgs_vec() == 2)                                                                                                           \
      hipLaunchKernelGGL((opt_guard_kernel<T, 2, PREVIEW>), grid, dim3(256), 0, stream_, ARGS, (const double *)opt_base_,           \
                         (const double *)opt_g_, (const double *)opt_vel_, opt_theta_, sitps_, (const int *)opt_ne_,                \
                         Ly_ * Lx_ * dp_, (long)slot_ * kOut, dp_);                                                                 \
    else if constexpr (!kCplx)                                                                                                      \
      hipLaunchKernelGGL((opt_guard_kernel<T, 1, PREVIEW>), grid, dim3(256), 0, stream_, ARGS, (const double *)opt_base_,           \
                         (const double *)opt_g_, (const double *)opt_vel_, opt_theta_, sitps_, (const int *)opt_ne_,                \
                         Ly_ * Lx_ * dp_, (long)slot_ * kOut, dp_);                                                                 \
    PG_CHECK_HIP(hipGetLastError());                                                                                                \
    state_adopted(); /* sitps_ changed: the walkers' environments are stale as after pepsgpu_state_upload */                        \
  } while (0)

template <typename T>
void Engine<T>::opt_base_restore() {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "opt_base_restore: call pepsgpu_opt_begin first");
  PG_REQUIRE(opt_base_saved_, 3, "opt_base_restore: no base saved (pepsgpu_opt_base_save)");
  OPT_GUARD_LAUNCH(false, OptStepArgs{});
}

template <typename T>
void Engine<T>::opt_preview(int rule, double lr, const double *params, int n_params) {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "opt_preview: call pepsgpu_opt_begin first");
  PG_REQUIRE(rule == OPT_SGD, 1, "opt_preview: only the SGD rule (0) has a preview; an SR / MinSR direction in g is rule 0 with (0, 0, 0)");
  PG_REQUIRE(opt_base_saved_, 3, "opt_preview: no base saved (pepsgpu_opt_base_save)");
  const OptStepArgs a = opt_sgd_args("opt_preview", lr, params, n_params);
  OPT_GUARD_LAUNCH(true, a);
}
#undef OPT_GUARD_LAUNCH

}  // namespace pepsgpu

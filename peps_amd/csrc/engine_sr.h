// Stochastic-reconfiguration S-matrix on the device: the O* samples of the walkers stay in HBM
// and S v = <delta_i O*_i>, delta_i = O*_i . v - mean(O*) . v  (centred scalar projection,
// optimizer/stochastic_reconfiguration_smatrix.h:37-99) is two HBM-bound sweeps over them.
// An O* sample is stored the way the reference's SITPS-shaped sample is populated: one D^4 block per
// site, belonging to the component the walker's configuration selects (mc_energy_grad_evaluator.h:257-270),
// i.e. [sample][site][D^4] of T plus the configuration [sample][site].
// Every entry and every kernel has one body for float, double and cplx<double> (TenElemT = QLTEN_Complex; SRSMatrix and MinSRTMatrix
// are templated over it): host and HBM vectors are doubles, Z = kOut of them per scalar, interleaved (re, im) pairs on a complex context.
#pragma once
#include "engine.h"

namespace pepsgpu {

// O*_i(site) = hole_i(site) / psi_i  from the resident hole store of the current walkers; psi_i arrives as log|psi_i| and its sign
// (ph_re; ph_im unused).  Complex: O*_i(site) = conj(1 / psi_i) Dag(hole_i)(site) = conj(hole) * (psi / |psi|) / |psi|
// (mc_energy_grad_evaluator.h:245-270), the unit phase psi / |psi| in (ph_re, ph_im).
template <typename T>
__global__ __launch_bounds__(256) void sr_append_kernel(const T *__restrict__ holes, const double *__restrict__ holes_ls,
                                                        const int *__restrict__ cfg, const double *__restrict__ logabs,
                                                        const double *__restrict__ ph_re, const double *__restrict__ ph_im,
                                                        T *__restrict__ o_out, int *__restrict__ cfg_out, int sites, long slot,
                                                        const int *__restrict__ site_ne) {
  const int w = blockIdx.z, site = blockIdx.y;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long base = ((long)w * sites + site) * slot;
  // only the first site_ne[site] elements of a slot hold the (compactly stored) hole; the rest is never written
  if (e < slot) {
    T v = T(0);
    if (e < site_ne[site]) {
      if constexpr (is_cplx<T>::value) {
        const double f = exp(holes_ls[(long)w * sites + site] - logabs[w]);
        const double hr = (double)holes[base + e].re, hi = -(double)holes[base + e].im;            // Dag(hole)
        v = T(f * (hr * ph_re[w] - hi * ph_im[w]), f * (hr * ph_im[w] + hi * ph_re[w]));
      } else {
        v = T(ph_re[w] * exp(holes_ls[(long)w * sites + site] - logabs[w]) * (double)holes[base + e]);
      }
    }
    o_out[base + e] = v;
  }
  if (e == 0) cfg_out[(long)w * sites + site] = cfg[(long)w * sites + site];
}

// delta[i] = sum_site < O*_i(site), v(site)[cfg_i(site)] > - shift - *shift_dev      (one block per sample)
// complex: <a, b> = sum conj(a) b  (SplitIndexTPS::operator*, split_index_tps.h:370-377)
template <typename T>
__global__ __launch_bounds__(256) void sr_delta_kernel(const T *__restrict__ o, const int *__restrict__ cfg,
                                                       const double *__restrict__ v, double shift_re, double shift_im,
                                                       double *__restrict__ delta, int sites, long slot, int dp,
                                                       const double *__restrict__ shift_dev = nullptr) {
  constexpr int Z = is_cplx<T>::value ? 2 : 1;
  __shared__ double s_red[4 * Z];
  const int i = blockIdx.x;
  double a[Z];
  for (int z = 0; z < Z; ++z) a[z] = 0.0;
  for (int site = 0; site < sites; ++site) {
    const T *oi = o + ((long)i * sites + site) * slot;
    const double *vs = v + Z * ((long)site * dp + cfg[(long)i * sites + site]) * slot;
    for (long e = threadIdx.x; e < slot; e += 256) {
      if constexpr (is_cplx<T>::value) {
        const double xr = (double)oi[e].re, xi = (double)oi[e].im, yr = vs[2 * e], yi = vs[2 * e + 1];
        a[0] += xr * yr + xi * yi;
        a[1] += xr * yi - xi * yr;
      } else {
        a[0] += (double)oi[e] * vs[e];
      }
    }
  }
  for (int z = 0; z < Z; ++z) {
    a[z] = wave_sum(a[z]);
    if ((threadIdx.x & 63) == 0) s_red[4 * z + (threadIdx.x >> 6)] = a[z];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double shift[2] = {shift_re, shift_im};
    for (int z = 0; z < Z; ++z)
      delta[Z * i + z] = s_red[4 * z] + s_red[4 * z + 1] + s_red[4 * z + 2] + s_red[4 * z + 3] - shift[z] - (shift_dev ? shift_dev[z] : 0.0);
  }
}

// out[site][s][e] = scale * sum_{i : cfg_i(site) == s} weight_i O*_i(site)[e]   (weight == nullptr: 1; complex weights on a complex T)
template <typename T>
__global__ __launch_bounds__(256) void sr_accum_kernel(const T *__restrict__ o, const int *__restrict__ cfg,
                                                       const double *__restrict__ weight, double scale, double *__restrict__ out,
                                                       int n, int sites, long slot, int dp) {
  constexpr int Z = is_cplx<T>::value ? 2 : 1;
  const int site = blockIdx.y;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= slot) return;
  for (int s = 0; s < dp; ++s) {
    double a[Z];
    for (int z = 0; z < Z; ++z) a[z] = 0.0;
    for (int i = 0; i < n; ++i) {
      if (cfg[(long)i * sites + site] != s) continue;
      if constexpr (is_cplx<T>::value) {
        const double wr = weight ? weight[2 * i] : 1.0, wi = weight ? weight[2 * i + 1] : 0.0;
        const T x = o[((long)i * sites + site) * slot + e];
        a[0] += wr * (double)x.re - wi * (double)x.im;
        a[1] += wr * (double)x.im + wi * (double)x.re;
      } else {
        a[0] += (weight ? weight[i] : 1.0) * (double)o[((long)i * sites + site) * slot + e];
      }
    }
    const long q = Z * (((long)site * dp + s) * slot + e);
    for (int z = 0; z < Z; ++z) out[q + z] = scale * a[z];
  }
}

// part[Z b .. Z b + Z) = sum over the block's grid-stride share of a[e] b[e] (Z = 1), of conj(a[e]) b[e] on n interleaved (re, im)
// pairs (Z = 2); sr_dot_final_kernel adds the partials in a fixed order (no atomics: the CG scalars are reproducible run to run)
template <int Z>
__global__ __launch_bounds__(256) void sr_dot_kernel(const double *__restrict__ a, const double *__restrict__ b, long n,
                                                     double *__restrict__ part) {
  __shared__ double s_red[4 * Z];
  double acc[Z];
  for (int z = 0; z < Z; ++z) acc[z] = 0.0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    if constexpr (Z == 2) {
      const double xr = a[2 * e], xi = a[2 * e + 1], yr = b[2 * e], yi = b[2 * e + 1];
      acc[0] += xr * yr + xi * yi;
      acc[1] += xr * yi - xi * yr;
    } else {
      acc[0] += a[e] * b[e];
    }
  }
  for (int z = 0; z < Z; ++z) {
    acc[z] = wave_sum(acc[z]);
    if ((threadIdx.x & 63) == 0) s_red[4 * z + (threadIdx.x >> 6)] = acc[z];
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int z = 0; z < Z; ++z) part[Z * blockIdx.x + z] = s_red[4 * z] + s_red[4 * z + 1] + s_red[4 * z + 2] + s_red[4 * z + 3];
}
template <int Z>
__global__ __launch_bounds__(64) void sr_dot_final_kernel(const double *__restrict__ part, int nblocks, double *__restrict__ out) {
  double acc[Z];
  for (int z = 0; z < Z; ++z) acc[z] = 0.0;
  for (int e = threadIdx.x; e < nblocks; e += 64)
    for (int z = 0; z < Z; ++z) acc[z] += part[Z * e + z];
  for (int z = 0; z < Z; ++z) acc[z] = wave_sum(acc[z]);
  if (threadIdx.x == 0)
    for (int z = 0; z < Z; ++z) out[z] = acc[z];
}

// y = alpha * x + beta * y on n entries, beta real; Z = 1: alpha = alpha_re, Z = 2: alpha complex on interleaved (re, im) pairs
template <int Z>
__global__ __launch_bounds__(256) void sr_axpby_kernel(double alpha_re, double alpha_im, const double *__restrict__ x, double beta,
                                                       double *__restrict__ y, long n) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    if constexpr (Z == 2) {
      const double xr = x[2 * e], xi = x[2 * e + 1];
      y[2 * e] = alpha_re * xr - alpha_im * xi + beta * y[2 * e];
      y[2 * e + 1] = alpha_re * xi + alpha_im * xr + beta * y[2 * e + 1];
    } else {
      y[e] = alpha_re * x[e] + beta * y[e];
    }
  }
}

// state layout of the C ABI ([site][s][L][D][R][U], legs zero padded to D) <-> the compact per-slot layout the
// device keeps site tensors, holes and O* samples in (true leg dimensions, row-major inside the D^4 slot)
template <typename T>
void Engine<T>::sr_convert(const double *src, double *dst, bool to_compact) const {
  const size_t n = (size_t)Ly_ * Lx_ * dp_ * slot_ * kOut;      // complex: interleaved (re, im) pairs
  std::fill(dst, dst + n, 0.0);
  const size_t m = sr_map_c_.size();
  for (size_t k = 0; k < m; ++k) {
    const size_t from = kOut * (size_t)(to_compact ? sr_map_p_[k] : sr_map_c_[k]), to = kOut * (size_t)(to_compact ? sr_map_c_[k] : sr_map_p_[k]);
    for (int z = 0; z < kOut; ++z) dst[to + z] = src[from + z];
  }
}

// sr_map_c_ / sr_map_p_ of sr_convert (a property of the lattice: built once per context)
template <typename T>
void Engine<T>::layout_maps() {
  if (!sr_map_c_.empty()) return;
  for (int r = 0; r < Ly_; ++r)
    for (int c = 0; c < Lx_; ++c) {
      int dd[4];
      site_dims(r, c, dd);
      for (int s = 0; s < dp_; ++s) {
        const size_t base = ((size_t)(r * Lx_ + c) * dp_ + s) * slot_;
        size_t o = 0;
        for (int a = 0; a < dd[0]; ++a)
          for (int b = 0; b < dd[1]; ++b)
            for (int cc = 0; cc < dd[2]; ++cc)
              for (int e = 0; e < dd[3]; ++e, ++o) {
                sr_map_c_.push_back((uint32_t)(base + o));
                sr_map_p_.push_back((uint32_t)(base + (((size_t)a * D_ + b) * D_ + cc) * D_ + e));
              }
      }
    }
}

template <typename T>
void Engine<T>::sr_begin(int max_samples) {
  PG_REQUIRE(max_samples > 0, 1, "sr_begin: need a positive sample capacity");
  sr_release();
  const size_t sites = (size_t)Ly_ * Lx_;
  sr_o_ = (T *)arena_.alloc(sizeof(T) * (size_t)max_samples * sites * slot_);
  sr_cfg_ = (int *)arena_.alloc(sizeof(int) * (size_t)max_samples * sites);
  sr_delta_ = (double *)arena_.alloc(sizeof(double) * (size_t)max_samples * kOut);
  sr_v_ = (double *)arena_.alloc(sizeof(double) * sites * dp_ * slot_ * kOut);
  sr_out_ = (double *)arena_.alloc(sizeof(double) * sites * dp_ * slot_ * kOut);
  layout_maps();
  sr_ne_ = (int *)arena_.alloc(sizeof(int) * sites);
  std::vector<int> ne(sites);
  for (int r = 0; r < Ly_; ++r)
    for (int c = 0; c < Lx_; ++c) {
      int dd[4];
      site_dims(r, c, dd);
      ne[r * Lx_ + c] = dd[0] * dd[1] * dd[2] * dd[3];
    }
  PG_CHECK_HIP(hipMemcpyAsync(sr_ne_, ne.data(), sizeof(int) * sites, hipMemcpyHostToDevice, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  sr_cap_ = max_samples;
  sr_n_ = 0;
}

template <typename T>
void Engine<T>::sr_release() {
  if (sr_o_) { arena_.free(sr_o_); arena_.free(sr_cfg_); arena_.free(sr_delta_); arena_.free(sr_v_); arena_.free(sr_out_); arena_.free(sr_ne_); }
  sr_ne_ = nullptr;
  sr_o_ = nullptr; sr_cfg_ = nullptr; sr_delta_ = nullptr; sr_v_ = nullptr; sr_out_ = nullptr;
  sr_cap_ = sr_n_ = 0;
}

template <typename T>
void Engine<T>::sr_append(const double *psi) {
  require_ready();
  PG_REQUIRE(sr_o_ != nullptr, 3, "sr_append: call pepsgpu_sr_begin first");
  PG_REQUIRE(holes_ != nullptr, 3, "sr_append: no holes stored (pepsgpu_punch_hole with out == NULL)");
  PG_REQUIRE(sr_n_ + nw_ <= sr_cap_, 1, "sr_append: sample store is full");
  std::vector<double> h((1 + kOut) * (size_t)nw_);      // log|psi|, then the sign | the unit phase (re, im)
  for (int w = 0; w < nw_; ++w) {
    if constexpr (kCplx) {
      const double a = std::hypot(psi[2 * w], psi[2 * w + 1]);
      PG_REQUIRE(a != 0.0, 5, "Wavefunction amplitude is near zero, causing division by zero.");
      h[w] = std::log(a); h[nw_ + w] = psi[2 * w] / a; h[2 * nw_ + w] = psi[2 * w + 1] / a;
    } else {
      PG_REQUIRE(psi[w] != 0.0, 5, "Wavefunction amplitude is near zero, causing division by zero.");
      h[w] = std::log(std::fabs(psi[w]));
      h[nw_ + w] = psi[w] < 0 ? -1.0 : 1.0;
    }
  }
  ArenaScope scope(arena_);      // (d goes back to the arena when a HIP call below throws)
  double *d = (double *)arena_.alloc(sizeof(double) * h.size());
  PG_CHECK_HIP(hipMemcpyAsync(d, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, stream_));
  const int sites = Ly_ * Lx_;
  hipLaunchKernelGGL(sr_append_kernel<T>, dim3((unsigned)((slot_ + 255) / 256), sites, nw_), dim3(256), 0, stream_,
                     (const T *)holes_, (const double *)holes_ls_, (const int *)cfg_, (const double *)d, (const double *)(d + nw_),
                     (const double *)(kCplx ? d + 2 * nw_ : nullptr), sr_o_ + (size_t)sr_n_ * sites * slot_,
                     sr_cfg_ + (size_t)sr_n_ * sites, sites, slot_, (const int *)sr_ne_);
  PG_CHECK_HIP(hipGetLastError());
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  arena_.free(d);
  sr_n_ += nw_;
}

template <typename T>
void Engine<T>::sr_sum(double *out) {
  PG_REQUIRE(sr_o_ != nullptr && sr_n_ > 0, 3, "sr_sum: no samples");
  const int sites = Ly_ * Lx_;
  const size_t n = (size_t)sites * dp_ * slot_ * kOut;
  hipLaunchKernelGGL(sr_accum_kernel<T>, dim3((unsigned)((slot_ + 255) / 256), sites), dim3(256), 0, stream_, (const T *)sr_o_,
                     (const int *)sr_cfg_, (const double *)nullptr, 1.0, sr_out_, sr_n_, sites, slot_, dp_);
  PG_CHECK_HIP(hipGetLastError());
  std::vector<double> h(n);
  PG_CHECK_HIP(hipMemcpyAsync(h.data(), sr_out_, n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  sr_convert(h.data(), out, false);
}

// out = scale * sum_i (O*_i . v - mean_dot_v) O*_i      (caller: all-reduce over ranks, + diag_shift * v)
template <typename T>
void Engine<T>::sr_matvec(const double *v, double mean_dot_v_re, double mean_dot_v_im, double scale, double *out) {
  PG_REQUIRE(kCplx || mean_dot_v_im == 0.0, 1, "sr_matvec: a real context takes a real mean_dot_v");
  PG_REQUIRE(sr_o_ != nullptr && sr_n_ > 0, 3, "sr_matvec: no samples");
  const int sites = Ly_ * Lx_;
  const size_t n = (size_t)sites * dp_ * slot_ * kOut;
  std::vector<double> h(n);
  sr_convert(v, h.data(), true);
  PG_CHECK_HIP(hipMemcpyAsync(sr_v_, h.data(), n * sizeof(double), hipMemcpyHostToDevice, stream_));
  hipLaunchKernelGGL(sr_delta_kernel<T>, dim3(sr_n_), dim3(256), 0, stream_, (const T *)sr_o_, (const int *)sr_cfg_,
                     (const double *)sr_v_, mean_dot_v_re, mean_dot_v_im, sr_delta_, sites, slot_, dp_);
  PG_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(sr_accum_kernel<T>, dim3((unsigned)((slot_ + 255) / 256), sites), dim3(256), 0, stream_, (const T *)sr_o_,
                     (const int *)sr_cfg_, (const double *)sr_delta_, scale, sr_out_, sr_n_, sites, slot_, dp_);
  PG_CHECK_HIP(hipGetLastError());
  PG_CHECK_HIP(hipMemcpyAsync(h.data(), sr_out_, n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  sr_convert(h.data(), out, false);
}

// ---------------------------------------------------------------------------------------------
// Device-resident natural-gradient solve: ConjugateGradientSolver (utility/conjugate_gradient_solver.h:181-276)
// on (S + diag_shift) x = b with every vector in HBM next to the samples (compact layout, f64).  One iteration =
// two sweeps over the sample store (S p) + a few axpy / dot kernels; the host reads back the handful of scalars
// its branches need (p.Ap, |p|^2 | |x|^2, |r|^2, r_prev.r) twice per iteration.  Every branch of the reference is
// kept: indefinite-matrix exit, stagnation detection, periodic residual recomputation, NaN/Inf exits, best-iterate
// tracking, orthogonality-based restart.
// The vectors are n entries of Z = kOut doubles.  a * b = sum conj(a) b is sr_dot_kernel<Z> over the n entries (Z doubles), NormSquare
// the real dot over the Z n doubles; alpha = rk / pap is complex on a complex context, beta real, and the restart test takes the real
// part of r_prev * r (:259-266).
template <typename T>
void Engine<T>::sr_cg_solve(const double *b, const double *x0, double diag_shift, int max_iter, double rel_tol,
                            double abs_tol, int recompute_interval, double ortho_threshold, double *x_out,
                            double *residual_norm, int *iterations, int *reason) {
  PG_REQUIRE(sr_o_ != nullptr && sr_n_ > 0, 3, "sr_cg_solve: no samples");
  ArenaScope scope(arena_);
  constexpr int Z = kOut;
  const int sites = Ly_ * Lx_;
  const long n = (long)sites * dp_ * slot_, nd = Z * n;
  const double scale = 1.0 / sr_n_;
  // Called from opt_natural_gradient with a fermionic decoration set, the vectors are in the range of E (extended layout) and the
  // stored-parameter equation (E^T S_ext E + shift) x = g reads Pi(S_ext v) + shift v = g^ on them: Pi is applied to every S v, and
  // every dot product (4 x the stored one, E^T E = 4 mask) is scaled back, so that the coefficients, the tolerances, the iteration
  // count and the reported norms are those of the stored-space solve.  Every other call takes the path it always took.
  const bool fproj = sr_cg_dev_ != nullptr && fd_d_ > 0 && opt_sign_ != nullptr;
  auto dvec = [&]() { return (double *)arena_.alloc(sizeof(double) * nd); };
  double *db = dvec(), *dx = dvec(), *dr = dvec(), *dp = dvec(), *dap = dvec(), *dbest = dvec(), *dprev = dvec(), *dmean = dvec();
  double *dsc = (double *)arena_.alloc(sizeof(double) * 8 * Z), *dmv = dsc + 7 * Z;      // the read-back slots, and Ostar_mean * v
  constexpr int DOT_BLOCKS = 512;
  double *dpart = (double *)arena_.alloc(sizeof(double) * Z * DOT_BLOCKS);
  auto nsq_into = [&](const double *a, double *out) {          // sum |a|^2: a real dot over the Z n doubles
    hipLaunchKernelGGL(sr_dot_kernel<1>, dim3(DOT_BLOCKS), dim3(256), 0, stream_, a, a, nd, dpart);
    hipLaunchKernelGGL(sr_dot_final_kernel<1>, dim3(1), dim3(64), 0, stream_, (const double *)dpart, DOT_BLOCKS, out);
  };
  auto dot_into = [&](const double *a, const double *b2, double *out) {          // sum conj(a) b2: Z doubles
    hipLaunchKernelGGL(sr_dot_kernel<Z>, dim3(DOT_BLOCKS), dim3(256), 0, stream_, a, b2, n, dpart);
    hipLaunchKernelGGL(sr_dot_final_kernel<Z>, dim3(1), dim3(64), 0, stream_, (const double *)dpart, DOT_BLOCKS, out);
  };
  std::vector<double> h(nd);
  auto upload = [&](const double *src, double *dst) {
    if (src && src == sr_cg_dev_) {      // already on the device, compact (engine_opt.h)
      PG_CHECK_HIP(hipMemcpyAsync(dst, src, nd * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    } else if (src) {
      sr_convert(src, h.data(), true);
      PG_CHECK_HIP(hipMemcpyAsync(dst, h.data(), nd * sizeof(double), hipMemcpyHostToDevice, stream_));
      PG_CHECK_HIP(hipStreamSynchronize(stream_));   // h is reused
    } else PG_CHECK_HIP(hipMemsetAsync(dst, 0, nd * sizeof(double), stream_));
  };
  auto copy = [&](double *dst, const double *src) {
    PG_CHECK_HIP(hipMemcpyAsync(dst, src, nd * sizeof(double), hipMemcpyDeviceToDevice, stream_));
  };
  const dim3 vg((unsigned)std::min<long>((n + 255) / 256, 2048)), vgd((unsigned)std::min<long>((nd + 255) / 256, 2048));
  auto axpby = [&](double alpha, const double *x, double beta, double *y) {       // real scalars: element-wise on the doubles
    hipLaunchKernelGGL(sr_axpby_kernel<1>, vgd, dim3(256), 0, stream_, alpha, 0.0, x, beta, y, nd);
  };
  auto zaxpby = [&](double ar, double ai, const double *x, double beta, double *y) {       // alpha of the element type
    hipLaunchKernelGGL(sr_axpby_kernel<Z>, vg, dim3(256), 0, stream_, ar, ai, x, beta, y, n);
  };
  auto read = [&](double *out, int k) {
    PG_CHECK_HIP(hipMemcpyAsync(out, dsc, sizeof(double) * k, hipMemcpyDeviceToHost, stream_));
    PG_CHECK_HIP(hipStreamSynchronize(stream_));
    if (fproj) for (int q = 0; q < k; ++q) out[q] *= 0.25;
  };
  // out = S v + diag_shift v     (SRSMatrix::operator*, stochastic_reconfiguration_smatrix.h:37-99)
  auto matvec = [&](const double *v, double *out) {
    dot_into(dmean, v, dmv);   // Ostar_mean * v = sum conj(mean) v
    hipLaunchKernelGGL(sr_delta_kernel<T>, dim3(sr_n_), dim3(256), 0, stream_, (const T *)sr_o_, (const int *)sr_cfg_, v, 0.0, 0.0,
                       sr_delta_, sites, slot_, dp_, (const double *)dmv);
    hipLaunchKernelGGL(sr_accum_kernel<T>, dim3((unsigned)((slot_ + 255) / 256), sites), dim3(256), 0, stream_, (const T *)sr_o_,
                       (const int *)sr_cfg_, (const double *)sr_delta_, scale, out, sr_n_, sites, slot_, dp_);
    PG_CHECK_HIP(hipGetLastError());
    if (fproj) opt_fermion_project(out);
    if (diag_shift != 0.0) axpby(diag_shift, v, 1.0, out);
  };
  auto finish = [&](const double *xsrc, double res_sq, int iters, int why) {
    const bool dev_out = sr_cg_dev_ && x_out == sr_cg_dev_;
    PG_CHECK_HIP(hipMemcpyAsync(dev_out ? x_out : h.data(), xsrc, nd * sizeof(double), dev_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream_));
    PG_CHECK_HIP(hipStreamSynchronize(stream_));
    if (!dev_out) sr_convert(h.data(), x_out, false);
    *residual_norm = std::sqrt(res_sq); *iterations = iters; *reason = why;
    for (double *v : {db, dx, dr, dp, dap, dbest, dprev, dmean, dsc, dpart}) arena_.free(v);
  };
  enum { kConverged = 0, kMaxIterations = 1, kIndefiniteMatrix = 2, kNumericalBreakdown = 3, kStagnated = 4 };

  // Ostar_mean
  hipLaunchKernelGGL(sr_accum_kernel<T>, dim3((unsigned)((slot_ + 255) / 256), sites), dim3(256), 0, stream_, (const T *)sr_o_,
                     (const int *)sr_cfg_, (const double *)nullptr, scale, dmean, sr_n_, sites, slot_, dp_);
  upload(b, db);
  upload(x0, dx);
  double s[4];
  matvec(dx, dap);
  copy(dr, db);
  axpby(-1.0, dap, 1.0, dr);                      // r = b - A x0
  nsq_into(db, dsc); nsq_into(dr, dsc + 1); read(s, 2);
  const double tol_sq = std::max(rel_tol * rel_tol * s[0], abs_tol * abs_tol);
  double r_norm_sq = s[1];
  if (r_norm_sq <= tol_sq) return finish(dx, r_norm_sq, 0, kConverged);
  copy(dp, dr); copy(dbest, dx); copy(dprev, dr);
  double best = r_norm_sq, rkp1 = r_norm_sq;
  int stagnation = 0;
  const double eps = 2.220446049250313e-16;
  for (int k = 0; k < max_iter; ++k) {
    const double rk = rkp1;
    matvec(dp, dap);
    dot_into(dp, dap, dsc); nsq_into(dp, dsc + Z); read(s, Z + 1);
    const double pap_re = s[0], pap_im = kCplx ? s[1] : 0.0, pp = s[Z];
    // detail::pap_is_valid (:142-148): Re > 0 and |Im| < 1e-10.  +inf passes, NaN does not, as in the reference: the NaN that +inf
    // makes of the residual is the kNumericalBreakdown exit below
    if (!(pap_re > 0.0 && std::fabs(pap_im) < 1e-10)) return finish(dbest, best, k, kIndefiniteMatrix);
    double a_re, a_im = 0.0;      // alpha = rk / pap
    if constexpr (kCplx) {
      const double den = pap_re * pap_re + pap_im * pap_im;
      a_re = rk * pap_re / den; a_im = -rk * pap_im / den;
    } else {
      a_re = rk / pap_re;
    }
    zaxpby(a_re, a_im, dp, 1.0, dx);
    if (recompute_interval > 0 && (k % recompute_interval) == recompute_interval - 1) {
      matvec(dx, dr);
      axpby(1.0, db, -1.0, dr);                   // r = b - A x
    } else zaxpby(-a_re, -a_im, dap, 1.0, dr);
    nsq_into(dx, dsc); nsq_into(dr, dsc + 1); dot_into(dprev, dr, dsc + 2); read(s, 2 + Z);
    if ((a_re * a_re + a_im * a_im) * pp < eps * eps * s[0]) {
      if (++stagnation >= 3) return finish(dbest, best, k + 1, kStagnated);
    } else stagnation = 0;
    rkp1 = s[1];
    if (!std::isfinite(rkp1)) return finish(dbest, best, k + 1, kNumericalBreakdown);
    if (rkp1 < best) { copy(dbest, dx); best = rkp1; }
    if (rkp1 <= tol_sq) return finish(dx, rkp1, k + 1, kConverged);
    if (k > 0 && std::fabs(s[2]) > ortho_threshold * rkp1) {   // orthogonality-based restart (real part of r_prev * r)
      copy(dp, dr); copy(dprev, dr);
      continue;
    }
    copy(dprev, dr);
    const double beta = rkp1 / rk;
    if (!std::isfinite(beta)) return finish(dbest, best, k + 1, kNumericalBreakdown);
    axpby(1.0, dr, beta, dp);                      // p = r + beta p
  }
  finish(dbest, best, max_iter, kMaxIterations);
}

// ---------------------------------------------------------------------------------------------
// MinSR building blocks (optimizer/minsr_tmatrix.h, optimizer_impl.h:1126-1215): raw Gram blocks of O* samples as one
// tensor GEMM over the compact parameter index (f64 accumulation), the weighted sum sum_i y_i O*_i, and a
// device-to-device copy of the local samples for the ring exchange of the multi-rank T matrix.
// A sample is expanded by its configuration into the SITPS-shaped vector the reference holds
// (component cfg_i(site) of every site, zeros elsewhere): the Gram block is then a plain GEMM over K = sites * d * D^4.
template <typename T>
__global__ __launch_bounds__(256) void sr_expand_kernel(const T *__restrict__ o, const int *__restrict__ cfg, T *__restrict__ out,
                                                        int sites, long slot, int dp, const int *__restrict__ site_ne) {
  const int i = blockIdx.z, site = blockIdx.y;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= slot) return;
  const int c = cfg[(long)i * sites + site];
  const T v = e < site_ne[site] ? o[((long)i * sites + site) * slot + e] : T(0);
  for (int s = 0; s < dp; ++s) out[(((long)i * sites + site) * dp + s) * slot + e] = s == c ? v : T(0);
}

// The walk over the row / column blocks of the Gram of the local store against the remote batch (remote_o == nullptr: against itself,
// blocks on and above the diagonal only).  ip_ij = O*_i * O*_j = sum conj(O*_i) O*_j (SplitIndexTPS::operator*): a complex context
// conjugates the A operand of the tensor GEMM (MinSRTMatrix is templated over TenElemT, minsr_tmatrix.h:38-150), a real one computes
// only the upper tiles of a diagonal block.
// Row blocks keep the 32-bit element offsets of the tensor GEMM in range (a sample is n elements long); the K index is split over the
// batch dimension of the launch so that a few hundred samples still fill the chip (split-K).  Every block is handed to
// sum(part, split, ni, nj, ib, jb) as its [split][ni][nj] partial results (kOut doubles each) in HBM.
template <typename T>
template <typename Sum>
void Engine<T>::sr_gram_walk(const void *remote_o, const int32_t *remote_cfg, int nb, Sum &&sum) {
  const int sites = Ly_ * Lx_;
  const long n = (long)sites * dp_ * slot_;
  const long lim = kCplx ? (1l << 30) : (1l << 31);
  PG_REQUIRE(n < lim, 1, "sr_gram: parameter count exceeds the 32-bit strides of the tensor GEMM");
  const int bs = (int)std::min<long>(1024, (lim - 1) / n) & ~63;
  PG_REQUIRE(bs >= 64, 1, "sr_gram: parameter count too large for the blocked Gram");
  auto expand = [&](const T *o, const int *cfg, int cnt, T *buf) {
    hipLaunchKernelGGL(sr_expand_kernel<T>, dim3((unsigned)((slot_ + 255) / 256), sites, cnt), dim3(256), 0, stream_, o, cfg, buf,
                       sites, slot_, dp_, (const int *)sr_ne_);
    PG_CHECK_HIP(hipGetLastError());
  };
  ArenaBuf<T> ea(arena_, (size_t)sr_n_ * n), er(arena_, remote_o ? (size_t)nb * n : 0);
  expand((const T *)sr_o_, (const int *)sr_cfg_, sr_n_, ea);
  if (remote_o) expand((const T *)remote_o, (const int *)remote_cfg, nb, er);
  const T *eb = remote_o ? er : ea;
  const int groups = sites * dp_;                       // K splits must keep whole (site, state) slots together
  for (int ib = 0; ib < sr_n_; ib += bs) {
    const int ni = std::min(bs, sr_n_ - ib);
    for (int jb = remote_o ? 0 : ib; jb < nb; jb += bs) {
      const int nj = std::min(bs, nb - jb);
      const long tiles = (long)((ni + 63) / 64) * ((nj + 63) / 64);
      int split = 1;
      for (int c = 1; c <= groups; ++c)
        if (groups % c == 0 && tiles * c <= 2048) split = c;
      const long chunk = n / split;
      ArenaBuf<double> d(arena_, (size_t)split * ni * nj * kOut);
      PG_CHECK_HIP(hipMemsetAsync(d, 0, sizeof(double) * (size_t)split * ni * nj * kOut, stream_));
      TGemmDesc g;
      g.I[2] = ni; g.sAi[2] = (int)n; g.sCi[2] = nj;
      g.K[2] = (int)chunk; g.sAk[2] = 1; g.sBk[2] = 1;
      g.J[2] = nj; g.sBj[2] = (int)n; g.sCj[2] = 1;
      g.wA = chunk; g.wB = chunk; g.wC = (long)ni * nj;
      g.nbatch = split;
      if constexpr (kCplx) {
        g.conjA = 1;
        tgemm_launch<T, T, T, T>(stream_, g, (const T *)ea + (size_t)ib * n, eb + (size_t)jb * n, (T *)(double *)d);
      } else {
        g.upper_only = (!remote_o && ib == jb) ? 1 : 0;
        tgemm_launch<T, T, double, double>(stream_, g, (const T *)ea + (size_t)ib * n, eb + (size_t)jb * n, (double *)d);
      }
      sum((const double *)d, split, ni, nj, ib, jb);
    }
  }
  PG_CHECK_HIP(hipStreamSynchronize(stream_));      // (the blocks go back to the arena here)
}

// out = [sr_n_][nb] entries of kOut doubles; the partial blocks are summed on the host in f64, in split order
template <typename T>
void Engine<T>::sr_gram(const void *remote_o, const int32_t *remote_cfg, int n_remote, double *out) {
  PG_REQUIRE(sr_o_ != nullptr && sr_n_ > 0, 3, "sr_gram: no samples");
  PG_REQUIRE(!remote_o || (remote_cfg && n_remote > 0), 1, "sr_gram: bad remote batch");
  const int nb = remote_o ? n_remote : sr_n_;
  std::vector<double> h((size_t)kOut * sr_n_ * nb, 0.0), part;
  sr_gram_walk(remote_o, remote_cfg, nb, [&](const double *d, int split, int ni, int nj, int ib, int jb) {
    part.resize((size_t)kOut * split * ni * nj);
    PG_CHECK_HIP(hipMemcpyAsync(part.data(), d, sizeof(double) * part.size(), hipMemcpyDeviceToHost, stream_));
    PG_CHECK_HIP(hipStreamSynchronize(stream_));
    for (int sp = 0; sp < split; ++sp)
      for (int i2 = 0; i2 < ni; ++i2) {
        const double *src = &part[kOut * (((size_t)sp * ni + i2) * nj)];
        double *dst = &h[kOut * ((size_t)(ib + i2) * nb + jb)];
        for (int j2 = 0; j2 < kOut * nj; ++j2) dst[j2] += src[j2];
      }
  });
  if (!remote_o)   // blocks below the diagonal were not computed: ip_ij = conj(ip_ji); ip_ii = sum |O*_i|^2 is real
    for (int i2 = 0; i2 < sr_n_; ++i2) {
      if (kCplx) h[2 * ((size_t)i2 * nb + i2) + 1] = 0.0;
      for (int j2 = 0; j2 < i2; ++j2) {
        h[kOut * ((size_t)i2 * nb + j2)] = h[kOut * ((size_t)j2 * nb + i2)];
        if (kCplx) h[2 * ((size_t)i2 * nb + j2) + 1] = -h[2 * ((size_t)j2 * nb + i2) + 1];
      }
    }
  std::copy(h.begin(), h.end(), out);
}

// g[ib + i][jb + j] = sum over the K splits of one Gram block, in the order the host loop of sr_gram adds them, for the entries on and
// above the diagonal; the entry below is its conjugate, a diagonal entry is real.  Z doubles per entry.
template <int Z>
__global__ __launch_bounds__(256) void sr_gram_reduce_kernel(const double *__restrict__ part, int split, int ni, int nj, int ib, int jb,
                                                             int ns, double *__restrict__ g) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)ni * nj) return;
  const int i = ib + (int)(e / nj), j = jb + (int)(e % nj);
  if (i > j) return;
  double acc[Z];
  for (int z = 0; z < Z; ++z) acc[z] = 0.0;
  for (int sp = 0; sp < split; ++sp)
    for (int z = 0; z < Z; ++z) acc[z] += part[Z * ((long)sp * ni * nj + e) + z];
  if (Z == 2 && i == j) acc[Z - 1] = 0.0;
  for (int z = 0; z < Z; ++z) g[Z * ((long)i * ns + j) + z] = acc[z];
  if (i != j) {
    g[Z * ((long)j * ns + i)] = acc[0];
    if (Z == 2) g[Z * ((long)j * ns + i) + 1] = -acc[Z - 1];
  }
}

// sr_gram of the local store against itself with the result left in HBM: the partial blocks summed by sr_gram_reduce_kernel in
// place of the host loop.  g = [sr_n_][sr_n_] doubles (interleaved pairs on a complex context).
template <typename T>
void Engine<T>::sr_gram_device(double *g) {
  PG_REQUIRE(sr_o_ != nullptr && sr_n_ > 0, 3, "sr_gram: no samples");
  sr_gram_walk(nullptr, nullptr, sr_n_, [&](const double *d, int split, int ni, int nj, int ib, int jb) {
    hipLaunchKernelGGL(sr_gram_reduce_kernel<kOut>, dim3((unsigned)(((long)ni * nj + 255) / 256)), dim3(256), 0, stream_, d, split, ni,
                       nj, ib, jb, sr_n_, g);
    PG_CHECK_HIP(hipGetLastError());
  });
}

// sum_i y_i O*_i, weights of the element type (complex: interleaved pairs in, interleaved pairs out)
template <typename T>
void Engine<T>::sr_weighted_sum(const double *y, double *out) {
  PG_REQUIRE(sr_o_ != nullptr && sr_n_ > 0, 3, "sr_weighted_sum: no samples");
  const int sites = Ly_ * Lx_;
  const size_t n = (size_t)sites * dp_ * slot_ * kOut;
  PG_CHECK_HIP(hipMemcpyAsync(sr_delta_, y, sizeof(double) * kOut * sr_n_, hipMemcpyHostToDevice, stream_));
  hipLaunchKernelGGL(sr_accum_kernel<T>, dim3((unsigned)((slot_ + 255) / 256), sites), dim3(256), 0, stream_, (const T *)sr_o_,
                     (const int *)sr_cfg_, (const double *)sr_delta_, 1.0, sr_out_, sr_n_, sites, slot_, dp_);
  PG_CHECK_HIP(hipGetLastError());
  std::vector<double> h(n);
  PG_CHECK_HIP(hipMemcpyAsync(h.data(), sr_out_, n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  sr_convert(h.data(), out, false);
}

// device-to-device copy of the local sample store (for torch.distributed send / recv of the ring exchange)
template <typename T>
void Engine<T>::sr_copy_samples(void *dst_o, int32_t *dst_cfg) {
  PG_REQUIRE(sr_o_ != nullptr && sr_n_ > 0, 3, "sr_copy_samples: no samples");
  const size_t sites = (size_t)Ly_ * Lx_;
  PG_CHECK_HIP(hipMemcpyAsync(dst_o, sr_o_, sizeof(T) * (size_t)sr_n_ * sites * slot_, hipMemcpyDeviceToDevice, stream_));
  PG_CHECK_HIP(hipMemcpyAsync(dst_cfg, sr_cfg_, sizeof(int) * (size_t)sr_n_ * sites, hipMemcpyDeviceToDevice, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
}

}  // namespace pepsgpu

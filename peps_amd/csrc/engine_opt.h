// Device-resident optimisation step (the first-order update rules of optimizer/optimizer_impl.h and the one-rank SR step):
// master parameters theta, the gradient / direction g and the rule state live in HBM in the layout of the accumulators
// S_O / S_EO ([row][col][s][D^4 slot], compact inside the slot, float64 or interleaved complex float64), so that
// "evaluate -> finish -> clip -> [natural gradient] -> step" never moves a tensor over PCIe.  Every kernel is element-wise and
// memory bound; the unused tail of a slot is never touched and stays exactly zero in every buffer.
//   begin     theta <- double(sitps_), rule state cleared
//   finish    g <- (S_EO - conj(E) S_O) / W                              GradAccumulatorT::Finish, exact_summation_energy_evaluator.h:286-295
//   norm      sum |g|^2 in two stages of fixed order (no atomics)        SplitIndexTPS::NormSquare
//   clip      element-wise, then global norm                             optimizer_impl.h:311-316, split_index_tps_impl.h:566-580
//   step      SGD (:949-990), AdaGrad (:1252-1307), Adam (:1327-1396): one fused pass that also writes sitps_ = T(theta)
//   scale     theta *= f, sitps_ = T(theta)                              NormalizeStateOrder1, monte_carlo_engine.h:206-240
//   (the base of a step -- save, restore, SGD preview -- for the spike rollback and the step selectors: engine_guard.h)
// ElementWiseInv(eps) is taken as 1 / (x + eps) in both AdaGrad and Adam ("Unpinned").
//
// Fermionic states (pepsgpu_fermion_decoration_set): the device holds 4 d decorated components per site, T''[s + d var] =
// sigma_var * T[s] =: E T.  Every optimizer vector stays in that extended layout and in the range of E, so the element-wise rule
// kernels above run unchanged (negating theta, g, velocity and m1 negates their results exactly; m2 and acc see |g|^2): a step on
// (E theta, Pi g_ext) is bit for bit E of the step on (theta, E^T g_ext), Pi = E mask E^T.  New for fermions: the sign table, Pi
// (alone and fused into the finish), the check at begin, the stored norm = 1/2 extended norm (E^T E = 4 mask), the SR hook.
//
// MinSR (minsr_direction): Optimizer::CalculateMinSRDirection_ on one rank (optimizer_impl.h:1126-1215, minsr_tmatrix.h:53-147,
// minsr_eigensolve.h:44-155) with everything that scales with Ns^2 or with the parameter count in HBM: raw Gram of the resident O*
// store -> four-term centering and 1 / Ns -> Jacobi eigensolver (eigh_jacobi.h) -> pseudo-inverse cutoff -> y = Z f(w) Z^H eps_bar ->
// g <- sum_i y_i O*_i - (sum_i y_i) (sum_i O*_i) / Ns.  The host sees the Ns local energies on the way in and four scalars on the way out.
#pragma once
#include "engine_sr.h"
#include "eigh_jacobi.h"

namespace pepsgpu {

enum { OPT_SGD = 0, OPT_ADAGRAD = 1, OPT_ADAM = 2 };

// scalars of one step, by value
struct OptStepArgs {
  double lr;
  double decay;          // 1 - lr * weight_decay (SGD, Adam); 1: no decay
  double mu;             // SGD momentum
  int nesterov;          // SGD
  double eps;            // AdaGrad, Adam
  double b1, b2;         // Adam
  double inv_bc1, inv_bc2;   // Adam: 1 / (1 - beta^t)
};

template <typename T> __device__ __forceinline__ void opt_store_state(T *s, long k, const double *th) { s[k] = T(th[0]); }
template <> __device__ __forceinline__ void opt_store_state<c128>(c128 *s, long k, const double *th) { s[k] = c128(th[0], th[1]); }
template <typename T> __device__ __forceinline__ void opt_load_state(const T *s, long k, double *th) { th[0] = (double)s[k]; }
template <> __device__ __forceinline__ void opt_load_state<c128>(const c128 *s, long k, double *th) { th[0] = s[k].re; th[1] = s[k].im; }

// Every element-wise kernel below: grid (ceil(slot / 256), sites * dp), one thread per element of one slot; only the live
// elements (e < ne[site]) are read or written.
#define OPT_ELEM_PROLOGUE                                                 \
  const int q = blockIdx.y;                                               \
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;             \
  if (e >= ne[q / dp]) return;                                            \
  const long k = (long)q * slot + e;

// theta <- double(sitps_)
template <typename T>
__global__ __launch_bounds__(256) void opt_begin_kernel(const T *__restrict__ sitps, double *__restrict__ theta,
                                                        const int *__restrict__ ne, long slot, int dp) {
  constexpr int Z = is_cplx<T>::value ? 2 : 1;
  OPT_ELEM_PROLOGUE
  double th[Z];
  opt_load_state<T>(sitps, k, th);
  for (int z = 0; z < Z; ++z) theta[Z * k + z] = th[z];
}

// g <- (S_EO - conj(E) S_O) / W        (e_im = -Im E: the conjugate is taken by the caller)
template <int Z>
__global__ __launch_bounds__(256) void opt_finish_kernel(const double *__restrict__ so, const double *__restrict__ seo,
                                                         double e_re, double ec_im, double w, double *__restrict__ g,
                                                         const int *__restrict__ ne, long slot, int dp) {
#pragma clang fp contract(off)
  OPT_ELEM_PROLOGUE
  if constexpr (Z == 1) {
    g[k] = (seo[k] - e_re * so[k]) / w;
  } else {
    const double sr = so[2 * k], si = so[2 * k + 1];
    g[2 * k] = (seo[2 * k] - (e_re * sr - ec_im * si)) / w;
    g[2 * k + 1] = (seo[2 * k + 1] - (e_re * si + ec_im * sr)) / w;
  }
}

// element-wise clip: real sign(x) min(|x|, c); complex x min(1, c / |x|)
template <int Z>
__global__ __launch_bounds__(256) void opt_clip_value_kernel(double *__restrict__ g, double c, const int *__restrict__ ne,
                                                             long slot, int dp) {
#pragma clang fp contract(off)
  OPT_ELEM_PROLOGUE
  if constexpr (Z == 1) {
    const double x = g[k];
    if (fabs(x) > c) g[k] = copysign(c, x);
  } else {
    const double xr = g[2 * k], xi = g[2 * k + 1];
    const double a = hypot(xr, xi);
    if (a > c) {
      const double f = c / a;
      g[2 * k] = xr * f; g[2 * k + 1] = xi * f;
    }
  }
}

// x *= f on the live elements (global-norm clip of g; with a state pointer: theta *= f, sitps_ = T(theta))
template <typename T, bool kState>
__global__ __launch_bounds__(256) void opt_scale_kernel(double *__restrict__ x, double f, T *__restrict__ sitps,
                                                        const int *__restrict__ ne, long slot, int dp) {
  constexpr int Z = is_cplx<T>::value ? 2 : 1;
  OPT_ELEM_PROLOGUE
  double th[Z];
  for (int z = 0; z < Z; ++z) { th[z] = x[Z * k + z] * f; x[Z * k + z] = th[z]; }
  if constexpr (kState) opt_store_state<T>(sitps, k, th);
}

// acc <- value on the live elements (AdaGrad: initial_accumulator_value)
__global__ __launch_bounds__(256) void opt_fill_kernel(double *__restrict__ x, double v, const int *__restrict__ ne, long slot,
                                                       int dp) {
  OPT_ELEM_PROLOGUE
  x[k] = v;
}

// ---- fermionic decoration: one byte per (site, stored state, element), bits 0-3 = sign bits of the variants, bit 4 = allowed ----
// Grid (ceil(slot / 256), sites * d): one thread per stored element, which owns its four decorated copies.
#define OPT_FERMION_PROLOGUE                                              \
  const int q = blockIdx.y;                                               \
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;             \
  const int site = q / d, s = q - site * d;                               \
  if (e >= ne[site]) return;                                              \
  const unsigned b = sign[(long)q * slot + e];                            \
  const long k0 = ((long)site * 4 * d + s) * slot + e, dk = (long)d * slot;

// t = allowed * sum_var sigma_var x_var (var = 0, 1, 2, 3 in this order), x_var <- sigma_var t
template <int Z>
__device__ __forceinline__ void opt_fermion_project_elem(double (*x)[Z], unsigned b) {
#pragma clang fp contract(off)
  for (int z = 0; z < Z; ++z) {
    double t = 0.0;
    for (int var = 0; var < 4; ++var) t += ((b >> var) & 1u) ? -x[var][z] : x[var][z];
    if (!(b & 16u)) t = 0.0;
    for (int var = 0; var < 4; ++var) x[var][z] = ((b >> var) & 1u) ? -t : t;
  }
}

// x <- Pi x in place
template <int Z>
__global__ __launch_bounds__(256) void opt_fermion_project_kernel(double *__restrict__ x, const uint8_t *__restrict__ sign,
                                                                  const int *__restrict__ ne, long slot, int d) {
#pragma clang fp contract(off)
  OPT_FERMION_PROLOGUE
  double v[4][Z];
  for (int var = 0; var < 4; ++var)
    for (int z = 0; z < Z; ++z) v[var][z] = x[Z * (k0 + var * dk) + z];
  opt_fermion_project_elem<Z>(v, b);
  for (int var = 0; var < 4; ++var)
    for (int z = 0; z < Z; ++z) x[Z * (k0 + var * dk) + z] = v[var][z];
}

// g <- Pi (S_EO - conj(E) S_O) / W: the finish of the four variants and the projection in one pass (8 reads, 4 writes)
template <int Z>
__global__ __launch_bounds__(256) void opt_finish_fermion_kernel(const double *__restrict__ so, const double *__restrict__ seo,
                                                                 double e_re, double ec_im, double w, double *__restrict__ g,
                                                                 const uint8_t *__restrict__ sign, const int *__restrict__ ne,
                                                                 long slot, int d) {
#pragma clang fp contract(off)
  OPT_FERMION_PROLOGUE
  double v[4][Z];
  for (int var = 0; var < 4; ++var) {
    const long k = k0 + var * dk;
    if constexpr (Z == 1) {
      v[var][0] = (seo[k] - e_re * so[k]) / w;
    } else {
      const double sr = so[2 * k], si = so[2 * k + 1];
      v[var][0] = (seo[2 * k] - (e_re * sr - ec_im * si)) / w;
      v[var][1] = (seo[2 * k + 1] - (e_re * si + ec_im * sr)) / w;
    }
  }
  opt_fermion_project_elem<Z>(v, b);
  for (int var = 0; var < 4; ++var)
    for (int z = 0; z < Z; ++z) g[Z * (k0 + var * dk) + z] = v[var][z];
}

// the check at begin: out[0] += number of stored elements with theta != Pi(theta) / 4 in any copy, out[1] = min of their sites.
// For a decorated state the comparison is exact: the copies differ by sign flips only and forbidden entries are exactly zero.
template <int Z>
__global__ __launch_bounds__(256) void opt_fermion_check_kernel(const double *__restrict__ theta, const uint8_t *__restrict__ sign,
                                                                const int *__restrict__ ne, long slot, int d, int *__restrict__ out) {
#pragma clang fp contract(off)
  OPT_FERMION_PROLOGUE
  double v[4][Z], p[4][Z];
  for (int var = 0; var < 4; ++var)
    for (int z = 0; z < Z; ++z) p[var][z] = v[var][z] = theta[Z * (k0 + var * dk) + z];
  opt_fermion_project_elem<Z>(p, b);
  bool bad = false;
  for (int var = 0; var < 4; ++var)
    for (int z = 0; z < Z; ++z) bad = bad || !(v[var][z] == 0.25 * p[var][z]);
  if (bad) {
    atomicAdd(out, 1);
    atomicMin(out + 1, site);
  }
}
#undef OPT_FERMION_PROLOGUE

// One double of the SGD rule (:949-990): the new theta from (theta, g, velocity); with momentum *vel_new is the new velocity.
// The rule acts on the real and the imaginary part alike.  opt_step_kernel<T, OPT_SGD> stores the velocity, the preview of
// engine_guard.h (SGDPreviewUpdate_, :1001) drops it: the arithmetic of the two is this one function.
__device__ __forceinline__ double opt_sgd_elem(const OptStepArgs &a, double th, double gz, double vel, double *vel_new) {
#pragma clang fp contract(off)
  if (a.decay != 1.0) th *= a.decay;
  double upd = gz;
  if (a.mu > 0.0) {
    const double v = a.mu * vel + gz;
    *vel_new = v;
    upd = a.nesterov ? a.mu * v + gz : v;
  }
  th += (-a.lr) * upd;
  return th;
}

// One fused pass per rule: reads theta, g and the rule's state, writes theta, the state and sitps_ = T(theta).
// s1 = velocity (SGD) / m1 (Adam), element type; s2 = acc (AdaGrad) / m2 (Adam), real.
// Contraction into fused multiply-adds is off: the result is the separately rounded arithmetic of the host restatement.
template <typename T, int RULE>
__global__ __launch_bounds__(256) void opt_step_kernel(OptStepArgs a, double *__restrict__ theta, const double *__restrict__ g,
                                                       double *__restrict__ s1, double *__restrict__ s2, T *__restrict__ sitps,
                                                       const int *__restrict__ ne, long slot, int dp) {
#pragma clang fp contract(off)
  constexpr int Z = is_cplx<T>::value ? 2 : 1;
  OPT_ELEM_PROLOGUE
  double th[Z], gz[Z];
  double g2 = 0.0;
  for (int z = 0; z < Z; ++z) {
    th[z] = theta[Z * k + z];
    gz[z] = g[Z * k + z];
    g2 += gz[z] * gz[z];
  }
  if constexpr (RULE == OPT_SGD) {
    for (int z = 0; z < Z; ++z) {
      double v = 0.0;
      th[z] = opt_sgd_elem(a, th[z], gz[z], a.mu > 0.0 ? s1[Z * k + z] : 0.0, &v);
      if (a.mu > 0.0) s1[Z * k + z] = v;
    }
  } else if constexpr (RULE == OPT_ADAGRAD) {
    const double acc = s2[k] + g2;
    s2[k] = acc;
    const double rate = 1.0 / (sqrt(acc) + a.eps);
    for (int z = 0; z < Z; ++z) th[z] += -((rate * gz[z]) * a.lr);
  } else {
    const double m2 = a.b2 * s2[k] + (1.0 - a.b2) * g2;
    s2[k] = m2;
    const double den = 1.0 / (sqrt(a.inv_bc2 * m2) + a.eps);
    for (int z = 0; z < Z; ++z) {
      if (a.decay != 1.0) th[z] *= a.decay;
      const double m1 = a.b1 * s1[Z * k + z] + (1.0 - a.b1) * gz[z];
      s1[Z * k + z] = m1;
      th[z] += -((den * (a.inv_bc1 * m1)) * a.lr);
    }
  }
  for (int z = 0; z < Z; ++z) theta[Z * k + z] = th[z];
  opt_store_state<T>(sitps, k, th);
}

// ---------------------------------------------------------------------------------------------
template <typename T>
void Engine<T>::opt_release() {
  lbfgs_release();      // (engine_lbfgs.h: its vectors have the extents of these)
  for (double *p : {opt_theta_, opt_g_, opt_vel_, opt_m1_, opt_m2_, opt_acc_, opt_part_}) arena_.free(p);
  arena_.free(opt_ne_);
  arena_.free(opt_sign_);
  arena_.free(vmc_snap_);
  vmc_snap_ = nullptr;
  arena_.free(opt_base_);
  opt_base_ = nullptr;
  opt_base_saved_ = false;
  for (double *p : {minsr_t_, minsr_v_, minsr_work_}) arena_.free(p);
  minsr_t_ = minsr_v_ = minsr_work_ = nullptr;
  minsr_cap_ = 0;
  opt_theta_ = opt_g_ = opt_vel_ = opt_m1_ = opt_m2_ = opt_acc_ = opt_part_ = nullptr;
  opt_ne_ = nullptr;
  opt_sign_ = nullptr;
  opt_t_ = 0;
  opt_acc_ready_ = false;
}

template <typename T>
void Engine<T>::opt_begin() {
  PG_REQUIRE(have_state_, 3, "opt_begin: no state uploaded (pepsgpu_state_upload)");
  const int sites = Ly_ * Lx_;
  PG_REQUIRE((long)sites * dp_ <= 65535, 1, "opt_begin: rows * cols * phys_dim exceeds the grid y limit");
  opt_release();
  layout_maps();
  try {
  const size_t n = (size_t)sites * dp_ * slot_;
  opt_theta_ = (double *)arena_.alloc(sizeof(double) * n * kOut);
  opt_g_ = (double *)arena_.alloc(sizeof(double) * n * kOut);
  opt_vel_ = (double *)arena_.alloc(sizeof(double) * n * kOut);
  opt_m1_ = (double *)arena_.alloc(sizeof(double) * n * kOut);
  opt_m2_ = (double *)arena_.alloc(sizeof(double) * n);
  opt_acc_ = (double *)arena_.alloc(sizeof(double) * n);
  opt_part_ = (double *)arena_.alloc(sizeof(double) * (kOptDotBlocks + 8));
  opt_ne_ = (int *)arena_.alloc(sizeof(int) * (sites + 2));
  std::vector<int> ne(sites + 2);
  ne[sites] = 0; ne[sites + 1] = sites;          // the check's count and first offending site
  for (int r = 0; r < Ly_; ++r)
    for (int c = 0; c < Lx_; ++c) {
      int dd[4];
      site_dims(r, c, dd);
      ne[r * Lx_ + c] = dd[0] * dd[1] * dd[2] * dd[3];
    }
  PG_CHECK_HIP(hipMemcpyAsync(opt_ne_, ne.data(), sizeof(int) * (sites + 2), hipMemcpyHostToDevice, stream_));
  std::vector<uint8_t> sign;                     // (a host temporary too)
  if (fd_d_ > 0) {
    sign = fermion_sign_table();
    opt_sign_ = (uint8_t *)arena_.alloc(sign.size());
    PG_CHECK_HIP(hipMemcpyAsync(opt_sign_, sign.data(), sign.size(), hipMemcpyHostToDevice, stream_));
  }
  for (double *p : {opt_theta_, opt_g_, opt_vel_, opt_m1_}) PG_CHECK_HIP(hipMemsetAsync(p, 0, sizeof(double) * n * kOut, stream_));
  for (double *p : {opt_m2_, opt_acc_}) PG_CHECK_HIP(hipMemsetAsync(p, 0, sizeof(double) * n, stream_));
  hipLaunchKernelGGL(opt_begin_kernel<T>, opt_grid(), dim3(256), 0, stream_, (const T *)sitps_, opt_theta_, (const int *)opt_ne_,
                     slot_, dp_);
  PG_CHECK_HIP(hipGetLastError());
  if (fd_d_ > 0) {
    hipLaunchKernelGGL(opt_fermion_check_kernel<kOut>, opt_fermion_grid(), dim3(256), 0, stream_, (const double *)opt_theta_,
                       (const uint8_t *)opt_sign_, (const int *)opt_ne_, slot_, fd_d_, opt_ne_ + sites);
    PG_CHECK_HIP(hipGetLastError());
    int bad[2] = {0, 0};
    PG_CHECK_HIP(hipMemcpyAsync(bad, opt_ne_ + sites, sizeof(bad), hipMemcpyDeviceToHost, stream_));
    PG_CHECK_HIP(hipStreamSynchronize(stream_));
    if (bad[0] != 0)
      throw Error(1, "opt_begin: the device state is not the decoration of a parity-even state: " + std::to_string(bad[0]) +
                         " stored elements differ from Pi(theta) / 4, the first at site (" + std::to_string(bad[1] / Lx_) + ", " +
                         std::to_string(bad[1] % Lx_) + ")");
  }
  PG_CHECK_HIP(hipStreamSynchronize(stream_));   // (ne is a host temporary)
  } catch (...) {
    opt_release();
    throw;
  }
}

template <typename T>
void Engine<T>::opt_end() {
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  opt_release();
}

// sum |x|^2 over the n * kOut doubles of an optimizer vector: per-block partial sums, then one wave adds them in a fixed order
template <typename T>
double Engine<T>::opt_norm_sq(const double *x) {
  const long n = (long)Ly_ * Lx_ * dp_ * slot_ * kOut;
  hipLaunchKernelGGL(sr_dot_kernel<1>, dim3(kOptDotBlocks), dim3(256), 0, stream_, x, x, n, opt_part_);
  hipLaunchKernelGGL(sr_dot_final_kernel<1>, dim3(1), dim3(64), 0, stream_, (const double *)opt_part_, (int)kOptDotBlocks,
                     opt_part_ + kOptDotBlocks);
  PG_CHECK_HIP(hipGetLastError());
  double out = 0.0;
  PG_CHECK_HIP(hipMemcpyAsync(&out, opt_part_ + kOptDotBlocks, sizeof(double), hipMemcpyDeviceToHost, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  return fd_d_ > 0 ? 0.25 * out : out;      // a vector in the range of E: stored norm^2 = extended norm^2 / 4 (E^T E = 4 mask)
}

template <typename T>
void Engine<T>::opt_fermion_project(double *x) {
  hipLaunchKernelGGL(opt_fermion_project_kernel<kOut>, opt_fermion_grid(), dim3(256), 0, stream_, x, (const uint8_t *)opt_sign_,
                     (const int *)opt_ne_, slot_, fd_d_);
  PG_CHECK_HIP(hipGetLastError());
}

// the sign table of opt_sign_ from nf and the bond parities, in the compact [L][D][R][U] element order of layout_maps()
template <typename T>
std::vector<uint8_t> Engine<T>::fermion_sign_table() const {
  const int sites = Ly_ * Lx_, d = fd_d_;
  std::vector<uint8_t> tab((size_t)sites * d * slot_, 0);
  for (int r = 0; r < Ly_; ++r)
    for (int c = 0; c < Lx_; ++c) {
      int dd[4];
      site_dims(r, c, dd);
      const uint8_t *par = fd_par_.data() + (size_t)(r * Lx_ + c) * 4 * D_;
      for (int s = 0; s < d; ++s) {
        uint8_t *row = tab.data() + ((size_t)(r * Lx_ + c) * d + s) * slot_;
        const int n = fd_nf_[s] & 1;
        size_t o = 0;
        for (int a = 0; a < dd[0]; ++a)
          for (int b = 0; b < dd[1]; ++b)
            for (int cc = 0; cc < dd[2]; ++cc)
              for (int e = 0; e < dd[3]; ++e, ++o) {
                const int l = par[a], dn = par[D_ + b], rr = par[2 * D_ + cc], u = par[3 * D_ + e];
                const int base = (u * n + u + dn * rr + l + l * u) & 1;
                const int allowed = ((l + dn + rr + u + n) & 1) == 0;
                row[o] = (uint8_t)((u << 1) | (base << 2) | (((base + l) & 1) << 3) | (allowed << 4));
              }
      }
    }
  return tab;
}

template <typename T>
void Engine<T>::fermion_decoration_set(int d, const int32_t *nf, const uint8_t *bond_parity) {
  PG_REQUIRE(opt_theta_ == nullptr, 1, "fermion_decoration_set: optimizer buffers exist (pepsgpu_opt_end first)");
  PG_REQUIRE(d >= 0, 1, "fermion_decoration_set: negative d");
  if (d == 0) { fd_d_ = 0; fd_nf_.clear(); fd_par_.clear(); return; }
  PG_REQUIRE(nf != nullptr && bond_parity != nullptr, 1, "fermion_decoration_set: null argument");
  PG_REQUIRE(dp_ == 4 * d, 1, "fermion_decoration_set: the context's phys_dim must be 4 * d (the decorated components)");
  for (int r = 0; r < Ly_; ++r)
    for (int c = 0; c < Lx_; ++c) {
      int dd[4];
      site_dims(r, c, dd);
      for (int leg = 0; leg < 4; ++leg)
        for (int i = 0; i < dd[leg]; ++i)
          PG_REQUIRE(bond_parity[((size_t)(r * Lx_ + c) * 4 + leg) * D_ + i] <= 1, 1, "fermion_decoration_set: a bond parity outside {0, 1}");
    }
  fd_d_ = d;
  fd_nf_.assign(nf, nf + d);
  fd_par_.assign(bond_parity, bond_parity + (size_t)Ly_ * Lx_ * 4 * D_);
}

template <typename T>
void Engine<T>::opt_gradient_from_accumulators(const double *e_loc_sum, double weight_sum, double *energy_out, double *grad_norm_out) {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "opt_gradient_from_accumulators: call pepsgpu_opt_begin first");
  PG_REQUIRE(so_ != nullptr, 3, "opt_gradient_from_accumulators: nothing accumulated");
  PG_REQUIRE(std::isfinite(weight_sum) && weight_sum > 0.0, 1, "opt_gradient_from_accumulators: weight_sum must be positive");
  for (int z = 0; z < kOut; ++z) PG_REQUIRE(std::isfinite(e_loc_sum[z]), 1, "opt_gradient_from_accumulators: non-finite e_loc_sum");
  const double e_re = e_loc_sum[0] / weight_sum, e_im = kCplx ? e_loc_sum[1] / weight_sum : 0.0;
  if (fd_d_ > 0)
    hipLaunchKernelGGL(opt_finish_fermion_kernel<kOut>, opt_fermion_grid(), dim3(256), 0, stream_, (const double *)so_,
                       (const double *)seo_, e_re, -e_im, weight_sum, opt_g_, (const uint8_t *)opt_sign_, (const int *)opt_ne_, slot_, fd_d_);
  else
    hipLaunchKernelGGL(opt_finish_kernel<kOut>, opt_grid(), dim3(256), 0, stream_, (const double *)so_, (const double *)seo_, e_re, -e_im,
                       weight_sum, opt_g_, (const int *)opt_ne_, slot_, dp_);
  PG_CHECK_HIP(hipGetLastError());
  const double nsq = opt_norm_sq(opt_g_);
  if (energy_out) { energy_out[0] = e_re; if (kCplx) energy_out[1] = e_im; }
  if (grad_norm_out) *grad_norm_out = std::sqrt(nsq);
}

template <typename T>
void Engine<T>::opt_set_gradient(const double *host) {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "opt_set_gradient: call pepsgpu_opt_begin first");
  const size_t n = (size_t)Ly_ * Lx_ * dp_ * slot_ * kOut;
  std::vector<double> h(n);
  sr_convert(host, h.data(), true);
  PG_CHECK_HIP(hipMemcpyAsync(opt_g_, h.data(), n * sizeof(double), hipMemcpyHostToDevice, stream_));
  if (fd_d_ > 0) opt_fermion_project(opt_g_);      // the derivative with respect to the extended components -> Pi g
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
}

template <typename T>
void Engine<T>::opt_read(const double *dev, double *host) {
  const size_t n = (size_t)Ly_ * Lx_ * dp_ * slot_ * kOut;
  std::vector<double> h(n);
  PG_CHECK_HIP(hipMemcpyAsync(h.data(), dev, n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  sr_convert(h.data(), host, false);
}
template <typename T>
void Engine<T>::opt_get_gradient(double *host) {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "opt_get_gradient: call pepsgpu_opt_begin first");
  opt_read(opt_g_, host);
}
template <typename T>
void Engine<T>::opt_read_state(double *host) {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "opt_read_state: call pepsgpu_opt_begin first");
  opt_read(opt_theta_, host);
}

// The parameters of the lowest energy so far (vmc_peps_optimizer_impl.h:118-121, tps_lowest_ = state) without a host hop: theta is
// copied device to device into a buffer of its own, which lives until opt_end / a new opt_begin / the context goes.
template <typename T>
void Engine<T>::vmc_snapshot_save() {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "vmc_snapshot_save: call pepsgpu_opt_begin first");
  const size_t bytes = sizeof(double) * (size_t)Ly_ * Lx_ * dp_ * slot_ * kOut;
  double *dst = vmc_snap_ ? vmc_snap_ : (double *)arena_.alloc(bytes);
  PG_CHECK_HIP(hipMemcpyAsync(dst, opt_theta_, bytes, hipMemcpyDeviceToDevice, stream_));
  vmc_snap_ = dst;
}
template <typename T>
void Engine<T>::vmc_snapshot_read(double *host) {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "vmc_snapshot_read: call pepsgpu_opt_begin first");
  PG_REQUIRE(vmc_snap_ != nullptr, 3, "vmc_snapshot_read: no snapshot (pepsgpu_vmc_snapshot_save)");
  opt_read(vmc_snap_, host);
}
template <typename T>
void Engine<T>::vmc_snapshot_clear() {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "vmc_snapshot_clear: call pepsgpu_opt_begin first");
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  arena_.free(vmc_snap_);
  vmc_snap_ = nullptr;
}

template <typename T>
void Engine<T>::opt_clip(double clip_value, double clip_norm, double *norm_before_out) {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "opt_clip: call pepsgpu_opt_begin first");
  PG_REQUIRE(!std::isnan(clip_value) && !std::isnan(clip_norm), 1, "opt_clip: NaN bound");
  double r = std::sqrt(opt_norm_sq(opt_g_));
  if (norm_before_out) *norm_before_out = r;
  if (clip_value > 0.0) {
    hipLaunchKernelGGL(opt_clip_value_kernel<kOut>, opt_grid(), dim3(256), 0, stream_, opt_g_, clip_value, (const int *)opt_ne_, slot_, dp_);
    PG_CHECK_HIP(hipGetLastError());
    if (clip_norm > 0.0) r = std::sqrt(opt_norm_sq(opt_g_));
  }
  if (clip_norm > 0.0 && r > 0.0 && r > clip_norm) {
    hipLaunchKernelGGL((opt_scale_kernel<T, false>), opt_grid(), dim3(256), 0, stream_, opt_g_, clip_norm / r, (T *)nullptr,
                       (const int *)opt_ne_, slot_, dp_);
    PG_CHECK_HIP(hipGetLastError());
  }
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
}

template <typename T>
void Engine<T>::opt_natural_gradient(double diag_shift, int max_iter, double rel_tol, double abs_tol, int recompute_interval,
                                     double ortho_threshold, double *residual_norm, int *iterations, int *reason,
                                     double *direction_norm_out) {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "opt_natural_gradient: call pepsgpu_opt_begin first");
  PG_REQUIRE(sr_o_ != nullptr && sr_n_ > 0, 3, "opt_natural_gradient: the sample store is empty (pepsgpu_sr_begin / pepsgpu_sr_append)");
  struct DevIO {      // b and x of the solve are this device vector for the length of the call
    double *&slot; DevIO(double *&s, double *p) : slot(s) { slot = p; } ~DevIO() { slot = nullptr; }
  } io(sr_cg_dev_, opt_g_);
  sr_cg_solve(opt_g_, nullptr, diag_shift, max_iter, rel_tol, abs_tol, recompute_interval, ortho_threshold, opt_g_, residual_norm,
              iterations, reason);
  if (direction_norm_out) *direction_norm_out = std::sqrt(opt_norm_sq(opt_g_));
}

// ---- MinSR ----
// m[i] = sum_j G_ij / Ns      (one wave per row)
template <int Z>
__global__ __launch_bounds__(64) void minsr_rowmean_kernel(const double *__restrict__ g, int ns, double *__restrict__ m) {
  const int i = blockIdx.x;
  double acc[Z];
  for (int z = 0; z < Z; ++z) acc[z] = 0.0;
  for (int j = threadIdx.x; j < ns; j += 64)
    for (int z = 0; z < Z; ++z) acc[z] += g[Z * ((long)i * ns + j) + z];
  for (int z = 0; z < Z; ++z) acc[z] = wave_sum(acc[z]);
  if (threadIdx.x == 0)
    for (int z = 0; z < Z; ++z) m[Z * i + z] = acc[z] / ns;
}
// T_ij = (G_ij - m_i - conj(m_j) + c) / Ns in place, c = sum_i m_i / Ns (minsr_tmatrix.h:141-147).  Every block adds c in the same
// fixed order; the entry below the diagonal is written as the conjugate of the one above, so T is exactly Hermitian.
template <int Z>
__global__ __launch_bounds__(256) void minsr_center_kernel(double *__restrict__ g, const double *__restrict__ m, int ns) {
#pragma clang fp contract(off)
  __shared__ double s_red[4][Z];
  double c[Z];
  for (int z = 0; z < Z; ++z) c[z] = 0.0;
  for (int i = threadIdx.x; i < ns; i += 256)
    for (int z = 0; z < Z; ++z) c[z] += m[Z * i + z];
  for (int z = 0; z < Z; ++z) c[z] = wave_sum(c[z]);
  if ((threadIdx.x & 63) == 0)
    for (int z = 0; z < Z; ++z) s_red[threadIdx.x >> 6][z] = c[z];
  __syncthreads();
  for (int z = 0; z < Z; ++z) c[z] = (s_red[0][z] + s_red[1][z] + s_red[2][z] + s_red[3][z]) / ns;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)ns * ns) return;
  const int i = (int)(e / ns), j = (int)(e % ns);
  if (i > j) return;
  const long ij = Z * ((long)i * ns + j), ji = Z * ((long)j * ns + i);
  const double vr = (((g[ij] - m[Z * i]) - m[Z * j]) + c[0]) / ns;
  g[ij] = vr; g[ji] = vr;
  if constexpr (Z == 2) {
    const double vi = i == j ? 0.0 : (((g[ij + 1] - m[2 * i + 1]) + m[2 * j + 1]) + c[1]) / ns;
    g[ij + 1] = vi; g[ji + 1] = -vi;
  }
}
// ApplyPseudoInverseCutoff (minsr_eigensolve.h:44-78) in one block: cutoff = r_pinv max|w| + a_pinv; soft: w^5 / (w^6 + cutoff^6), 0 where
// the denominator is 0; hard: 1 / w where |w| > cutoff.  info = [max|w| (NaN when an eigenvalue is not finite), cutoff, #{|w| > cutoff}]
__global__ __launch_bounds__(256) void minsr_cutoff_kernel(const double *__restrict__ w, int ns, double r_pinv, double a_pinv, int soft,
                                                           double *__restrict__ fw, double *__restrict__ info) {
#pragma clang fp contract(off)
  __shared__ double s_max[256];
  __shared__ int s_cnt[256];
  double mx = 0.0;
  int bad = 0;
  for (int i = threadIdx.x; i < ns; i += 256) {
    const double x = fabs(w[i]);
    if (!(x <= 1.79769313486231570815e308)) bad = 1;
    mx = fmax(mx, x);
  }
  s_max[threadIdx.x] = mx; s_cnt[threadIdx.x] = bad;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) { s_max[threadIdx.x] = fmax(s_max[threadIdx.x], s_max[threadIdx.x + st]); s_cnt[threadIdx.x] |= s_cnt[threadIdx.x + st]; }
    __syncthreads();
  }
  const double lam = s_max[0];
  const int anybad = s_cnt[0];
  __syncthreads();
  const double cutoff = r_pinv * lam + a_pinv;
  const double c2 = cutoff * cutoff, c6 = c2 * c2 * c2;
  int kept = 0;
  for (int i = threadIdx.x; i < ns; i += 256) {
    const double x = w[i];
    double f = 0.0;
    if (soft) {
      const double x2 = x * x, den = x2 * x2 * x2 + c6;
      if (den != 0.0) f = x2 * x2 * x / den;
    } else if (fabs(x) > cutoff) f = 1.0 / x;
    fw[i] = f;
    kept += fabs(x) > cutoff ? 1 : 0;
  }
  s_cnt[threadIdx.x] = kept;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) s_cnt[threadIdx.x] += s_cnt[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) { info[0] = anybad ? nan("") : lam; info[1] = cutoff; info[2] = (double)s_cnt[0]; }
}
// u_k = f(w_k) sum_r conj(Z_rk) eps_bar_r,  eps_bar_r = conj(E_r - E) / Ns (optimizer_impl.h:1139-1146); zt = Z^T, one wave per k
template <int Z>
__global__ __launch_bounds__(64) void minsr_project_kernel(const double *__restrict__ zt, const double *__restrict__ fw,
                                                           const double *__restrict__ eloc, const double *__restrict__ energy, int ns,
                                                           double *__restrict__ u) {
  const int k = blockIdx.x;
  double acc[Z];
  for (int z = 0; z < Z; ++z) acc[z] = 0.0;
  for (int r = threadIdx.x; r < ns; r += 64) {
    const double er = (eloc[Z * r] - energy[0]) / ns, vr = zt[Z * ((long)k * ns + r)];
    if constexpr (Z == 1) acc[0] += vr * er;
    else {
      const double ei = -(eloc[2 * r + 1] - energy[1]) / ns, vi = zt[2 * ((long)k * ns + r) + 1];
      acc[0] += vr * er + vi * ei;
      acc[1] += vr * ei - vi * er;
    }
  }
  for (int z = 0; z < Z; ++z) acc[z] = wave_sum(acc[z]);
  if (threadIdx.x == 0)
    for (int z = 0; z < Z; ++z) u[Z * k + z] = fw[k] * acc[z];
}
// y_r = sum_k Z_rk u_k: one lane per r, lanes along a row of zt
template <int Z>
__global__ __launch_bounds__(256) void minsr_expand_kernel(const double *__restrict__ zt, const double *__restrict__ u, int ns,
                                                          double *__restrict__ y) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= ns) return;
  double acc[Z];
  for (int z = 0; z < Z; ++z) acc[z] = 0.0;
  for (int k = 0; k < ns; ++k) {
    const double vr = zt[Z * ((long)k * ns + r)], ur = u[Z * k];
    if constexpr (Z == 1) acc[0] += vr * ur;
    else {
      const double vi = zt[2 * ((long)k * ns + r) + 1], ui = u[2 * k + 1];
      acc[0] += vr * ur - vi * ui;
      acc[1] += vr * ui + vi * ur;
    }
  }
  for (int z = 0; z < Z; ++z) y[Z * r + z] = acc[z];
}
// out = sum_r y_r      (one wave, fixed order)
template <int Z>
__global__ __launch_bounds__(64) void minsr_ysum_kernel(const double *__restrict__ y, int ns, double *__restrict__ out) {
  double acc[Z];
  for (int z = 0; z < Z; ++z) acc[z] = 0.0;
  for (int r = threadIdx.x; r < ns; r += 64)
    for (int z = 0; z < Z; ++z) acc[z] += y[Z * r + z];
  for (int z = 0; z < Z; ++z) acc[z] = wave_sum(acc[z]);
  if (threadIdx.x == 0)
    for (int z = 0; z < Z; ++z) out[z] = acc[z];
}
// g <- wsum - ysum * osum / Ns on the live elements      (optimizer_impl.h:1196-1212)
template <int Z>
__global__ __launch_bounds__(256) void minsr_combine_kernel(const double *__restrict__ wsum, const double *__restrict__ osum,
                                                            const double *__restrict__ ysum, int ns, double *__restrict__ g,
                                                            const int *__restrict__ ne, long slot, int dp) {
#pragma clang fp contract(off)
  OPT_ELEM_PROLOGUE
  if constexpr (Z == 1) {
    g[k] = wsum[k] - ysum[0] * osum[k] / ns;
  } else {
    const double sr = osum[2 * k], si = osum[2 * k + 1];
    g[2 * k] = wsum[2 * k] - (ysum[0] * sr - ysum[1] * si) / ns;
    g[2 * k + 1] = wsum[2 * k + 1] - (ysum[0] * si + ysum[1] * sr) / ns;
  }
}

template <typename T>
void Engine<T>::minsr_direction(const double *eloc, const double *energy, double r_pinv, double a_pinv, int soft_cutoff,
                                double *direction_norm_out, double *info_out) {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "minsr_direction: call pepsgpu_opt_begin first");
  PG_REQUIRE(fd_d_ == 0, 1, "minsr_direction: not available with a fermionic decoration (T in the stored parameters is not built)");
  PG_REQUIRE(sr_o_ != nullptr && sr_n_ > 0, 3, "minsr_direction: the sample store is empty (pepsgpu_sr_begin / pepsgpu_sr_append)");
  PG_REQUIRE(eloc != nullptr && energy != nullptr, 1, "minsr_direction: null eloc / energy");
  PG_REQUIRE(std::isfinite(r_pinv) && std::isfinite(a_pinv) && r_pinv >= 0.0 && a_pinv >= 0.0, 1,
             "minsr_direction: r_pinv and a_pinv must be finite and non-negative");
  for (int z = 0; z < kOut; ++z) PG_REQUIRE(std::isfinite(energy[z]), 1, "minsr_direction: non-finite energy");
  const int ns = sr_n_;
  for (long e = 0; e < (long)ns * kOut; ++e) PG_REQUIRE(std::isfinite(eloc[e]), 1, "minsr_direction: non-finite local energy");
  const size_t nn = (size_t)ns * ns * kOut, ew = eigh_work_doubles(ns);
  if (minsr_cap_ < ns) {
    for (double *p : {minsr_t_, minsr_v_, minsr_work_}) arena_.free(p);
    minsr_t_ = minsr_v_ = minsr_work_ = nullptr;
    minsr_cap_ = 0;
    minsr_t_ = (double *)arena_.alloc(sizeof(double) * nn);
    minsr_v_ = (double *)arena_.alloc(sizeof(double) * nn);
    minsr_work_ = (double *)arena_.alloc(sizeof(double) * (ew + (size_t)ns * (2 + 3 * kOut) + 8));
    minsr_cap_ = ns;
  }
  double *w = minsr_work_ + ew, *fw = w + ns, *m = fw + ns, *u = m + (size_t)ns * kOut, *de = u + (size_t)ns * kOut;
  double *den = de + (size_t)ns * kOut, *ysum = den + 2, *dinfo = ysum + 2;
  const int sites = Ly_ * Lx_;
  sr_gram_device(minsr_t_);
  hipLaunchKernelGGL(minsr_rowmean_kernel<kOut>, dim3(ns), dim3(64), 0, stream_, (const double *)minsr_t_, ns, m);
  hipLaunchKernelGGL(minsr_center_kernel<kOut>, dim3((unsigned)(((long)ns * ns + 255) / 256)), dim3(256), 0, stream_, minsr_t_,
                     (const double *)m, ns);
  PG_CHECK_HIP(hipGetLastError());
  int sweeps = 0;
  const bool converged = eigh_jacobi(stream_, ns, kCplx, minsr_t_, minsr_v_, w, minsr_work_, &sweeps);
  if (!converged) throw Error(6, "minsr_direction: the Jacobi eigensolver reached its sweep cap");
  hipLaunchKernelGGL(minsr_cutoff_kernel, dim3(1), dim3(256), 0, stream_, (const double *)w, ns, r_pinv, a_pinv, soft_cutoff ? 1 : 0, fw, dinfo);
  PG_CHECK_HIP(hipGetLastError());
  double info[3];
  PG_CHECK_HIP(hipMemcpyAsync(info, dinfo, sizeof(info), hipMemcpyDeviceToHost, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  if (!std::isfinite(info[0])) throw Error(2, "minsr_direction: the T matrix has non-finite eigenvalues (non-finite O* samples)");
  PG_CHECK_HIP(hipMemcpyAsync(de, eloc, sizeof(double) * (size_t)ns * kOut, hipMemcpyHostToDevice, stream_));
  PG_CHECK_HIP(hipMemcpyAsync(den, energy, sizeof(double) * kOut, hipMemcpyHostToDevice, stream_));
  hipLaunchKernelGGL(minsr_project_kernel<kOut>, dim3(ns), dim3(64), 0, stream_, (const double *)minsr_t_, (const double *)fw,
                     (const double *)de, (const double *)den, ns, u);
  hipLaunchKernelGGL(minsr_expand_kernel<kOut>, dim3((ns + 255) / 256), dim3(256), 0, stream_, (const double *)minsr_t_, (const double *)u,
                     ns, sr_delta_);
  hipLaunchKernelGGL(minsr_ysum_kernel<kOut>, dim3(1), dim3(64), 0, stream_, (const double *)sr_delta_, ns, ysum);
  PG_CHECK_HIP(hipGetLastError());
  // the back-substitution: the kernels behind pepsgpu_sr_weighted_sum (-> sr_out_) and pepsgpu_sr_sum (-> sr_v_), device to device
  const dim3 ag((unsigned)((slot_ + 255) / 256), sites);
  hipLaunchKernelGGL(sr_accum_kernel<T>, ag, dim3(256), 0, stream_, (const T *)sr_o_, (const int *)sr_cfg_, (const double *)sr_delta_, 1.0,
                     sr_out_, ns, sites, slot_, dp_);
  hipLaunchKernelGGL(sr_accum_kernel<T>, ag, dim3(256), 0, stream_, (const T *)sr_o_, (const int *)sr_cfg_, (const double *)nullptr, 1.0,
                     sr_v_, ns, sites, slot_, dp_);
  hipLaunchKernelGGL(minsr_combine_kernel<kOut>, opt_grid(), dim3(256), 0, stream_, (const double *)sr_out_, (const double *)sr_v_,
                     (const double *)ysum, ns, opt_g_, (const int *)opt_ne_, slot_, dp_);
  PG_CHECK_HIP(hipGetLastError());
  const double nsq = opt_norm_sq(opt_g_);      // (synchronises: eloc / energy have been read)
  if (direction_norm_out) *direction_norm_out = std::sqrt(nsq);
  if (info_out) { info_out[0] = info[0]; info_out[1] = info[1]; info_out[2] = info[2]; info_out[3] = (double)sweeps; }
}

// the scalars of an SGD step from (momentum, nesterov, weight_decay): one reading for opt_step and opt_preview
template <typename T>
OptStepArgs Engine<T>::opt_sgd_args(const char *who, double lr, const double *params, int n_params) const {
  PG_REQUIRE(std::isfinite(lr) && lr >= 0.0, 1, std::string(who) + ": the learning rate must be finite and non-negative");
  PG_REQUIRE(n_params == 3 && params != nullptr, 1, std::string(who) + ": wrong n_params (SGD 3, AdaGrad 2, Adam 4)");
  for (int i = 0; i < n_params; ++i) PG_REQUIRE(std::isfinite(params[i]), 1, std::string(who) + ": non-finite rule parameter");
  PG_REQUIRE(params[0] >= 0.0 && params[2] >= 0.0, 1, std::string(who) + ": negative SGD momentum / weight_decay");
  OptStepArgs a{};
  a.lr = lr; a.decay = 1.0;
  a.mu = params[0]; a.nesterov = params[1] != 0.0;
  if (params[2] > 0.0) a.decay = 1.0 - lr * params[2];
  return a;
}

template <typename T>
void Engine<T>::opt_step(int rule, double lr, const double *params, int n_params) {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "opt_step: call pepsgpu_opt_begin first");
  PG_REQUIRE(std::isfinite(lr) && lr >= 0.0, 1, "opt_step: the learning rate must be finite and non-negative");
  PG_REQUIRE(rule == OPT_SGD || rule == OPT_ADAGRAD || rule == OPT_ADAM, 1, "opt_step: unknown rule (0 SGD, 1 AdaGrad, 2 Adam)");
  static const int want[3] = {3, 2, 4};
  PG_REQUIRE(n_params == want[rule] && params != nullptr, 1, "opt_step: wrong n_params (SGD 3, AdaGrad 2, Adam 4)");
  for (int i = 0; i < n_params; ++i) PG_REQUIRE(std::isfinite(params[i]), 1, "opt_step: non-finite rule parameter");
  OptStepArgs a{};
  a.lr = lr; a.decay = 1.0;
  const dim3 grid = opt_grid();
  if (rule == OPT_SGD) {
    a = opt_sgd_args("opt_step", lr, params, n_params);
    hipLaunchKernelGGL((opt_step_kernel<T, OPT_SGD>), grid, dim3(256), 0, stream_, a, opt_theta_, (const double *)opt_g_, opt_vel_,
                       (double *)nullptr, sitps_, (const int *)opt_ne_, slot_, dp_);
  } else if (rule == OPT_ADAGRAD) {   // (epsilon, initial_accumulator_value)
    PG_REQUIRE(params[0] >= 0.0 && params[1] >= 0.0, 1, "opt_step: negative AdaGrad epsilon / initial_accumulator_value");
    a.eps = params[0];
    if (!opt_acc_ready_) {
      if (params[1] != 0.0) {
        hipLaunchKernelGGL(opt_fill_kernel, grid, dim3(256), 0, stream_, opt_acc_, params[1], (const int *)opt_ne_, slot_, dp_);
        PG_CHECK_HIP(hipGetLastError());
      }
      opt_acc_ready_ = true;
    }
    hipLaunchKernelGGL((opt_step_kernel<T, OPT_ADAGRAD>), grid, dim3(256), 0, stream_, a, opt_theta_, (const double *)opt_g_,
                       (double *)nullptr, opt_acc_, sitps_, (const int *)opt_ne_, slot_, dp_);
  } else {                            // (beta1, beta2, epsilon, weight_decay)
    PG_REQUIRE(params[0] >= 0.0 && params[0] < 1.0 && params[1] >= 0.0 && params[1] < 1.0, 1, "opt_step: Adam beta outside [0, 1)");
    PG_REQUIRE(params[2] >= 0.0 && params[3] >= 0.0, 1, "opt_step: negative Adam epsilon / weight_decay");
    ++opt_t_;
    a.b1 = params[0]; a.b2 = params[1]; a.eps = params[2];
    if (params[3] > 0.0) a.decay = 1.0 - lr * params[3];
    a.inv_bc1 = 1.0 / (1.0 - std::pow(a.b1, (double)opt_t_));
    a.inv_bc2 = 1.0 / (1.0 - std::pow(a.b2, (double)opt_t_));
    hipLaunchKernelGGL((opt_step_kernel<T, OPT_ADAM>), grid, dim3(256), 0, stream_, a, opt_theta_, (const double *)opt_g_, opt_m1_,
                       opt_m2_, sitps_, (const int *)opt_ne_, slot_, dp_);
  }
  PG_CHECK_HIP(hipGetLastError());
  state_adopted();      // sitps_ changed: the walkers' environments are stale as after pepsgpu_state_upload
}

template <typename T>
void Engine<T>::opt_scale_state(double factor) {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "opt_scale_state: call pepsgpu_opt_begin first");
  PG_REQUIRE(std::isfinite(factor), 1, "opt_scale_state: non-finite factor");
  hipLaunchKernelGGL((opt_scale_kernel<T, true>), opt_grid(), dim3(256), 0, stream_, opt_theta_, factor, sitps_, (const int *)opt_ne_,
                     slot_, dp_);
  PG_CHECK_HIP(hipGetLastError());
  state_adopted();
}

#undef OPT_ELEM_PROLOGUE

}  // namespace pepsgpu

// L-BFGS on the device-resident optimizer buffers (optimizer/optimizer_impl.h of the reference: ResetLBFGSState_ :1404-1413,
// UpdateLBFGSHistoryFromAnchor_ :1443-1486, ComputeLBFGSSearchDirection_ :1488-1532, the descent guard :620-641, the trial point of
// StrongWolfeLBFGSStep_ :1581-1595, the anchor :847-850).  Every vector -- the ring of (s_i, y_i), the anchor (theta_a, g_a), the
// direction d and the base (theta_b, g_b) of the current search -- lives in HBM in the layout of opt_theta_; all are zeroed at begin and
// only their live elements are ever written, so the padding stays exactly zero and the dots run over the whole padded length.
//   update     s = theta - theta_a, y = g - g_a into the free ring slot and <s,y>, <y,y>, <s,s> in one pass; damping y += c s in a
//              second one; a pushed pair adds its two rows of the Gram matrix of the ring (one multi-dot launch each)
//   direction  <g, s_i>, <g, y_i> in one pass; the two-loop recursion on the host in the coefficients of [s_1..s_m, y_1..y_m, g]
//              (double); d = -(c_g g + sum_j c_j b_j) with <d,d> and <g,d> in one pass; norm cap; descent guard; base <- (theta, g)
//   trial      theta = theta_b + alpha d, sitps_ = T(theta) in one pass (alpha = 0: a copy)
//   slope      <g, d>
//   commit     anchor <-> base (pointers)
// Reductions: per-block partial sums, then one wave per scalar adds them in a fixed order (no atomics): the same call on the same
// buffers gives the same bytes.  Kernels are memory bound: 16-byte loads where the rows allow it (slot * kOut even), at most 2048 blocks
// with grid strides over the rows (blockIdx.y) and inside a row (blockIdx.x).
// Complex states: RealInnerProduct_ (:1398-1401) is the plain dot over the interleaved doubles.  Fermionic decoration: every vector is a
// linear combination of theta and Pi g, so it stays in the range of E and the kernels run unchanged; every inner product that leaves
// this file or meets a threshold is the stored one, 1/4 of the extended one (E^T E = 4 mask, as in opt_norm_sq).
// The descent-reset counter survives the reset it counts (the reference's ResetLBFGSState_ zeroes all three counters, so its own
// counter can never be read as anything but 0); pepsgpu_lbfgs_reset and pepsgpu_lbfgs_begin zero the three.
#pragma once
#include "engine_opt.h"

namespace pepsgpu {

enum { LBFGS_NONE = 0, LBFGS_PUSHED = 1, LBFGS_PUSHED_DAMPED = 2, LBFGS_SKIPPED = 3 };

struct LbfgsVecs { const double *p[64]; };      // up to 2 * 32 history vectors, by value
struct LbfgsCoef { double c[64]; };

template <int V> __device__ __forceinline__ void lb_load(const double *p, double (&x)[V]) {
  if constexpr (V == 2) { const double2 t = *reinterpret_cast<const double2 *>(p); x[0] = t.x; x[1] = t.y; }
  else x[0] = *p;
}
// nlive: live doubles from p on
template <int V> __device__ __forceinline__ void lb_store(double *p, const double (&x)[V], long nlive) {
  if constexpr (V == 2) {
    if (nlive >= 2) *reinterpret_cast<double2 *>(p) = make_double2(x[0], x[1]);
    else if (nlive == 1) p[0] = x[0];
  } else if (nlive >= 1) p[0] = x[0];
}

// rows q = (site, component) of rowlen = slot * Z doubles, the first ne[site] * Z of them live; o = offset of the thread's V doubles
#define LB_FOR_EACH                                                                                    \
  for (int q = blockIdx.y; q < nrows; q += gridDim.y)                                                  \
    for (long e = ((long)blockIdx.x * 256 + threadIdx.x) * V, o = (long)q * rowlen + e,                \
              live = (long)ne[q / dp] * z - e;                                                         \
         e < rowlen; e += (long)gridDim.x * 256 * V, o += (long)gridDim.x * 256 * V, live -= (long)gridDim.x * 256 * V)

// part[block][j] = the block's share of acc[j], j < k (k <= KMAX <= 64)
template <int KMAX>
__device__ __forceinline__ void lb_block_partials(double (&acc)[KMAX], int k, double *__restrict__ part) {
  __shared__ double s_red[4][KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j)
    if (j < k) {
      const double a = wave_sum(acc[j]);
      if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][j] = a;
    }
  __syncthreads();
  const int j = threadIdx.x;
  if (j < k) part[((long)blockIdx.y * gridDim.x + blockIdx.x) * k + j] = ((s_red[0][j] + s_red[1][j]) + s_red[2][j]) + s_red[3][j];
}

// out[j] = sum over the blocks of part[block][j]: one wave per j, fixed order
__global__ __launch_bounds__(64) void lbfgs_reduce_kernel(const double *__restrict__ part, int nblocks, int k, double *__restrict__ out) {
  const int j = blockIdx.x;
  double acc = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 64) acc += part[(long)b * k + j];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) out[j] = acc;
}

// s = theta - theta_a, y = g - g_a; partial sums of <s,y>, <y,y>, <s,s>
template <int V>
__global__ __launch_bounds__(256) void lbfgs_diff_kernel(const double *__restrict__ theta, const double *__restrict__ theta_a,
                                                         const double *__restrict__ g, const double *__restrict__ g_a,
                                                         double *__restrict__ s, double *__restrict__ y, double *__restrict__ part,
                                                         const int *__restrict__ ne, int nrows, long rowlen, int dp, int z) {
#pragma clang fp contract(off)
  double acc[3] = {0.0, 0.0, 0.0};
  LB_FOR_EACH {
    double a[V], b[V], sv[V], yv[V];
    lb_load<V>(theta + o, a); lb_load<V>(theta_a + o, b);
    for (int i = 0; i < V; ++i) sv[i] = a[i] - b[i];
    lb_load<V>(g + o, a); lb_load<V>(g_a + o, b);
    for (int i = 0; i < V; ++i) yv[i] = a[i] - b[i];
    lb_store<V>(s + o, sv, live); lb_store<V>(y + o, yv, live);
    for (int i = 0; i < V; ++i) { acc[0] += sv[i] * yv[i]; acc[1] += yv[i] * yv[i]; acc[2] += sv[i] * sv[i]; }
  }
  lb_block_partials<3>(acc, 3, part);
}

// y += c s; partial sums of <s,y>, <y,y>
template <int V>
__global__ __launch_bounds__(256) void lbfgs_damp_kernel(const double *__restrict__ s, double *__restrict__ y, double c,
                                                         double *__restrict__ part, const int *__restrict__ ne, int nrows, long rowlen,
                                                         int dp, int z) {
#pragma clang fp contract(off)
  double acc[2] = {0.0, 0.0};
  LB_FOR_EACH {
    double sv[V], yv[V];
    lb_load<V>(s + o, sv); lb_load<V>(y + o, yv);
    for (int i = 0; i < V; ++i) yv[i] = yv[i] + c * sv[i];
    lb_store<V>(y + o, yv, live);
    for (int i = 0; i < V; ++i) { acc[0] += sv[i] * yv[i]; acc[1] += yv[i] * yv[i]; }
  }
  lb_block_partials<2>(acc, 2, part);
}

// partial sums of <x, b_j>, j < k: one accumulator per vector in registers, every vector read once
template <int KMAX, int V>
__global__ __launch_bounds__(256) void lbfgs_mdot_kernel(const double *__restrict__ x, LbfgsVecs vecs, int k, double *__restrict__ part,
                                                         const int *__restrict__ ne, int nrows, long rowlen, int dp, int z) {
  double acc[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) acc[j] = 0.0;
  LB_FOR_EACH {
    (void)live;
    double xv[V];
    lb_load<V>(x + o, xv);
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
      if (j < k) {
        double b[V];
        lb_load<V>(vecs.p[j] + o, b);
        for (int i = 0; i < V; ++i) acc[j] += xv[i] * b[i];
      }
  }
  lb_block_partials<KMAX>(acc, k, part);
}

// d = -(cg g + sum_{j < k} c_j b_j) in this order; partial sums of <d,d>, <g,d>
template <int KMAX, int V>
__global__ __launch_bounds__(256) void lbfgs_combine_kernel(const double *__restrict__ g, double cg, LbfgsVecs vecs, LbfgsCoef coef, int k,
                                                            double *__restrict__ d, double *__restrict__ part,
                                                            const int *__restrict__ ne, int nrows, long rowlen, int dp, int z) {
#pragma clang fp contract(off)
  double acc[2] = {0.0, 0.0};
  LB_FOR_EACH {
    double gv[V], t[V];
    lb_load<V>(g + o, gv);
    for (int i = 0; i < V; ++i) t[i] = cg * gv[i];
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
      if (j < k) {
        double b[V];
        lb_load<V>(vecs.p[j] + o, b);
        for (int i = 0; i < V; ++i) t[i] += coef.c[j] * b[i];
      }
    for (int i = 0; i < V; ++i) t[i] = -t[i];
    lb_store<V>(d + o, t, live);
    for (int i = 0; i < V; ++i) { acc[0] += t[i] * t[i]; acc[1] += gv[i] * t[i]; }
  }
  lb_block_partials<2>(acc, 2, part);
}

// d *= f; partial sums of <d,d>, <g,d>      (the norm cap, :1524-1529)
template <int V>
__global__ __launch_bounds__(256) void lbfgs_scale_kernel(const double *__restrict__ g, double f, double *__restrict__ d,
                                                          double *__restrict__ part, const int *__restrict__ ne, int nrows, long rowlen,
                                                          int dp, int z) {
#pragma clang fp contract(off)
  double acc[2] = {0.0, 0.0};
  LB_FOR_EACH {
    double gv[V], t[V];
    lb_load<V>(g + o, gv); lb_load<V>(d + o, t);
    for (int i = 0; i < V; ++i) t[i] *= f;
    lb_store<V>(d + o, t, live);
    for (int i = 0; i < V; ++i) { acc[0] += t[i] * t[i]; acc[1] += gv[i] * t[i]; }
  }
  lb_block_partials<2>(acc, 2, part);
}

// theta = theta_b + alpha d (alpha = 0: theta_b itself), sitps_ = T(theta); contraction off as in opt_step_kernel
template <typename T, int V>
__global__ __launch_bounds__(256) void lbfgs_trial_kernel(const double *__restrict__ theta_b, const double *__restrict__ d, double alpha,
                                                          double *__restrict__ theta, T *__restrict__ sitps,
                                                          const int *__restrict__ ne, int nrows, long rowlen, int dp) {
#pragma clang fp contract(off)
  constexpr int z = is_cplx<T>::value ? 2 : 1;
  static_assert(V % z == 0, "a complex element is never split between two threads");
  LB_FOR_EACH {
    if (live <= 0) break;                 // nothing is reduced here: the padding is not even read
    double tb[V], dv[V], th[V];
    lb_load<V>(theta_b + o, tb); lb_load<V>(d + o, dv);
    for (int i = 0; i < V; ++i) th[i] = alpha == 0.0 ? tb[i] : tb[i] + alpha * dv[i];
    lb_store<V>(theta + o, th, live);
    for (int i = 0; i < V; i += z)
      if (i < live) opt_store_state<T>(sitps, (o + i) / z, th + i);
  }
}
#undef LB_FOR_EACH

// ---------------------------------------------------------------------------------------------
template <typename T>
void Engine<T>::lbfgs_release() {
  for (double *p : lb_s_) arena_.free(p);
  for (double *p : lb_y_) arena_.free(p);
  lb_s_.clear(); lb_y_.clear();
  for (double *p : {lb_theta_a_, lb_g_a_, lb_theta_b_, lb_g_b_, lb_d_, lb_part_}) arena_.free(p);
  lb_theta_a_ = lb_g_a_ = lb_theta_b_ = lb_g_b_ = lb_d_ = lb_part_ = nullptr;
  lb_m_ = 0;
  lb_head_ = lb_count_ = 0;
  lb_has_anchor_ = lb_has_dir_ = false;
  lb_skip_ = lb_damp_ = lb_descent_reset_ = 0;
  lb_rho_.clear(); lb_sy_.clear(); lb_yy_.clear(); lb_gram_.clear();
}

template <typename T>
dim3 Engine<T>::lbfgs_grid() const {
  const long per_row = ((long)slot_ * kOut / lbfgs_vec() + 255) / 256;
  const unsigned bx = (unsigned)std::min<long>(std::max<long>(per_row, 1), kLbfgsMaxBlocks);
  const unsigned by = (unsigned)std::min<long>((long)Ly_ * Lx_ * dp_, std::max<long>(kLbfgsMaxBlocks / bx, 1));
  return dim3(bx, by);
}

template <typename T>
void Engine<T>::lbfgs_begin(int history_size) {
  PG_REQUIRE(opt_theta_ != nullptr, 3, "lbfgs_begin: call pepsgpu_opt_begin first");
  PG_REQUIRE(history_size >= 1 && history_size <= kLbfgsMaxHistory, 1, "lbfgs_begin: history_size must be in [1, 32]");
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  lbfgs_release();
  try {
    const size_t bytes = sizeof(double) * (size_t)Ly_ * Lx_ * dp_ * slot_ * kOut;
    auto vec = [&]() {
      double *p = (double *)arena_.alloc(bytes);
      PG_CHECK_HIP(hipMemsetAsync(p, 0, bytes, stream_));
      return p;
    };
    lb_m_ = history_size;
    for (int i = 0; i <= history_size; ++i) { lb_s_.push_back(vec()); lb_y_.push_back(vec()); }
    lb_theta_a_ = vec(); lb_g_a_ = vec(); lb_theta_b_ = vec(); lb_g_b_ = vec(); lb_d_ = vec();
    lb_part_ = (double *)arena_.alloc(sizeof(double) * ((size_t)kLbfgsMaxBlocks * 64 + 64));
    const int nv = 2 * (history_size + 1);
    lb_rho_.assign(history_size + 1, 0.0); lb_sy_.assign(history_size + 1, 0.0); lb_yy_.assign(history_size + 1, 0.0);
    lb_gram_.assign((size_t)nv * nv, 0.0);
    PG_CHECK_HIP(hipStreamSynchronize(stream_));
  } catch (...) {
    lbfgs_release();
    throw;
  }
}

template <typename T>
void Engine<T>::lbfgs_end() {
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  lbfgs_release();
}

// ResetLBFGSState_: history, anchor, pending direction and the three counters; the buffers stay
template <typename T>
void Engine<T>::lbfgs_reset() {
  PG_REQUIRE(lb_m_ > 0, 3, "lbfgs_reset: call pepsgpu_lbfgs_begin first");
  lb_head_ = lb_count_ = 0;
  lb_has_anchor_ = lb_has_dir_ = false;
  lb_skip_ = lb_damp_ = lb_descent_reset_ = 0;
}

// the k sums a kernel left as per-block partials in lb_part_ -> host, scaled to the stored inner product
template <typename T>
void Engine<T>::lbfgs_reduce(int nblocks, int k, double *host_out) {
  double *out = lb_part_ + (size_t)kLbfgsMaxBlocks * 64;
  hipLaunchKernelGGL(lbfgs_reduce_kernel, dim3(k), dim3(64), 0, stream_, (const double *)lb_part_, nblocks, k, out);
  PG_CHECK_HIP(hipGetLastError());
  PG_CHECK_HIP(hipMemcpyAsync(host_out, out, sizeof(double) * k, hipMemcpyDeviceToHost, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  if (fd_d_ > 0)
    for (int j = 0; j < k; ++j) host_out[j] *= 0.25;
}

#define LB_DISPATCH_K(k, CALL)                      \
  do {                                              \
    if ((k) <= 4) { constexpr int KMAX = 4; CALL; }        \
    else if ((k) <= 8) { constexpr int KMAX = 8; CALL; }   \
    else if ((k) <= 16) { constexpr int KMAX = 16; CALL; } \
    else if ((k) <= 32) { constexpr int KMAX = 32; CALL; } \
    else { constexpr int KMAX = 64; CALL; }                \
  } while (0)
#define LB_ROWS (const int *)opt_ne_, Ly_ * Lx_ * dp_, (long)slot_ * kOut, dp_

// host_out[j] = <x, vecs[j]>, j < k <= 64
template <typename T>
void Engine<T>::lbfgs_mdot(const double *x, const double *const *vecs, int k, double *host_out) {
  LbfgsVecs l{};
  for (int j = 0; j < k; ++j) l.p[j] = vecs[j];
  const dim3 grid = lbfgs_grid();
  if (lbfgs_vec() == 2)
    LB_DISPATCH_K(k, hipLaunchKernelGGL((lbfgs_mdot_kernel<KMAX, 2>), grid, dim3(256), 0, stream_, x, l, k, lb_part_, LB_ROWS, (int)kOut));
  else
    LB_DISPATCH_K(k, hipLaunchKernelGGL((lbfgs_mdot_kernel<KMAX, 1>), grid, dim3(256), 0, stream_, x, l, k, lb_part_, LB_ROWS, (int)kOut));
  PG_CHECK_HIP(hipGetLastError());
  lbfgs_reduce((int)(grid.x * grid.y), k, host_out);
}

// lb_d_ = -(cg g + sum_j coef[j] vecs[j]); dd = <d,d>, gd = <g,d>
template <typename T>
void Engine<T>::lbfgs_combine(const double *const *vecs, const double *coef, int k, double cg, double *dd, double *gd) {
  LbfgsVecs l{};
  LbfgsCoef c{};
  for (int j = 0; j < k; ++j) { l.p[j] = vecs[j]; c.c[j] = coef[j]; }
  const dim3 grid = lbfgs_grid();
  if (lbfgs_vec() == 2)
    LB_DISPATCH_K(k, hipLaunchKernelGGL((lbfgs_combine_kernel<KMAX, 2>), grid, dim3(256), 0, stream_, (const double *)opt_g_, cg, l, c, k,
                                        lb_d_, lb_part_, LB_ROWS, (int)kOut));
  else
    LB_DISPATCH_K(k, hipLaunchKernelGGL((lbfgs_combine_kernel<KMAX, 1>), grid, dim3(256), 0, stream_, (const double *)opt_g_, cg, l, c, k,
                                        lb_d_, lb_part_, LB_ROWS, (int)kOut));
  PG_CHECK_HIP(hipGetLastError());
  double r[2];
  lbfgs_reduce((int)(grid.x * grid.y), 2, r);
  *dd = r[0]; *gd = r[1];
}

// UpdateLBFGSHistoryFromAnchor_ (:1443-1486)
template <typename T>
void Engine<T>::lbfgs_update(double min_curvature, int use_damping, int *outcome, double *curvature) {
  PG_REQUIRE(lb_m_ > 0, 3, "lbfgs_update: call pepsgpu_lbfgs_begin first");
  PG_REQUIRE(!std::isnan(min_curvature), 1, "lbfgs_update: NaN min_curvature");
  if (outcome) *outcome = LBFGS_NONE;
  if (curvature) *curvature = 0.0;
  if (!lb_has_anchor_) return;
  const int ring = lb_m_ + 1, p = (lb_head_ + lb_count_) % ring;      // the free slot
  const dim3 grid = lbfgs_grid();
  const int nblocks = (int)(grid.x * grid.y);
  if (lbfgs_vec() == 2)
    hipLaunchKernelGGL(lbfgs_diff_kernel<2>, grid, dim3(256), 0, stream_, (const double *)opt_theta_, (const double *)lb_theta_a_,
                       (const double *)opt_g_, (const double *)lb_g_a_, lb_s_[p], lb_y_[p], lb_part_, LB_ROWS, (int)kOut);
  else
    hipLaunchKernelGGL(lbfgs_diff_kernel<1>, grid, dim3(256), 0, stream_, (const double *)opt_theta_, (const double *)lb_theta_a_,
                       (const double *)opt_g_, (const double *)lb_g_a_, lb_s_[p], lb_y_[p], lb_part_, LB_ROWS, (int)kOut);
  PG_CHECK_HIP(hipGetLastError());
  double r[3];
  lbfgs_reduce(nblocks, 3, r);
  double sy = r[0], yy = r[1];
  bool damped = false;
  if (sy <= min_curvature && use_damping && yy > std::numeric_limits<double>::epsilon()) {
    const double delta = min_curvature - sy + 1e-15;
    if (lbfgs_vec() == 2)
      hipLaunchKernelGGL(lbfgs_damp_kernel<2>, grid, dim3(256), 0, stream_, (const double *)lb_s_[p], lb_y_[p], delta / yy, lb_part_, LB_ROWS,
                         (int)kOut);
    else
      hipLaunchKernelGGL(lbfgs_damp_kernel<1>, grid, dim3(256), 0, stream_, (const double *)lb_s_[p], lb_y_[p], delta / yy, lb_part_, LB_ROWS,
                         (int)kOut);
    PG_CHECK_HIP(hipGetLastError());
    lbfgs_reduce(nblocks, 2, r);
    sy = r[0]; yy = r[1];
    damped = true;
    ++lb_damp_;
  }
  if (curvature) *curvature = sy;
  if (sy <= min_curvature) {
    ++lb_skip_;
    if (outcome) *outcome = LBFGS_SKIPPED;
    return;
  }
  lb_rho_[p] = 1.0 / sy; lb_sy_[p] = sy; lb_yy_[p] = yy;
  ++lb_count_;
  if (lb_count_ > lb_m_) { lb_head_ = (lb_head_ + 1) % ring; lb_count_ = lb_m_; }
  // the rows of the new s and y in the Gram matrix of the ring (a damped y is read after its correction)
  const int nv = 2 * ring;
  std::vector<const double *> vecs;
  std::vector<int> idx;
  for (int i = 0; i < lb_count_; ++i) {
    const int q = (lb_head_ + i) % ring;
    vecs.push_back(lb_s_[q]); idx.push_back(q);
    vecs.push_back(lb_y_[q]); idx.push_back(ring + q);
  }
  std::vector<double> row(vecs.size());
  for (int which = 0; which < 2; ++which) {
    const int a = which ? ring + p : p;
    lbfgs_mdot(which ? lb_y_[p] : lb_s_[p], vecs.data(), (int)vecs.size(), row.data());
    for (size_t j = 0; j < vecs.size(); ++j) lb_gram_[(size_t)a * nv + idx[j]] = lb_gram_[(size_t)idx[j] * nv + a] = row[j];
  }
  if (outcome) *outcome = damped ? LBFGS_PUSHED_DAMPED : LBFGS_PUSHED;
}

// ComputeLBFGSSearchDirection_ (:1488-1532) in the coefficients of [s_1..s_m, y_1..y_m, g], then the descent guard (:620-641)
template <typename T>
void Engine<T>::lbfgs_direction(double min_curvature, double max_direction_norm, double *dphi0, double *norm, int *was_reset) {
  PG_REQUIRE(lb_m_ > 0, 3, "lbfgs_direction: call pepsgpu_lbfgs_begin first");
  PG_REQUIRE(!std::isnan(min_curvature) && !std::isnan(max_direction_norm), 1, "lbfgs_direction: NaN parameter");
  const int ring = lb_m_ + 1, nv = 2 * ring, m = lb_count_;
  if (was_reset) *was_reset = 0;
  double dd = 0.0, gd = 0.0;
  if (m > 0) {
    std::vector<const double *> vecs(2 * m);
    std::vector<int> idx(2 * m);
    for (int i = 0; i < m; ++i) {
      const int q = (lb_head_ + i) % ring;
      vecs[i] = lb_s_[q]; idx[i] = q;
      vecs[m + i] = lb_y_[q]; idx[m + i] = ring + q;
    }
    std::vector<double> bg(2 * m);          // <b_j, g>
    lbfgs_mdot(opt_g_, vecs.data(), 2 * m, bg.data());
    auto gram = [&](int a, int b) { return lb_gram_[(size_t)idx[a] * nv + idx[b]]; };
    // <b_a, v> for v = sum_j c[j] b_j + cg g
    auto dot = [&](int a, const std::vector<double> &c, double cg) {
      double acc = 0.0;
      for (int j = 0; j < 2 * m; ++j) acc += c[j] * gram(a, j);
      return acc + cg * bg[a];
    };
    std::vector<double> c(2 * m, 0.0), alpha(m, 0.0);
    double cg = 1.0;
    for (int i = m; i-- > 0;) {
      const int q = idx[i];
      alpha[i] = lb_rho_[q] * dot(i, c, cg);
      c[m + i] += -alpha[i];
    }
    const int last = idx[m - 1];
    double gamma = 1.0;
    if (lb_yy_[last] > std::numeric_limits<double>::epsilon() && lb_sy_[last] > min_curvature) gamma = lb_sy_[last] / lb_yy_[last];
    for (double &x : c) x *= gamma;
    cg *= gamma;
    for (int i = 0; i < m; ++i) {
      const double beta = lb_rho_[idx[i]] * dot(m + i, c, cg);
      c[i] += alpha[i] - beta;
    }
    lbfgs_combine(vecs.data(), c.data(), 2 * m, cg, &dd, &gd);
  } else {
    lbfgs_combine(nullptr, nullptr, 0, 1.0, &dd, &gd);
  }
  double nrm = std::sqrt(dd);
  if (max_direction_norm > 0.0 && nrm > max_direction_norm && nrm > 0.0) {      // :1524-1529, with or without a history
    const dim3 grid = lbfgs_grid();
    const double f = max_direction_norm / nrm;
    if (lbfgs_vec() == 2)
      hipLaunchKernelGGL(lbfgs_scale_kernel<2>, grid, dim3(256), 0, stream_, (const double *)opt_g_, f, lb_d_, lb_part_, LB_ROWS, (int)kOut);
    else
      hipLaunchKernelGGL(lbfgs_scale_kernel<1>, grid, dim3(256), 0, stream_, (const double *)opt_g_, f, lb_d_, lb_part_, LB_ROWS, (int)kOut);
    PG_CHECK_HIP(hipGetLastError());
    double r[2];
    lbfgs_reduce((int)(grid.x * grid.y), 2, r);
    dd = r[0]; gd = r[1];
    nrm = std::sqrt(dd);
  }
  if (gd >= 0.0) {        // not a descent direction: drop the history and the anchor, d = -g (uncapped, as the reference)
    ++lb_descent_reset_;
    lb_head_ = lb_count_ = 0;
    lb_has_anchor_ = false;
    lbfgs_combine(nullptr, nullptr, 0, 1.0, &dd, &gd);
    nrm = std::sqrt(dd);
    if (was_reset) *was_reset = 1;
  }
  const size_t bytes = sizeof(double) * (size_t)Ly_ * Lx_ * dp_ * slot_ * kOut;
  PG_CHECK_HIP(hipMemcpyAsync(lb_theta_b_, opt_theta_, bytes, hipMemcpyDeviceToDevice, stream_));
  PG_CHECK_HIP(hipMemcpyAsync(lb_g_b_, opt_g_, bytes, hipMemcpyDeviceToDevice, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  lb_has_dir_ = true;
  if (dphi0) *dphi0 = gd;
  if (norm) *norm = nrm;
}

template <typename T>
void Engine<T>::lbfgs_trial(double alpha) {
  PG_REQUIRE(lb_m_ > 0, 3, "lbfgs_trial: call pepsgpu_lbfgs_begin first");
  PG_REQUIRE(lb_has_dir_, 3, "lbfgs_trial: no search direction (pepsgpu_lbfgs_direction)");
  PG_REQUIRE(std::isfinite(alpha) && alpha >= 0.0, 1, "lbfgs_trial: the step length must be finite and non-negative");
  const dim3 grid = lbfgs_grid();
  if (lbfgs_vec() == 2)
    hipLaunchKernelGGL((lbfgs_trial_kernel<T, 2>), grid, dim3(256), 0, stream_, (const double *)lb_theta_b_, (const double *)lb_d_, alpha,
                       opt_theta_, sitps_, LB_ROWS);
  else if constexpr (!kCplx)
    hipLaunchKernelGGL((lbfgs_trial_kernel<T, 1>), grid, dim3(256), 0, stream_, (const double *)lb_theta_b_, (const double *)lb_d_, alpha,
                       opt_theta_, sitps_, LB_ROWS);
  PG_CHECK_HIP(hipGetLastError());
  state_adopted();      // sitps_ changed: the walkers' environments are stale as after pepsgpu_state_upload
}

template <typename T>
void Engine<T>::lbfgs_slope(double *dphi) {
  PG_REQUIRE(lb_m_ > 0, 3, "lbfgs_slope: call pepsgpu_lbfgs_begin first");
  PG_REQUIRE(lb_has_dir_, 3, "lbfgs_slope: no search direction (pepsgpu_lbfgs_direction)");
  const double *v = opt_g_;
  lbfgs_mdot(lb_d_, &v, 1, dphi);
}

// the anchor becomes the base of the search that just ended (:847-850); the old anchor's buffers take the next base
template <typename T>
void Engine<T>::lbfgs_commit() {
  PG_REQUIRE(lb_m_ > 0, 3, "lbfgs_commit: call pepsgpu_lbfgs_begin first");
  PG_REQUIRE(lb_has_dir_, 3, "lbfgs_commit: no search direction (pepsgpu_lbfgs_direction)");
  std::swap(lb_theta_a_, lb_theta_b_);
  std::swap(lb_g_a_, lb_g_b_);
  lb_has_anchor_ = true;
  lb_has_dir_ = false;
}

template <typename T>
void Engine<T>::lbfgs_get_direction(double *host) {
  PG_REQUIRE(lb_m_ > 0, 3, "lbfgs_get_direction: call pepsgpu_lbfgs_begin first");
  opt_read(lb_d_, host);
}

// pair `index` of the history, 0 = oldest
template <typename T>
void Engine<T>::lbfgs_get_pair(int index, double *s_host, double *y_host) {
  PG_REQUIRE(lb_m_ > 0, 3, "lbfgs_get_pair: call pepsgpu_lbfgs_begin first");
  PG_REQUIRE(index >= 0 && index < lb_count_, 4, "lbfgs_get_pair: index outside the history");
  const int q = (lb_head_ + index) % (lb_m_ + 1);
  if (s_host) opt_read(lb_s_[q], s_host);
  if (y_host) opt_read(lb_y_[q], y_host);
}

// out[0..3] = skipped pairs, damped pairs, descent resets, pairs in the history
template <typename T>
void Engine<T>::lbfgs_counters(long *out) {
  PG_REQUIRE(lb_m_ > 0, 3, "lbfgs_counters: call pepsgpu_lbfgs_begin first");
  out[0] = lb_skip_; out[1] = lb_damp_; out[2] = lb_descent_reset_; out[3] = lb_count_;
}

#undef LB_DISPATCH_K
#undef LB_ROWS

}  // namespace pepsgpu

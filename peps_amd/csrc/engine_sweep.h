// One row (or column) of nearest-neighbour exchange updates of the Monte-Carlo sweep on the device
// (MCUpdateSquareNNUpdateBaseOBC::operator() + MCUpdateSquareNNExchangeOBC::TwoSiteNNUpdateLocalImpl, square_nn_updater.h:25-83,
// :142-189; TPSWaveFunctionComponent::UpdateLocal, wave_function_component.h:345-378).
//
// The host-driven form pays, per bond, a candidate upload, the read-back of psi', the Metropolis test on the host, an upload of
// the whole configuration table for the accepted walkers and two stream synchronisations: 264 bonds x ~3 ms per sweep of 8192
// walkers, 3-4 x the contraction work (7.6 k sweeps/s against 29 k amplitude-equivalents).  Here ONE call runs a
// whole slice: InitBTen + GrowFullBTen of the slice, then per bond the replacement trace of the exchanged pair (candidate table
// built on the device), the Metropolis test, the exchange in the device's configuration table, and the BTen window shift -- no
// host round trip inside the slice.
//
// Identical chains: the reference draws a uniform deviate only when the spins differ and |psi'| < |psi| (square_nn_updater.h:
// 160-170).  The host hands over, per walker, the NEXT `n_uniform` deviates of that walker's std::mt19937 stream (drawn ahead into
// a queue, qlpeps_gpu.h: LookAhead); the kernel consumes them in order and reports how many it took, the host pops exactly
// those -- the deviates a walker consumes are the ones the reference's updater would have drawn, in the same order.
//
// Environment bookkeeping: UpdateLocal erases the environments that cross an updated site (EraseEnvsAfterUpdate).  Inside a slice
// pass that erase never removes anything the pass still holds (LEFT covers [0, col), RIGHT covers (col + 1, N): checked against
// the reference's flow), so it is applied unconditionally -- the decision "did any walker accept" would cost a read-back per bond.
#pragma once
#include <algorithm>
#include <atomic>
#include <vector>
#include "engine.h"
#include "engine_nnn.h"

namespace pepsgpu {

// amplitude helpers, uniform over the real (double) and the complex (cplx<double>) accumulation type
__device__ __forceinline__ double sw_abs(double x) { return fabs(x); }
__device__ __forceinline__ double sw_abs(const cplx<double> &x) { return sqrt(x.re * x.re + x.im * x.im); }
__device__ __forceinline__ double sw_scaled(double x, double s) { return x * s; }
__device__ __forceinline__ cplx<double> sw_scaled(const cplx<double> &x, double s) { return cplx<double>(x.re * s, x.im * s); }

// The candidate of the "exchange" move on the bond (s1, s2).  tab == nullptr: cand[w] = (cfg[w][s2], cfg[w][s1]), the exchanged
// pair (bosons).  tab [dp * dp][2] (round 6): the pair the move proposes for the states (a, b) = tab[a * dp + b] -- a fermionic state
// lives on the device as extended states (state + d * variant, pepsgpu.h) and the exchange of two sites adjacent in the mode order
// changes their variants by a rule that is local in (a, b) (TPSWaveFunctionComponent::DeviceStatesNN of the host layer tabulates it).
// same[w] = 1 when the move is the identity (square_nn_updater.h:149-151 returns before any contraction, and so do the environment
// steps of the replacement trace here).
__global__ void sweep_swap_cand_kernel(const int *__restrict__ cfg, int sites, int s1, int s2, int *__restrict__ cand,
                                       int *__restrict__ same, int n, const int *__restrict__ tab = nullptr, int dp = 0) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  const int a = cfg[(long)w * sites + s1], b = cfg[(long)w * sites + s2];
  const int c1 = tab ? tab[2 * (a * dp + b)] : b, c2 = tab ? tab[2 * (a * dp + b) + 1] : a;
  cand[2 * w] = c1;
  cand[2 * w + 1] = c2;
  same[w] = (c1 == a && c2 == b);
}

// Metropolis test of the exchange (square_nn_updater.h:149-170) and the accepted exchange itself
template <typename AccT>
__global__ void sweep_metropolis_exchange_kernel(int *__restrict__ cfg, int sites, int s1, int s2, const AccT *__restrict__ res,
                                                 const double *__restrict__ lsum, AccT *__restrict__ amp,
                                                 const double *__restrict__ uni, int nu, int *__restrict__ uptr,
                                                 int *__restrict__ acc, int *__restrict__ overrun, int *__restrict__ acc_now, int n,
                                                 const int *__restrict__ cand, const int *__restrict__ same) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  acc_now[w] = 0;                                         // (1: this bond's exchange was accepted)
  if (same[w]) return;                                    // :149-151
  const AccT psi_b = sw_scaled(AccT(res[w]), exp(lsum[w]));
  const double pa = sw_abs(amp[w]), pb = sw_abs(psi_b);
  bool exchange;
  if (pb >= pa) exchange = true;
  else {
    const double div = pb / pa;
    const int q = uptr[w];
    if (q >= nu) { *overrun = 1; return; }               // (cannot happen: the host hands over one deviate per bond of the slice)
    exchange = uni[(long)w * nu + q] < div * div;
    uptr[w] = q + 1;
  }
  if (exchange) {
    cfg[(long)w * sites + s1] = cand[2 * w];
    cfg[(long)w * sites + s2] = cand[2 * w + 1];
    amp[w] = psi_b;
    acc[w] += 1;
    acc_now[w] = 1;
  }
}

// every pair of states of the bond as the candidate table of one replacement trace: cand[w][k] = (k / dim, k % dim)
__global__ void sweep_all_cand_kernel(int *__restrict__ cand, int dim, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int nc = dim * dim;
  if (e >= n * nc) return;
  const int k = e % nc;
  cand[2 * e] = k / dim;
  cand[2 * e + 1] = k % dim;
}

// MCUpdateSquareNNFullSpaceUpdateOBC::TwoSiteNNUpdateLocalImpl (square_nn_updater.h:253-293) for one bond: the weights
// |psi_k / psi|^2 of the dim^2 states of the pair (the current one keeps its stored amplitude), SuwaTodoStateUpdate
// (suwa_todo_update.h:53-112) with the walker's next deviate, and the accepted move.  The deviate: the reference draws
// std::uniform_real_distribution<long double> from a std::mt19937, i.e. generate_canonical<long double, 64> = two 32-bit words,
// (w0 + 2^32 w1) / 2^64 -- the host hands over the two raw words per bond (always two: the count does not depend on the data), so a
// walker consumes its engine exactly as the reference's updater does.  The arithmetic here is float64 where the reference's is
// long double: a decision differs only when the deviate falls within 2^-53 of a boundary of the cumulative weights.
constexpr int SW_MAXC = 16;
// SuwaTodoStateUpdate (suwa_todo_update.h:53-112) for nc <= SW_MAXC states: wt (modified: the largest weight is swapped to the front, as
// the reference does), init = the current state, (w0, w1) = the two engine words of the long double draw.  Returns the new state.
__device__ __forceinline__ int sw_suwa_todo_decide(double *wt, int nc, int init, unsigned w0, unsigned w1) {
  int mx = 0;
  for (int k = 1; k < nc; ++k)
    if (wt[k] > wt[mx]) mx = k;                           // std::max_element: the first of equal maxima
  if (mx != 0) { const double t = wt[0]; wt[0] = wt[mx]; wt[mx] = t; }
  if (init == mx) init = 0;
  else if (init == 0) init = mx;
  double cs[SW_MAXC];
  cs[0] = wt[0];
  for (int k = 1; k < nc; ++k) cs[k] = cs[k - 1] + wt[k];
  const double S = cs[nc - 1];
  const double s_im1 = init == 0 ? 0.0 : cs[init - 1];
  double start = s_im1 + wt[0];
  if (start >= S) start -= S;
  double u = ((double)w0 + 4294967296.0 * (double)w1) * 5.421010862427522e-20;      // / 2^64
  if (u >= 1.0) u = 0.9999999999999999;
  const double hi = nextafter(start + wt[init], start);
  double x = u * (hi - start) + start;
  if (x >= S) x -= S;
  int fin = 0;
  while (fin < nc && !(cs[fin] > x)) ++fin;               // std::upper_bound
  if (fin >= nc) fin = nc - 1;
  if (mx != 0) {
    if (fin == 0) fin = mx;
    else if (fin == mx) fin = 0;
  }
  return fin;
}

// a chain of the update on one weight vector (kernel test: the reference's unit cases against the host's long double form)
__global__ void sweep_suwa_todo_chain_kernel(const double *__restrict__ weights, int nc, int init, const unsigned *__restrict__ words, int steps,
                                             int *__restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int st = init;
  for (int s = 0; s < steps; ++s) {
    double wt[SW_MAXC];
    for (int k = 0; k < nc; ++k) wt[k] = weights[k];
    st = sw_suwa_todo_decide(wt, nc, st, words[2 * s], words[2 * s + 1]);
    out[s] = st;
  }
}

template <typename AccT>
__global__ void sweep_suwa_todo_kernel(int *__restrict__ cfg, int sites, int s1, int s2, int dim, const AccT *__restrict__ res,
                                       const double *__restrict__ lsum, AccT *__restrict__ amp, const unsigned *__restrict__ words,
                                       int words_per_walker, int bond, int *__restrict__ acc, int *__restrict__ acc_now, int n) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  const int nc = dim * dim;
  const int c1 = cfg[(long)w * sites + s1], c2 = cfg[(long)w * sites + s2];
  const int init0 = c1 * dim + c2;
  const double sc = exp(lsum[w]);
  const AccT a0 = amp[w];
  const double pa = sw_abs(a0);
  double wt[SW_MAXC];
  for (int k = 0; k < nc; ++k) {
    const double r = (k == init0) ? 1.0 : sw_abs(sw_scaled(AccT(res[(long)w * nc + k]), sc)) / pa;
    wt[k] = r * r;
  }
  const int fin = sw_suwa_todo_decide(wt, nc, init0, words[(long)w * words_per_walker + 2 * bond], words[(long)w * words_per_walker + 2 * bond + 1]);
  const int changed = fin != init0;
  acc_now[w] = changed;
  if (changed) {
    cfg[(long)w * sites + s1] = fin / dim;
    cfg[(long)w * sites + s2] = fin % dim;
    amp[w] = sw_scaled(AccT(res[(long)w * nc + fin]), sc);
    acc[w] += 1;
  }
}

// dst[w] = src[w] for the walkers with take[w] != 0 (len elements per walker)
template <typename T>
__global__ void sweep_take_kernel(T *__restrict__ dst, const T *__restrict__ src, long len, const int *__restrict__ take) {
  const int w = blockIdx.y;
  if (!take[w]) return;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < len; e += (long)gridDim.x * blockDim.x) dst[(long)w * len + e] = src[(long)w * len + e];
}

__global__ void sweep_gather_slice_kernel(const int *__restrict__ cfg, int sites, int first, int stride, int len, int *__restrict__ out, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * len) return;
  const int w = e / len, j = e - w * len;
  out[e] = cfg[(long)w * sites + first + j * stride];
}

// one scalar of the accumulation type into a host-layout double array (complex: an interleaved (re, im) pair)
__device__ __forceinline__ void sw_put(double *o, double x) { o[0] = x; }
__device__ __forceinline__ void sw_put(double *o, const cplx<double> &x) { o[0] = x.re; o[1] = x.im; }

// One-site candidates of site s from a table: cand[w][k] = tab[cfg[w][s] * nc + k] (the one-site energy slice; TFIM: tab = {1, 0})
__global__ void slice_onsite_cand_kernel(const int *__restrict__ cfg, int sites, int s, const int *__restrict__ tab, int nc,
                                         int *__restrict__ cand, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * nc) return;
  const int w = e / nc, k = e - w * nc;
  cand[e] = tab[cfg[(long)w * sites + s] * nc + k];
}

// psi'[w][k] = res[w][k] exp(lsum[w]) into columns col .. col + nc - 1 of a [n][stride] table of AccT scalars, stored as doubles
// (complex: interleaved).  same[w] != 0 (nc == 1): the move was the identity and its trace was skipped -- psi' = psi, the value
// already in column same_col.
template <typename AccT>
__global__ void slice_store_value_kernel(const AccT *__restrict__ res, const double *__restrict__ lsum, double *__restrict__ out,
                                         int stride, int col, int nc, const int *__restrict__ same, int same_col, int n) {
  constexpr int ko = (int)(sizeof(AccT) / sizeof(double));
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * nc) return;
  const int w = e / nc, k = e - w * nc;
  double *o = out + ((long)w * stride + col + k) * ko;
  if (same && same[w]) {
    const double *src = out + ((long)w * stride + same_col) * ko;
    for (int q = 0; q < ko; ++q) o[q] = src[q];
    return;
  }
  sw_put(o, sw_scaled(res[e], exp(lsum[w])));
}

// One row (HORIZONTAL) or column (VERTICAL) of the lattice as the slice functions below walk it: N positions j = 0 .. N - 1, the
// environment that grows with j (lo: LEFT / UP) and the one that shrinks (hi: RIGHT / DOWN).  All the orientation logic of a slice.
struct SliceGeom {
  int orient, slice, Lx, N, lo, hi;
  SliceGeom(int orient_, int slice_, int Lx_, int Ly_) : orient(orient_), slice(slice_), Lx(Lx_) {
    PG_REQUIRE(orient == HORIZONTAL || orient == VERTICAL, 1, "bad orientation");
    const bool h = orient == HORIZONTAL;
    PG_REQUIRE(slice >= 0 && slice < (h ? Ly_ : Lx_), 1, "slice outside the lattice");
    N = h ? Lx_ : Ly_;
    lo = h ? LEFT : UP;
    hi = h ? RIGHT : DOWN;
  }
  int row(int j) const { return orient == HORIZONTAL ? slice : j; }
  int col(int j) const { return orient == HORIZONTAL ? j : slice; }
  int site(int j) const { return row(j) * Lx + col(j); }                    // flat index into a walker's configuration
  int first() const { return site(0); }                                      // sweep_gather_slice_kernel: site(j) = first + j stride
  int stride() const { return site(1) - site(0); }
};

// status 4 unless every state of a table handed over by the host is one of the dp states of a site
inline void require_states(const int32_t *tab, size_t len, int dp, const char *msg) {
  for (size_t e = 0; e < len; ++e) PG_REQUIRE(tab[e] >= 0 && tab[e] < dp, 4, msg);
}

// InitBTen + GrowFullBTen of the slice: the growing environment empty, the shrinking one down to the last `remain` positions
template <typename T>
void Engine<T>::begin_slice(const SliceGeom &g, int remain) {
  init_bten(g.lo, g.slice);
  grow_full_bten(g.hi, g.slice, remain, 1);
}

// The part every sweep slice shares.  dcnt = [consumed n][accepted n][overrun 1] is zeroed, the slice's environments are set up
// (begin_slice with the width of the move's window), `moves` runs the slice's moves on the device, and ONE read-back ends the call: the
// amplitudes damp [n] into amp_out, the counters, and the states of the slice, which also go into the host mirror hcfg_.
// From the first move on the device's configuration table may hold moves the host has not seen: whatever fails after that, the
// mirror is brought back in step before the failure is reported.
template <typename T>
template <typename Moves>
void Engine<T>::sweep_slice_frame(const SliceGeom &g, int window, const Acc *damp, int *dcnt, double *amp_out, int32_t *consumed_out,
                                  int32_t *accepted_out, int32_t *slice_states_out, Moves &&moves) {
  const int sites = Ly_ * Lx_, N = g.N;
  ArenaBuf<int> dslice(arena_, (size_t)nw_ * N);
  std::vector<int> hs((size_t)nw_ * N), hc(2 * (size_t)nw_ + 1);
  try {
    PG_CHECK_HIP(hipMemsetAsync(dcnt, 0, sizeof(int) * hc.size(), stream_));
    begin_slice(g, window);
    moves();
    hipLaunchKernelGGL(sweep_gather_slice_kernel, dim3((nw_ * N + 255) / 256), dim3(256), 0, stream_, (const int *)cfg_, sites, g.first(),
                       g.stride(), N, dslice, nw_);
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipMemcpyAsync(amp_out, damp, sizeof(Acc) * nw_, hipMemcpyDeviceToHost, stream_));
    PG_CHECK_HIP(hipMemcpyAsync(hs.data(), dslice, sizeof(int) * hs.size(), hipMemcpyDeviceToHost, stream_));
    PG_CHECK_HIP(hipMemcpyAsync(hc.data(), dcnt, sizeof(int) * hc.size(), hipMemcpyDeviceToHost, stream_));
    PG_CHECK_HIP(hipStreamSynchronize(stream_));
    PG_REQUIRE(hc[2 * (size_t)nw_] == 0, 5, "device-side slice sweep: uniform deviates exhausted");
    for (int w = 0; w < nw_; ++w) {
      if (consumed_out) consumed_out[w] = hc[w];
      if (accepted_out) accepted_out[w] = hc[nw_ + w];
      for (int j = 0; j < N; ++j) {
        const int v = hs[(size_t)w * N + j];
        hcfg_[(size_t)w * sites + g.site(j)] = v;
        if (slice_states_out) slice_states_out[(size_t)w * N + j] = v;
      }
    }
  } catch (...) {
    (void)hipMemcpy(hcfg_.data(), cfg_, sizeof(int) * (size_t)nw_ * sites, hipMemcpyDeviceToHost);
    throw;
  }
}

// One row / column of the energy evaluation (SquareNNNModelEnergySolver::CalEnergyAndHolesImpl, square_nnn_energy_solver.h:
// 116-200 row pass, bond_traversal_mixin.h:120-144 column pass) for models whose nearest-neighbour off-diagonal term is the
// exchange of the two site states (XXZ, J1-J2, t-J ...): InitBTen + GrowFullBTen, psi of the slice, and for every bond the
// amplitude of the configuration with the two states exchanged -- all on the device, ONE read-back per slice (psi [n] and
// psi_ex [n][N-1]); with punch_holes the hole of every site of the slice is stored in HBM on the way (PunchHole, :163).
// Real element types only (the contract of pepsgpu_nn_exchange_slice; energy_slice_impl covers both).
template <typename T>
void Engine<T>::nn_exchange_slice(int orient, int slice, int punch_holes, double *psi_out, double *psi_ex_out) {
  require_ready();
  PG_REQUIRE(!kCplx, 1, "pepsgpu_nn_exchange_slice: real element types only (complex contexts: pepsgpu_nn_exchange_slice_tab)");
  energy_slice_impl(0, orient, slice, punch_holes, nullptr, 1, 0, psi_out, psi_ex_out);
}

// The energy slice of both element types (results in Acc, host arrays interleaved for complex), two kinds of move:
//   mode 0, the exchange move on each bond: table = the pair table [dp^2][2] of sweep_swap_cand_kernel (nullptr: the swap);
//     psi_per_bond != 0: per bond the Trace of the window before that bond's replacement trace as well (the fermionic hooks,
//     SquareSpinlessFermion / SquaretJVModel::EvaluateBondEnergy), psi_out [n][N-1]; else psi_out [n] from the first window.
//     val_out [n][N-1]: the exchanged amplitude of bond j (psi of the bond where the move is the identity).
//     remain: GrowFullBTen(.., 1) with holes (the row pass, :143), 2 without (the column pass).
//   mode 1, the one-site move on each site (TransverseFieldIsingSquareOBC::CalEnergyAndHoles, transverse_field_ising_square_obc.h:
//     211-247): per site j and candidate k the amplitude with the site's state s replaced by table[s * n_cand + k] (ReplaceOneSiteTrace,
//     :195-203), the BTen window shifted after every site; val_out [n][N][n_cand].  GrowFullBTen(.., 1): the trace of the first site
//     needs the far environment down to the second site, with or without holes.
// Both leave the environments as the per-site / per-bond host path does and punch the holes of the slice into HBM when asked.
template <typename T>
void Engine<T>::energy_slice_impl(int mode, int orient, int slice, int punch_holes, const int32_t *table, int n_cand, int psi_per_bond,
                                  double *psi_out, double *val_out) {
  require_ready();
  PG_REQUIRE(mode == 0 || mode == 1, 1, "energy slice: bad mode");
  const SliceGeom g(orient, slice, Lx_, Ly_);
  const int N = g.N;
  PG_REQUIRE(psi_out && val_out, 1, "null buffer");
  const int nc = mode == 1 ? n_cand : 1;
  PG_REQUIRE(nc >= 1, 1, "energy slice: n_cand < 1");
  PG_REQUIRE(mode == 0 || table, 1, "one-site slice: null site table");
  const size_t tab_len = !table ? 0 : mode == 0 ? 2 * (size_t)dp_ * dp_ : (size_t)dp_ * nc;
  require_states(table, tab_len, dp_, "energy slice table: state out of range");
  const bool per_bond = mode == 0 && psi_per_bond;
  const int sites = Ly_ * Lx_;
  if (punch_holes && !holes_) {
    holes_ = (T *)arena_.alloc(sizeof(T) * (size_t)maxw_ * Ly_ * Lx_ * slot_);
    holes_ls_ = (double *)arena_.alloc(sizeof(double) * (size_t)maxw_ * Ly_ * Lx_);
  }
  // value table [n][stride] of Acc scalars.  mode 0: psi in column psi_col(j), psi_ex of bond j in column ex_col(j); mode 1: psi in
  // column 0, candidate k of site j in column 1 + j nc + k
  const int stride = mode == 1 ? 1 + N * nc : (per_bond ? 2 * (N - 1) : N);
  auto psi_col = [&](int j) { return per_bond ? j : 0; };
  auto ex_col = [&](int j) { return per_bond ? N - 1 + j : 1 + j; };
  ArenaBuf<double> dval(arena_, kOut * (size_t)nw_ * stride);
  ArenaBuf<int> dcand(arena_, (mode == 1 ? (size_t)nc : 3) * (size_t)nw_);
  int *dsame = mode == 0 ? dcand + 2 * (size_t)nw_ : nullptr;
  ArenaBuf<int> dtab(arena_, tab_len);
  if (dtab) PG_CHECK_HIP(hipMemcpyAsync(dtab, table, sizeof(int) * tab_len, hipMemcpyHostToDevice, stream_));
  const int remain = (mode == 1 || punch_holes) ? 1 : 2;
  begin_slice(g, remain);
  const int gb = (nw_ + 255) / 256;
  // res exp(lsum) of a trace into column col (frees res and lsum)
  auto store = [&](Acc *res, double *lsum, int col, int ncs, const int *same, int same_col) {
    hipLaunchKernelGGL(slice_store_value_kernel<Acc>, dim3((nw_ * ncs + 255) / 256), dim3(256), 0, stream_, (const Acc *)res,
                       (const double *)lsum, dval, stride, col, ncs, same, same_col, nw_);
    PG_CHECK_HIP(hipGetLastError());
    arena_.free(res); arena_.free(lsum);
  };
  if (!per_bond) {
    double *lsum = nullptr;
    Acc *res = nn_trace_device(g.row(0), g.col(0), orient, 1, nullptr, &lsum);
    store(res, lsum, 0, 1, nullptr, 0);
  }
  for (int j = 0; j < N; ++j) {
    const int r1 = g.row(j), c1 = g.col(j);
    if (punch_holes) punch_hole(r1, c1, orient, nullptr);
    if (mode == 1) {
      hipLaunchKernelGGL(slice_onsite_cand_kernel, dim3((nw_ * nc + 255) / 256), dim3(256), 0, stream_, (const int *)cfg_, sites,
                         g.site(j), (const int *)dtab, nc, dcand, nw_);
      PG_CHECK_HIP(hipGetLastError());
      double *lsum = nullptr;
      Acc *res = one_trace_device(r1, c1, orient, nc, dcand, &lsum);
      store(res, lsum, 1 + j * nc, nc, nullptr, 0);
      if (j + 1 < N) shift_bten_window(g.hi);
    } else if (j + 1 < N) {
      if (per_bond) {
        double *lsum = nullptr;
        Acc *res = nn_trace_device(r1, c1, orient, 1, nullptr, &lsum);
        store(res, lsum, psi_col(j), 1, nullptr, 0);
      }
      hipLaunchKernelGGL(sweep_swap_cand_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)cfg_, sites, g.site(j), g.site(j + 1),
                         dcand, dsame, nw_, (const int *)dtab, dp_);
      PG_CHECK_HIP(hipGetLastError());
      double *lsum = nullptr;
      Acc *res = nn_trace_device(r1, c1, orient, 1, dcand, &lsum, dsame);
      store(res, lsum, ex_col(j), 1, dsame, psi_col(j));
      if (remain == 1 || j + 2 < N) shift_bten_window(g.hi);
    }
  }
  std::vector<double> h((size_t)kOut * nw_ * stride);
  PG_CHECK_HIP(hipMemcpyAsync(h.data(), dval, sizeof(double) * h.size(), hipMemcpyDeviceToHost, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  auto put = [&](double *dst, size_t i, int w, int col) {
    for (int q = 0; q < kOut; ++q) dst[i * kOut + q] = h[((size_t)w * stride + col) * kOut + q];
  };
  for (int w = 0; w < nw_; ++w) {
    if (mode == 1) {
      put(psi_out, w, w, 0);
      for (int e = 0; e < N * nc; ++e) put(val_out, (size_t)w * N * nc + e, w, 1 + e);
    } else {
      if (!per_bond) put(psi_out, w, w, 0);
      for (int j = 0; j + 1 < N; ++j) {
        if (per_bond) put(psi_out, (size_t)w * (N - 1) + j, w, psi_col(j));
        put(val_out, (size_t)w * (N - 1) + j, w, ex_col(j));
      }
    }
  }
}

// ---- the diagonal bonds of a row pair (SquareNNNModelEnergySolver::CalEnergyAndHolesImpl, square_nnn_energy_solver.h:203-265) and the
// links of a row / column pair (spin_onehalf_triangle_heisenbergJ1J2_sqrpeps.h:350-398, :425-442) ----
// Both exchanges across a two-row window are candidates of ONE replacement of its four corner sites, as replace_plaquette_trace
// batches candidates.  s0 .. s3 = the flat indices of the corners in the order upper-left, lower-left, lower-right, upper-right: of the
// plaquette (r, c) .. (r+1, c+1), of the 2 x 3 window (r, c) .. (r+1, c+2) of a row pair (the flat sqrt5 links) or of the 3 x 2 window
// (r, c) .. (r+2, c+1) of a column pair (the steep ones).  cand[w][q][4] = the corner states with the ends of the q-th requested
// exchange swapped, kind = q ? kind1 : kind0: LEFTUP_TO_RIGHTDOWN swaps the upper-left and the lower-right corner, LEFTDOWN_TO_RIGHTUP
// the lower-left and the upper-right one; the other two corners keep their own states.  flag[w][q] (the batch_flag convention of the
// tensor GEMM): >= 0 where the move is the identity (equal end states; the reference returns before any contraction,
// square_spin_onehalf_xxz_obc.h:107-134), -1 where the entry has work.
__global__ void corner_exchange_cand_kernel(const int *__restrict__ cfg, int sites, int s0, int s1, int s2, int s3, int nc, int kind0,
                                            int kind1, int *__restrict__ cand, int *__restrict__ flag, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * nc) return;
  const int w = e / nc, q = e - w * nc, kind = q ? kind1 : kind0;
  const long cw = (long)w * sites;
  const int c0 = cfg[cw + s0], c1 = cfg[cw + s1], c2 = cfg[cw + s2], c3 = cfg[cw + s3];
  int *c = cand + 4 * (long)e;
  if (kind == LEFTUP_TO_RIGHTDOWN) { c[0] = c2; c[1] = c1; c[2] = c0; c[3] = c3; flag[e] = c0 == c2 ? 1 : -1; }
  else { c[0] = c0; c[1] = c3; c[2] = c2; c[3] = c1; flag[e] = c1 == c3 ? 1 : -1; }
}

inline std::atomic<long> &nnn_slice_calls() {   // completed nnn_exchange_slice calls of the process (pepsgpu_diag_nnn_slice_calls)
  static std::atomic<long> n{0};
  return n;
}

inline std::atomic<long> &link_slice_calls() {   // completed link_exchange_slice calls of the process (pepsgpu_diag_link_slice_calls)
  static std::atomic<long> n{0};
  return n;
}

// The closure of the pair slices, trace_dot4_kernel: out[w * w_stride + (q ? slot1 : slot0)] = a . b exp(lsum[w]) of entry (w, q)
// (an entry whose flag is >= 0 keeps what the table holds); gives the halves back.
template <typename T>
void Engine<T>::close_dot4(PlaqHalves &h, int nc, const int *flag, int slot0, int slot1, long w_stride, double *out) {
  const DTen<T> &a = h.a.t;
  hipLaunchKernelGGL((trace_dot4_kernel<T, Acc>), dim3(nw_ * nc), dim3(256), 0, stream_, (const T *)a.p, (const T *)h.b.t.p, a.n, a.d[0],
                     a.d[1], a.d[2], a.d[3], (const double *)h.lsum, flag, nc, slot0, slot1, w_stride, out);
  PG_CHECK_HIP(hipGetLastError());
  free_halves(h);
}

// The walk the two-row slices share, over the windows of the row pair (HORIZONTAL) / column pair (VERTICAL) that starts at slice1.
// Kind k is bit k of the mask: 0 / 1 the diagonals of the plaquette at position j (span 1, a row pair only), 2 / 3 the sqrt5 links of
// the 2 x 3 / 3 x 2 window at j (span 2, while j + 2 < N); even kinds join the upper-left and the lower-right corner, odd ones the
// other two.  The pair and the mask (legal: the bits a caller may set) are checked and the BMPS of the pair probed (status 3 before
// anything is touched); the value table dval [ntab] is zeroed; begin() states the slice's own refusals and sets up its BTen2 chains.
// Per window the requested kinds whose ends differ for ANY walker (differ(w, sa, sb) on the host mirror) are packed into a
// RowPairPlaq and window(p, dval) runs under its own ArenaScope where there is one (else nothing is launched and the zeros stay);
// advance(j) moves the chains on after every position; epilogue(dval), then ONE read-back of the table into host_out.
template <typename T>
template <typename Differ, typename Begin, typename Window, typename Advance, typename Epilogue>
void Engine<T>::pair_walk(const char *what, int orient, int slice1, int mask, int legal, size_t ntab, double *host_out, Differ &&differ,
                          Begin &&begin, Window &&window, Advance &&advance, Epilogue &&epilogue) {
  const bool hor = orient == HORIZONTAL;
  const int N = hor ? Lx_ : Ly_;
  PG_REQUIRE(slice1 >= 0 && slice1 + 1 < (hor ? Ly_ : Lx_), 1, std::string(what) + ": slice pair outside the lattice");
  PG_REQUIRE(mask >= 1 && !(mask & ~legal), 1, std::string(what) + ": the mask must be non-zero and within " + std::to_string(legal));
  (void)bmps_at_slice(hor ? UP : LEFT, slice1);
  (void)bmps_at_slice(hor ? DOWN : RIGHT, slice1 + 1);
  ArenaBuf<double> dval(arena_, ntab);
  PG_CHECK_HIP(hipMemsetAsync(dval, 0, sizeof(double) * ntab, stream_));
  begin();
  for (int j = 0; j + (hor ? 1 : 2) < N; ++j) {
    for (int span = hor ? 1 : 2; span <= 2 && j + span < N; ++span) {
      const int s0 = hor ? slice1 * Lx_ + j : j * Lx_ + slice1, down = (hor ? 1 : span) * Lx_, right = hor ? span : 1;
      RowPairPlaq p{j, span, {s0, s0 + down, s0 + down + right, s0 + right}, {0, 0}, 0};
      for (int q = 0; q < 2; ++q) {
        if (!((mask >> (2 * span - 2 + q)) & 1)) continue;
        bool any = false;
        for (int w = 0; w < nw_ && !any; ++w) any = differ(w, p.s[q], p.s[q + 2]);
        if (any) p.kinds[p.nc++] = 2 * span - 2 + q;
      }
      if (p.nc > 0) {
        ArenaScope scope(arena_);
        window(p, (double *)dval);
      }
    }
    advance(j);
  }
  epilogue((double *)dval);
  PG_CHECK_HIP(hipMemcpyAsync(host_out, dval, sizeof(double) * ntab, hipMemcpyDeviceToHost, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
}

// The window body of the two exchange slices: the candidates of corner_exchange_cand_kernel (dcand: candidates [n][2][4], then flags
// [n][2]) between the growing BTen2 before the window and the one behind it -- the intermediate tensors of replace_nnn_trace /
// replace_sqrt5_trace over the candidates -- closed by trace_dot4_kernel, which writes psi' = res exp(lsum) straight into slot
// `kind` of position p.j of the value table dval [n][N - 1][nk].
template <typename T>
void Engine<T>::exchange_window(int orient, int slice1, const RowPairPlaq &p, int *dcand, int nk, double *dval) {
  const bool hor = orient == HORIZONTAL;
  const int nc = p.nc, k0 = p.kinds[0], k1 = p.kinds[nc - 1], lo = hor ? LEFT : UP, np = (hor ? Lx_ : Ly_) - 1;
  int *dflag = dcand + 8 * (size_t)nw_;
  const int replaced[4] = {0, 1, 2, 3};
  hipLaunchKernelGGL(corner_exchange_cand_kernel, dim3((nw_ * nc + 255) / 256), dim3(256), 0, stream_, (const int *)cfg_, Ly_ * Lx_, p.s[0],
                     p.s[1], p.s[2], p.s[3], nc, k0 & 1, k1 & 1, dcand, dflag, nw_);
  PG_CHECK_HIP(hipGetLastError());
  PG_REQUIRE(bten2_size(lo) > p.j, 3, "exchange slice: growing BTen2 missing");
  PlaqHalves h = window_halves(orient, p.span, hor ? slice1 : p.j, hor ? p.j : slice1, bten2_[lo][p.j],
                               bten2_at_slice(hor ? RIGHT : DOWN, p.j + p.span), dcand, 4, replaced, nc, dflag);
  close_dot4(h, nc, dflag, k0, k1, (long)np * nk, dval + (size_t)kOut * nk * p.j);
}

// One row pair of the diagonal-bond pass on the device: InitBTen2(LEFT, row1), GrowFullBTen2(RIGHT, row1, 2, init), then for every
// column the amplitudes of the configuration with the ends of each requested diagonal exchanged and ShiftBTen2Window(RIGHT, row1)
// (after the last column too, as the host loop does) -- ONE read-back at the end (pair_walk).  Bosonic configurations: the
// walkers' own table, no configuration override active (status 3 otherwise).  diag_mask: bit 0 LEFTUP_TO_RIGHTDOWN, bit 1
// LEFTDOWN_TO_RIGHTUP.  val_out [n][Lx - 1][2] (complex: interleaved): 0.0 for a diagonal that is not in the mask and for an identity
// move.  A diagonal that is masked off, or the identity for EVERY walker (the host mirror of the configurations tells), is no
// candidate at all (the `any` test of the per-bond hooks); a plaquette without candidates only shifts the window.
template <typename T>
void Engine<T>::nnn_exchange_slice(int row1, int diag_mask, double *val_out) {
  require_ready();
  PG_REQUIRE(val_out, 1, "null buffer");
  PG_REQUIRE(Lx_ >= 2, 1, "diagonal slice: row pair outside the lattice");
  const int sites = Ly_ * Lx_;
  ArenaBuf<int> dcand(arena_, 10 * (size_t)nw_);
  pair_walk(
      "diagonal slice", HORIZONTAL, row1, diag_mask, 3, (size_t)kOut * nw_ * (Lx_ - 1) * 2, val_out,
      [&](int w, int sa, int sb) { return hcfg_[(size_t)w * sites + sa] != hcfg_[(size_t)w * sites + sb]; },
      [&] {
        // (the candidate kernel reads the walkers' own configuration table for all four sites of a plaquette: a configuration override
        // -- cfg_override_slice, a BMPSWalker operation -- would be ignored where the per-plaquette calls honour it, so it is refused)
        PG_REQUIRE(!ovr_on_, 3, "diagonal slice: a configuration override is active (bosonic configurations only)");
        init_bten2(LEFT, row1);
        grow_full_bten2(RIGHT, row1, 2, 1);
      },
      [&](const RowPairPlaq &p, double *dval) { exchange_window(HORIZONTAL, row1, p, dcand, 2, dval); },
      [&](int) { shift_bten2_window(RIGHT, row1); }, [](double *) {});
  nnn_slice_calls() += 1;
}

// One row pair (HORIZONTAL, slice1 = row r) or column pair (VERTICAL, slice1 = column c) of the link pass of the triangular J1-J2 model
// on the device, ONE read-back at the end and no upload (pair_walk).  link_mask bit k requests kind k:
//   HORIZONTAL  0 diagonal (r, c)-(r+1, c+1), 1 diagonal (r+1, c)-(r, c+1), 2 flat link (r, c)-(r+1, c+2), 3 flat link (r+1, c)-(r, c+2);
//   VERTICAL    2 steep link (r, c)-(r+2, c+1), 3 steep link (r+2, c)-(r, c+1)   (bits 0 and 1: status 1).
// HORIZONTAL: InitBTen2(LEFT, r), GrowFullBTen2(RIGHT, r, 2, init), then per column the diagonals, the flat links and
// ShiftBTen2Window(RIGHT, r), after the last column too.  VERTICAL (Ly >= 3): InitBTen2(UP, c), GrowFullBTen2(DOWN, c, 3, init), then
// per row the steep links and ShiftBTen2Window(DOWN, c) while row + 3 < Ly.  val_out [n][N - 1][4] (N = Lx / Ly; complex:
// interleaved): the amplitude with the two end states of the link exchanged; 0.0 for a kind that is masked off, for equal end states
// and where the window has no such link.  Bosonic configurations only: an active configuration override is status 3.
template <typename T>
void Engine<T>::link_exchange_slice(int orient, int slice1, int link_mask, double *val_out) {
  require_ready();
  PG_REQUIRE(val_out, 1, "null buffer");
  PG_REQUIRE(orient == HORIZONTAL || orient == VERTICAL, 1, "bad orientation");
  const bool hor = orient == HORIZONTAL;
  PG_REQUIRE(hor || Ly_ >= 3, 1, "link slice: a column pair needs three rows");
  const int N = hor ? Lx_ : Ly_, sites = Ly_ * Lx_, lo = hor ? LEFT : UP, hi = hor ? RIGHT : DOWN;
  ArenaBuf<int> dcand(arena_, 10 * (size_t)nw_);
  pair_walk(
      "link slice", orient, slice1, link_mask, hor ? 15 : 12, (size_t)kOut * nw_ * (N - 1) * 4, val_out,
      [&](int w, int sa, int sb) { return hcfg_[(size_t)w * sites + sa] != hcfg_[(size_t)w * sites + sb]; },
      [&] {
        // (the candidate kernel reads the walkers' own configuration table, as in nnn_exchange_slice)
        PG_REQUIRE(!ovr_on_, 3, "link slice: a configuration override is active (bosonic configurations only)");
        init_bten2(lo, slice1);
        grow_full_bten2(hi, slice1, hor ? 2 : 3, 1);
      },
      [&](const RowPairPlaq &p, double *dval) { exchange_window(orient, slice1, p, dcand, 4, dval); },
      [&](int j) { if (hor || j + 3 < N) shift_bten2_window(hi, slice1); }, [](double *) {});
  link_slice_calls() += 1;
}

// ---- the fermionic diagonal hop of a row pair (square_spinless_fermion.h:161-200, square_tJ_model.h:424-463) ----
// A fermionic state lives on the device as extended states e = s + d v: physical state s, variant v = parity of the fermion count up
// to and including the site in row-major order (pepsgpu.h).  The hop along a plaquette diagonal exchanges the physical states of its
// two ends; the variants of the four plaquette sites under the hopped configuration follow from the four extended states alone.
// e0 .. e3 = the states of (r, c), (r+1, c), (r+1, c+1), (r, c+1), n_k = occ bit of s_k:
//   before0 = v0 ^ n0          fermions strictly before (r, c)
//   mid     = (v1 ^ n1) ^ v3   fermions strictly between (r, c+1) and (r+1, c): the rest of row r and the start of row r+1
// and with the hopped states s', n' = occ(s'): v0' = before0 ^ n0', v3' = v0' ^ n3', v1' = v3' ^ mid ^ n1', v2' = v1' ^ n2'.
// Jordan-Wigner sign of the hop: (r, c) <-> (r+1, c+1) crosses (r, c+1) .. (r+1, c), (-1)^(v0 ^ v1); (r+1, c) <-> (r, c+1) crosses
// the sites between them, (-1)^mid.  The variants of every OTHER site between the two ends flip: the twisted environments of
// nnn_hop_slice_fermion.
// own[w][4] = e0 .. e3 (optional); per entry (w, q), kind = q ? kind1 : kind0: cand[w][q][4] the hopped extended states, flag[w][q] = -1
// where the hop is allowed (occ differs at the two ends; batch_flag convention: -1 has work) else 1, sign[w * sign_stride + kind] =
// +1 / -1 / 0 (forbidden).
__global__ void nnn_hop_cand_kernel(const int *__restrict__ cfg, int sites, int s0, int s1, int s2, int s3, int d, unsigned occ_bits,
                                    int nc, int kind0, int kind1, int *__restrict__ own, int *__restrict__ cand, int *__restrict__ flag,
                                    int *__restrict__ sign, long sign_stride, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * nc) return;
  const int w = e / nc, q = e - w * nc, kind = q ? kind1 : kind0;
  const long cw = (long)w * sites;
  const int e0 = cfg[cw + s0], e1 = cfg[cw + s1], e2 = cfg[cw + s2], e3 = cfg[cw + s3];
  if (own && q == 0) { int *o = own + 4 * (long)w; o[0] = e0; o[1] = e1; o[2] = e2; o[3] = e3; }
  const int p0 = e0 % d, p1 = e1 % d, p2 = e2 % d, p3 = e3 % d;
  const int v0 = (e0 / d) & 1, v1 = (e1 / d) & 1, v3 = (e3 / d) & 1;
  auto occ = [&](int s) { return (int)((occ_bits >> s) & 1u); };
  const int before0 = v0 ^ occ(p0), mid = (v1 ^ occ(p1)) ^ v3;
  const bool lurd = kind == LEFTUP_TO_RIGHTDOWN;
  const int h0 = lurd ? p2 : p0, h1 = lurd ? p1 : p3, h2 = lurd ? p0 : p2, h3 = lurd ? p3 : p1;
  const int w0 = before0 ^ occ(h0), w3 = w0 ^ occ(h3), w1 = w3 ^ mid ^ occ(h1), w2 = w1 ^ occ(h2);
  int *c = cand + 4 * (long)e;
  c[0] = h0 + d * w0; c[1] = h1 + d * w1; c[2] = h2 + d * w2; c[3] = h3 + d * w3;
  const bool allowed = lurd ? occ(p0) != occ(p2) : occ(p1) != occ(p3);
  flag[e] = allowed ? -1 : 1;
  const int par = lurd ? (v0 ^ v1) : mid;
  sign[(long)w * sign_stride + kind] = allowed ? (par ? -1 : 1) : 0;
}

// dst = the configuration table with the variant of every site of row `row` flipped: e -> e + d if e / d == 0, else e - d
__global__ void nnn_flip_row_kernel(const int *__restrict__ cfg, int *__restrict__ dst, int sites, int Lx, int row, int d, int n) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)n * sites) return;
  const int s = (int)(e % sites), v = cfg[e];
  dst[e] = (s / Lx == row) ? (v / d == 0 ? v + d : v - d) : v;
}

// val[e] *= sign[e] over the value table of the hop slice (complex: both components); sign 0 entries are zeros already
__global__ void nnn_hop_sign_kernel(double *__restrict__ val, const int *__restrict__ sign, int ko, long n) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  if (sign[e] < 0)
    for (int z = 0; z < ko; ++z) val[e * ko + z] = -val[e * ko + z];
}

// occ [d] (0 / 1 each, d <= 32) as the bit mask nnn_hop_cand_kernel takes; status 1 otherwise
inline unsigned hop_occ_bits(int d, const int32_t *occ) {
  PG_REQUIRE(d >= 1 && d <= 32, 1, "fermionic hop: 1 <= d <= 32 physical states");
  unsigned bits = 0;
  for (int s = 0; s < d; ++s) {
    PG_REQUIRE(occ[s] == 0 || occ[s] == 1, 1, "fermionic hop: occupation numbers must be 0 or 1");
    bits |= (unsigned)occ[s] << s;
  }
  return bits;
}

inline std::atomic<long> &nnn_hop_slice_calls() {   // completed nnn_hop_slice_fermion calls of the process
  static std::atomic<long> n{0};
  return n;
}

// One row pair of the fermionic diagonal hop on the device: the body of the row loop of the host's AddNNNHopEnergyLocal
// (peps_amd/host/qlpeps_gpu.h) with ONE read-back at the end and no upload.
//   set 0: GrowFullBTen2(RIGHT, row1, 2, true), InitBTen2(LEFT, row1) under the walkers' own configurations;
//   set 1: the RIGHT chain with row row1 variant-flipped, the LEFT chain with row row1 + 1 variant-flipped (the two flipped tables are
//   built once by nnn_flip_row_kernel; switching what the site picks read is a pointer change);
//   per plaquette psi from the walkers' own four states between the set-0 LEFT and RIGHT, jw psi' of each requested diagonal from
//   the hopped states (nnn_hop_cand_kernel) between the set-1 LEFT and RIGHT, closed by trace_dot4_kernel into the tables; then both
//   LEFT chains advance one column.
// A diagonal that is masked off or forbidden for every walker (host mirror) is no candidate; a plaquette without candidates only
// advances the chains and keeps psi_out = 0.  psi_out [n][Lx - 1], val_out [n][Lx - 1][2] (complex: interleaved).
// On return and on any error set 0 is selected and no override is active; set 1 keeps the twisted chains of this row pair.
template <typename T>
void Engine<T>::nnn_hop_slice_fermion(int row1, int d, const int32_t *occ, int diag_mask, double *psi_out, double *val_out) {
  require_ready();
  PG_REQUIRE(psi_out && val_out && occ, 1, "null buffer");
  PG_REQUIRE(d >= 1 && 4 * d == dp_, 1, "hop slice: the context's physical dimension must be 4 d (extended states), d <= 32");
  PG_REQUIRE(Lx_ >= 2, 1, "hop slice: row pair outside the lattice");
  const unsigned occ_bits = hop_occ_bits(d, occ);
  const int row2 = row1 + 1, sites = Ly_ * Lx_, np = Lx_ - 1;
  auto hocc = [&](int w, int s) { return (occ_bits >> (hcfg_[(size_t)w * sites + s] % d)) & 1u; };
  const size_t npsi = (size_t)kOut * nw_ * np, nval = 2 * npsi;               // the table: psi [n][np], then val [n][np][2]
  ArenaBuf<int> dflip(arena_, 2 * (size_t)nw_ * sites);                       // the table with row1 flipped, with row2 flipped
  int *flip0 = dflip, *flip1 = dflip + (size_t)nw_ * sites;
  ArenaBuf<int> dcand(arena_, 14 * (size_t)nw_ + 2 * (size_t)nw_ * np);       // own [n][4], candidates [n][2][4], flags [n][2], signs [n][np][2]
  int *down = dcand, *dhcand = dcand + 4 * (size_t)nw_, *dflag = dcand + 12 * (size_t)nw_, *dsign = dcand + 14 * (size_t)nw_;
  const int replaced[4] = {0, 1, 2, 3};
  std::vector<double> h(npsi + nval);
  TwistScope twist{*this};
  pair_walk(
      "hop slice", HORIZONTAL, row1, diag_mask, 3, npsi + nval, h.data(), [&](int w, int sa, int sb) { return hocc(w, sa) != hocc(w, sb); },
      [&] {
        PG_REQUIRE(!ovr_on_ && bten2_active_ == 0, 3, "hop slice: a configuration override or the second BTen2 set is active");
        for (int w = 0; w < nw_; ++w)
          for (int s = row1 * Lx_; s < (row2 + 1) * Lx_; ++s)
            PG_REQUIRE(hcfg_[(size_t)w * sites + s] / d < 2, 3, "hop slice: column-major extended states (variant >= 2) in the row pair");
        PG_CHECK_HIP(hipMemsetAsync(dsign, 0, sizeof(int) * 2 * (size_t)nw_ * np, stream_));
        const unsigned gf = (unsigned)(((long)nw_ * sites + 255) / 256);
        hipLaunchKernelGGL(nnn_flip_row_kernel, dim3(gf), dim3(256), 0, stream_, (const int *)cfg_, flip0, sites, Lx_, row1, d, nw_);
        hipLaunchKernelGGL(nnn_flip_row_kernel, dim3(gf), dim3(256), 0, stream_, (const int *)cfg_, flip1, sites, Lx_, row2, d, nw_);
        PG_CHECK_HIP(hipGetLastError());
        twist.use(0, nullptr, -1);
        grow_full_bten2(RIGHT, row1, 2, 1);
        init_bten2(LEFT, row1);
        twist.use(1, flip0, row1);
        grow_full_bten2(RIGHT, row1, 2, 1);
        twist.use(1, flip1, row2);
        init_bten2(LEFT, row1);
      },
      [&](const RowPairPlaq &p, double *dval) {      // (set 1 is the active one here)
        const int nc = p.nc, k0 = p.kinds[0], k1 = p.kinds[nc - 1], col1 = p.j, kr = Lx_ - 2 - col1;
        hipLaunchKernelGGL(nnn_hop_cand_kernel, dim3((nw_ * nc + 255) / 256), dim3(256), 0, stream_, (const int *)cfg_, sites, p.s[0], p.s[1],
                           p.s[2], p.s[3], d, occ_bits, nc, k0, k1, down, dhcand, dflag, dsign + 2 * col1, (long)np * 2, nw_);
        PG_CHECK_HIP(hipGetLastError());
        for (int set = 0; set < 2; ++set) {          // psi from the walkers' own four states, then jw psi' from the hopped ones
          const std::vector<BTenDev> &ls = bten2_of_set(set, LEFT), &rs = bten2_of_set(set, RIGHT);
          PG_REQUIRE((int)ls.size() > col1 && kr >= 0 && kr < (int)rs.size(), 3, "hop slice: BTen2 environment missing");
          const int *tab = set == 0 ? down : dhcand, *fl = set == 0 ? nullptr : dflag;
          PlaqHalves hv = window_halves(HORIZONTAL, 1, row1, col1, ls[col1], rs[kr], tab, 4, replaced, set == 0 ? 1 : nc, fl);
          if (set == 0) close_dot4(hv, 1, nullptr, 0, 0, (long)np, dval + (size_t)kOut * col1);
          else close_dot4(hv, nc, dflag, k0, k1, (long)np * 2, dval + npsi + (size_t)kOut * 2 * col1);
        }
      },
      [&](int col1) {
        if (col1 + 2 >= Lx_) return;
        grow_bten2_step(LEFT, row1);                 // both LEFT chains advance over column col1 (set 1 under the flipped row row2)
        twist.use(0, nullptr, -1);
        grow_bten2_step(LEFT, row1);
        twist.use(1, flip1, row2);
      },
      [&](double *dval) {
        twist.use(0, nullptr, -1);
        const long ne = (long)nw_ * np * 2;
        hipLaunchKernelGGL(nnn_hop_sign_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, stream_, dval + npsi, (const int *)dsign,
                           kOut, ne);
        PG_CHECK_HIP(hipGetLastError());
      });
  std::copy(h.begin(), h.begin() + npsi, psi_out);
  std::copy(h.begin() + npsi, h.end(), val_out);
  nnn_hop_slice_calls() += 1;
}

// ---- pair moves on the nearest-neighbour bonds of a fermionic state (the bond-singlet order of the t-J model,
// square_tJ_model.h:546-603: the two electrons of a bond removed, or put into an empty bond) ----
// The two sites of a bond along a row (column) are adjacent in the row-major (column-major) mode order, so a move that keeps the
// fermion parity of the pair changes the variants of these two sites only (extended state e = s + d v: v = 0 / 1 the parity of the
// fermions up to and including the site in row-major order, v = 2 / 3 that of the fermions strictly before it in column-major order):
//   row-major     before = v1 ^ n(a);  e1' = a' + d (before ^ n(a')),      e2' = b' + d (before ^ n(a') ^ n(b'))
//   column-major  before = v1 & 1;     e1' = a' + d (2 + before),          e2' = b' + d (2 + (before ^ n(a')))
// the rule of the exchange table of the host layer (TPSWaveFunctionComponent::ExchangeTable) for any (a', b').  ptab [d * d][2][2]
// over PHYSICAL states: candidate k of the pair (a, b) is (a'_k, b'_k), (-1, -1) for none.  Per walker nc = (xtab ? 1 : 0) + 2 slots
// cand [n][nc][2]: the exchange slot first when xtab [dp * dp][2] (the table of sweep_swap_cand_kernel over extended states) is given,
// with same[w] = 1 where that move is the identity, then the two pair slots; a walker without candidate k keeps its own two states
// in that slot.  sign [n][2] = Sigma(S') / Sigma(S) of the decoration, Sigma = (-1)^(nf (nf + 1) / 2): -1 where the fermion number
// changes by +-2, +1 where it is unchanged, 0 for "no candidate".
__global__ void pair_cand_kernel(const int *__restrict__ cfg, int sites, int s1, int s2, int d, unsigned occ_bits, int col_major,
                                 const int *__restrict__ ptab, const int *__restrict__ xtab, int dp, int *__restrict__ cand,
                                 int *__restrict__ same, int *__restrict__ sign, int n) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  const int e1 = cfg[(long)w * sites + s1], e2 = cfg[(long)w * sites + s2];
  const int a = e1 % d, b = e2 % d;
  auto occ = [&](int s) { return (int)((occ_bits >> s) & 1u); };
  const int before = col_major ? ((e1 / d) & 1) : (((e1 / d) & 1) ^ occ(a));
  const int slot0 = xtab ? 1 : 0, nc = slot0 + 2;
  int *c = cand + 2 * (long)w * nc;
  if (xtab) {
    const int x1 = xtab[2 * (e1 * dp + e2)], x2 = xtab[2 * (e1 * dp + e2) + 1];
    c[0] = x1;
    c[1] = x2;
    same[w] = (x1 == e1 && x2 == e2);
  }
  for (int k = 0; k < 2; ++k) {
    const int pa = ptab[4 * (a * d + b) + 2 * k], pb = ptab[4 * (a * d + b) + 2 * k + 1];
    int c1 = e1, c2 = e2, sg = 0;
    if (pa >= 0) {
      const int na = occ(pa), nb = occ(pb);
      c1 = pa + d * (col_major ? 2 + before : before ^ na);
      c2 = pb + d * (col_major ? 2 + (before ^ na) : before ^ na ^ nb);
      sg = (na + nb == occ(a) + occ(b)) ? 1 : -1;
    }
    c[2 * (slot0 + k)] = c1;
    c[2 * (slot0 + k) + 1] = c2;
    sign[2 * w + k] = sg;
  }
}

// The values of one bond of the pair slice into the table out [n][stride] of AccT scalars (stored as doubles, complex interleaved):
// res [n][nc] with lsum [n] from the replacement trace over the slots of pair_cand_kernel.  The exchange slot (same != nullptr) goes
// to column ex_col -- psi of the bond, already in column psi_col, where the move is the identity; pair slot k goes to column
// pair_col + k as sign res exp(lsum), exactly 0.0 where sign is 0.
template <typename AccT>
__global__ void pair_store_kernel(const AccT *__restrict__ res, const double *__restrict__ lsum, const int *__restrict__ sign,
                                  const int *__restrict__ same, double *__restrict__ out, int stride, int psi_col, int ex_col,
                                  int pair_col, int n) {
  constexpr int ko = (int)(sizeof(AccT) / sizeof(double));
  const int slot0 = same ? 1 : 0, nc = slot0 + 2;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * nc) return;
  const int w = e / nc, q = e - w * nc;
  if (q < slot0) {
    double *o = out + ((long)w * stride + ex_col) * ko;
    if (same[w]) {
      const double *src = out + ((long)w * stride + psi_col) * ko;
      for (int z = 0; z < ko; ++z) o[z] = src[z];
    } else {
      sw_put(o, sw_scaled(res[e], exp(lsum[w])));
    }
    return;
  }
  const int k = q - slot0, sg = sign[2 * w + k];
  double *o = out + ((long)w * stride + pair_col + k) * ko;
  if (sg == 0) {
    for (int z = 0; z < ko; ++z) o[z] = 0.0;
  } else {
    sw_put(o, sw_scaled(res[e], (double)sg * exp(lsum[w])));
  }
}

// the tables of a pair slice as the host hands them over: occ [d] (status 1 outside {0, 1}); pair_table [d * d][2][2] with entries in
// [-1, d), a candidate either (-1, -1) or two states that keep the fermion parity of the pair (status 1 otherwise)
inline unsigned require_pair_tables(int d, const int32_t *occ, const int32_t *pair_table) {
  const unsigned occ_bits = hop_occ_bits(d, occ);
  for (int a = 0; a < d; ++a)
    for (int b = 0; b < d; ++b)
      for (int k = 0; k < 2; ++k) {
        const int pa = pair_table[4 * (a * d + b) + 2 * k], pb = pair_table[4 * (a * d + b) + 2 * k + 1];
        PG_REQUIRE(pa >= -1 && pa < d && pb >= -1 && pb < d, 1, "pair table: entry outside [-1, d)");
        PG_REQUIRE((pa < 0) == (pb < 0), 1, "pair table: a candidate with only one -1");
        PG_REQUIRE(pa < 0 || ((occ[pa] + occ[pb] + occ[a] + occ[b]) & 1) == 0, 1, "pair table: a candidate changes the fermion parity of the pair");
      }
  return occ_bits;
}

inline std::atomic<long> &pair_slice_calls() {   // completed nn_pair_slice_fermion calls of the process (pepsgpu_diag_pair_slice_calls)
  static std::atomic<long> n{0};
  return n;
}

// One row / column of a fermionic context for the measurement of pair operators next to the bond energy: the sibling of mode 0 of
// energy_slice_impl with psi per bond and without holes (GrowFullBTen(.., 2), the window shifted while j + 2 < N).  Per bond one
// Trace (psi), the candidates of pair_cand_kernel built on the device from the walkers' own configuration table, ONE replacement
// trace over all of them and pair_store_kernel; ONE read-back at the end, no per-bond upload.  psi_out [n][N - 1], ex_out [n][N - 1]
// (written when exchange_table is given), pair_out [n][N - 1][2]; complex: interleaved.
template <typename T>
void Engine<T>::nn_pair_slice_fermion(int orient, int slice, int d, const int32_t *occ, const int32_t *pair_table,
                                      const int32_t *exchange_table, double *psi_out, double *ex_out, double *pair_out) {
  nn_pair_slice_body(orient, slice, 0, d, occ, pair_table, exchange_table, psi_out, ex_out, pair_out);
  pair_slice_calls() += 1;
}

inline std::atomic<long> &hop_slice_calls() {    // completed nn_hop_slice_fermion calls of the process (pepsgpu_diag_hop_slice_calls)
  static std::atomic<long> n{0};
  return n;
}

// The pair slice without an exchange slot for models whose bond term is up to two hops (the Hubbard model, square_hubbard_model.h:
// 200-262: Trace + ReplaceNNSiteTrace of the hopped pairs per bond).  punch_holes != 0: the row pass of the energy evaluation,
// GrowFullBTen(.., 1, true), the hole of every site punched into HBM before that site's bond and the window shifted after the last
// bond too (mode 0 of energy_slice_impl).
template <typename T>
void Engine<T>::nn_hop_slice_fermion(int orient, int slice, int punch_holes, int d, const int32_t *occ, const int32_t *hop_table,
                                     double *psi_out, double *hop_out) {
  nn_pair_slice_body(orient, slice, punch_holes, d, occ, hop_table, nullptr, psi_out, nullptr, hop_out);
  hop_slice_calls() += 1;
}

// The body of the two entries above.  punch_holes == 0 is the pair slice as described there; punch_holes != 0 grows the shrinking
// environment down to the last ONE position, punches the hole of site j before bond j (and of the last site after the last bond) and
// shifts the window after every bond.
template <typename T>
void Engine<T>::nn_pair_slice_body(int orient, int slice, int punch_holes, int d, const int32_t *occ, const int32_t *pair_table,
                                   const int32_t *exchange_table, double *psi_out, double *ex_out, double *pair_out) {
  require_ready();
  const SliceGeom g(orient, slice, Lx_, Ly_);
  PG_REQUIRE(occ && pair_table && psi_out && pair_out && (!exchange_table || ex_out), 1, "null buffer");
  PG_REQUIRE(d >= 1 && 4 * d == dp_, 1, "pair slice: the context's physical dimension must be 4 d (extended states), d <= 32");
  const unsigned occ_bits = require_pair_tables(d, occ, pair_table);
  const size_t xlen = exchange_table ? 2 * (size_t)dp_ * dp_ : 0;
  require_states(exchange_table, xlen, dp_, "pair slice: exchange table state out of range");
  const bool hor = orient == HORIZONTAL;
  const int N = g.N, sites = Ly_ * Lx_, np = N - 1;
  (void)bmps_at_slice(hor ? UP : LEFT, slice);
  (void)bmps_at_slice(hor ? DOWN : RIGHT, slice);
  // (the candidate kernel reads the walkers' own configuration table: an override would be ignored where the per-bond calls honour it)
  PG_REQUIRE(!ovr_on_, 3, "pair slice: a configuration override is active");
  for (int w = 0; w < nw_; ++w)
    for (int j = 0; j < N; ++j)
      PG_REQUIRE((hcfg_[(size_t)w * sites + g.site(j)] / d >= 2) == !hor, 3,
                 "pair slice: extended states of the other mode order in the slice (rows: variants 0 / 1, columns: 2 / 3)");
  const int slot0 = exchange_table ? 1 : 0, nc = slot0 + 2;
  // value table [n][stride] of Acc scalars: psi of bond j in column j, its exchanged amplitude in np + j, its pair slots in 2 np + 2 j + k
  const int stride = 4 * np;
  ArenaBuf<double> dval(arena_, kOut * (size_t)nw_ * std::max(stride, 1));
  ArenaBuf<int> dcand(arena_, (2 * (size_t)nc + 3) * (size_t)nw_);           // candidates [n][nc][2], same [n], signs [n][2]
  int *dsame = dcand + 2 * (size_t)nc * nw_, *dsign = dsame + nw_;
  ArenaBuf<int> dtab(arena_, 4 * (size_t)d * d + xlen);
  int *dxtab = exchange_table ? dtab + 4 * (size_t)d * d : nullptr;
  PG_CHECK_HIP(hipMemcpyAsync(dtab, pair_table, sizeof(int) * 4 * (size_t)d * d, hipMemcpyHostToDevice, stream_));
  if (dxtab) PG_CHECK_HIP(hipMemcpyAsync(dxtab, exchange_table, sizeof(int) * xlen, hipMemcpyHostToDevice, stream_));
  if (punch_holes && !holes_) {
    holes_ = (T *)arena_.alloc(sizeof(T) * (size_t)maxw_ * Ly_ * Lx_ * slot_);
    holes_ls_ = (double *)arena_.alloc(sizeof(double) * (size_t)maxw_ * Ly_ * Lx_);
  }
  begin_slice(g, punch_holes ? 1 : 2);
  const int gb = (nw_ + 255) / 256;
  for (int j = 0; j < N; ++j) {
    const int r1 = g.row(j), c1 = g.col(j);
    if (punch_holes) punch_hole(r1, c1, orient, nullptr);
    if (j + 1 >= N) break;
    {
      double *lsum = nullptr;
      Acc *res = nn_trace_device(r1, c1, orient, 1, nullptr, &lsum);
      hipLaunchKernelGGL(slice_store_value_kernel<Acc>, dim3(gb), dim3(256), 0, stream_, (const Acc *)res, (const double *)lsum, dval,
                         stride, j, 1, (const int *)nullptr, 0, nw_);
      PG_CHECK_HIP(hipGetLastError());
      arena_.free(res); arena_.free(lsum);
    }
    hipLaunchKernelGGL(pair_cand_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)cfg_, sites, g.site(j), g.site(j + 1), d, occ_bits,
                       hor ? 0 : 1, (const int *)dtab, (const int *)dxtab, dp_, dcand, dxtab ? dsame : nullptr, dsign, nw_);
    PG_CHECK_HIP(hipGetLastError());
    double *lsum = nullptr;
    Acc *res = nn_trace_device(r1, c1, orient, nc, dcand, &lsum);
    hipLaunchKernelGGL(pair_store_kernel<Acc>, dim3((nw_ * nc + 255) / 256), dim3(256), 0, stream_, (const Acc *)res, (const double *)lsum,
                       (const int *)dsign, dxtab ? (const int *)dsame : nullptr, dval, stride, j, np + j, 2 * np + 2 * j, nw_);
    PG_CHECK_HIP(hipGetLastError());
    arena_.free(res); arena_.free(lsum);
    if (punch_holes || j + 2 < N) shift_bten_window(g.hi);
  }
  std::vector<double> h((size_t)kOut * nw_ * stride);
  if (!h.empty()) PG_CHECK_HIP(hipMemcpyAsync(h.data(), dval, sizeof(double) * h.size(), hipMemcpyDeviceToHost, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  for (int w = 0; w < nw_; ++w) {
    const double *row = h.data() + (size_t)w * stride * kOut;
    std::copy(row, row + (size_t)np * kOut, psi_out + (size_t)w * np * kOut);
    if (exchange_table) std::copy(row + (size_t)np * kOut, row + 2 * (size_t)np * kOut, ex_out + (size_t)w * np * kOut);
    std::copy(row + 2 * (size_t)np * kOut, row + 4 * (size_t)np * kOut, pair_out + 2 * (size_t)w * np * kOut);
  }
}

// ---- three-site exchange (MCUpdateSquareTNN3SiteExchange::TNN3SiteUpdateImpl, square_3site_updater.h:109-158) ----
// Triple table [dp^3][TNN3_TAB]: entry e1 dp^2 + e2 dp + e3 holds m (the number of distinct permutations of the triple: 1, 3 or 6),
// init (the position of the triple itself among them) and six slots of three states, the permutations in std::next_permutation order
// of the sorted triple (fermions: of the sorted physical triple, as extended states); unused slots repeat slot 0.
constexpr int TNN3_TAB = 2 + 6 * 3;

// Bosonic triple table of dp states (the table pepsgpu_sweep_slice_tnn3 builds when it is given none).  The host layer states the same
// rule (TNN3TripleTable, peps_amd/host/qlpeps_gpu.h); pepsgpu_diag_tnn3_table exposes this copy so that tests/test_cpu_tnn3.py checks
// the two against each other.
inline std::vector<int32_t> tnn3_boson_table(int dp) {
  std::vector<int32_t> tab((size_t)dp * dp * dp * TNN3_TAB);
  for (int e = 0; e < dp * dp * dp; ++e) {
    const int t0[3] = {e / (dp * dp), (e / dp) % dp, e % dp};
    int p[3] = {t0[0], t0[1], t0[2]};
    std::sort(p, p + 3);
    int32_t *row = tab.data() + (size_t)e * TNN3_TAB;
    int m = 0, init = 0;
    do {
      if (p[0] == t0[0] && p[1] == t0[1] && p[2] == t0[2]) init = m;
      for (int q = 0; q < 3; ++q) row[2 + 3 * m + q] = p[q];
      ++m;
    } while (std::next_permutation(p, p + 3));
    for (int k = m; k < 6; ++k)
      for (int q = 0; q < 3; ++q) row[2 + 3 * k + q] = row[2 + q];
    row[0] = m;
    row[1] = init;
  }
  return tab;
}

// Per walker: the triple (s1, s2, s3) of the configuration looked up in the table -> nslot candidate slots cand [w][nslot][3],
// m and init (meta [w][2]) and skip[w] = (m == 1: all three states equal, no trace and no draw, :118)
__global__ void tnn3_cand_kernel(const int *__restrict__ cfg, int sites, int s1, int s2, int s3, const int *__restrict__ tab, int dp,
                                 int nslot, int *__restrict__ cand, int *__restrict__ meta, int *__restrict__ skip, int n) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  const long cw = (long)w * sites;
  const int e = (cfg[cw + s1] * dp + cfg[cw + s2]) * dp + cfg[cw + s3];
  const int *t = tab + (long)e * TNN3_TAB;
  for (int k = 0; k < 3 * nslot; ++k) cand[(long)w * 3 * nslot + k] = t[2 + k];
  meta[2 * w] = t[0];
  meta[2 * w + 1] = t[1];
  skip[w] = t[0] <= 1;
}

// amp[w] = res[w] exp(lsum[w]): the amplitude reset at the start of a slice (square_3site_updater.h:39-42)
template <typename AccT>
__global__ void tnn3_reset_amp_kernel(const AccT *__restrict__ res, const double *__restrict__ lsum, AccT *__restrict__ amp, int n) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w < n) amp[w] = sw_scaled(res[w], exp(lsum[w]));
}

__device__ __forceinline__ double sw_norm_div(double x, double s) { const double r = x / s; return r * r; }
__device__ __forceinline__ double sw_norm_div(const cplx<double> &x, double s) {
  const double re = x.re / s, im = x.im / s;
  return re * re + im * im;
}

// :123-156 for one triple: psis (the stored amplitude at init), weights norm(psi / max |psi|), SuwaTodoStateUpdate with the walker's
// next two engine words (taken only when m > 1, counted in used[w]), and the move
template <typename AccT>
__global__ void tnn3_decide_kernel(int *__restrict__ cfg, int sites, int s1, int s2, int s3, const AccT *__restrict__ res,
                                   const double *__restrict__ lsum, AccT *__restrict__ amp, const int *__restrict__ cand,
                                   const int *__restrict__ meta, int nslot, const unsigned *__restrict__ words, int n_words,
                                   int *__restrict__ used, int *__restrict__ acc, int n) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  const int m = meta[2 * w], init = meta[2 * w + 1];
  if (m <= 1) return;
  const double sc = exp(lsum[w]);
  const AccT a0 = amp[w];
  // (psi_i recomputed in each unrolled loop rather than kept in an array indexed at run time: that array went to scratch)
  auto psi = [&](int i) { return i == init ? a0 : sw_scaled(AccT(res[(long)w * nslot + i]), sc); };
  double mx = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (i < m) mx = fmax(mx, sw_abs(psi(i)));
  double wt[SW_MAXC];
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (i < m) wt[i] = sw_norm_div(psi(i), mx);
  const int q = used[w];
  const unsigned *wd = words + (long)w * n_words + q;
  const int fin = sw_suwa_todo_decide(wt, m, init, wd[0], wd[1]);
  used[w] = q + 2;
  if (fin != init) {
    const int *c = cand + ((long)w * nslot + fin) * 3;
    cfg[(long)w * sites + s1] = c[0];
    cfg[(long)w * sites + s2] = c[1];
    cfg[(long)w * sites + s3] = c[2];
    amp[w] = psi(fin);
    acc[w] += 1;
  }
}

// One row / column of three-site exchange moves (MCUpdateSquareTNN3SiteUpdateBase::operator(), square_3site_updater.h:28-91):
// InitBTen + GrowFullBTen(.., 3), the amplitude reset to the trace of the first window, then per triple the candidates from the
// triple table, their replacement traces (walkers with three equal states skipped), the Suwa-Todo decision and the move, and the
// BTen window shift -- one read-back at the end.
// Environment bookkeeping: at triple j the pass holds LEFT over [0, j), RIGHT over [j + 3, N) and the BMPS of the other rows
// (columns); EraseEnvsAfterUpdate of the sites j .. j + 2 only drops LEFT beyond j + 1 .. j + 3 and RIGHT beyond N - j - 2 .. N - j,
// levels the pass does not hold, so it is applied unconditionally as in the two-site slice.
template <typename T>
void Engine<T>::sweep_slice_tnn3(int orient, int slice, const int32_t *triple_table, int n_words, const uint32_t *words, double *amp_out,
                                 int32_t *consumed_out, int32_t *accepted_out, int32_t *slice_states_out) {
  require_ready();
  const SliceGeom g(orient, slice, Lx_, Ly_);
  PG_REQUIRE(Ly_ >= 3 && Lx_ >= 3, 1, "three-site slice: the lattice needs at least 3 rows and 3 columns");
  PG_REQUIRE(words && n_words >= 2 * (g.N - 2), 1, "three-site slice: two engine words per triple of the slice are needed");
  const int sites = Ly_ * Lx_, nslot = dp_ == 2 ? 3 : 6, gb = (nw_ + 255) / 256;
  const size_t ntab = (size_t)dp_ * dp_ * dp_ * TNN3_TAB;
  std::vector<int32_t> own;
  if (!triple_table) { own = tnn3_boson_table(dp_); triple_table = own.data(); }
  for (size_t e = 0; e < ntab; e += TNN3_TAB) {
    const int32_t *t = triple_table + e;
    PG_REQUIRE((t[0] == 1 || t[0] == 3 || t[0] == 6) && t[0] <= nslot && t[1] >= 0 && t[1] < t[0], 4,
               "triple table: bad permutation count or initial slot");
    require_states(t + 2, TNN3_TAB - 2, dp_, "triple table: state out of range");
  }
  ArenaBuf<Acc> damp(arena_, nw_);
  ArenaBuf<unsigned> dwords(arena_, (size_t)nw_ * n_words);
  ArenaBuf<int> dcnt(arena_, 2 * (size_t)nw_ + 1);                          // used words [n], accepted moves [n], (overrun: never set)
  ArenaBuf<int> dcand(arena_, (3 * (size_t)nslot + 3) * (size_t)nw_);
  int *dmeta = dcand + 3 * (size_t)nslot * nw_, *dskip = dmeta + 2 * (size_t)nw_;
  ArenaBuf<int> dtab(arena_, ntab);
  PG_CHECK_HIP(hipMemcpyAsync(dwords, words, sizeof(unsigned) * (size_t)nw_ * n_words, hipMemcpyHostToDevice, stream_));
  PG_CHECK_HIP(hipMemcpyAsync(dtab, triple_table, sizeof(int) * ntab, hipMemcpyHostToDevice, stream_));
  sweep_slice_frame(g, 3, damp, dcnt, amp_out, consumed_out, accepted_out, slice_states_out, [&] {
    {
      double *lsum = nullptr;
      Acc *res = tnn_trace_device(g.row(0), g.col(0), orient, 1, nullptr, &lsum);
      hipLaunchKernelGGL(tnn3_reset_amp_kernel<Acc>, dim3(gb), dim3(256), 0, stream_, (const Acc *)res, (const double *)lsum, damp, nw_);
      PG_CHECK_HIP(hipGetLastError());
      arena_.free(res);
      arena_.free(lsum);
    }
    for (int j = 0; j + 2 < g.N; ++j) {
      const int s1 = g.site(j), s2 = g.site(j + 1), s3 = g.site(j + 2);
      hipLaunchKernelGGL(tnn3_cand_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)cfg_, sites, s1, s2, s3, (const int *)dtab, dp_,
                         nslot, dcand, dmeta, dskip, nw_);
      PG_CHECK_HIP(hipGetLastError());
      double *lsum = nullptr;
      Acc *res = tnn_trace_device(g.row(j), g.col(j), orient, nslot, dcand, &lsum, dskip);
      hipLaunchKernelGGL(tnn3_decide_kernel<Acc>, dim3(gb), dim3(256), 0, stream_, cfg_, sites, s1, s2, s3, (const Acc *)res,
                         (const double *)lsum, damp, (const int *)dcand, (const int *)dmeta, nslot, (const unsigned *)dwords, n_words,
                         dcnt, dcnt + nw_, nw_);
      PG_CHECK_HIP(hipGetLastError());
      arena_.free(res);
      arena_.free(lsum);
      for (int k = 0; k < 3; ++k) erase_envs_after_update(g.row(j + k), g.col(j + k));
      if (j + 3 < g.N) shift_bten_window(g.hi);
    }
  });
}

template <typename T>
void Engine<T>::grow_bten_step_reuse(int pos, ArenaBuf<T> &half, long half_n, const int *take) {
  require_ready();
  int pre = (pos + 3) % 4, nxt = (pos + 1) % 4;
  int bs = bten_size(pos);
  PG_REQUIRE(bs > 0, 3, "GrowBTenStep: BTen not initialised");
  int n, r, c;
  switch (pos) {
    case DOWN: c = bmps_size(LEFT) - 1; n = Ly_; r = n - bs; break;
    case UP: c = bmps_size(LEFT) - 1; n = Ly_; r = bs - 1; break;
    case LEFT: r = bmps_size(UP) - 1; n = Lx_; c = bs - 1; break;
    default: r = bmps_size(UP) - 1; n = Lx_; c = n - bs; break;
  }
  PG_REQUIRE(bs <= n && !bmps_[pre].empty() && !bmps_[nxt].empty(), 3, "GrowBTenStep: environment missing");
  SiteSel sel = cfg_site(r, c);
  const BMPSDev &b1 = bmps_[pre].back(), &b2 = bmps_[nxt].back();
  auto lv = [](const BMPSDev &b, int j) -> const int * { return (int)b.live.size() > j ? b.live[j] : nullptr; };
  const BTenDev &bt = bten_[pos].back();
  BTenDev nb = bten_step(pos, bt, b1.t[n - bs], sel, b2.t[bs - 1], 1, false, 1, lv(b1, n - bs), lv(b1, n - bs + 1), lv(b2, bs - 1),
                         lv(b2, bs), take);
  try {      // (nb is not owned by anything yet: an error below must not leave it in the arena)
    PG_REQUIRE(nb.t.n == half_n, 3, "GrowBTenStep: the kept half step has another shape");
    hipLaunchKernelGGL(sweep_take_kernel<T>, dim3((unsigned)std::min<long>(8, (nb.t.n + 255) / 256), nw_), dim3(256), 0, stream_, nb.t.p,
                       (const T *)half, (long)nb.t.n, take);
    PG_CHECK_HIP(hipGetLastError());
    half.reset();
    nb.logscale = (double *)arena_.alloc(sizeof(double) * nw_);
    PG_CHECK_HIP(hipMemcpyAsync(nb.logscale, bt.logscale, sizeof(double) * nw_, hipMemcpyDeviceToDevice, stream_));
    normalize(nb.t.p, nb.t.n, nb.t.n, nw_, nb.logscale);
  } catch (...) {
    if (nb.t.p) arena_.free(nb.t.p);
    if (nb.logscale) arena_.free(nb.logscale);
    throw;
  }
  bten_[pos].push_back(nb);
}

// One slice of the sweep of the exchange updater on the device: per bond the candidate (pair_table == nullptr: the swap of the two
// states; else the tabulated pair, see sweep_swap_cand_kernel), its replacement trace, the Metropolis test and the move.
// amp_inout: [n] amplitudes of the accumulation type (complex: interleaved).
template <typename T>
void Engine<T>::sweep_slice_exchange(int orient, int slice, int n_uniform, const double *uniforms, const int32_t *pair_table,
                                     double *amp_inout, int32_t *consumed_out, int32_t *accepted_out, int32_t *slice_states_out) {
  require_ready();
  const SliceGeom g(orient, slice, Lx_, Ly_);
  PG_REQUIRE(n_uniform >= g.N - 1 && uniforms, 1, "one uniform deviate per bond of the slice is needed");
  const size_t ntab = pair_table ? 2 * (size_t)dp_ * dp_ : 0;
  require_states(pair_table, ntab, dp_, "pair table: state out of range");
  const int sites = Ly_ * Lx_, gb = (nw_ + 255) / 256;
  ArenaBuf<Acc> damp(arena_, nw_);
  ArenaBuf<double> duni(arena_, (size_t)nw_ * n_uniform);
  ArenaBuf<int> dcnt(arena_, 2 * (size_t)nw_ + 1);
  int *dacc = dcnt + nw_, *dover = dcnt + 2 * nw_;
  ArenaBuf<int> dcand(arena_, 4 * (size_t)nw_);                             // candidate pair [n][2], same [n], accepted on this bond [n]
  int *dsame = dcand + 2 * (size_t)nw_, *dnow = dsame + nw_;
  ArenaBuf<int> dtab(arena_, ntab);
  ArenaBuf<T> half(arena_, 0);                                               // the kept half step of the bond in flight
  PG_CHECK_HIP(hipMemcpyAsync(damp, amp_inout, sizeof(Acc) * nw_, hipMemcpyHostToDevice, stream_));
  PG_CHECK_HIP(hipMemcpyAsync(duni, uniforms, sizeof(double) * (size_t)nw_ * n_uniform, hipMemcpyHostToDevice, stream_));
  if (dtab) PG_CHECK_HIP(hipMemcpyAsync(dtab, pair_table, sizeof(int) * ntab, hipMemcpyHostToDevice, stream_));
  sweep_slice_frame(g, 2, damp, dcnt, amp_inout, consumed_out, accepted_out, slice_states_out, [&] {
    for (int j = 0; j + 1 < g.N; ++j) {
      const int r1 = g.row(j), c1 = g.col(j), s1 = g.site(j), s2 = g.site(j + 1);
      hipLaunchKernelGGL(sweep_swap_cand_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)cfg_, sites, s1, s2, dcand, dsame, nw_,
                         (const int *)dtab, dp_);
      PG_CHECK_HIP(hipGetLastError());
      // the left half of the replacement trace IS the next environment tensor of the walkers that accept the exchange (the same
      // kernel on the same operands): it is kept, and the growth step behind the Metropolis test runs for the others only
      const bool reuse = j + 2 < g.N;
      BTenDev t2;
      double *lsum = nullptr;
      Acc *res = nn_trace_device(r1, c1, orient, 1, dcand, &lsum, dsame, reuse ? &t2 : nullptr);
      if (reuse) half.reset(t2.t.p);
      hipLaunchKernelGGL(sweep_metropolis_exchange_kernel<Acc>, dim3(gb), dim3(256), 0, stream_, cfg_, sites, s1, s2, (const Acc *)res,
                         (const double *)lsum, damp, (const double *)duni, n_uniform, dcnt, dacc, dover, dnow, nw_, (const int *)dcand,
                         (const int *)dsame);
      PG_CHECK_HIP(hipGetLastError());
      arena_.free(res);
      arena_.free(lsum);
      erase_envs_after_update(r1, c1);
      erase_envs_after_update(g.row(j + 1), g.col(j + 1));
      if (reuse) {
        clear_bten(g.hi, bten_size(g.hi) - 1);
        grow_bten_step_reuse(g.lo, half, (long)t2.t.n, dnow);
      }
    }
  });
}

// One slice of the sweep of the full-space updater on the device: per bond ONE replacement trace over all phys_dim^2 states of the
// pair, then the Suwa-Todo decision and the move (sweep_suwa_todo_kernel).  words: [n][2 (N - 1)], two engine words per bond.
template <typename T>
void Engine<T>::sweep_slice_fullspace(int orient, int slice, int phys_dim, const uint32_t *words, double *amp_inout,
                                      int32_t *accepted_out, int32_t *slice_states_out) {
  require_ready();
  const SliceGeom g(orient, slice, Lx_, Ly_);
  PG_REQUIRE(phys_dim >= 1 && phys_dim <= dp_ && phys_dim * phys_dim <= SW_MAXC && words, 1, "full-space slice: 1 <= phys_dim, phys_dim^2 <= 16, two engine words per bond");
  const int sites = Ly_ * Lx_, gb = (nw_ + 255) / 256, nc = phys_dim * phys_dim, nwords = 2 * (g.N - 1);
  ArenaBuf<Acc> damp(arena_, nw_);
  ArenaBuf<unsigned> dwords(arena_, (size_t)nw_ * nwords);
  ArenaBuf<int> dcnt(arena_, 2 * (size_t)nw_ + 1);                          // (consumed: unused, the count is fixed), accepted [n]
  ArenaBuf<int> dcand(arena_, (2 * (size_t)nc + 1) * (size_t)nw_);          // candidate pairs [n][nc][2], changed on this bond [n]
  int *dnow = dcand + 2 * (size_t)nc * nw_;
  PG_CHECK_HIP(hipMemcpyAsync(damp, amp_inout, sizeof(Acc) * nw_, hipMemcpyHostToDevice, stream_));
  PG_CHECK_HIP(hipMemcpyAsync(dwords, words, sizeof(unsigned) * (size_t)nw_ * nwords, hipMemcpyHostToDevice, stream_));
  sweep_slice_frame(g, 2, damp, dcnt, amp_inout, nullptr, accepted_out, slice_states_out, [&] {
    hipLaunchKernelGGL(sweep_all_cand_kernel, dim3((nw_ * nc + 255) / 256), dim3(256), 0, stream_, dcand, phys_dim, nw_);
    PG_CHECK_HIP(hipGetLastError());
    for (int j = 0; j + 1 < g.N; ++j) {
      double *lsum = nullptr;
      Acc *res = nn_trace_device(g.row(j), g.col(j), orient, nc, dcand, &lsum);
      hipLaunchKernelGGL(sweep_suwa_todo_kernel<Acc>, dim3(gb), dim3(256), 0, stream_, cfg_, sites, g.site(j), g.site(j + 1), phys_dim,
                         (const Acc *)res, (const double *)lsum, damp, (const unsigned *)dwords, nwords, j, dcnt + nw_, dnow, nw_);
      PG_CHECK_HIP(hipGetLastError());
      arena_.free(res);
      arena_.free(lsum);
      erase_envs_after_update(g.row(j), g.col(j));
      erase_envs_after_update(g.row(j + 1), g.col(j + 1));
      if (j + 2 < g.N) shift_bten_window(g.hi);
    }
  });
}

// ---- Suwa-Todo moves inside a tabulated sector of each bond (MCUpdateSquareNNHubbardU1U1OBC::TwoSiteNNUpdateLocalImpl,
// square_hubbard_u1u1_updater.h:95-157: the pairs with the (N_up, N_down) of the bond) ----
// Sector table [d * d][2 + 2 max_cand] over PHYSICAL states, row a * d + b of the pair (a, b): m (the size of its sector), init (the
// slot of the pair itself), then max_cand slots (a'_k, b'_k) in the order the updater enumerates them; slots m .. max_cand - 1 are
// (-1, -1).  sector_row_len is the row length.
__host__ __device__ inline int sector_row_len(int max_cand) { return 2 + 2 * max_cand; }

// The table as the host hands it over: status 4 for a state outside [-1, d); status 1 for a row with m outside [1, max_cand], init
// outside [0, m), a -1 in a used slot or a state in an unused one, a slot `init` that is not the pair itself or (fermions: occ given)
// a candidate that changes the fermion parity of the pair.  Returns the occupation bits (0 for a bosonic table).
inline unsigned require_sector_table(int d, const int32_t *occ, int max_cand, const int32_t *tab) {
  PG_REQUIRE(max_cand >= 1 && max_cand <= SW_MAXC, 1, "sector table: 1 <= max_cand <= 16");
  PG_REQUIRE(d >= 1 && tab, 1, "sector table: d < 1 or a null table");
  const unsigned occ_bits = occ ? hop_occ_bits(d, occ) : 0u;
  const int len = sector_row_len(max_cand);
  for (int a = 0; a < d; ++a)
    for (int b = 0; b < d; ++b) {
      const int32_t *t = tab + (size_t)(a * d + b) * len;
      for (int k = 0; k < 2 * max_cand; ++k) PG_REQUIRE(t[2 + k] >= -1 && t[2 + k] < d, 4, "sector table: state out of range");
      PG_REQUIRE(t[0] >= 1 && t[0] <= max_cand && t[1] >= 0 && t[1] < t[0], 1, "sector table: bad sector size or initial slot");
      for (int k = 0; k < max_cand; ++k) {
        const int pa = t[2 + 2 * k], pb = t[3 + 2 * k];
        PG_REQUIRE(k < t[0] ? (pa >= 0 && pb >= 0) : (pa < 0 && pb < 0), 1, "sector table: a used slot with -1 or an unused slot with a state");
        PG_REQUIRE(k >= t[0] || !occ || ((occ[pa] + occ[pb] + occ[a] + occ[b]) & 1) == 0, 1,
                   "sector table: a candidate changes the fermion parity of the pair");
      }
      PG_REQUIRE(t[2 + 2 * t[1]] == a && t[3 + 2 * t[1]] == b, 1, "sector table: the initial slot is not the pair itself");
    }
  return occ_bits;
}

// Per walker: the physical pair (a, b) of the bond (s1, s2) looked up in the sector table -> max_cand candidate slots cand [w][max_cand][2]
// and meta [w][2] = (m, init).  mode 0: a bosonic table, the slots are the states themselves; mode 1 / 2: a fermionic context in
// row-major / column-major order, the extended states of the two sites by the rule of pair_cand_kernel (the candidates keep the fermion
// parity of the pair, so only these two variants change).  A walker without candidate k keeps its own pair in slot k.
__global__ void sector_cand_kernel(const int *__restrict__ cfg, int sites, int s1, int s2, int d, unsigned occ_bits, int mode,
                                   const int *__restrict__ tab, int max_cand, int *__restrict__ cand, int *__restrict__ meta, int n) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  const int e1 = cfg[(long)w * sites + s1], e2 = cfg[(long)w * sites + s2];
  const int a = e1 % d, b = e2 % d;
  auto occ = [&](int s) { return (int)((occ_bits >> s) & 1u); };
  const int col_major = mode == 2;
  const int before = mode == 0 ? 0 : col_major ? ((e1 / d) & 1) : (((e1 / d) & 1) ^ occ(a));
  const int *t = tab + (long)(a * d + b) * sector_row_len(max_cand);
  const int m = t[0];
  int *c = cand + 2 * (long)w * max_cand;
  for (int k = 0; k < max_cand; ++k) {
    const int pa = t[2 + 2 * k], pb = t[3 + 2 * k];
    int c1 = e1, c2 = e2;
    if (k < m && pa >= 0 && pb >= 0) {
      if (mode == 0) {
        c1 = pa;
        c2 = pb;
      } else {
        const int na = occ(pa), nb = occ(pb);
        c1 = pa + d * (col_major ? 2 + before : before ^ na);
        c2 = pb + d * (col_major ? 2 + (before ^ na) : before ^ na ^ nb);
      }
    }
    c[2 * k] = c1;
    c[2 * k + 1] = c2;
  }
  meta[2 * w] = m;
  meta[2 * w + 1] = t[1];
}

// :127-156 for one bond: the weights |psi_k / psi|^2 of the m states of the sector (the current one keeps its stored amplitude, weight
// 1, as in sweep_suwa_todo_kernel), SuwaTodoStateUpdate with the walker's next two engine words -- taken only when m > 1 (:114-116),
// the cursor is used[w] -- and the move.
template <typename AccT>
__global__ void sector_decide_kernel(int *__restrict__ cfg, int sites, int s1, int s2, const AccT *__restrict__ res,
                                     const double *__restrict__ lsum, AccT *__restrict__ amp, const int *__restrict__ cand,
                                     const int *__restrict__ meta, int max_cand, const unsigned *__restrict__ words, int n_words,
                                     int *__restrict__ used, int *__restrict__ acc, int n) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  const int m = meta[2 * w], init = meta[2 * w + 1];
  if (m <= 1) return;
  const int q = used[w];
  if (q + 2 > n_words) return;                              // (never: the host requires two words per bond of the slice)
  const double sc = exp(lsum[w]);
  const double pa = sw_abs(amp[w]);
  double wt[SW_MAXC];
  for (int k = 0; k < m; ++k) {
    const double r = (k == init) ? 1.0 : sw_abs(sw_scaled(AccT(res[(long)w * max_cand + k]), sc)) / pa;
    wt[k] = r * r;
  }
  const unsigned *wd = words + (long)w * n_words + q;
  const int fin = sw_suwa_todo_decide(wt, m, init, wd[0], wd[1]);
  used[w] = q + 2;
  if (fin != init) {
    const int *c = cand + ((long)w * max_cand + fin) * 2;
    cfg[(long)w * sites + s1] = c[0];
    cfg[(long)w * sites + s2] = c[1];
    amp[w] = sw_scaled(AccT(res[(long)w * max_cand + fin]), sc);
    acc[w] += 1;
  }
}

inline std::atomic<long> &sector_slice_calls() {   // completed sweep_slice_sector calls of the process (pepsgpu_diag_sector_slice_calls)
  static std::atomic<long> n{0};
  return n;
}

// One row / column of MCUpdateSquareNNUpdateBaseOBC::operator() (square_nn_updater.h:41-55 / :62-76) with the sector move: InitBTen +
// GrowFullBTen(.., 2), then per bond the candidates of the sector table, ONE replacement trace over the max_cand slots, the Suwa-Todo
// decision and the move, and the BTen window shift while j + 2 < N -- one read-back at the end.  occ != nullptr: a fermionic context
// (4 d == phys_dim, the extended states derived on the device); occ == nullptr: a bosonic one (d == phys_dim).
template <typename T>
void Engine<T>::sweep_slice_sector(int orient, int slice, int d, const int32_t *occ, int max_cand, const int32_t *sector_table,
                                   int n_words, const uint32_t *words, double *amp_inout, int32_t *consumed_out, int32_t *accepted_out,
                                   int32_t *slice_states_out) {
  require_ready();
  const SliceGeom g(orient, slice, Lx_, Ly_);
  PG_REQUIRE(words && amp_inout && consumed_out && accepted_out && sector_table, 1, "null buffer");
  PG_REQUIRE(n_words >= 2 * (g.N - 1), 1, "sector slice: two engine words per bond of the slice are needed");
  PG_REQUIRE(d >= 1 && (occ ? 4 * d == dp_ : d == dp_), 1,
             "sector slice: the context's physical dimension must be 4 d (fermions: occ given) or d (bosons: occ NULL)");
  const unsigned occ_bits = require_sector_table(d, occ, max_cand, sector_table);
  const bool hor = orient == HORIZONTAL;
  const int sites = Ly_ * Lx_, gb = (nw_ + 255) / 256, N = g.N;
  (void)bmps_at_slice(hor ? UP : LEFT, slice);
  (void)bmps_at_slice(hor ? DOWN : RIGHT, slice);
  // (the candidate kernel reads the walkers' own configuration table)
  PG_REQUIRE(!ovr_on_, 3, "sector slice: a configuration override is active");
  if (occ)
    for (int w = 0; w < nw_; ++w)
      for (int j = 0; j < N; ++j)
        PG_REQUIRE((hcfg_[(size_t)w * sites + g.site(j)] / d >= 2) == !hor, 3,
                   "sector slice: extended states of the other mode order in the slice (rows: variants 0 / 1, columns: 2 / 3)");
  const int mode = !occ ? 0 : hor ? 1 : 2;
  const size_t ntab = (size_t)d * d * sector_row_len(max_cand), nwd = (size_t)nw_ * std::max(n_words, 1);
  ArenaBuf<Acc> damp(arena_, nw_);
  ArenaBuf<unsigned> dwords(arena_, nwd);
  ArenaBuf<int> dcnt(arena_, 2 * (size_t)nw_ + 1);                          // used words [n], accepted moves [n], (overrun: never set)
  ArenaBuf<int> dcand(arena_, (2 * (size_t)max_cand + 2) * (size_t)nw_);    // candidates [n][max_cand][2], meta [n][2]
  int *dmeta = dcand + 2 * (size_t)max_cand * nw_;
  ArenaBuf<int> dtab(arena_, ntab);
  PG_CHECK_HIP(hipMemcpyAsync(damp, amp_inout, sizeof(Acc) * nw_, hipMemcpyHostToDevice, stream_));
  if (n_words > 0) PG_CHECK_HIP(hipMemcpyAsync(dwords, words, sizeof(unsigned) * (size_t)nw_ * n_words, hipMemcpyHostToDevice, stream_));
  PG_CHECK_HIP(hipMemcpyAsync(dtab, sector_table, sizeof(int) * ntab, hipMemcpyHostToDevice, stream_));
  sweep_slice_frame(g, 2, damp, dcnt, amp_inout, consumed_out, accepted_out, slice_states_out, [&] {
    for (int j = 0; j + 1 < N; ++j) {
      const int s1 = g.site(j), s2 = g.site(j + 1);
      hipLaunchKernelGGL(sector_cand_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)cfg_, sites, s1, s2, d, occ_bits, mode,
                         (const int *)dtab, max_cand, dcand, dmeta, nw_);
      PG_CHECK_HIP(hipGetLastError());
      double *lsum = nullptr;
      Acc *res = nn_trace_device(g.row(j), g.col(j), orient, max_cand, dcand, &lsum);
      hipLaunchKernelGGL(sector_decide_kernel<Acc>, dim3(gb), dim3(256), 0, stream_, cfg_, sites, s1, s2, (const Acc *)res,
                         (const double *)lsum, damp, (const int *)dcand, (const int *)dmeta, max_cand, (const unsigned *)dwords, n_words,
                         dcnt, dcnt + nw_, nw_);
      PG_CHECK_HIP(hipGetLastError());
      arena_.free(res);
      arena_.free(lsum);
      erase_envs_after_update(g.row(j), g.col(j));
      erase_envs_after_update(g.row(j + 1), g.col(j + 1));
      if (j + 2 < N) shift_bten_window(g.hi);
    }
  });
  sector_slice_calls() += 1;
}

}  // namespace pepsgpu

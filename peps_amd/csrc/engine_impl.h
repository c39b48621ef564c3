// Row absorption and small helpers of Engine<T> (see engine.h for the algorithm statement).
#pragma once
#include "engine.h"
#include "jacobi_reg.h"

namespace pepsgpu {

__global__ void add_logs_kernel(double *acc, const double *a, const double *b, const double *c, const double *d, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) acc[i] += (a ? a[i] : 0.0) + (b ? b[i] : 0.0) + (c ? c[i] : 0.0) + (d ? d[i] : 0.0);
}

template <typename T>
void Engine<T>::add_logs(double *acc, const double *a, const double *b, const double *c, const double *d) {
  hipLaunchKernelGGL(add_logs_kernel, dim3((nw_ + 255) / 256), dim3(256), 0, stream_, acc, a, b, c, d, nw_);
}
template <typename T>
void Engine<T>::add_log(double *acc, const double *a) {
  add_logs(acc, a, nullptr, nullptr, nullptr);
}

// Jacobi dispatch: LDS-resident generic kernel when the block fits, register-resident kernel for
// the f32 bulk blocks (<= 256 x 256), global-memory generic kernel otherwise (f64 bulk blocks).
// mid_hi > 0: walkers with 32 < rows <= mid_hi are on the preconditioned mid route (absorb_impl) and are skipped here.
template <typename T>
bool Engine<T>::jacobi_small_ok(int len, int m, const int *mdyn) {
  if constexpr (sizeof(T) == 4) return len <= 256 && (mdyn || m <= JR_SMALL_ROWS);
  return false;
}

template <typename T>
bool Engine<T>::launch_jacobi(T *M, long wM, int m, int len, int use_lds, size_t need, const int *mdyn, int mdyn_mul, int mid_hi,
                              const JrSelect *sel, int rows_cap) {
  int small = 0;
  bool sel_used = false;
  if constexpr (sizeof(T) == 4) {
    // walkers whose block has at most 32 existing rows: one wave each; the kernels below return at once for those walkers
    if (jacobi_small_ok(len, m, mdyn)) {
      small = 1;
      // (small batches: giving every walker with <= 32 rows a wave of its own on the sixteen-lanes-per-row tournament -- four pairs
      // per instruction instead of the pairs of a walker one after the other -- was measured as a latency measure: one walker
      // 18.0 -> 19.6 ms per amplitude, 2048 walkers 34.4 -> 40.4 ms: the exchange rounds and the ranking prologue of that kernel
      // cost more than the shorter pair chain saves)
      // walkers with <= 16 rows first (low register count: all of them resident at once)
      if (len <= 64) {          // short rows (shrunk bonds): four walkers per wave, 16 lanes x 4 columns
        hipLaunchKernelGGL((jacobi_rows_tiny4_kernel<4>), dim3((nw_ + 15) / 16), dim3(256), 0, stream_, (float *)M, wM, m, len, len, 40,
                           sweeps_, mdyn, mdyn_mul, nw_, sel ? *sel : JrSelect());
        sel_used = sel != nullptr;
      } else if (len <= 128) {  // ... 16 lanes x 8 columns
        hipLaunchKernelGGL((jacobi_rows_tiny4_kernel<8>), dim3((nw_ + 15) / 16), dim3(256), 0, stream_, (float *)M, wM, m, len, len, 40,
                           sweeps_, mdyn, mdyn_mul, nw_, sel ? *sel : JrSelect());
        sel_used = sel != nullptr;
      } else
        hipLaunchKernelGGL(jacobi_rows_tiny_kernel, dim3((nw_ + 3) / 4), dim3(256), 0, stream_, (float *)M, wM, m, len, len, 40,
                           sweeps_, mdyn, mdyn_mul, nw_);
      PG_CHECK_HIP(hipGetLastError());
      if (m <= JR_BR || (rows_cap > 0 && rows_cap <= JR_BR)) return sel_used;
      // walkers with 17..32 rows: the sixteen-lanes-per-row tournament with one wave per walker (four players of two blocks of
      // four rows, four pairs per wave instruction) or, for short rows, the one-pair-per-instruction kernel; measured, jacobi
      // category per step of 4096 walkers: full-rank state 58.7 -> 54.6 ms, real state 515 -> 500 ms
      if (len > 128)
        launch_jacobi_grp<1, 16>(stream_, nw_, (float *)M, wM, m, len, len, 40, sweeps_, mdyn, mdyn_mul, JR_BR, JR_SMALL_ROWS);
      else if (len > 64)
        launch_jacobi_grp<1, 8>(stream_, nw_, (float *)M, wM, m, len, len, 40, sweeps_, mdyn, mdyn_mul, JR_BR, JR_SMALL_ROWS);
      else
        hipLaunchKernelGGL(jacobi_rows_small_kernel, dim3((nw_ + 3) / 4), dim3(256), 0, stream_, (float *)M, wM, m, len, len, 40,
                           sweeps_, mdyn, mdyn_mul, nw_, 1);
      PG_CHECK_HIP(hipGetLastError());
      if (m <= JR_SMALL_ROWS || (rows_cap > 0 && rows_cap <= JR_SMALL_ROWS)) return sel_used;
    }
    if (mid_hi && m <= mid_hi) return sel_used;        // every remaining walker is on the mid route
    const int skip = mid_hi ? mid_hi : small;          // rows <= max(skip, 32) are taken elsewhere
    if (!use_lds && m <= 256 && len <= 256) {
      hipLaunchKernelGGL(jacobi_rows_reg256_kernel, dim3(nw_), dim3(512), 0, stream_, (float *)M, wM, m, len, len, 40,
                         sweeps_, mdyn, mdyn_mul, skip);
      PG_CHECK_HIP(hipGetLastError());
      return sel_used;
    }
    hipLaunchKernelGGL(jacobi_rows_kernel<T>, dim3(nw_), dim3(1024), use_lds ? need : 0, stream_, M, wM, m, len, len, 40,
                       use_lds, sweeps_, mdyn, mdyn_mul, skip);
    PG_CHECK_HIP(hipGetLastError());
    return sel_used;
  }
  int skip_le = 0;
  if constexpr (std::is_same<T, double>::value) {
    // f64: walkers with at most JR_BR live rows of at most 128 elements in the register kernel (16 or 32 lanes per row)
    if (len <= 128 && (mdyn || m <= JR_BR)) {
      if (len <= 64)
        hipLaunchKernelGGL((jacobi_rows_tiny_f64_kernel<4, 16>), dim3((nw_ + 15) / 16), dim3(256), 0, stream_, (double *)M, wM, m, len, len,
                           40, sweeps_, mdyn, mdyn_mul, nw_);
      else
        hipLaunchKernelGGL((jacobi_rows_tiny_f64_kernel<4, 32>), dim3((nw_ + 7) / 8), dim3(256), 0, stream_, (double *)M, wM, m, len, len,
                           40, sweeps_, mdyn, mdyn_mul, nw_);
      PG_CHECK_HIP(hipGetLastError());
      if (m <= JR_BR) return sel_used;
      skip_le = JR_BR;
    }
  }
  // (float64 tail of the function: a 64 x 256 block of doubles is 131.6 KB, 0.6 KB above JACOBI_LDS_MAX -- the second row of every
  // stack at C4 ran its 18-20 sweeps from global memory; one block per CU with the block in LDS is the better trade up to 136 KB)
  if (!use_lds && need <= 136 * 1024) {
    use_lds = 1;
    allow_dynamic_lds(reinterpret_cast<const void *>(&jacobi_rows_kernel<T>), need);
  }
  // the static block does not fit LDS: 64 KB of dynamic LDS (two blocks per CU as before) for the walkers whose live rows do
  if (!use_lds && mdyn) {
    // (136 KB at one block per CU for blocks like C5's 144 x 145 doubles was measured: C5 f64 2 273 -> 2 109 amp/s -- not adopted)
    constexpr int CAP = 64 * 1024;
    allow_dynamic_lds(reinterpret_cast<const void *>(&jacobi_rows_kernel<T>), (size_t)CAP);
    hipLaunchKernelGGL(jacobi_rows_kernel<T>, dim3(nw_), dim3(1024), CAP, stream_, M, wM, m, len, len, 40, 2, sweeps_, mdyn, mdyn_mul,
                       small, skip_le, CAP);
    PG_CHECK_HIP(hipGetLastError());
    return sel_used;
  }
  hipLaunchKernelGGL(jacobi_rows_kernel<T>, dim3(nw_), dim3(1024), use_lds ? need : 0, stream_, M, wM, m, len, len, 40,
                     use_lds, sweeps_, mdyn, mdyn_mul, small, skip_le);
  PG_CHECK_HIP(hipGetLastError());
  return sel_used;
}

// BMPS::MultiplyMPO with SVD compression (bmps_impl.h:404-437, :756-862, :225-263), Q-less form.
// `num` = index of the absorbed row (UP/DOWN) or column (LEFT/RIGHT); sites are visited in the
// storage order of the BMPS (reversed for UP/RIGHT, bmps_impl.h:694-699).
//
// Rank-adaptive carry: the Cholesky kernel drops the rows of R_{i+1} that are numerically zero
// (below the rounding of the T-typed data) and reports the live count per walker; every launch
// that runs over the carry index m (X = R.A, P = X.W, the Gram's K index, M = R.T, the Jacobi)
// takes that count as a per-walker dynamic extent.  Buffers keep their static (worst case) shape.
// The new bonds get the static size chi unless the absorbed BMPS shows that far fewer states are alive
// (bond b of the new BMPS sits above bond b of the absorbed one and grows by a few states per row): then the
// static size is the previous row's maximum live count plus a margin.  After the absorption one small read-back
// checks that no walker filled a shrunk bond; if one did, the absorption is repeated at full size (rare).
template <typename T>
void Engine<T>::absorb(int pos, int num) {
  if constexpr (kCplx) {
    // complex element type: the plain static-shape form of the same algorithm (engine_cplx.h); variational schemes: engine_var.h
    BMPSDev out = (scheme_ != 0 && mps_len(pos) > 2) ? absorb_variational(pos, num, bmps_[pos].back()) : absorb_simple(pos, num, bmps_[pos].back());
    bmps_[pos].push_back(std::move(out));
  } else {
    if (scheme_ != 0 && mps_len(pos) > 2) {   // bmps_impl.h:419-430: N == 2 always takes the SVD path
      BMPSDev out = absorb_variational(pos, num, bmps_[pos].back());
      bmps_[pos].push_back(std::move(out));
      return;
    }
    BMPSDev out = absorb_svd(pos, num, bmps_[pos].back());
    bmps_[pos].push_back(std::move(out));
  }
}

template <typename T>
typename Engine<T>::BMPSDev Engine<T>::absorb_svd(int pos, int num, const BMPSDev &in) {
  ArenaScope scope(arena_);   // a throw inside returns every temporary and the half-built BMPS to the arena
  BMPSDev out;
  // A row whose hint-sized attempt had to be redone (its bonds grow faster than the margin: the first rows of a dense state)
  // goes straight to the full size the next time the same row is absorbed (the walkers of the next step look like these);
  // forgotten with the state (state_upload).
  char &redo_seen = redo_seen_[pos][num];
  // A hinted attempt that fails leaves walkers half processed (a walker the skipped fallback would have taken carries no live
  // rows, so its Y vanishes and the norm kernels raise its sticky flag): the persistent walker flags are snapshot before such an
  // attempt and put back when it is redone -- only the attempt that produced the result may flag a walker.
  int *flag_keep = nullptr;
  if (!redo_seen) {
    flag_keep = (int *)arena_.alloc(sizeof(int) * (size_t)nw_);
    PG_CHECK_HIP(hipMemcpyAsync(flag_keep, flag_, sizeof(int) * (size_t)nw_, hipMemcpyDeviceToDevice, stream_));
  }
  // (a throw while a kernel of the truncation route runs on the side stream: that kernel still reads and writes buffers the
  // ArenaScope is about to hand back -- wait for it first)
  auto impl = [&](bool full) {
    try { return absorb_impl(pos, num, full, in, out); }
    catch (...) { (void)hipStreamSynchronize(side_stream_); throw; }
  };
  if (redo_seen || !impl(false)) {
    if (!redo_seen) {
      ++n_redo_; free_bmps(out); out = BMPSDev();
      PG_CHECK_HIP(hipMemcpyAsync(flag_, flag_keep, sizeof(int) * (size_t)nw_, hipMemcpyDeviceToDevice, stream_));
    }
    redo_seen = 1;
    PG_REQUIRE(impl(true), 5, "MultiplyMPO: internal error (full-size absorption reported clipping)");
  }
  if (flag_keep) arena_.free(flag_keep);
  return out;
}

// diagnostics: one per-walker device array on the host (forces a sync)
template <typename T>
template <typename U>
std::vector<U> Engine<T>::dbg_read(const U *dev) {
  std::vector<U> h(nw_);
  PG_CHECK_HIP(hipMemcpyAsync(h.data(), dev, nw_ * sizeof(U), hipMemcpyDeviceToHost, stream_));
  PG_CHECK_HIP(hipStreamSynchronize(stream_));
  return h;
}

// Forward loop (R_{i+1} from P_i = R_i (A_i x W_i)), backward loop (truncate right to left), verify.
template <typename T>
bool Engine<T>::absorb_impl(int pos, int num, bool full_bonds, const BMPSDev &in, BMPSDev &out) {
  AbsorbState s;
  absorb_begin(s, pos, num, full_bonds, in, out);
  const int N = s.N;
  for (int i = 0; i + 1 < N; ++i) {
    const SiteDims d = absorb_site(s, i);
    PG_REQUIRE(s.R[i].d[1] == d.l && s.R[i].d[2] == d.a, 3, "MultiplyMPO: bond dimension mismatch");
    forward_factor(s, d, i, forward_pair(s, d, i));
  }
  out.t.resize(N);
  out.logscale = (double *)arena_.alloc(sizeof(double) * nw_);
  PG_CHECK_HIP(hipMemcpyAsync(out.logscale, in.logscale, sizeof(double) * nw_, hipMemcpyDeviceToDevice, stream_));
  s.Y = ones3();
  for (int i = N - 1; i >= 0; --i) {
    const SiteDims d = absorb_site(s, i);
    PG_REQUIRE(s.Y.d[0] == d.l2 && s.Y.d[1] == d.a2, 3, "MultiplyMPO: bond dimension mismatch (backward)");
    const bool precise = precise_site(s, i);
    // Layout of Tt (internal to this site step: written once, read by M = R Tt and by Y = Tt V^T): with the partially live
    // bond k2 innermost the live part of a (l, a) slice is u runs of k2_live floats (40 bytes in 64-byte requests); with the
    // full leg u innermost it is ONE run of k2_live * u floats.  Not at i == 0, where Tt becomes the first tensor (u, k2).
    const bool tsw = i > 0 && sizeof(T) == 4;
    // the backward pair of a precise site runs on the float64-accumulating chained kernel (round 5; f32 in round 4)
    DTen<T> Tt = backward_pair(s, d, i, tsw, sizeof(T) == 4 && precise);
    if (i == 0) {
      PG_REQUIRE(d.l == 1 && d.a == 1, 3, "MultiplyMPO: left boundary bond is not trivial");
      Tt.d[0] = 1; Tt.d[1] = d.u; Tt.d[2] = d.k2; Tt.d[3] = 1;
      prof_begin(PROF_NORM, 0.0, 0.0);
      normalize(Tt.p, Tt.n, Tt.n, nw_, out.logscale);
      prof_end();
      inject(INJ_V, Tt.p, Tt.n);
      out.t[0] = Tt;
      break;
    }
    PG_REQUIRE(s.R[i].d[1] == d.l && s.R[i].d[2] == d.a, 3, "MultiplyMPO: carry dimension mismatch");
    bool dense_site = false;
    DTen<T> M = carry_times_tt(s, d, i, Tt, tsw, dense_site);
    const TruncOut t = truncate_site(s, d, i, M, precise);
    next_y(s, d, i, Tt, t, tsw, dense_site, precise);
  }
  if (s.yscale) arena_.free(s.yscale);
  return absorb_verify(s);
}

// Live bond dimensions of the absorbing BMPS (per walker, device) and of the one being built: every contraction runs over
// the live part of a bond only; persistent tensors stay zero padded.
template <typename T>
void Engine<T>::absorb_begin(AbsorbState &s, int pos, int num, bool full_bonds, const BMPSDev &in, BMPSDev &out) {
  const int N = mps_len(pos);
  PG_REQUIRE((int)in.t.size() == N, 3, "MultiplyMPO: MPS/MPO length mismatch");
  s.pos = pos; s.num = num; s.N = N; s.full_bonds = full_bonds; s.in = &in; s.out = &out;
  s.ll = (pos + 3) % 4; s.lp = pos; s.lr = (pos + 1) % 4; s.lu = (pos + 2) % 4;
  s.clive = in.live;
  s.clive.resize(N + 1, nullptr);
  if (!rank_adapt()) std::fill(s.clive.begin(), s.clive.end(), nullptr);
  s.kn.assign(N + 1, nullptr);
  s.cur_kmax = in.kmax;
  s.cur_kmax.resize(N + 1, -1);
  s.kstat.assign(N + 1, 0); s.kfull.assign(N + 1, 0);
  s.assume_fused.assign(N + 1, 0);
  s.assume_rows.assign(N, 0);
  s.R.assign(N, DTen<T>());
  s.mdyn.assign(N, nullptr);
  s.mmul.assign(N, 1);
  s.R_tri.assign(N, 0);
  s.R[0] = ones3();
}

// Sites are visited in the storage order of the BMPS (reversed for UP / RIGHT, bmps_impl.h:694-699).
template <typename T>
SiteDims Engine<T>::absorb_site(const AbsorbState &s, int i) const {
  SiteDims d;
  switch (s.pos) {
    case DOWN: d.r = s.num; d.c = i; break;
    case UP: d.r = s.num; d.c = s.N - 1 - i; break;
    case LEFT: d.r = i; d.c = s.num; break;
    default: d.r = s.N - 1 - i; d.c = s.num; break;
  }
  site_dims(d.r, d.c, d.dd);
  site_strides(d.r, d.c, d.st);
  d.ll = s.ll; d.lp = s.lp; d.lr = s.lr; d.lu = s.lu;
  const DTen<T> &A = s.in->t[i];
  d.a = A.d[0]; d.p = A.d[1]; d.a2 = A.d[2];
  d.l = d.dd[s.ll]; d.l2 = d.dd[s.lr]; d.u = d.dd[s.lu];
  PG_REQUIRE(d.p == d.dd[s.lp], 3, "MultiplyMPO: bond dimension mismatch");
  d.m = s.R[i].d[0];
  d.k2 = s.Y.d[2];          // (1 during the forward loop, which does not use it)
  d.la = d.l * d.a; d.uk = d.u * d.k2;
  return d;
}

// X = R A and P = X W: chained in one launch where X fits LDS (f32), else two launches.  Returns P [m, u, l2, a2].
template <typename T>
DTen<T> Engine<T>::forward_pair(AbsorbState &s, const SiteDims &d, int i) {
  const DTen<T> &A = s.in->t[i], &Ri = s.R[i];
  const int acc64 = acc64_stages();
  DTen<T> X = alloc_ten(d.m * d.l, d.p, d.a2);
  DTen<T> P = alloc_ten(d.m, d.u, d.l2, d.a2);
  TGemmDesc gx = desc_x(d, Ri.n, A.n, X.n, nw_, s.mdyn[i], s.mmul[i], s.clive[i], s.clive[i + 1]);
  TGemmDesc gp = desc_p(d, X.n, P.n, nw_, s.mdyn[i], s.mmul[i], s.clive[i + 1]);
  const double flx = 2.0 * nw_ * (double)(d.m * d.l) * d.a * (double)(d.p * d.a2);
  const double flp = 2.0 * nw_ * (double)(d.m * d.a2) * (double)(d.l * d.p) * (double)(d.l2 * d.u);
  int *chain_flag = nullptr;
  int chained = 0;
  if constexpr (sizeof(T) == 4) {
    if (!(acc64 & 1)) {
      // both contractions in one launch, X stays in LDS; walkers whose live X does not fit are flagged and take the
      // two separate launches below
      chain_flag = (int *)arena_.alloc(sizeof(int) * nw_);
      TGemmDesc g2 = gp;
      const SiteSel ss = cfg_site(d.r, d.c);
      g2.selA = ss.sel; g2.selA_mul = slot_; g2.selA_inc = ss.inc; g2.seldivA = 1; g2.wA = 0;
      TGemmChainMap mp;
      mp.mapK[1] = 2; mp.mapK[2] = 4;      // K2 = (l, p): l = I1[2], p = J1[1]
      mp.mapJ[1] = 1; mp.mapJ[2] = 5;      // J2 = (m, a2): m = I1[1], a2 = J1[2]
      prof_begin(PROF_CHAIN, flx + flp, flx + flp);
      // 96: the carry of the row absorbed before ran at a hundred or more live rows here (a dense walker batch)
      chained = tgemm_chain_launch(stream_, gx, g2, mp, (const float *)Ri.p, (const float *)A.p, (const float *)sel_base(ss),
                                   (float *)P.p, chain_flag, 1, carry_hint(*s.in, i) > 96, 0, s.R_tri[i] ? 1 : 0);
      prof_end();
      if (!chained) { arena_.free(chain_flag); chain_flag = nullptr; }
    }
  }
  if (chained < 2) {   // the two separate launches: for the entries the chain declined (all of them when it did not run)
    gx.batch_flag = chain_flag; gp.batch_flag = chain_flag;
    prof_begin(PROF_CONTRACT, chain_flag ? 0.0 : flx, chain_flag ? 0.0 : flx);
    if (acc64 & 1) tgemm_launch<T, T, T, Acc>(stream_, gx, Ri.p, A.p, X.p);
    else tgemm_launch<T, T, T, T>(stream_, gx, Ri.p, A.p, X.p);
    prof_end();
    prof_begin(PROF_CONTRACT, chain_flag ? 0.0 : flp, chain_flag ? 0.0 : flp);
    launch_site_gemm_a(gp, cfg_site(d.r, d.c), 1, X.p, P.p, (acc64 & 1) != 0);
    prof_end();
  }
  if (chain_flag) arena_.free(chain_flag);
  free_ten(X);
  inject(INJ_P, P.p, P.n);
  return P;
}

// R_{i+1} with R^T R = P^T P, three cases: compress early with the fused factor; keep the rows of P; Gram + Cholesky with
// the fused / low-rank / blocked cascade.  Consumes P.
//
// Rank-adaptive carry: the Cholesky kernels drop the rows of R_{i+1} that are numerically zero (below the rounding of the
// T-typed data) and report the live count per walker; every launch that runs over the carry index m takes that count as a
// per-walker dynamic extent.  Buffers keep their static (worst case) shape.
template <typename T>
void Engine<T>::forward_factor(AbsorbState &s, const SiteDims &d, int i, DTen<T> P) {
  const bool adaptive = rank_adapt();
  const int rows = d.m * d.u, cols = d.l2 * d.a2;
  const int *mdyn = s.mdyn[i], *live_a2 = s.clive[i + 1];
  const int rmul = s.mmul[i] * d.u;     // live rows of P = live rows of R_i times u (m is P's outer index)
  // 14: the small rank cap of the factor kernels -- the carry of the row absorbed before ran above it at the next site
  const bool hint_dense = carry_hint(*s.in, i + 1) > 14;
  constexpr int FUSED_KCAP = sizeof(T) == 4 ? 96 : 48;   // rows of P a thread of the fused kernel holds in registers
  const double fl_qr = nw_ * 2.0 * (2.0 * cols * (double)rows * rows - 2.0 / 3.0 * (double)rows * rows * rows);
  if (rows < cols && adaptive && cols <= 256 && rows >= 16 && rows <= FUSED_KCAP) {
    // Fewer rows than columns, but already more rows than the usual numerical rank: compress now
    // (gram_chol_lowrank_kernel) instead of letting the carry grow by the factor u per site until it
    // reaches the column count.  Walkers whose rank exceeds the kernel's cap keep their rows of P.
    s.R[i + 1] = alloc_ten(cols, d.l2, d.a2);
    DTen<T> &Rn = s.R[i + 1];
    int *ml = (int *)arena_.alloc(sizeof(int) * nw_);
    prof_begin(PROF_CHOL, fl_qr, 0.0);
    int *flist = (int *)arena_.alloc(sizeof(int) * (nw_ + 1));
    launch_gram_chol_lowrank<T, FUSED_KCAP>(stream_, nw_, (const T *)P.p, P.n, cols, mdyn, rmul, rows, Rn.p, Rn.n, ml, d.a2, live_a2, 1,
                                            hint_dense, flist);
    arena_.free(flist);
    hipLaunchKernelGGL(adopt_rows_flagged_kernel<T>, dim3(nw_), dim3(256), 0, stream_, (const T *)P.p, P.n, cols, mdyn, rmul, rows, Rn.p,
                       Rn.n, ml, d.a2, live_a2);
    PG_CHECK_HIP(hipGetLastError());
    prof_end();
    s.mdyn[i + 1] = ml;
    s.mmul[i + 1] = 1;
    free_ten(P);
  } else if (rows < cols) {
    // economy QR would return R = Q^T P with rows x cols; any R with R^T R = P^T P serves
    // (rows == cols goes through the Cholesky: a triangular carry makes the Jacobi converge 3x faster)
    P.d[0] = rows; P.d[1] = d.l2; P.d[2] = d.a2; P.d[3] = 1;
    // reference op here: QR of the (rows x cols) block, rows < cols (swap R,C)
    prof_begin(PROF_NORM, fl_qr, 0.0);
    if (live_a2) {
      hipLaunchKernelGGL(zero_dead_cols_kernel<T>, dim3(nw_), dim3(256), 0, stream_, P.p, P.n, cols, mdyn, rmul, rows, d.a2, live_a2,
                         (const int *)nullptr);
      PG_CHECK_HIP(hipGetLastError());
    }
    normalize(P.p, P.n, P.n, nw_, nullptr, s.mdyn[i], rmul * cols);
    prof_end();
    s.R[i + 1] = P;
    s.mdyn[i + 1] = s.mdyn[i];
    s.mmul[i + 1] = rmul;
  } else {
    s.R[i + 1] = alloc_ten(cols, d.l2, d.a2);
    DTen<T> &Rn = s.R[i + 1];
    int *ml = adaptive ? (int *)arena_.alloc(sizeof(int) * nw_) : nullptr;
    // Low-rank walkers: the factor straight from the live rows of P, no Gram matrix in memory
    // (gram_chol_lowrank_kernel); it flags the walkers it cannot take (ml = -1) and the Gram GEMM
    // and the Cholesky kernels of forward_gram_chol then run for those only.
    const bool fused = ml && cols <= 256 && (mdyn || rows <= FUSED_KCAP);
    // Hint of the row absorbed before: its carry stayed at <= 24 rows on both sides of this site, well inside what the fused
    // factor covers (rank 32, 288 rows) -- the launches for the walkers it would flag (Gram, low-rank and blocked Cholesky:
    // ~66 us per site on an empty list) are not issued.  Verified after the absorption: a walker left flagged (ml < 0) fails
    // the attempt and the absorption is redone with every launch (absorb_svd), as for the other hints.
    static const bool force_skip_fb = getenv("PEPSGPU_FORCE_SKIP_FALLBACK") != nullptr;     // tests: a wrong hint
    const int h0 = carry_hint(*s.in, i), h1 = carry_hint(*s.in, i + 1);
    const bool skip_fb = fused && !s.full_bonds && sizeof(T) == 4 && (force_skip_fb || (h0 >= 0 && h0 <= 24 && h1 >= 0 && h1 <= 24));
    if (fused) {
      // more live rows than one pass holds (moderate rank): fold the rows of P in over up to four passes
      // (covers K <= KCAP + 3 (KCAP - 32) rows); walkers beyond that, or of rank > 32, are flagged
      const int npass = (mdyn && rows > FUSED_KCAP) ? 4 : 1;
      prof_begin(PROF_CHOL, 0.0, 0.0);
      int *flist = (int *)arena_.alloc(sizeof(int) * (nw_ + 1));
      launch_gram_chol_lowrank<T, FUSED_KCAP>(stream_, nw_, (const T *)P.p, P.n, cols, mdyn, rmul, rows, Rn.p, Rn.n, ml, d.a2, live_a2, npass,
                                              hint_dense, flist);
      arena_.free(flist);
      prof_end();
    }
    if (skip_fb) s.assume_fused[i + 1] = 1;
    else forward_gram_chol(s, d, i, P, ml, fused);
    if (dbg_sweeps_ && ml) {   // diagnostics: numerical rank of the carry (forces a sync)
      for (int v : dbg_read(ml)) { live_sum_ += v; live_full_ += cols; live_max_ = std::max<long>(live_max_, v); }
    }
    s.mdyn[i + 1] = ml;
    s.mmul[i + 1] = 1;
    // R[i + 1] is a Cholesky factor with compacted rows (row j zero before column j): the contractions that read it skip its zero
    // blocks (round 6; PEPSGPU_TRI=0: off).  Set here, where every kernel keeps the column order, not where a walker may keep its
    // rows of P.
    static const bool use_tri = getenv("PEPSGPU_TRI") == nullptr || atoi(getenv("PEPSGPU_TRI")) != 0;
    s.R_tri[i + 1] = use_tri && ml != nullptr;
    free_ten(P);
  }
  inject(INJ_R, s.R[i + 1].p, s.R[i + 1].n);
}

// G = P^T P in float64 and its Cholesky factor, for every walker or (fused) for the walkers the fused factor flagged:
// low-rank kernel first, the blocked kernel for what it hands on.
template <typename T>
void Engine<T>::forward_gram_chol(AbsorbState &s, const SiteDims &d, int i, DTen<T> &P, int *ml, bool fused) {
  const int rows = d.m * d.u, cols = d.l2 * d.a2;
  const int *mdyn = s.mdyn[i], *live_a2 = s.clive[i + 1];
  const int rmul = s.mmul[i] * d.u;
  const int *flagged = fused ? ml : nullptr;
  DTen<T> &Rn = s.R[i + 1];
  double *G = (double *)arena_.alloc(sizeof(double) * (size_t)cols * cols * nw_);
  const bool gram_direct = cols >= 32 && cols <= 256;
  if (live_a2 && !gram_direct) {   // the Gram GEMM reads whole rows: define the never-written columns (flagged walkers only)
    hipLaunchKernelGGL(zero_dead_cols_kernel<T>, dim3(nw_), dim3(256), 0, stream_, P.p, P.n, cols, mdyn, rmul, rows, d.a2, live_a2, flagged);
    PG_CHECK_HIP(hipGetLastError());
  }
  // algorithmic flops of the op this replaces: geqrf + orgqr of (rows x cols)
  // (executed flops of this category are counted on the device only: the launch runs for the flagged walkers)
  prof_begin(PROF_GRAM, nw_ * 2.0 * (2.0 * rows * (double)cols * cols - 2.0 / 3.0 * (double)cols * cols * cols), 0.0);
  if (gram_direct)   // wave-per-block streaming kernel (gram.h): no LDS, no barrier; dead columns masked at the load
    launch_gram_cols_f64<T>(stream_, nw_, (const T *)P.p, P.n, cols, cols, mdyn, rmul, rows, G, flagged, d.a2, live_a2, tg_flop_counter,
                            tg_byte_counter);
  else
    tgemm_launch<T, T, double, double>(stream_, desc_cols_gram(rows, cols, P.n, nw_, mdyn, rmul, false, flagged, false), P.p, P.p, G);
  prof_end();
  const size_t smem = chol_smem_bytes(cols);
  PG_REQUIRE(smem <= 150 * 1024 && cols < 32768, 1, "Cholesky panel does not fit LDS (D*chi too large)");
  allow_dynamic_lds(reinterpret_cast<const void *>(&chol_upper_kernel<T>), smem);
  prof_begin(PROF_CHOL, 0.0, 0.0);   // (executed flops of this category: the MFMA flops of the fused Gram kernels, counted on the device)
  // CH_LR_CAP + 8: the carry of the row absorbed before ran well above the cap of the low-rank kernel at the next site -- every
  // walker would spend 32 steps there only to be handed on; the blocked kernel takes any rank
  const bool above_cap = carry_hint(*s.in, i + 1) > CH_LR_CAP + 8;
  const bool lowrank = ml && cols <= 256 * CH_LR_Q && !above_cap;
  if (lowrank) {   // walkers of rank <= CH_LR_CAP finish here; the others are flagged for the blocked kernel
    const size_t lsm = chol_lowrank_smem_bytes(cols);
    allow_dynamic_lds(reinterpret_cast<const void *>(&chol_lowrank_kernel<T>), lsm);
    hipLaunchKernelGGL(chol_lowrank_kernel<T>, dim3(nw_), dim3(256), lsm, stream_, (const double *)G, (long)cols * cols, cols, Rn.p, Rn.n, ml,
                       fused ? 1 : 0);
    PG_CHECK_HIP(hipGetLastError());
  }
  launch_chol_upper<T>(stream_, nw_, G, (long)cols * cols, cols, Rn.p, Rn.n, ml, (lowrank || fused) ? 1 : 0);
  prof_end();
  arena_.free(G);
}

// "Precise" sites (f32 engine): where the carry is not of low rank -- the row absorbed before ran more than 24 live
// carry rows at this site, or gives no hint yet (the first three rows of a stack) -- the places where f32 rounding showed in the
// amplitude get float64-grade arithmetic: the backward pair Z1 = A Y, Tt = W Z1 (round 5) and Y = Tt V^T accumulate in float64 on
// the f64 matrix cores (columns of small sigma are differences of O(sigma_1) terms), and the rows of Vt are made orthonormal by a
// Newton-Schulz step in float64 (ortho_rows_kernel).  The low-rank headline state keeps the f32 forms.
template <typename T>
bool Engine<T>::precise_site(const AbsorbState &s, int i) const {
  if constexpr (sizeof(T) == 4) {
    static const int precise = getenv("PEPSGPU_PRECISE") ? atoi(getenv("PEPSGPU_PRECISE")) : 1;    // 0 never, 1 auto, 2 always
    // (rows whose predecessor gives no hint yet -- the first three of a stack -- go by what the SAME row of the SAME stack showed
    // the last time it was absorbed, carry_seen_: unknown on a fresh state -> precise)
    const int seen = carry_seen_[s.pos][s.num];
    const int h = carry_hint(*s.in, i);
    // 24: above it the carry is no longer "low rank" (the fused factor's comfortable range, see forward_factor)
    return precise == 2 || (precise == 1 && (h >= 0 ? h > 24 : (seen < 0 || seen > 24)));
  }
  return false;
}

// Z1 = A Y and Tt = W Z1: chained in one launch where Z1 fits LDS (f32), else two launches.  Consumes Y; returns Tt
// [l, a, u, k2] ([l, a, k2, u] when tsw).
template <typename T>
DTen<T> Engine<T>::backward_pair(AbsorbState &s, const SiteDims &d, int i, bool tsw, bool tt_f64) {
  const DTen<T> &A = s.in->t[i];
  const int acc64 = acc64_stages();
  DTen<T> Z1 = alloc_ten(d.a, d.p, d.l2, d.k2);
  DTen<T> Tt = alloc_ten(d.l, d.a, d.u, d.k2);
  TGemmDesc gz = desc_z1(d, A.n, s.Y.n, Z1.n, nw_, s.clive[i], s.clive[i + 1], s.kn[i + 1]);
  if constexpr (sizeof(T) == 4) { if (s.y_scaled) gz.scale_in = s.yscale; }
  // i == 0: Tt becomes the (persistent, zero padded) first tensor
  TGemmDesc gt = desc_tt(d, tsw, Z1.n, Tt.n, nw_, s.clive[i], s.kn[i + 1], i == 0);
  const double flz = 2.0 * nw_ * (double)(d.a * d.p) * d.a2 * (double)(d.l2 * d.k2);
  const double flt = 2.0 * nw_ * (double)(d.a * d.k2) * (double)(d.p * d.l2) * (double)(d.l * d.u);
  int *chain_flag = nullptr;
  int chained = 0;
  if constexpr (sizeof(T) == 4) {
    if (!(acc64 & 2)) {   // Z1 stays in LDS (see the forward pair)
      chain_flag = (int *)arena_.alloc(sizeof(int) * nw_);
      TGemmDesc g2 = gt;
      const SiteSel ss = cfg_site(d.r, d.c);
      g2.selA = ss.sel; g2.selA_mul = slot_; g2.selA_inc = ss.inc; g2.seldivA = 1; g2.wA = 0;
      TGemmChainMap mp;
      mp.mapK[1] = 2; mp.mapK[2] = 4;      // K2 = (p, l2): p = I1[2], l2 = J1[1]
      mp.mapJ[1] = 1; mp.mapJ[2] = 5;      // J2 = (a, k2): a = I1[1], k2 = J1[2]
      prof_begin(PROF_CHAIN, 0.0, flz + flt);
      // 96: dense carry at this site (see forward_pair)
      chained = tgemm_chain_launch(stream_, gz, g2, mp, (const float *)A.p, (const float *)s.Y.p, (const float *)sel_base(ss),
                                   (float *)Tt.p, chain_flag, 1, carry_hint(*s.in, i) > 96, tt_f64 ? 1 : 0);
      prof_end();
      if (!chained) { arena_.free(chain_flag); chain_flag = nullptr; }
    }
  }
  if (chained < 2) {
    gz.batch_flag = chain_flag; gt.batch_flag = chain_flag;
    prof_begin(PROF_CONTRACT, 0.0, chain_flag ? 0.0 : flz);
    gz.acc64 = tt_f64; gt.acc64 = tt_f64;     // (entries the chain declined: the wave-per-tile kernel honours it)
    if (acc64 & 2) tgemm_launch<T, T, T, Acc>(stream_, gz, A.p, s.Y.p, Z1.p);
    else tgemm_launch<T, T, T, T>(stream_, gz, A.p, s.Y.p, Z1.p);
    prof_end();
    prof_begin(PROF_CONTRACT, 0.0, chain_flag ? 0.0 : flt);
    launch_site_gemm_a(gt, cfg_site(d.r, d.c), 1, Z1.p, Tt.p, (acc64 & 2) != 0);
    prof_end();
  }
  if (chain_flag) arena_.free(chain_flag);
  free_ten(Z1);
  free_ten(s.Y);
  inject(INJ_T, Tt.p, Tt.n);
  return Tt;
}

// M[m,(u,k2)] = R_i Tt.  dense_site (hint of the row absorbed before): the carry ran above 96 live rows at this site, the
// class of the LDS-tiled / workgroup-per-walker kernels; next_y routes by it too.
template <typename T>
DTen<T> Engine<T>::carry_times_tt(AbsorbState &s, const SiteDims &d, int i, const DTen<T> &Tt, bool tsw, bool &dense_site) {
  const DTen<T> &Ri = s.R[i];
  const int acc64 = acc64_stages();
  DTen<T> M = alloc_ten(d.m, d.uk, 1);
  dense_site = carry_hint(*s.in, i) > 96 && d.la >= 128 && d.uk >= 128;
  // (the LDS-tiled and workgroup-per-walker kernels of a dense site keep the (u, k2) enumeration of the columns)
  const bool k2_outer = sizeof(T) == 4 && !dense_site && !(acc64 & 4) && (tgemm_thin() & TG_THIN_LANES);
  TGemmDesc g = desc_m(d, tsw, Ri.n, Tt.n, M.n, nw_, s.mdyn[i], s.mmul[i], s.clive[i], s.kn[i + 1], true, k2_outer);
  g.prefer_tiled = dense_site;
  prof_begin(PROF_CONTRACT, 0.0, 2.0 * nw_ * (double)d.m * d.la * (double)d.uk);
  bool mg_done = false;
  if constexpr (sizeof(T) == 4) {
    // dense carry: the workgroup-per-walker kernel (mgemm_dense.h): R and Tt through LDS once, eight waves x 32 columns
    if (dense_site && !(acc64 & 4) && d.m > 128 && mgemm_dense_ok(d.m, d.la, d.a, d.u, d.k2, Ri.n, Tt.n, Ri.p, Tt.p)) {
      launch_mgemm_dense(stream_, nw_, (const float *)Ri.p, Ri.n, (const float *)Tt.p, Tt.n, (float *)M.p, M.n, d.m, d.la, d.a, d.u, d.k2,
                         tsw ? 1 : 0, (const int *)s.mdyn[i], s.mmul[i], (const int *)s.clive[i], (const int *)s.kn[i + 1], tg_flop_counter,
                         tg_byte_counter, s.R_tri[i] ? 1 : 0);
      mg_done = true;
    }
  }
  if (!mg_done) {
    if (acc64 & 4) tgemm_launch<T, T, T, Acc>(stream_, g, Ri.p, Tt.p, M.p);
    else tgemm_launch<T, T, T, T>(stream_, g, Ri.p, Tt.p, M.p);
  }
  prof_end();
  inject(INJ_M, M.p, M.n);
  return M;
}

// Rows of M -> mutually orthogonal (sigma_k v_k^T), the chi largest normalised into V.  Every walker is taken by exactly one
// of: the f32 mid route (trunc_mid_*), a float64 dense route (trunc_f64_*), the general Jacobi + select.  Consumes M.
template <typename T>
typename Engine<T>::TruncOut Engine<T>::truncate_site(AbsorbState &s, const SiteDims &d, int i, DTen<T> &M, bool precise) {
  const int m = d.m, uk = d.uk;
  MidRoute mr = trunc_mid_prepare(s, d, i, M);
  // static size of the new bond and the tensor it leads to (before the Jacobi: the kernel of the walkers with few live rows
  // selects and normalises their rows into V itself).  The new bonds get the static size chi unless the absorbed BMPS shows that
  // far fewer states are alive (bond b of the new BMPS sits above bond b of the absorbed one and grows by a few states per row):
  // then the static size is the previous row's maximum live count plus a margin, verified by absorb_verify.
  TruncOut t;
  t.k_full = std::min(chi_, std::min(m, uk));
  t.k = t.k_full;
  if (!s.full_bonds && rank_adapt() && s.cur_kmax[i] >= 0) {
    const int want = s.cur_kmax[i] + std::max(2, s.cur_kmax[i] / 4);
    t.k = std::min(t.k_full, (want + 3) & ~3);
  }
  s.kstat[i] = t.k; s.kfull[i] = t.k_full;
  PG_REQUIRE(m <= 1024, 1, "bond dimension too large for select_rows_kernel");
  t.V = alloc_ten(t.k, d.u, d.k2);
  if (rank_adapt()) s.kn[i] = (int *)arena_.alloc(sizeof(int) * nw_);
  t.kn_i = s.kn[i];
  if constexpr (std::is_same<T, double>::value) {
    static const bool no_route_env = getenv("PEPSGPU_NO_F64_DENSE_ROUTE") != nullptr;
    static const int f64_pivot_env = getenv("PEPSGPU_F64_PIVOT") ? atoi(getenv("PEPSGPU_F64_PIVOT")) : 1;   // 0: the two-Cholesky route of round 5
    const DenseRouteChoice rc = dense_route_choice(no_route_env, f64_pivot_env);
    const bool no_route = rc.off;
    const int f64_pivot = rc.pivot;
    // oversampled subspace: 2 chi directions, at most three quarters of the rank M can have (the right-edge sites are 256 x 64);
    // trunc_err > 0 keeps the general path (the truncation rule wants every singular value)
    const int kq = std::min(2 * t.k_full, (3 * std::min(m, uk)) / 4);
    const bool route_ok = !no_route && rank_adapt() && trunc_err_ == 0.0 && m <= 256 && uk <= 256 && kq <= 64 && kq >= t.k_full + 8 && i > 0;
    // pivoted route: blocks of 64 .. 256 rows (measured, real state at 2 048 walkers: 443 amp/s with the route above 128 rows only, 490 from 64)
    if (f64_pivot && route_ok && m > 63 && uk % 4 == 0) trunc_f64_pivot(s, d, i, M, kq, t);
    // (round-5 form: not on blocks with more rows than columns.  Their rank ends at uk by shape, so the unpivoted factor of M M^T
    // meets dependent rows while directions of weight are still open and decides at the rounding level which rows it keeps; on a
    // 200 x 128 block with a flat tail of 6e-5 sigma_1 one walker in four lost 6e-8 of sigma_1, and no guard of the route prices it)
    else if (route_ok && m > 128 && m <= uk) trunc_f64_two_chol(s, d, i, M, kq, t);
  }
  trunc_jacobi(s, d, i, M, mr, t);
  prof_begin(PROF_SELECT, 0.0, 0.0);
  // (behind the rank hint "no walker above 16 rows" the short-row Jacobi has selected every walker itself: the launch would
  // return at once for all of them -- 15 us x 160 sites per step of 49 152 walkers; a miss is caught by the same read-back)
  const bool skip_select = t.sel_done && !mr.on && s.assume_rows[i] > 0 && s.assume_rows[i] <= JR_BR;
  if (!skip_select)
    hipLaunchKernelGGL(select_rows_kernel<T>, dim3(nw_), dim3(256), 0, stream_, (const T *)M.p, M.n, m, uk, uk, t.k, t.V.p, t.V.n,
                       (T *)nullptr, 0L, (const int *)s.mdyn[i], s.mmul[i], t.kn_i, trunc_err_, chi_min_, (double *)nullptr,
                       (const int *)(t.route_flag ? t.select_skip : mr.midflag), 0, t.sel_done ? JR_BR : 0);
  PG_CHECK_HIP(hipGetLastError());
  if (t.route_flag) {
    diag_keep_route_flag(t.route_flag);
    if (t.early) {      // the side stream's walkers: joined before anything reads V / kn of this site
      PG_CHECK_HIP(hipStreamWaitEvent(stream_, ev_join_, 0));
      // (their buffers go back to the arena: it hands them out to launches on stream_ only, which are ordered behind the join)
      arena_.free(t.early); arena_.free(t.fb_early);
      t.early = nullptr; t.fb_early = nullptr;
    }
    arena_.free(t.route_flag); arena_.free(t.gen_rows); arena_.free(t.select_skip);
    t.route_flag = nullptr; t.gen_rows = nullptr; t.select_skip = nullptr;
  }
  if (mr.on) trunc_mid_finish(s, d, i, M, mr, t);    // (closes the PROF_SELECT bracket behind its first select)
  else prof_end();
  free_ten(M);
  if constexpr (sizeof(T) == 4) {
    const size_t osm = ortho_rows_smem(t.k, uk);
    if (precise && t.k >= 2 && t.k <= 64 && osm <= 96 * 1024) {
      allow_dynamic_lds(reinterpret_cast<const void *>(&ortho_rows_kernel), osm);
      prof_begin(PROF_SELECT, 0.0, 0.0);
      hipLaunchKernelGGL(ortho_rows_kernel, dim3(nw_), dim3(256), osm, stream_, (float *)t.V.p, t.V.n, t.k, uk, (const int *)t.kn_i, uk + 1,
                         (const int *)t.ortho_skip);
      PG_CHECK_HIP(hipGetLastError());
      prof_end();
    }
  }
  if (t.ortho_skip) { arena_.free(t.ortho_skip); t.ortho_skip = nullptr; }
  inject(INJ_V, t.V.p, t.V.n);
  s.out->t[i] = t.V;
  return t;
}

// The general one-sided Jacobi on M for the walkers no route took, and -- in the same profile bracket -- the Jacobi of the mid
// route on its small factors.
template <typename T>
void Engine<T>::trunc_jacobi(AbsorbState &s, const SiteDims &d, int i, DTen<T> &M, MidRoute &mr, TruncOut &t) {
  const int m = d.m, uk = d.uk;
  const size_t need = sizeof(T) * (size_t)m * (uk | 1);
  const int use_lds = need <= JACOBI_LDS_MAX;
  if (use_lds) allow_dynamic_lds(reinterpret_cast<const void *>(&jacobi_rows_kernel<T>), need);
  {   // reference op: gesdd of the (m x uk) block: 4 r c^2 + 22 c^3, r >= c
    const double rr = std::max(m, uk), cc = std::min(m, uk);
    // category 3 = register kernel (bulk blocks), 7 = generic LDS/global kernel (edge blocks)
    const bool bulk = sizeof(T) == 4 && ((!use_lds && m <= 256 && uk <= 256) || mr.on);
    prof_begin(bulk ? PROF_JACOBI : PROF_JACOBI_EDGE, nw_ * (4.0 * rr * cc * cc + 22.0 * cc * cc * cc), 0.0);
  }
  JrSelect jsel;
  if constexpr (sizeof(T) == 4) {
    if (t.kn_i) { jsel.V = (float *)t.V.p; jsel.wV = t.V.n; jsel.k = t.k; jsel.klive_out = t.kn_i; jsel.trunc_err = trunc_err_; jsel.dmin = chi_min_; }
    // span-only truncation (PEPSGPU_TRUNC_SPAN=0: the sweeps for every walker); a truncation-error rule needs the singular values
    jsel.span = trunc_err_ == 0.0 && trunc_span();
  }
  // Size classes of the Jacobi kernels above the carry rank of the row absorbed before (+ margin) are not launched (each
  // is a launch of nw blocks that return at once); the live counts read back at the end of this absorption verify it,
  // a miss redoes the absorption without hints (absorb_svd).
  int rows_cap = 0;
  if constexpr (sizeof(T) == 4) {
    static const int force_cap = getenv("PEPSGPU_FORCE_ROWS_CAP") ? atoi(getenv("PEPSGPU_FORCE_ROWS_CAP")) : 0;   // tests: a wrong hint
    const int h = carry_hint(*s.in, i);
    if (!s.full_bonds && rank_adapt() && s.mdyn[i] && !mr.on) {
      if (force_cap) rows_cap = force_cap;
      // margins 3 / 6: the carry rank grows by a few states per row; JR_BR / JR_SMALL_ROWS: the two small size classes
      else if (h >= 0) rows_cap = h + 3 <= JR_BR ? JR_BR : (h + 6 <= JR_SMALL_ROWS ? JR_SMALL_ROWS : 0);
    }
  }
  s.assume_rows[i] = rows_cap;
  t.sel_done = launch_jacobi(M.p, M.n, m, uk, use_lds, need, t.route_flag ? t.gen_rows : s.mdyn[i], t.route_flag ? 1 : s.mmul[i],
                             mr.on ? mr.MID_HI : 0, jsel.V ? &jsel : nullptr, rows_cap);
  if constexpr (sizeof(T) == 4) {
    if (mr.on) trunc_mid_jacobi(mr);
  }
  prof_end();
  ++n_jacobi_;
  if (dbg_sweeps_) {   // diagnostics only: per-launch sweep counts (forces a sync)
    long mx = 0, live = 0, sw_sum = 0, live_mx = 0, span = 0, span_back = 0;
    const bool span_asked = t.sel_done && jsel.span;
    for (int v : dbg_read(sweeps_)) {
      mx = std::max<long>(mx, v & 0xFF); sw_sum += v & 0xFF; live += v >> 8; live_mx = std::max<long>(live_mx, v >> 8);
      // span walkers: zero sweeps and live rows; with the path asked for, a short-row walker that swept kept more than k directions
      if (span_asked && (v >> 8) > 0 && (v >> 8) <= JR_BR) { if ((v & 0xFF) == 0) ++span; else ++span_back; }
    }
    jacobi_sweeps_sum_ += mx;
    jacobi_sweeps_max_ = std::max(jacobi_sweeps_max_, mx);
    if (getenv("PEPSGPU_DEBUG_VERBOSE"))
      fprintf(stderr, "[pepsgpu] jacobi m=%d len=%d sweeps max=%ld mean=%.2f live_rows_mean=%.1f live_rows_max=%ld span=%ld span_fell_back=%ld\n",
              m, uk, mx, (double)sw_sum / nw_, (double)live / nw_, live_mx, span, span_back);
  }
}

// Ynew[(l,a),q] = Tt V^T, normalised (fused into the launch where it can be).  Consumes Tt.
template <typename T>
void Engine<T>::next_y(AbsorbState &s, const SiteDims &d, int i, const DTen<T> &Tt, const TruncOut &t, bool tsw, bool dense_site, bool precise) {
  const int acc64 = acc64_stages();
  const int k = t.k;
  DTen<T> Yn = alloc_ten(d.l, d.a, k);
  TGemmDesc g = desc_y(d, k, tsw, Tt.n, t.V.n, Yn.n, nw_, s.clive[i], s.kn[i + 1], s.kn[i], true, false);
  g.prefer_tiled = dense_site;
  // Y on precise sites: the wave-per-tile kernel with float64 accumulation (tg_direct_body_f64, round 5; the norm stays fused into
  // the launch).  (measured, round 5, real state at C4, n = 256 vs the f64 mode: max 6.8e-6 / median 1.67e-6 at 2 235 amp/s (4 096
  // walkers); float64 accumulation on the LDS-tiled kernel + separate normalisation (round 4) 8.0e-6 / 1.81e-6 at 2 200)
  if constexpr (sizeof(T) == 4) {
    g.acc64 = precise ? 1 : 0;
    // (the wave-per-tile kernel is the one that honours acc64: round 4 left prefer_tiled set on dense sites, so its "mode 1"
    // measurement ran the LDS-tiled f32 kernel there -- the "drain removes a third only" of HISTORY 3e was that, not the drain)
    if (g.acc64) g.prefer_tiled = false;
  }
  // The norm of Yn comes out of the launch that writes it (squares of the stored values, summed in registers) as a
  // per-walker scale that the contraction reading Yn at the next site applies to its own result: no pass over Yn.
  bool fused_norm = false;
  if constexpr (sizeof(T) == 4) {
    if (!acc64 && rank_adapt() && s.kn[i] && tgemm_one_block_direct(g)) {
      if (!s.yscale) s.yscale = (float *)arena_.alloc(sizeof(float) * nw_);
      g.scale_out = s.yscale; g.norm_log = s.out->logscale; g.norm_flag = flag_;
      fused_norm = true;
    }
  }
  // reference op: res[i-1] . (u s)  (bmps_impl.h:254): 2 (m_{i-1} D_u) m_i k_i
  const int u_prev = absorb_site(s, i - 1).u;
  prof_begin(PROF_CONTRACT, 2.0 * nw_ * (double)s.R[i - 1].d[0] * u_prev * (double)d.m * k, 2.0 * nw_ * (double)d.la * d.uk * (double)k);
  if (acc64 & 8) tgemm_launch<T, T, T, Acc>(stream_, g, Tt.p, t.V.p, Yn.p);
  else tgemm_launch<T, T, T, T>(stream_, g, Tt.p, t.V.p, Yn.p);
  prof_end();
  s.y_scaled = fused_norm;
  if (!s.y_scaled) {
    prof_begin(PROF_NORM, 0.0, 0.0);
    normalize(Yn.p, Yn.n, Yn.n, nw_, s.out->logscale);
    prof_end();
  }
  inject(INJ_Y, Yn.p, Yn.n);
  arena_.free(Tt.p);
  s.Y = Yn;
}

// One small read-back per absorption: the maximum live count of every new bond and of every carry; the three rules that
// fail a hinted attempt (absorb_svd then redoes it at full size).  Frees the carries.
template <typename T>
bool Engine<T>::absorb_verify(AbsorbState &s) {
  const int N = s.N;
  BMPSDev &out = *s.out;
  out.live = s.kn;
  out.kmax.assign(N + 1, -1);
  out.mlmax.assign(N, -1);
  out.depth = s.in->depth + 1;
  bool ok = true;
  if (rank_adapt()) {
    const int ntab = 3 * N + 1;
    std::vector<const int *> htab(ntab, nullptr);
    for (int b = 0; b <= N; ++b) htab[b] = s.kn[b];
    for (int i = 0; i < N; ++i) htab[N + 1 + i] = s.mdyn[i];
    for (int i = 0; i < N; ++i) htab[2 * N + 1 + i] = s.assume_fused[i] ? s.mdyn[i] : nullptr;   // (read as "any entry negative")
    std::vector<int> hmax(ntab, -1);
    const int **dtab = (const int **)arena_.alloc(sizeof(int *) * ntab);
    int *dmax = (int *)arena_.alloc(sizeof(int) * ntab);
    PG_CHECK_HIP(hipMemcpyAsync(dtab, htab.data(), sizeof(int *) * ntab, hipMemcpyHostToDevice, stream_));
    hipLaunchKernelGGL(max_over_walkers_kernel, dim3(ntab), dim3(256), 0, stream_, (const int *const *)dtab, nw_, dmax, 2 * N + 1);
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipMemcpyAsync(hmax.data(), dmax, sizeof(int) * ntab, hipMemcpyDeviceToHost, stream_));
    PG_CHECK_HIP(hipStreamSynchronize(stream_));
    arena_.free(dtab); arena_.free(dmax);
    for (int b = 0; b <= N; ++b) out.kmax[b] = hmax[b];
    for (int i = 0; i < N; ++i) out.mlmax[i] = s.mdyn[i] ? std::min(s.R[i].d[0], hmax[N + 1 + i] * s.mmul[i]) : s.R[i].d[0];
    if (!ovr_on_) {      // (a BMPSWalker's foreign MPO says nothing about the network's own row)
      int mx = 0;
      for (int i = 0; i < N; ++i) mx = std::max(mx, out.mlmax[i]);
      carry_seen_[s.pos][s.num] = mx;
    }
    for (int i = 1; i < N; ++i)
      if (s.kstat[i] < s.kfull[i] && out.kmax[i] >= s.kstat[i]) ok = false;   // a walker filled a shrunk bond: maybe clipped
    for (int i = 0; i < N; ++i)
      if (s.assume_rows[i] > 0 && out.mlmax[i] > s.assume_rows[i]) ok = false;   // a rank hint was missed: rows left unrotated
    for (int i = 0; i < N; ++i)
      if (s.assume_fused[i] && hmax[2 * N + 1 + i] > 0) ok = false;            // a walker the fused factor flagged had no fallback
  }
  for (auto &t : s.R) arena_.free(t.p);
  {   // the dynamic-extent arrays (several R_i may share one)
    int *last = nullptr;
    for (int *p : s.mdyn)
      if (p && p != last) { arena_.free(p); last = p; }
  }
  if (ok) ++n_absorb_;
  return ok;
}

// Mid route (f32, 32 < live rows <= 128: the usual size of the carry on states of higher rank): the Jacobi runs on
// the triangular factor B of the small Gram matrix instead of on M itself,
//     G = M M^T (f64 MFMA, ml x ml),  B^T B = G (Cholesky),  rows of B --Jacobi--> sigma_k u_k^T,
//     Vt = rows of (U^T M) normalised,
// the preconditioned one-sided Jacobi SVD (Drmac / Veselic): rows are ml <= 128 long instead of u * k2, the
// triangular factor converges in about half the sweeps, and four walkers share a CU.  sigma and Vt are those of M:
// select_rows_kernel sees the same singular values, the truncation rule is unchanged.
// Round 3: the route reaches 256 live rows.  A state of the rank of a real PEPS carries ~190-240 live rows, but M = R Tt is
// numerically of rank ~60-100 at the f32 floor (the singular values of the truncation input fall by five orders of magnitude
// over the first 32): the Cholesky of M M^T drops the dependent rows, the Jacobi runs on the <= 128 live rows of B (256 long)
// instead of on the 240 rows of M (19 sweeps of the 256 x 256 register kernel: 80 % of the step before).
//
// This half decides whether the site takes the route and leaves the factor Bt (two-level form: and B2) with its row counts.
template <typename T>
typename Engine<T>::MidRoute Engine<T>::trunc_mid_prepare(AbsorbState &s, const SiteDims &d, int i, const DTen<T> &M) {
  MidRoute mr;
  const int m = d.m, uk = d.uk;
  const int h = carry_hint(*s.in, i);
  // h + 12 <= 128: no walker came near 128 live rows at this site -> the route keeps its <= 128-row form
  // (walkers that do exceed 128 rows are then taken by the general kernels: time, never correctness)
  const bool hint_le128 = !s.full_bonds && h >= 0 && h + 12 <= 128;
  mr.MID_HI = (m > 128 && !hint_le128) ? 256 : 128;
  mr.GS = std::min(m, mr.MID_HI);
  if constexpr (sizeof(T) == 4) {
    static const bool no_mid = getenv("PEPSGPU_NO_MIDROUTE") != nullptr;
    // 24 (the carry rank grows by a few states per row): a hint at or below it says no walker is near 32 live rows at this
    // site -> skip the route's launches; walkers that do exceed 32 rows are then taken by the general kernels.  NO hint: route.
    const bool near = h < 0 || h > 24;
    mr.on = !no_mid && rank_adapt() && m > JR_SMALL_ROWS && uk <= 1024 && near;
  }
  if (!mr.on) return mr;
  const int GS = mr.GS;
  constexpr bool is_f32 = sizeof(T) == 4;
  mr.midflag = (int *)arena_.alloc(sizeof(int) * nw_);
  mr.nmid = (int *)arena_.alloc(sizeof(int) * nw_);
  mr.mB = (int *)arena_.alloc(sizeof(int) * nw_);
  PG_CHECK_HIP(hipMemsetAsync(mr.mB, 0, sizeof(int) * nw_, stream_));
  const int lo = jacobi_small_ok(uk, m, s.mdyn[i]) ? JR_SMALL_ROWS : 0;
  hipLaunchKernelGGL(mid_route_flag_kernel, dim3((nw_ + 255) / 256), dim3(256), 0, stream_, (const int *)s.mdyn[i], s.mmul[i], m, lo,
                     mr.MID_HI, nw_, mr.midflag, mr.nmid);
  PG_CHECK_HIP(hipGetLastError());
  mr.Bt = alloc_ten(GS, GS, 1);
  prof_begin(PROF_TRUNC_GRAM, 0.0, 0.0);
  if constexpr (is_f32)   // G = M M^T and its Cholesky in one kernel, G resident in LDS (trunc_mid.h)
    launch_mid_gram_chol<T>(stream_, nw_, (const T *)M.p, M.n, uk, (const int *)mr.nmid, (const int *)mr.midflag, GS, mr.Bt.p, mr.Bt.n, mr.mB);
  if (!is_f32 || GS > 128) {
    // the walkers the fused kernel does not take (more than 128 live rows): Gram through HBM
    int *hiflag = mr.midflag, *nhi = mr.nmid;
    if (is_f32) {
      hiflag = (int *)arena_.alloc(sizeof(int) * nw_);
      nhi = (int *)arena_.alloc(sizeof(int) * nw_);
      hipLaunchKernelGGL(mid_route_flag_kernel, dim3((nw_ + 255) / 256), dim3(256), 0, stream_, (const int *)s.mdyn[i], s.mmul[i], m, 128,
                         mr.MID_HI, nw_, hiflag, nhi);
      PG_CHECK_HIP(hipGetLastError());
    }
    double *Gm = (double *)arena_.alloc(sizeof(double) * (size_t)GS * GS * nw_);
    bool rowgram = false;
    if constexpr (is_f32) {
      if (uk % 16 == 0 && M.n % 4 == 0 && m <= 256) {   // streaming wave-per-block kernel (gram.h)
        // Round 6: the first compression as a diagonally PIVOTED factorisation stopped after pivot_cap rows (chol_pivot.h): the
        // truncation keeps chi of the directions, the pivot order puts the dominant ones first -- no walker keeps more than 64 rows,
        // so the second level never sees the 65..128-row class nor the > 128-row stragglers.  PEPSGPU_PIVOT_CHOL=0: the full
        // factorisation in the natural order (round 3-5); = 56 (default) / 64: the cap (measured, real leg at 8192 walkers: 2 371 amp/s
        // without, 2 626 with 64 rows at two blocks per SIMD, 2 699 with 56 at three; graded subspace error of the prototype 3.7e-8 / 6e-8
        // median against 2.1e-7 of the unpivoted factor).
        static const int pivot_cap = getenv("PEPSGPU_PIVOT_CHOL") ? atoi(getenv("PEPSGPU_PIVOT_CHOL")) : 56;
        // (the cap leaves chi + 24 rows of oversampling: 56 rows up to chi = 32 -- three blocks per SIMD --, 64 up to chi = 40)
        const int kf = std::min(chi_, std::min(m, uk));
        const int kcap = (kf + 24 <= std::min(64, pivot_cap)) ? std::min(64, pivot_cap) : 64;
        mr.pivoted = pivot_cap > 0 && GS > 128 && gram_rows_i8_ok(M.p, m) && kf + 24 <= kcap;
        launch_gram_rows_f64<T>(stream_, nw_, (const T *)M.p, M.n, uk, m, (const int *)nhi, Gm, (long)GS * GS, GS, (const int *)hiflag,
                                tg_flop_counter, tg_byte_counter, mr.pivoted ? 1 : 0);
        rowgram = true;
        if (mr.pivoted)
          launch_chol_pivot<T>(stream_, nw_, (const double *)Gm, (long)GS * GS, GS, mr.Bt.p, mr.Bt.n, mr.mB, GS, (const int *)nhi, 1,
                               (const int *)hiflag, kcap);
      }
    }
    if (!rowgram) tgemm_launch<T, T, double, double>(stream_, desc_rows_gram(m, uk, GS, M.n, nw_, nhi, nullptr, false, hiflag, false), M.p, M.p, Gm);
    if (!mr.pivoted) {
      const size_t smem = chol_smem_bytes(GS);
      allow_dynamic_lds(reinterpret_cast<const void *>(&chol_upper_kernel<T>), smem);
      launch_chol_upper<T>(stream_, nw_, Gm, (long)GS * GS, GS, mr.Bt.p, mr.Bt.n, mr.mB, 0, GS, (const int *)nhi, 1, (const int *)hiflag);
    }
    arena_.free(Gm);
    if constexpr (is_f32) {
      if (GS > 128) trunc_mid_two_level(mr, hiflag, i);
    }
    if (is_f32) { arena_.free(hiflag); arena_.free(nhi); }
  }
  prof_end();
  return mr;
}

// Second level (walkers with more than 128 live rows of M whose factor B kept at most 128 rows -- the usual case: the
// truncation input of a real PEPS is of numerical rank 60-100): the rows of B are as long as M has live rows (up to
// 256), so the same compression is applied once more, B2^T B2 = B B^T (r x r, LDS resident: the fused kernel with B in
// the place of M), and the Jacobi runs on the r x r factor B2 (rows <= 128 long: the sixteen-lanes-per-row tournament at
// its fast size).  Rotated rows of B2 = sigma_k w_k^T (w: left singular vectors of B); sigma_k u_k^T = w_k^T B.
template <typename T>
void Engine<T>::trunc_mid_two_level(MidRoute &mr, const int *hiflag, int i) {
  mr.two_level = true;
  mr.flagA = (int *)arena_.alloc(sizeof(int) * nw_);
  mr.rowsA = (int *)arena_.alloc(sizeof(int) * nw_);
  mr.flag2 = (int *)arena_.alloc(sizeof(int) * nw_);
  mr.rows2 = (int *)arena_.alloc(sizeof(int) * nw_);
  mr.mB2 = (int *)arena_.alloc(sizeof(int) * nw_);
  PG_CHECK_HIP(hipMemsetAsync(mr.mB2, 0, sizeof(int) * nw_, stream_));
  mr.big_list = (int *)arena_.alloc(sizeof(int) * (nw_ + 1));
  PG_CHECK_HIP(hipMemsetAsync(mr.big_list + nw_, 0, sizeof(int), stream_));     // the count sits behind the list
  hipLaunchKernelGGL(mid_split_kernel, dim3((nw_ + 255) / 256), dim3(256), 0, stream_, (const int *)mr.midflag, hiflag, (const int *)mr.mB, 128,
                     nw_, mr.flagA, mr.rowsA, mr.flag2, mr.rows2, mr.big_list, mr.big_list + nw_);
  PG_CHECK_HIP(hipGetLastError());
  mr.B2 = alloc_ten(128, 128, 1);
  if constexpr (sizeof(T) == 4)
    launch_mid_gram_chol<T>(stream_, nw_, (const T *)mr.Bt.p, mr.Bt.n, mr.GS, (const int *)mr.rows2, (const int *)mr.flag2, 128, mr.B2.p, mr.B2.n,
                            mr.mB2);
  if (dbg_verbose()) {   // diagnostics: rows kept by the two compressions
    const std::vector<int> hm = dbg_read(mr.nmid), h1 = dbg_read(mr.mB), h2 = dbg_read(mr.mB2);
    long s0 = 0, s1 = 0, s2 = 0, x0 = 0, x1 = 0, x2 = 0;
    for (int w = 0; w < nw_; ++w) { s0 += hm[w]; s1 += h1[w]; s2 += h2[w]; x0 = std::max<long>(x0, hm[w]); x1 = std::max<long>(x1, h1[w]); x2 = std::max<long>(x2, h2[w]); }
    fprintf(stderr, "[pepsgpu] trunc site %d: live rows of M mean %.1f max %ld -> B mean %.1f max %ld -> B2 mean %.1f max %ld\n", i, (double)s0 / nw_, x0,
            (double)s1 / nw_, x1, (double)s2 / nw_, x2);
  }
}

// The Jacobi of the mid route on its factors.
// <= 64 live rows: two waves per walker, else four; rows of 16 lanes, four pairs per wave instruction (jacobi_rows_grp_kernel)
template <typename T>
void Engine<T>::trunc_mid_jacobi(MidRoute &mr) {
  const int GS = mr.GS;
  float *B = (float *)mr.Bt.p, *B2 = (float *)mr.B2.p;
  const long wB = mr.Bt.n, wB2 = mr.B2.n;
  if (GS <= 128) {
    launch_jacobi_grp<2, 8>(stream_, nw_, B, wB, GS, GS, GS, 40, sweeps_, (const int *)mr.mB, 1, 0);
    if (GS > 64) launch_jacobi_grp<4, 8>(stream_, nw_, B, wB, GS, GS, GS, 40, sweeps_, (const int *)mr.mB, 1, 64);
  } else if (mr.two_level) {
    // on B itself: the walkers with at most 128 live rows of M (B at most 128 columns wide) and, on the 256 x 256
    // register kernel, those whose factor kept more than 128 rows; on B2: everybody else
    launch_jacobi_grp<2, 8>(stream_, nw_, B, wB, GS, 128, GS, 40, sweeps_, (const int *)mr.rowsA, 1, 0);
    launch_jacobi_grp<4, 8>(stream_, nw_, B, wB, GS, 128, GS, 40, sweeps_, (const int *)mr.rowsA, 1, 64);
    // (2048 blocks of 144 KB LDS cost ~0.9 ms even when every block returns at once: a small grid walks the list of the
    // walkers that need it, usually empty)
    // ... on the side stream: the few blocks run beside the launches below (which touch other walkers) instead of holding
    // the whole device for ~0.8 ms; joined before the rows of B are selected
    if (!mr.pivoted) {      // (a pivoted first factor keeps at most 64 rows: the list is empty by construction)
      PG_CHECK_HIP(hipEventRecord(ev_fork_, stream_));
      PG_CHECK_HIP(hipStreamWaitEvent(side_stream_, ev_fork_, 0));
      hipLaunchKernelGGL(jacobi_rows_reg256_list_kernel, dim3(std::min(nw_, 128)), dim3(512), 0, side_stream_, B, wB, GS, GS, GS, 40, sweeps_,
                         (const int *)mr.rowsA, 1, 128, (const int *)mr.big_list, (const int *)(mr.big_list + nw_));
      PG_CHECK_HIP(hipEventRecord(ev_join_, side_stream_));
      mr.side_pending = true;
    }
    // (size classes by row length -- <2,4> for r <= 64, <3,5>, <3,6>, <4,8> -- were measured in round 3: 533 -> 576 ms per
    // step of 4096 dense walkers; the tournament is bound by its exchange / reduction latency, not by the FMAs of a pair)
    launch_jacobi_grp<2, 8>(stream_, nw_, B2, wB2, 128, 128, 128, 40, sweeps_, (const int *)mr.mB2, 1, 0);
    if (!mr.pivoted) launch_jacobi_grp<4, 8>(stream_, nw_, B2, wB2, 128, 128, 128, 40, sweeps_, (const int *)mr.mB2, 1, 64);
  } else {
    // rows of B up to 256 long (sixteen columns per lane); more than 128 live rows of B: the 256 x 256 register kernel
    launch_jacobi_grp<2, 16>(stream_, nw_, B, wB, GS, GS, GS, 40, sweeps_, (const int *)mr.mB, 1, 0);
    launch_jacobi_grp<4, 16>(stream_, nw_, B, wB, GS, GS, GS, 40, sweeps_, (const int *)mr.mB, 1, 64);
    hipLaunchKernelGGL(jacobi_rows_reg256_kernel, dim3(nw_), dim3(512), 0, stream_, B, wB, GS, GS, GS, 40, sweeps_, (const int *)mr.mB, 1, 128);
  }
  PG_CHECK_HIP(hipGetLastError());
}

// Second half of the mid route, entered inside the PROF_SELECT bracket of truncate_site (closed behind the first select here):
// sigma_k u_k^T = the rotated rows of B, the chi largest, normalised -> U^T (k x GS), kB = how many are live; V' = U^T M;
// polish.  Frees everything the route holds except ortho_skip (TruncOut).
template <typename T>
void Engine<T>::trunc_mid_finish(AbsorbState &s, const SiteDims &d, int i, const DTen<T> &M, MidRoute &mr, TruncOut &t) {
  const int m = d.m, uk = d.uk, k = t.k, GS = mr.GS;
  if (mr.side_pending) { PG_CHECK_HIP(hipStreamWaitEvent(stream_, ev_join_, 0)); mr.side_pending = false; }
  int *kB = (int *)arena_.alloc(sizeof(int) * nw_);
  PG_CHECK_HIP(hipMemsetAsync(kB, 0, sizeof(int) * nw_, stream_));
  DTen<T> Ut = alloc_ten(k, GS, 1);
  hipLaunchKernelGGL(select_rows_kernel<T>, dim3(nw_), dim3(256), 0, stream_, (const T *)mr.Bt.p, mr.Bt.n, GS, GS, GS, k, Ut.p, Ut.n,
                     (T *)nullptr, 0L, (const int *)(mr.two_level ? mr.rowsA : mr.mB), 1, kB, trunc_err_, chi_min_, (double *)nullptr,
                     (const int *)(mr.two_level ? mr.flagA : mr.midflag), 1);
  PG_CHECK_HIP(hipGetLastError());
  prof_end();
  if (mr.two_level) {
    // W = the chi largest rotated rows of B2, normalised (truncation rule applied here); U^T = rows of W B, normalised
    int *kB2 = (int *)arena_.alloc(sizeof(int) * nw_);
    PG_CHECK_HIP(hipMemsetAsync(kB2, 0, sizeof(int) * nw_, stream_));
    DTen<T> W = alloc_ten(k, 128, 1), T1 = alloc_ten(k, GS, 1);
    prof_begin(PROF_SELECT, 0.0, 0.0);
    hipLaunchKernelGGL(select_rows_kernel<T>, dim3(nw_), dim3(256), 0, stream_, (const T *)mr.B2.p, mr.B2.n, 128, 128, 128, k, W.p, W.n,
                       (T *)nullptr, 0L, (const int *)mr.mB2, 1, kB2, trunc_err_, chi_min_, (double *)nullptr, (const int *)mr.flag2, 1);
    PG_CHECK_HIP(hipGetLastError());
    prof_end();
    prof_begin(PROF_TRUNC_APPLY, 0.0, 0.0);
    tgemm_launch<T, T, T, double>(stream_, desc_rows_times(k, 128, 128, GS, W.n, mr.Bt.n, T1.n, nw_, nullptr, mr.rows2, mr.flag2), W.p, mr.Bt.p,
                                  T1.p);
    prof_end();
    prof_begin(PROF_SELECT, 0.0, 0.0);
    hipLaunchKernelGGL(select_rows_kernel<T>, dim3(nw_), dim3(256), 0, stream_, (const T *)T1.p, T1.n, k, GS, GS, k, Ut.p, Ut.n, (T *)nullptr,
                       0L, (const int *)kB2, 1, kB, 0.0, 0, (double *)nullptr, (const int *)mr.flag2, 1);
    PG_CHECK_HIP(hipGetLastError());
    prof_end();
    free_ten(W); free_ten(T1); free_ten(mr.B2);
    arena_.free(kB2); arena_.free(mr.flagA); arena_.free(mr.rowsA); arena_.free(mr.flag2); arena_.free(mr.rows2); arena_.free(mr.mB2);
    arena_.free(mr.big_list);
  }
  // V' = U^T M (k x uk): row q is sigma_q v_q^T up to the rounding of u_q -- an error of 1e-7 in u_q brings in the
  // dominant directions with weight 1e-7 sigma_1, which is NOT small against a row of size sigma_q << sigma_1.  So the k
  // rows are not normalised as they come: they are polished (trunc_mid_polish).
  DTen<T> Vp = alloc_ten(k, d.u, d.k2);
  prof_begin(PROF_TRUNC_APPLY, 0.0, 0.0);
  tgemm_launch<T, T, T, double>(stream_, desc_rows_times(k, GS, m, uk, Ut.n, M.n, Vp.n, nw_, nullptr, mr.nmid, mr.midflag), Ut.p, M.p,
                                Vp.p);   // f64 accumulation: small sigma_q are differences
  prof_end();
  const bool qr_done = trunc_mid_polish(d, mr, t, Vp, kB);
  free_ten(mr.Bt); free_ten(Ut); free_ten(Vp);
  if (qr_done) t.ortho_skip = mr.midflag; else arena_.free(mr.midflag);     // (the walkers rows_qr took are orthonormal already)
  arena_.free(mr.nmid); arena_.free(kB);
  arena_.free(mr.mB);
}

// The k rows of V' -> V.  Round 6: only the span of the k rows leaves the site, so the rows are made orthonormal in float64 in
// one launch (rows_qr.h: Cholesky-QR of the unit-scaled rows in their order, i.e. Gram-Schmidt from the dominant direction down;
// live count by the same floor); returns true when it did.  PEPSGPU_ROWS_QR=0 (rounds 3-5): the rows are handed to the one-sided
// Jacobi once more (a k-row problem: the one-wave kernels), which restores their mutual orthogonality relative to each row's own
// norm in one or two sweeps; what is left is contamination by the discarded directions only, of relative size 1e-7.
template <typename T>
bool Engine<T>::trunc_mid_polish(const SiteDims &d, MidRoute &mr, TruncOut &t, DTen<T> &Vp, const int *kB) {
  const int k = t.k, uk = d.uk;
  if constexpr (sizeof(T) == 4) {
    static const int rows_qr = getenv("PEPSGPU_ROWS_QR") ? atoi(getenv("PEPSGPU_ROWS_QR")) : 1;
    if (rows_qr && t.kn_i && rows_qr_ok(k, uk)) {
      prof_begin(PROF_SELECT, 0.0, 0.0);
      launch_rows_qr(stream_, nw_, (const float *)Vp.p, Vp.n, k, uk, kB, (float *)t.V.p, t.V.n, t.kn_i, (const int *)mr.midflag);
      prof_end();
      return true;
    }
  }
  const size_t need = sizeof(T) * (size_t)k * (uk | 1);
  const int use_lds = need <= JACOBI_LDS_MAX;
  if (use_lds) allow_dynamic_lds(reinterpret_cast<const void *>(&jacobi_rows_kernel<T>), need);
  prof_begin(PROF_JACOBI, 0.0, 0.0);
  launch_jacobi(Vp.p, Vp.n, k, uk, use_lds, need, kB, 1);      // walkers off the route have kB = 0 rows
  prof_end();
  prof_begin(PROF_SELECT, 0.0, 0.0);   // normalise, count the live rows; the truncation rule was applied on B already
  hipLaunchKernelGGL(select_rows_kernel<T>, dim3(nw_), dim3(256), 0, stream_, (const T *)Vp.p, Vp.n, k, uk, uk, k, t.V.p, t.V.n, (T *)nullptr,
                     0L, kB, 1, t.kn_i, 0.0, 0, (double *)nullptr, (const int *)mr.midflag, 1);
  PG_CHECK_HIP(hipGetLastError());
  prof_end();
  return false;
}

// ---- float64 engine, dense site: preconditioned truncation with oversampling ----------------------------------------------------
// The f64 mode on a dense state spent 98 % of its time in the general one-sided Jacobi on the 256 x 256 block M (25 amp/s at C4:
// with the rows in global memory a sweep is 255 passes over the matrix).  The Gram-preconditioned route of the f32 engine cannot
// be taken over as it is: the Cholesky of M M^T in float64 perturbs the boundary between the kept direction chi and the discarded
// direction chi + 1 by ~3e-14 s_1^2 / (s_chi^2 - s_chi+1^2), i.e. ~5e-9 per truncation at s_chi / s_1 = 2e-5 -- too much for the
// 1e-8 parity of this mode.  With OVERSAMPLING it can: the route only has to deliver a subspace U of kq = 2 chi dimensions that
// CONTAINS the top-chi left singular subspace -- the mixing that matters is then between direction chi and direction 2 chi + 1,
// smaller by s_2chi+1 / s_chi+1 and with a gap of s_chi^2 (~1e-10 per truncation on the real state) -- and the exact top-chi
// singular vectors inside it come from an accurate float64 Jacobi on Z = U^T M, kq x uk (Rayleigh-Ritz on M itself), LDS resident.
// Walkers that leave a route take the general kernels as before (route_flag = 0).
//
// Round 6: the subspace from a diagonally PIVOTED factorisation of G = M M^T stopped after kq rows (chol_pivot.h; measured on
// the truncation inputs of the real state in float64, scripts/proto_subspace.py: the kept sigma_k v_k lost by the subspace of 64
// pivot rows 2.5e-10 median / 4.4e-9 max of sigma_1, 56 rows 1.8e-9 / 1.9e-8), made orthonormal by a Cholesky-QR2 in float64
// (chol_solve_rows_kernel: U = L^-1 B twice), sharpened by ONE step of subspace iteration on M itself (U <- orth(orth(U M) M^T): the
// part outside shrinks by (sigma_kq+1 / sigma_chi)^2 ~ 3e-3) and followed by the accurate Jacobi on Z = U M.
// No Gram-resolution cliff (a pivoted factor simply stops at the numerical rank: C5's synthetic state keeps 30-47 directions and
// stays on the route) and no Jacobi on a 128 x 128 factor.
template <typename T>
void Engine<T>::trunc_f64_pivot(AbsorbState &s, const SiteDims &d, int i, const DTen<T> &M, int kq, TruncOut &t) {
  const int m = d.m, uk = d.uk, GSd = d.m;
  const int gb = (nw_ + 255) / 256;
  int *rflag = t.route_flag = (int *)arena_.alloc(sizeof(int) * nw_);
  t.gen_rows = (int *)arena_.alloc(sizeof(int) * nw_);
  int *rowsM = (int *)arena_.alloc(sizeof(int) * nw_), *mB1 = (int *)arena_.alloc(sizeof(int) * nw_);
  double *resid = (double *)arena_.alloc(sizeof(double) * nw_);
  PG_CHECK_HIP(hipMemsetAsync(mB1, 0, sizeof(int) * nw_, stream_));
  hipLaunchKernelGGL(f64_route_init_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)s.mdyn[i], s.mmul[i], m, nw_, rowsM, rflag);
  PG_CHECK_HIP(hipGetLastError());
  prof_begin(PROF_TRUNC_GRAM, 0.0, 0.0);
  double *Gm = (double *)arena_.alloc(sizeof(double) * (size_t)GSd * GSd * nw_);
  DTen<T> Bq = alloc_ten(64, GSd, 1), Zt = alloc_ten(64, uk, 1);
  double *Sq = (double *)arena_.alloc(sizeof(double) * 64 * 64 * (size_t)nw_);
  // both triangles: the pivoted factorisation reads whole rows
  tgemm_launch<T, T, double, double>(stream_, desc_rows_gram(m, uk, GSd, M.n, nw_, rowsM, nullptr, true, rflag, false), M.p, M.p, Gm);
  // The factorisation only SELECTS rows of M here (pivot order, down to the rounding noise of G: thresh_scale 0): what the
  // Gram cannot resolve (directions below 2.4e-7 sigma_1 -- C5's synthetic state has ~25 above it for chi = 24: taking the factor
  // itself as the basis left the f64 amplitude at 2.9e-7) comes from the rows themselves, Gram-Schmidt'ed in float64.
  const int slots = chol_pivot_slots(kq);
  int *piv = (int *)arena_.alloc(sizeof(int) * (size_t)slots * nw_);
  launch_chol_pivot<T>(stream_, nw_, (const double *)Gm, (long)GSd * GSd, GSd, Bq.p, Bq.n, mB1, GSd, (const int *)rowsM, 1, (const int *)rflag, kq,
                       resid, 0.0, piv);
  arena_.free(Gm);
  hipLaunchKernelGGL(gather_rows_kernel<T>, dim3(64, nw_), dim3(256), 0, stream_, (const T *)M.p, M.n, uk, (const int *)piv, slots,
                     (const int *)mB1, Zt.p, Zt.n, (const int *)rflag);
  PG_CHECK_HIP(hipGetLastError());
  arena_.free(piv);
  auto orthonormalise = [&](DTen<T> &X, int len, const int *lenlive) {     // Cholesky-QR2 of the mB1 rows of X (in place)
    for (int pass = 0; pass < 2; ++pass) {
      tgemm_launch<T, T, double, double>(stream_, desc_rows_gram(64, len, 64, X.n, nw_, mB1, lenlive, false, rflag, false), X.p, X.p, Sq);
      hipLaunchKernelGGL(chol_solve_rows_kernel, dim3(nw_), dim3(256), 0, stream_, (const double *)Sq, 64L * 64, 64, (double *)X.p, X.n, len,
                         (const int *)mB1, (const int *)rflag);
      PG_CHECK_HIP(hipGetLastError());
    }
  };
  auto times_mt = [&](const DTen<T> &Q, DTen<T> &Uout) {      // U = Q M^T (rows of Q: uk long; rows of U: GSd long, zeros beyond the live rows of M)
    tgemm_launch<T, T, T, double>(stream_, desc_rows_times_t(64, uk, m, GSd, Q.n, M.n, Uout.n, nw_, mB1, rowsM, true, rflag, false), Q.p, M.p,
                                  Uout.p);
  };
  auto times_m = [&](const DTen<T> &U, DTen<T> &Zout) {       // Z = U M (rows of U: GSd long, live part rowsM)
    tgemm_launch<T, T, T, double>(stream_, desc_rows_times(64, GSd, m, uk, U.n, M.n, Zout.n, nw_, mB1, rowsM, rflag), U.p, M.p, Zout.p);
  };
  orthonormalise(Zt, uk, nullptr);                            // Q0: the selected rows of M, orthonormal (right space)
  prof_end();
  prof_begin(PROF_TRUNC_APPLY, 0.0, 0.0);
  times_mt(Zt, Bq);                                           // the pivoted factor itself, from M: B = Q0 M^T
  prof_end();
  prof_begin(PROF_TRUNC_GRAM, 0.0, 0.0);
  orthonormalise(Bq, GSd, rowsM);
  prof_end();
  prof_begin(PROF_TRUNC_APPLY, 0.0, 0.0);
  times_m(Bq, Zt);
  prof_end();
  prof_begin(PROF_TRUNC_GRAM, 0.0, 0.0);
  orthonormalise(Zt, uk, nullptr);      // (each half step re-orthonormalised: U M M^T has the SQUARED condition, 1e12 -- no Gram survives it)
  prof_end();
  prof_begin(PROF_TRUNC_APPLY, 0.0, 0.0);
  times_mt(Zt, Bq);                                           // one step of subspace iteration: U <- orth(orth(U M) M^T)
  prof_end();
  prof_begin(PROF_TRUNC_GRAM, 0.0, 0.0);
  orthonormalise(Bq, GSd, rowsM);
  prof_end();
  prof_begin(PROF_TRUNC_APPLY, 0.0, 0.0);
  times_m(Bq, Zt);
  prof_end();
  prof_begin(PROF_JACOBI, 0.0, 0.0);
  {   // the accurate SVD inside the subspace: one-sided Jacobi on the <= kq rows of Z, LDS resident
    const size_t needz = sizeof(T) * (size_t)kq * (uk | 1);
    allow_dynamic_lds(reinterpret_cast<const void *>(&jacobi_rows_kernel<T>), needz);
    hipLaunchKernelGGL(jacobi_rows_kernel<T>, dim3(nw_), dim3(1024), needz, stream_, Zt.p, Zt.n, kq, uk, uk, 40, 1, sweeps_, (const int *)mB1, 1,
                       0, 0);
    PG_CHECK_HIP(hipGetLastError());
  }
  prof_end();
  prof_begin(PROF_SELECT, 0.0, 0.0);
  hipLaunchKernelGGL(select_rows_kernel<T>, dim3(nw_), dim3(256), 0, stream_, (const T *)Zt.p, Zt.n, kq, uk, uk, t.k, t.V.p, t.V.n, (T *)nullptr,
                     0L, (const int *)mB1, 1, t.kn_i, 0.0, chi_min_, (double *)nullptr, (const int *)rflag, 1);
  PG_CHECK_HIP(hipGetLastError());
  // guard: a cap that cut into the spectrum (resid > 0) is priced by what one step of subspace iteration leaves of it,
  // resid (sigma_1 / sigma_chi)^2; a walker above the tolerance takes the general kernel
  hipLaunchKernelGGL(f64_pivot_guard_kernel<double>, dim3(nw_), dim3(256), 0, stream_, (const double *)Zt.p, Zt.n, uk, (const int *)mB1,
                     t.k_full, (const double *)resid, 3e-2, rflag);
  PG_CHECK_HIP(hipGetLastError());
  prof_end();
  if (dbg_verbose()) {
    const std::vector<int> hf = dbg_read(rflag), hk = dbg_read(mB1);
    const std::vector<double> hr = dbg_read(resid);
    long on = 0, sk = 0; double rmx = 0.0;
    for (int w = 0; w < nw_; ++w) { on += hf[w] < 0; sk += hk[w]; rmx = std::max(rmx, hr[w]); }
    fprintf(stderr, "[pepsgpu] f64 pivoted route site %d (m = %d, uk = %d, kq = %d): %ld of %d walkers on the route, pivot rows mean %.1f, residual pivot max %.2e\n",
            i, m, uk, kq, on, nw_, (double)sk / nw_, rmx);
  }
  // the others: the general kernels on their live rows (the route's walkers count zero rows there)
  t.select_skip = (int *)arena_.alloc(sizeof(int) * nw_);
  hipLaunchKernelGGL(f64_route_fallback_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)rflag, (const int *)rowsM, nw_, t.gen_rows,
                     (const int *)nullptr, t.select_skip);
  PG_CHECK_HIP(hipGetLastError());
  free_ten(Bq); free_ten(Zt);
  arena_.free(Sq); arena_.free(rowsM); arena_.free(mB1); arena_.free(resid);
}

// Round 5 (PEPSGPU_F64_PIVOT=0, blocks above 128 rows): the subspace from two Gram + Cholesky compressions (B^T B = M M^T,
// B2^T B2 = B B^T) and a Jacobi on the small factor B2; both Jacobi problems (<= 128 x 128 and 64 x 256 doubles) live in LDS.
// Walkers whose factors keep fewer than chi + 4 (or more than 128) rows leave the route.
template <typename T>
void Engine<T>::trunc_f64_two_chol(AbsorbState &s, const SiteDims &d, int i, const DTen<T> &M, int kq, TruncOut &t) {
  const int m = d.m, uk = d.uk, GSd = d.m, k_full = t.k_full;
  // a walker stays on the route with as few as chi + 4 directions above the resolution of a Gram: the guard prices what its
  // factors dropped (C5: the synthetic fermionic state keeps 30-47 of kq = 48; real state: the edge sites)
  const int route_lo = std::min(kq, k_full + 4);
  int *rflag = t.route_flag = (int *)arena_.alloc(sizeof(int) * nw_);
  t.gen_rows = (int *)arena_.alloc(sizeof(int) * nw_);
  int *rowsM = (int *)arena_.alloc(sizeof(int) * nw_), *mB1 = (int *)arena_.alloc(sizeof(int) * nw_);
  int *mB2 = (int *)arena_.alloc(sizeof(int) * nw_), *kW = (int *)arena_.alloc(sizeof(int) * nw_);
  PG_CHECK_HIP(hipMemsetAsync(mB1, 0, sizeof(int) * nw_, stream_));
  PG_CHECK_HIP(hipMemsetAsync(mB2, 0, sizeof(int) * nw_, stream_));
  PG_CHECK_HIP(hipMemsetAsync(kW, 0, sizeof(int) * nw_, stream_));
  const int gb = (nw_ + 255) / 256;
  hipLaunchKernelGGL(f64_route_init_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)s.mdyn[i], s.mmul[i], m, nw_, rowsM, rflag);
  PG_CHECK_HIP(hipGetLastError());
  const bool rdbg = dbg_verbose();
  long stage_on[2] = {0, 0}, stage_hi = 0, stage_lo = 0;
  auto count_on = [&](int st) {     // diagnostics: walkers still on the route after a stage
    if (rdbg) for (int v : dbg_read(rflag)) stage_on[st] += v < 0;
  };
  prof_begin(PROF_TRUNC_GRAM, 0.0, 0.0);
  double *Gm = (double *)arena_.alloc(sizeof(double) * (size_t)GSd * GSd * nw_);
  DTen<T> B1 = alloc_ten(GSd, GSd, 1);
  // G = M M^T over the live rows (upper triangle) and its factor, for the walkers flagged by `flag` (nullptr: all), with the
  // pivot threshold scaled by `scale`
  auto factor_m = [&](const int *flag, double scale) {
    tgemm_launch<T, T, double, double>(stream_, desc_rows_gram(m, uk, GSd, M.n, nw_, rowsM, nullptr, false, flag, false), M.p, M.p, Gm);
    launch_chol_upper<T>(stream_, nw_, Gm, (long)GSd * GSd, GSd, B1.p, B1.n, mB1, 0, GSd, (const int *)rowsM, 1, flag, scale);
  };
  factor_m(nullptr, 1.0);
  // Second chance for the walkers whose factor kept more than 128 rows (1-3 of 1 024 per site on the real state -- each of them
  // would otherwise cost a whole general Jacobi, ~40 ms per site whatever the batch): the Gram again (the factorisation works in
  // place) and the factor with the pivot threshold REDO_SCALE times higher, i.e. directions below sqrt(REDO_SCALE) 2.4e-7 s_1
  // dropped; the guard prices exactly that for them.  Who still keeps more than 128 rows leaves the route.
  constexpr double REDO_SCALE = 64.0;
  int *redo = (int *)arena_.alloc(sizeof(int) * nw_), *lvl = (int *)arena_.alloc(sizeof(int) * nw_);
  hipLaunchKernelGGL(f64_route_redo_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)mB1, 128, nw_, redo, lvl);
  PG_CHECK_HIP(hipGetLastError());
  factor_m(redo, REDO_SCALE);
  // ... and a third one at REDO_SCALE^2 for what is still above 128 rows (flat spectra: the guard decides whether that is good enough)
  hipLaunchKernelGGL(f64_route_redo_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)mB1, 128, nw_, redo, lvl, 2);
  PG_CHECK_HIP(hipGetLastError());
  factor_m(redo, REDO_SCALE * REDO_SCALE);
  arena_.free(redo);
  arena_.free(Gm);
  // walkers whose first factor kept more than 128 or fewer than kq rows leave the route
  if (rdbg) for (int v : dbg_read(mB1)) { stage_hi += v > 128; stage_lo += v < route_lo; }
  hipLaunchKernelGGL(f64_route_check_kernel, dim3(gb), dim3(256), 0, stream_, rflag, mB1, route_lo, 128, nw_);
  PG_CHECK_HIP(hipGetLastError());
  count_on(0);
  // The few walkers that leave here (1-3 of 1 024 per site with more than 128 rows, some tens at the edge sites) each cost a whole
  // general Jacobi from global memory, ~50 ms per site whatever the batch: it starts NOW on the side stream, beside the route.
  {
    t.early = (int *)arena_.alloc(sizeof(int) * nw_);
    t.fb_early = (int *)arena_.alloc(sizeof(int) * nw_);
    PG_CHECK_HIP(hipMemcpyAsync(t.early, rflag, sizeof(int) * nw_, hipMemcpyDeviceToDevice, stream_));
    hipLaunchKernelGGL(f64_route_fallback_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)rflag, (const int *)rowsM, nw_, t.fb_early,
                       (const int *)nullptr, (int *)nullptr);
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipEventRecord(ev_fork_, stream_));
    PG_CHECK_HIP(hipStreamWaitEvent(side_stream_, ev_fork_, 0));
    constexpr int CAPS = 64 * 1024;
    allow_dynamic_lds(reinterpret_cast<const void *>(&jacobi_rows_kernel<T>), (size_t)CAPS);
    hipLaunchKernelGGL(jacobi_rows_kernel<T>, dim3(nw_), dim3(1024), CAPS, side_stream_, M.p, M.n, m, uk, uk, 40, 2, sweeps_,
                       (const int *)t.fb_early, 1, 0, 0, CAPS);
    hipLaunchKernelGGL(select_rows_kernel<T>, dim3(nw_), dim3(256), 0, side_stream_, (const T *)M.p, M.n, m, uk, uk, t.k, t.V.p, t.V.n,
                       (T *)nullptr, 0L, (const int *)s.mdyn[i], s.mmul[i], t.kn_i, trunc_err_, chi_min_, (double *)nullptr, (const int *)t.early, 0);
    PG_CHECK_HIP(hipGetLastError());
    PG_CHECK_HIP(hipEventRecord(ev_join_, side_stream_));
  }
  double *G2 = (double *)arena_.alloc(sizeof(double) * (size_t)128 * 128 * nw_);
  DTen<T> B2 = alloc_ten(128, 128, 1);
  // G2 = B B^T (r x r, r = mB1 <= 128), the rows of B are GSd long (zero beyond the live rows of M)
  tgemm_launch<T, T, double, double>(stream_, desc_rows_gram(128, GSd, 128, B1.n, nw_, mB1, rowsM, false, rflag, false), B1.p, B1.p, G2);
  launch_chol_upper<T>(stream_, nw_, G2, 128L * 128, 128, B2.p, B2.n, mB2, 0, 128, (const int *)mB1, 1, (const int *)rflag);
  arena_.free(G2);
  hipLaunchKernelGGL(f64_route_check_kernel, dim3(gb), dim3(256), 0, stream_, rflag, mB2, route_lo, 128, nw_);
  PG_CHECK_HIP(hipGetLastError());
  count_on(1);
  prof_end();
  auto jacobi_lds = [&](DTen<T> &X, int rows, int len, const int *live) {   // LDS-resident one-sided Jacobi on the live rows of X
    prof_begin(PROF_JACOBI, 0.0, 0.0);
    const size_t need = sizeof(T) * (size_t)rows * (len | 1);
    allow_dynamic_lds(reinterpret_cast<const void *>(&jacobi_rows_kernel<T>), need);
    hipLaunchKernelGGL(jacobi_rows_kernel<T>, dim3(nw_), dim3(1024), need, stream_, X.p, X.n, rows, len, len, 40, 1, sweeps_, live, 1, 0, 0);
    PG_CHECK_HIP(hipGetLastError());
    prof_end();
  };
  // kout rows of X (rows x len, `live` of them rotated) selected and normalised into O; live count to kn_out
  auto select = [&](const DTen<T> &X, int rows, int len, int kout, DTen<T> &O, const int *live, int *kn_out, int dmin) {
    prof_begin(PROF_SELECT, 0.0, 0.0);
    hipLaunchKernelGGL(select_rows_kernel<T>, dim3(nw_), dim3(256), 0, stream_, (const T *)X.p, X.n, rows, len, len, kout, O.p, O.n, (T *)nullptr,
                       0L, live, 1, kn_out, 0.0, dmin, (double *)nullptr, (const int *)rflag, 1);
    PG_CHECK_HIP(hipGetLastError());
    prof_end();
  };
  jacobi_lds(B2, 128, 128, mB2);      // rotated rows of B2 = sigma_q w_q^T (128 x 129 doubles)
  DTen<T> Wt = alloc_ten(kq, 128, 1), T1 = alloc_ten(kq, GSd, 1), Uq = alloc_ten(kq, GSd, 1), Zt = alloc_ten(kq, uk, 1);
  select(B2, 128, 128, kq, Wt, mB2, kW, 0);
  prof_begin(PROF_TRUNC_APPLY, 0.0, 0.0);   // sigma_q u_q^T = w_q^T B
  tgemm_launch<T, T, T, double>(stream_, desc_rows_times(kq, 128, 128, GSd, Wt.n, B1.n, T1.n, nw_, nullptr, mB1, rflag), Wt.p, B1.p, T1.p);
  prof_end();
  select(T1, kq, GSd, kq, Uq, kW, nullptr, 0);
  prof_begin(PROF_TRUNC_APPLY, 0.0, 0.0);   // Z = U^T M (kq x uk): its rows span the oversampled subspace exactly (float64 product with M itself)
  tgemm_launch<T, T, T, double>(stream_, desc_rows_times(kq, GSd, m, uk, Uq.n, M.n, Zt.n, nw_, nullptr, rowsM, rflag), Uq.p, M.p, Zt.p);
  prof_end();
  jacobi_lds(Zt, kq, uk, kW);         // the accurate SVD inside the subspace (64 x 257 doubles)
  select(Zt, kq, uk, t.k, t.V, kW, t.kn_i, chi_min_);
  // guard (f64_route_guard_kernel): a spectrum that falls to the resolution of a Gram inside the subspace leaves the route
  constexpr double guard_tol = 1e-10;
  hipLaunchKernelGGL(f64_route_guard_kernel<double>, dim3(nw_), dim3(256), 0, stream_, (const double *)Zt.p, Zt.n, uk, (const int *)kW, k_full,
                     guard_tol, rflag, kq, (const int *)lvl, 5.7e-14 * REDO_SCALE, 5.7e-14 * REDO_SCALE * REDO_SCALE, 5.7e-14, 0);
  PG_CHECK_HIP(hipGetLastError());
  if (rdbg) {   // diagnostics: who stays on the route, rows kept by the two compressions
    const std::vector<int> hf = dbg_read(rflag), h0 = dbg_read(rowsM), hk = dbg_read(kW);
    long on = 0, s0 = 0, sk = 0, x0 = 0;
    for (int w = 0; w < nw_; ++w) { on += hf[w] < 0; s0 += h0[w]; sk += hf[w] < 0 ? hk[w] : 0; x0 = std::max<long>(x0, h0[w]); }
    fprintf(stderr, "[pepsgpu] f64 dense route site %d (m = %d, uk = %d, kq = %d): %ld of %d walkers on the route (after the first factor %ld: %ld above 128 rows, %ld below kq; after the second %ld), live rows of M mean %.1f max %ld, kept directions mean %.1f\n",
            i, m, uk, kq, on, nw_, stage_on[0], stage_hi, stage_lo, stage_on[1], (double)s0 / nw_, x0, on ? (double)sk / on : 0.0);
  }
  // the others: the general kernels on their live rows (the route's walkers count zero rows there)
  t.select_skip = (int *)arena_.alloc(sizeof(int) * nw_);
  hipLaunchKernelGGL(f64_route_fallback_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)rflag, (const int *)rowsM, nw_, t.gen_rows,
                     (const int *)t.early, t.select_skip);
  PG_CHECK_HIP(hipGetLastError());
  free_ten(B1); free_ten(B2); free_ten(Wt); free_ten(T1); free_ten(Uq); free_ten(Zt);
  arena_.free(rowsM); arena_.free(mB1); arena_.free(mB2); arena_.free(kW); arena_.free(lvl);
}

// Diagnostics (pepsgpu_diag_truncate_site): the truncation of ONE interior site -- truncate_site itself (float64) or
// truncate_site_simple (complex) -- on nb given matrices M [nb][m][u * k2], with the walker count, the route choice and the
// copy of the route flag set for the duration of the call.  rows (float64 only, nullable): live rows of M per entry.
template <typename T>
void Engine<T>::diag_truncate_site(const void *M_host, int nb, int m, int u, int k2, const int32_t *rows, int route, void *V_out,
                                   int32_t *klive_out, int32_t *route_flag_out) {
  if constexpr (sizeof(T) == 4) {
    throw Error(1, "diag_truncate_site: float64 and complex contexts only");
  } else {
    PG_REQUIRE(M_host && V_out && klive_out && route_flag_out, 1, "diag_truncate_site: null buffer");
    PG_REQUIRE(nb >= 1 && nb <= maxw_, 1, "diag_truncate_site: nb must be in [1, max_walkers]");
    PG_REQUIRE(m >= 1 && m <= 1024 && u >= 1 && k2 >= 1 && (long)u * k2 <= 1024, 1, "diag_truncate_site: bad sizes");
    PG_REQUIRE(route >= 0 && route <= 3, 1, "diag_truncate_site: route is 0 .. 3");
    PG_REQUIRE(!(kCplx && rows), 1, "diag_truncate_site: the complex path has no live extents");
    if (rows)
      for (int b = 0; b < nb; ++b) PG_REQUIRE(rows[b] >= 0 && rows[b] <= m, 1, "diag_truncate_site: rows[b] must be in [0, m]");
    ArenaScope scope(arena_);
    struct Restore {      // the context's own walker count and route choice come back on every way out
      Engine<T> &e; int nw, route;
      ~Restore() { e.nw_ = nw; e.route_override_ = route; e.diag_flag_out_ = nullptr; }
    } restore{*this, nw_, route_override_};
    nw_ = nb;
    route_override_ = route;
    const int uk = u * k2, i = 1;     // (the routes want an interior site: i > 0)
    SiteDims d;
    d.u = u; d.k2 = k2; d.m = m; d.uk = uk;
    ArenaBuf<int> flag(arena_, (size_t)nb);
    PG_CHECK_HIP(hipMemsetAsync((int *)flag, 0, sizeof(int) * nb, stream_));      // no route launched: the general kernels took everybody
    diag_flag_out_ = (int *)flag;
    DTen<T> M = alloc_ten(m, uk, 1);
    PG_CHECK_HIP(hipMemcpyAsync(M.p, M_host, sizeof(T) * (size_t)M.n * nb, hipMemcpyHostToDevice, stream_));
    DTen<T> V;
    std::vector<int32_t> kl(nb, -1);
    if constexpr (kCplx) {
      V = truncate_site_simple(d, i, M);
    } else {
      BMPSDev in, out;               // (in.depth = 0: no hint of a row absorbed before)
      AbsorbState s;
      s.N = 2; s.in = &in; s.out = &out;
      out.t.resize(2);
      s.kn.assign(3, nullptr); s.clive.assign(3, nullptr);
      s.cur_kmax.assign(3, -1); s.kstat.assign(3, 0); s.kfull.assign(3, 0);
      s.assume_fused.assign(3, 0); s.assume_rows.assign(2, 0);
      s.R.assign(2, DTen<T>()); s.mdyn.assign(2, nullptr); s.mmul.assign(2, 1); s.R_tri.assign(2, 0);
      ArenaBuf<int> drows(arena_, rows ? (size_t)nb : 0);
      if (rows) {
        PG_CHECK_HIP(hipMemcpyAsync((int *)drows, rows, sizeof(int) * nb, hipMemcpyHostToDevice, stream_));
        s.mdyn[i] = (int *)drows;
      }
      const TruncOut t = truncate_site(s, d, i, M, false);
      V = t.V;
      if (t.kn_i) {
        PG_CHECK_HIP(hipMemcpyAsync(kl.data(), t.kn_i, sizeof(int) * nb, hipMemcpyDeviceToHost, stream_));
        PG_CHECK_HIP(hipStreamSynchronize(stream_));
        arena_.free(t.kn_i);
      }
    }
    PG_CHECK_HIP(hipMemcpyAsync(V_out, V.p, sizeof(T) * (size_t)V.n * nb, hipMemcpyDeviceToHost, stream_));
    PG_CHECK_HIP(hipMemcpyAsync(route_flag_out, (int *)flag, sizeof(int) * nb, hipMemcpyDeviceToHost, stream_));
    PG_CHECK_HIP(hipStreamSynchronize(stream_));
    std::copy(kl.begin(), kl.end(), klive_out);
    free_ten(V);
  }
}

}  // namespace pepsgpu

// Row absorption for the COMPLEX element type: the Q-less algorithm of engine.h in its plain form -- static, zero padded
// shapes, no rank / bond adaptivity, generic tensor GEMM on the vector ALUs -- with the conjugations a complex SVD needs:
//
//   forward   P_i = R_i (A_i x W_i),   R_{i+1}^H R_{i+1} = P_i^H P_i          (Hermitian Gram, complex float64)
//   backward  T_i = (A_i x W_i) Y_{i+1},  M_i = R_i T_i,  rows of M_i --complex Jacobi--> sigma_k v_k^H,
//             Vt_i = chi largest rows, normalised  (= V^H of qlten::SVD, bmps_impl.h:235-238),   Y_i = T_i Vt_i^H
//
// Reference: BMPS::MultiplyMPOSVDCompress_ (bmps_impl.h:756-862) + RightCanonicalizeTruncate (:225-263) with
// TenElemT = QLTEN_Complex; no Dag() appears in the reference's absorption, the conjugates are inside qlten::QR / SVD.
// Parity-grade (kernels of linalg_cplx.h), not tuned: the throughput path of this library is real f32.
#pragma once
#include "engine.h"
#include "linalg_cplx.h"

namespace pepsgpu {

template <typename T>
typename Engine<T>::BMPSDev Engine<T>::absorb_simple(int pos, int num, const BMPSDev &in) {
  ArenaScope scope(arena_);
  BMPSDev out;
  AbsorbState s;
  absorb_begin(s, pos, num, true, in, out);
  const int N = s.N;

  // ---------------- forward ----------------
  for (int i = 0; i + 1 < N; ++i) {
    const SiteDims d = absorb_site(s, i);
    const DTen<T> &A = in.t[i], &Ri = s.R[i];
    PG_REQUIRE(Ri.d[1] == d.l && Ri.d[2] == d.a, 3, "MultiplyMPO: bond dimension mismatch");
    DTen<T> X = alloc_ten(d.m * d.l, d.p, d.a2);
    DTen<T> P = alloc_ten(d.m, d.u, d.l2, d.a2);
    TGemmDesc gp = desc_p(d, X.n, P.n, nw_, nullptr, 1, nullptr);
    tgemm_launch<T, T, T, T>(stream_, desc_x(d, Ri.n, A.n, X.n, nw_, nullptr, 1, nullptr, nullptr), Ri.p, A.p, X.p);
    launch_site_gemm_a(gp, cfg_site(d.r, d.c), 1, X.p, P.p);
    free_ten(X);
    const int rows = d.m * d.u, cols = d.l2 * d.a2;
    if (rows < cols) {          // any R with R^H R = P^H P serves, P itself included
      P.d[0] = rows; P.d[1] = d.l2; P.d[2] = d.a2; P.d[3] = 1;
      normalize(P.p, P.n, P.n, nw_, nullptr);
      s.R[i + 1] = P;
    } else {
      PG_REQUIRE(cols <= 1024, 1, "D * chi too large for the complex Cholesky kernel");
      Acc *G = (Acc *)arena_.alloc(sizeof(Acc) * (size_t)cols * cols * nw_);
      s.R[i + 1] = alloc_ten(cols, d.l2, d.a2);
      DTen<T> &Rn = s.R[i + 1];
      tgemm_launch<T, T, Acc, Acc>(stream_, desc_cols_gram(rows, cols, P.n, nw_, nullptr, 1, true, nullptr, true), P.p, P.p, G);   // G = P^H P
      if constexpr (kCplx) {
        hipLaunchKernelGGL(chol_upper_cplx_kernel<T>, dim3(nw_), dim3(1024), 0, stream_, (c128 *)G, (long)cols * cols, cols, Rn.p, Rn.n,
                           (int *)nullptr);
      } else {
        const size_t smem = chol_smem_bytes(cols);
        allow_dynamic_lds(reinterpret_cast<const void *>(&chol_upper_kernel<T>), smem);
        hipLaunchKernelGGL(chol_upper_kernel<T>, dim3(nw_), dim3(256), smem, stream_, (double *)G, (long)cols * cols, cols, Rn.p, Rn.n,
                           (int *)nullptr);
      }
      PG_CHECK_HIP(hipGetLastError());
      arena_.free(G);
      free_ten(P);
    }
  }

  // ---------------- backward ----------------
  out.t.resize(N);
  out.live.assign(N + 1, nullptr);
  out.logscale = (double *)arena_.alloc(sizeof(double) * nw_);
  PG_CHECK_HIP(hipMemcpyAsync(out.logscale, in.logscale, sizeof(double) * nw_, hipMemcpyDeviceToDevice, stream_));
  s.Y = ones3();   // [l2, a2, k2]
  for (int i = N - 1; i >= 0; --i) {
    const SiteDims d = absorb_site(s, i);
    const DTen<T> &A = in.t[i];
    const int m = d.m, uk = d.uk;
    PG_REQUIRE(s.Y.d[0] == d.l2 && s.Y.d[1] == d.a2, 3, "MultiplyMPO: bond dimension mismatch (backward)");
    DTen<T> Z1 = alloc_ten(d.a, d.p, d.l2, d.k2);
    DTen<T> Tt = alloc_ten(d.l, d.a, d.u, d.k2);
    TGemmDesc gt = desc_tt(d, false, Z1.n, Tt.n, nw_, nullptr, nullptr, false);
    tgemm_launch<T, T, T, T>(stream_, desc_z1(d, A.n, s.Y.n, Z1.n, nw_, nullptr, nullptr, nullptr), A.p, s.Y.p, Z1.p);
    launch_site_gemm_a(gt, cfg_site(d.r, d.c), 1, Z1.p, Tt.p);
    free_ten(Z1);
    free_ten(s.Y);
    if (i == 0) {
      PG_REQUIRE(d.l == 1 && d.a == 1, 3, "MultiplyMPO: left boundary bond is not trivial");
      Tt.d[0] = 1; Tt.d[1] = d.u; Tt.d[2] = d.k2; Tt.d[3] = 1;
      normalize(Tt.p, Tt.n, Tt.n, nw_, out.logscale);
      out.t[0] = Tt;
      break;
    }
    PG_REQUIRE(s.R[i].d[1] == d.l && s.R[i].d[2] == d.a, 3, "MultiplyMPO: carry dimension mismatch");
    DTen<T> M = alloc_ten(m, uk, 1);
    tgemm_launch<T, T, T, T>(stream_, desc_m(d, false, s.R[i].n, Tt.n, M.n, nw_, nullptr, 1, nullptr, nullptr, false), s.R[i].p, Tt.p, M.p);
    DTen<T> V = truncate_site_simple(d, i, M);
    const int k = V.d[0];
    out.t[i] = V;
    DTen<T> Yn = alloc_ten(d.l, d.a, k);
    // Y[(l,a),q] = sum_{(u,k2)} Tt[(l,a),(u,k2)] conj(Vt[q,(u,k2)])
    tgemm_launch<T, T, T, T>(stream_, desc_y(d, k, false, Tt.n, V.n, Yn.n, nw_, nullptr, nullptr, nullptr, false, true), Tt.p, V.p, Yn.p);
    normalize(Yn.p, Yn.n, Yn.n, nw_, out.logscale);
    free_ten(Tt);
    s.Y = Yn;
  }
  for (auto &t : s.R) arena_.free(t.p);
  out.kmax.assign(N + 1, -1);
  out.mlmax.assign(N, -1);
  out.depth = in.depth + 1;
  ++n_absorb_;
  return out;
}

// The truncation of one site of absorb_simple: rows of M -> the k = min(chi, m, uk) largest (sigma_q v_q^H) normalised into V,
// by a dense route where the site takes one and by the general Jacobi for the walkers no route kept.  Consumes M.
template <typename T>
DTen<T> Engine<T>::truncate_site_simple(const SiteDims &d, int i, DTen<T> &M) {
  const int m = d.m, uk = d.uk;
  const int k = std::min(chi_, std::min(m, uk));
  PG_REQUIRE(m <= 1024, 1, "bond dimension too large for select_rows_kernel");
  DTen<T> V = alloc_ten(k, d.u, d.k2);
  // ---- dense sites, complex element type (round 5): the oversampled route of the float64 engine (engine_impl.h has the statement
  // and the error argument) with the Hermitian forms.  The complex one-sided Jacobi on the 256 x 256 block was 96 % of a dense
  // amplitude (6.6 amp/s at C4 whatever the batch).  Static shapes (this path has no live extents); walkers a route does not keep
  // (rflag >= 0) take the general kernel as before.
  int *rflag = nullptr;
  if constexpr (kCplx) {
    static const bool no_route_env = getenv("PEPSGPU_NO_C128_DENSE_ROUTE") != nullptr;
    static const int f64_pivot_env = getenv("PEPSGPU_F64_PIVOT") ? atoi(getenv("PEPSGPU_F64_PIVOT")) : 1;   // 0: the two-Cholesky route of round 5
    const DenseRouteChoice rc = dense_route_choice(no_route_env, f64_pivot_env);
    const bool no_route = rc.off;
    const int f64_pivot = rc.pivot;
    const int kq = std::min(2 * k, (3 * std::min(m, uk)) / 4);
    const bool route_ok = !no_route && trunc_err_ == 0.0 && m <= 256 && uk <= 256 && kq <= 64 && kq >= k + 8;
    if (f64_pivot && route_ok && m >= 64) rflag = trunc_c128_rangefinder(d, M, k, kq, V);
    else if (route_ok && m > 128 && m <= uk) rflag = trunc_c128_two_chol(d, i, M, k, kq, V);   // (m <= uk: see truncate_site, engine_impl.h)
  }
  // the general kernel: every walker, or -- behind the route -- the walkers that left it (rflag >= 0)
  if constexpr (kCplx) {
    hipLaunchKernelGGL(jacobi_rows_cplx_kernel<T>, dim3(nw_), dim3(1024), 0, stream_, M.p, M.n, m, uk, uk, 60, sweeps_,
                       (const int *)rflag, 0);
  } else {
    hipLaunchKernelGGL(jacobi_rows_kernel<T>, dim3(nw_), dim3(1024), 0, stream_, M.p, M.n, m, uk, uk, 60, 0, sweeps_,
                       (const int *)nullptr, 1, 0);
  }
  PG_CHECK_HIP(hipGetLastError());
  ++n_jacobi_;
  hipLaunchKernelGGL(select_rows_kernel<T>, dim3(nw_), dim3(256), 0, stream_, (const T *)M.p, M.n, m, uk, uk, k, V.p, V.n,
                     (T *)nullptr, 0L, (const int *)nullptr, 1, (int *)nullptr, trunc_err_, chi_min_, (double *)nullptr,
                     (const int *)rflag, rflag ? 0 : 1);
  PG_CHECK_HIP(hipGetLastError());
  if (rflag) { diag_keep_route_flag(rflag); arena_.free(rflag); rflag = nullptr; }
  free_ten(M);
  return V;
}

// Round 6: the oversampled subspace from a RANDOMISED range finder -- a fixed table of signs times M, three re-orthonormalised steps
// of subspace iteration (every half step a Cholesky-QR2 in complex float64, chol_solve_rows_cplx_kernel), then the complex
// Jacobi on Z = U M.  What lies outside the kq = 2 chi directions enters direction chi damped by (sigma_kq+1 / sigma_chi)^6
// (~2e-8 on a state of the real spectrum): no Gram of M, no factorisation, no Jacobi on a 128 x 128 factor.  A spectrum that does not
// fall like that (flat at kq, or a cliff just behind chi) would be delivered with a visible loss -- 3e-2 of sigma_1 on sigma_j =
// 10^(-2 j / 256): the guard at the end prices the leakage from the rotated rows of Z and hands such walkers to the general kernel.  (The float64 route
// selects its start rows by a pivoted factorisation, chol_pivot.h; a complex factor column does not fit a thread's registers.)
// Returns the route flag (< 0: the walker's rows are in V); the caller frees it.
template <typename T>
int *Engine<T>::trunc_c128_rangefinder(const SiteDims &d, const DTen<T> &M, int k, int kq, DTen<T> &V) {
  const int m = d.m, uk = d.uk;
  const int gb = (nw_ + 255) / 256;
  int *rflag = (int *)arena_.alloc(sizeof(int) * nw_);
  int *rowsM = (int *)arena_.alloc(sizeof(int) * nw_);
  hipLaunchKernelGGL(f64_route_init_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)nullptr, 1, m, nw_, rowsM, rflag);
  arena_.free(rowsM);
  DTen<T> Om = alloc_ten(kq, m, 1);           // (only the first walker's slice is used: the table is shared, batch stride 0)
  hipLaunchKernelGGL(sign_table_kernel<T>, dim3((kq * m + 255) / 256), dim3(256), 0, stream_, Om.p, kq, m);
  PG_CHECK_HIP(hipGetLastError());
  DTen<T> Qz = alloc_ten(kq, uk, 1), Uz = alloc_ten(kq, m, 1);
  Acc *Sq = (Acc *)arena_.alloc(sizeof(Acc) * 64 * 64 * (size_t)nw_);
  auto orth = [&](DTen<T> &X, int len) {      // Cholesky-QR2 of the kq rows of X (in place)
    for (int pass = 0; pass < 2; ++pass) {
      tgemm_launch<T, T, Acc, Acc>(stream_, desc_rows_gram(kq, len, 64, X.n, nw_, nullptr, nullptr, false, nullptr, true), X.p, X.p, Sq);
      hipLaunchKernelGGL(chol_solve_rows_cplx_kernel, dim3(nw_), dim3(256), 0, stream_, (const c128 *)Sq, 64L * 64, 64, (c128 *)X.p, X.n, len, kq,
                         (const int *)nullptr);
      PG_CHECK_HIP(hipGetLastError());
    }
  };
  auto times_m = [&](const DTen<T> &U, long wU, DTen<T> &Zout) {       // Z = U M (kq x uk)
    tgemm_launch<T, T, T, T>(stream_, desc_rows_times(kq, m, m, uk, wU, M.n, Zout.n, nw_, nullptr, nullptr, nullptr), U.p, M.p, Zout.p);
  };
  auto times_mh = [&](const DTen<T> &Q, DTen<T> &Uout) {               // U = Q M^H (kq x m)
    tgemm_launch<T, T, T, T>(stream_, desc_rows_times_t(kq, uk, m, m, Q.n, M.n, Uout.n, nw_, nullptr, nullptr, false, nullptr, true), Q.p, M.p,
                             Uout.p);
  };
  times_m(Om, 0L, Qz);                          // the sketch: signs times M
  constexpr int iters = 3;
  for (int it = 0; it < iters; ++it) {
    orth(Qz, uk);
    times_mh(Qz, Uz);
    orth(Uz, m);
    times_m(Uz, Uz.n, Qz);
  }
  hipLaunchKernelGGL(jacobi_rows_cplx_kernel<T>, dim3(nw_), dim3(1024), 0, stream_, Qz.p, Qz.n, kq, uk, uk, 60, sweeps_, (const int *)rflag, 1);
  hipLaunchKernelGGL(select_rows_kernel<T>, dim3(nw_), dim3(256), 0, stream_, (const T *)Qz.p, Qz.n, kq, uk, uk, k, V.p, V.n, (T *)nullptr, 0L,
                     (const int *)nullptr, 1, (int *)nullptr, 0.0, chi_min_, (double *)nullptr, (const int *)rflag, 1);
  PG_CHECK_HIP(hipGetLastError());
  // guard (rangefinder_guard_kernel): a walker whose spectrum inside the subspace does not price the leakage of the three steps below
  // the tolerance leaves the route; the caller's general Jacobi and select redo it (they run for rflag >= 0).  1e-11: the loss is at
  // most 8 x the priced value (tests/test_cpu_trunc_route_ref.py), i.e. below 1e-10, the level of the float64 route's own algorithmic
  // loss; a spectrum of the real state's shape prices at 1e-13, a flat one or a cliff behind chi at 4e-9 or more.
  constexpr double guard_tol = 1e-11;
  hipLaunchKernelGGL(rangefinder_guard_kernel<T>, dim3(nw_), dim3(256), 0, stream_, (const T *)Qz.p, Qz.n, uk, kq, k, iters, guard_tol, rflag);
  PG_CHECK_HIP(hipGetLastError());
  if (dbg_verbose()) {   // diagnostics: who stays on the route
    long on = 0;
    for (int v : dbg_read(rflag)) on += v < 0;
    fprintf(stderr, "[pepsgpu] c128 range finder (m = %d, uk = %d, kq = %d): %ld of %d walkers on the route\n", m, uk, kq, on, nw_);
  }
  free_ten(Om); free_ten(Qz); free_ten(Uz);
  arena_.free(Sq);
  return rflag;
}

// Round 5 (PEPSGPU_F64_PIVOT=0, blocks above 128 rows): the two-level route of the float64 engine (trunc_f64_two_chol) with the
// Hermitian forms: B^H B = M M^H, B2^H B2 = B B^H, rotated rows of B2 = sigma w^H, w^H B = sigma u^H, Z = U^H M, complex Jacobi on
// the 2 chi rows of Z.  Walkers whose factors keep more than 128 or fewer than chi + 4 rows, or whom the guard rejects, leave the
// route.  Returns the route flag; the caller frees it.
template <typename T>
int *Engine<T>::trunc_c128_two_chol(const SiteDims &d, int i, const DTen<T> &M, int k, int kq, DTen<T> &V) {
  const int m = d.m, uk = d.uk;
  const int gb = (nw_ + 255) / 256, route_lo = std::min(kq, k + 4);
  constexpr double REDO_SCALE = 64.0;
  int *rflag = (int *)arena_.alloc(sizeof(int) * nw_);
  int *rowsM = (int *)arena_.alloc(sizeof(int) * nw_), *mB1 = (int *)arena_.alloc(sizeof(int) * nw_);
  int *mB2 = (int *)arena_.alloc(sizeof(int) * nw_), *kW = (int *)arena_.alloc(sizeof(int) * nw_);
  int *redo = (int *)arena_.alloc(sizeof(int) * nw_), *lvl = (int *)arena_.alloc(sizeof(int) * nw_);
  PG_CHECK_HIP(hipMemsetAsync(mB1, 0, sizeof(int) * nw_, stream_));
  PG_CHECK_HIP(hipMemsetAsync(mB2, 0, sizeof(int) * nw_, stream_));
  PG_CHECK_HIP(hipMemsetAsync(kW, 0, sizeof(int) * nw_, stream_));
  hipLaunchKernelGGL(f64_route_init_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)nullptr, 1, m, nw_, rowsM, rflag);
  Acc *Gm = (Acc *)arena_.alloc(sizeof(Acc) * (size_t)m * m * nw_);
  DTen<T> B1 = alloc_ten(m, m, 1);
  // G = M M^H (upper triangle) and its factor for the walkers flagged by `flag` (nullptr: all), pivot threshold scaled by `scale`
  auto factor_m = [&](const int *flag, double scale) {
    tgemm_launch<T, T, Acc, Acc>(stream_, desc_rows_gram(m, uk, m, M.n, nw_, nullptr, nullptr, false, flag, true), M.p, M.p, Gm);
    hipLaunchKernelGGL(chol_upper_cplx_kernel<T>, dim3(nw_), dim3(1024), 0, stream_, (c128 *)Gm, (long)m * m, m, B1.p, B1.n, mB1, flag, scale);
  };
  factor_m(nullptr, 1.0);
  // second chance for the walkers whose factor kept more than 128 rows: pivot threshold x REDO_SCALE (the guard prices it)
  hipLaunchKernelGGL(f64_route_redo_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)mB1, 128, nw_, redo, lvl);
  factor_m(redo, REDO_SCALE);
  hipLaunchKernelGGL(f64_route_redo_kernel, dim3(gb), dim3(256), 0, stream_, (const int *)mB1, 128, nw_, redo, lvl, 2);
  factor_m(redo, REDO_SCALE * REDO_SCALE);
  PG_CHECK_HIP(hipGetLastError());
  arena_.free(Gm);
  hipLaunchKernelGGL(f64_route_check_kernel, dim3(gb), dim3(256), 0, stream_, rflag, mB1, route_lo, 128, nw_);
  Acc *G2 = (Acc *)arena_.alloc(sizeof(Acc) * (size_t)128 * 128 * nw_);
  PG_CHECK_HIP(hipMemsetAsync(G2, 0, sizeof(Acc) * (size_t)128 * 128 * nw_, stream_));   // (the factor kernel reads the full order)
  DTen<T> B2 = alloc_ten(128, 128, 1);
  // G2 = B B^H over the kept rows of B (<= 128; rows of B are m long)
  tgemm_launch<T, T, Acc, Acc>(stream_, desc_rows_gram(128, m, 128, B1.n, nw_, mB1, nullptr, false, rflag, true), B1.p, B1.p, G2);
  hipLaunchKernelGGL(chol_upper_cplx_kernel<T>, dim3(nw_), dim3(1024), 0, stream_, (c128 *)G2, 128L * 128, 128, B2.p, B2.n, mB2,
                     (const int *)rflag, 1.0);
  PG_CHECK_HIP(hipGetLastError());
  arena_.free(G2);
  hipLaunchKernelGGL(f64_route_check_kernel, dim3(gb), dim3(256), 0, stream_, rflag, mB2, route_lo, 128, nw_);
  hipLaunchKernelGGL(jacobi_rows_cplx_kernel<T>, dim3(nw_), dim3(1024), 0, stream_, B2.p, B2.n, 128, 128, 128, 60, sweeps_, (const int *)rflag, 1);
  PG_CHECK_HIP(hipGetLastError());
  DTen<T> Wt = alloc_ten(kq, 128, 1), T1 = alloc_ten(kq, m, 1), Uq = alloc_ten(kq, m, 1), Zt = alloc_ten(kq, uk, 1);
  // kout rows of X (rows x len, `live` of them rotated) selected and normalised into O
  auto select = [&](const DTen<T> &X, int rows, int len, int kout, DTen<T> &O, const int *live, int *kn_out, int dmin) {
    hipLaunchKernelGGL(select_rows_kernel<T>, dim3(nw_), dim3(256), 0, stream_, (const T *)X.p, X.n, rows, len, len, kout, O.p, O.n, (T *)nullptr,
                       0L, live, 1, kn_out, 0.0, dmin, (double *)nullptr, (const int *)rflag, 1);
  };
  select(B2, 128, 128, kq, Wt, mB2, kW, 0);
  PG_CHECK_HIP(hipGetLastError());
  // sigma_q u_q^H = w_q^H B
  tgemm_launch<T, T, T, T>(stream_, desc_rows_times(kq, 128, 128, m, Wt.n, B1.n, T1.n, nw_, nullptr, mB1, rflag), Wt.p, B1.p, T1.p);
  select(T1, kq, m, kq, Uq, kW, nullptr, 0);
  PG_CHECK_HIP(hipGetLastError());
  // Z = U^H M (kq x uk)
  tgemm_launch<T, T, T, T>(stream_, desc_rows_times(kq, m, m, uk, Uq.n, M.n, Zt.n, nw_, nullptr, nullptr, rflag), Uq.p, M.p, Zt.p);
  hipLaunchKernelGGL(jacobi_rows_cplx_kernel<T>, dim3(nw_), dim3(1024), 0, stream_, Zt.p, Zt.n, kq, uk, uk, 60, sweeps_, (const int *)rflag, 1);
  select(Zt, kq, uk, k, V, kW, nullptr, chi_min_);
  constexpr double guard_tol = 1e-10;
  hipLaunchKernelGGL(f64_route_guard_kernel<T>, dim3(nw_), dim3(256), 0, stream_, (const T *)Zt.p, Zt.n, uk, (const int *)kW, k, guard_tol, rflag,
                     kq, (const int *)lvl, 5.7e-14 * REDO_SCALE, 5.7e-14 * REDO_SCALE * REDO_SCALE, 5.7e-14, 0);
  PG_CHECK_HIP(hipGetLastError());
  if (dbg_verbose()) {   // diagnostics: who stays on the route
    const std::vector<int> hf = dbg_read(rflag), h1 = dbg_read(mB1), h2 = dbg_read(mB2), hk = dbg_read(kW);
    long on = 0, s1 = 0, s2 = 0, sk = 0, z1 = 0, z2 = 0;
    for (int w = 0; w < nw_; ++w) { on += hf[w] < 0; s1 += h1[w]; s2 += h2[w]; sk += hf[w] < 0 ? hk[w] : 0; z1 += h1[w] == 0; z2 += h2[w] == 0; }
    fprintf(stderr, "[pepsgpu] c128 dense route site %d (m = %d, uk = %d, kq = %d): %ld of %d walkers on the route; first factor rows mean %.1f (%ld off), second %.1f (%ld off), kept directions mean %.1f\n",
            i, m, uk, kq, on, nw_, (double)s1 / nw_, z1, (double)s2 / nw_, z2, on ? (double)sk / on : 0.0);
  }
  free_ten(B1); free_ten(B2); free_ten(Wt); free_ten(T1); free_ten(Uq); free_ten(Zt);
  arena_.free(rowsM); arena_.free(mB1); arena_.free(mB2); arena_.free(kW); arena_.free(redo); arena_.free(lvl);
  return rflag;
}

}  // namespace pepsgpu

// Float64 eigendecomposition A = Z diag(w) Z^H of a real symmetric or complex Hermitian n x n matrix resident in HBM: the
// replicated eigensolve of MinSR (optimizer/minsr_eigensolve.h:101-155: dsyev / zheev on the Ns x Ns matrix T) without a host
// LAPACK.  n is bounded by memory only; nothing is assumed to fit in LDS.
//
// Method: two-sided parallel Jacobi with round-robin pairing.  m = n rounded up to even players meet in m - 1 rounds of m / 2
// disjoint pairs (p, q); an odd n gets a bye (the player m - 1 does not exist: its pair rotates nothing and no padding row is
// ever read or written).  One round is two launches:
//   eigh_rot_kernel     one lane per pair: (c, sigma) of J = [[c, sigma], [-conj(sigma), c]] that diagonalises the 2 x 2 block
//                       [[a_pp, a_pq], [conj(a_pq), a_qq]]; a pair with |a_pq| <= thr = eps |A|_F / n is left alone (identity)
//                       and the others are counted in HBM;
//   eigh_apply_kernel   A <- J^H A J for the product J of the round's rotations: the pairs partition the indices, so the
//                       2 x 2 blocks A[{p_i, q_i}, {p_j, q_j}] partition the matrix, and lane (i, j) rewrites its own block in place
//                       from J_i and J_j alone.  The same launch rotates the rows p_i, q_i of V = Z^T.
// The two-sided form is used because the one-sided (Hestenes) iteration on the columns of an INDEFINITE matrix converges to its
// singular vectors: eigenvalues +x and -x share a singular value and their eigenvectors are not separated (A = [[0, 1], [1, 0]]
// has orthogonal columns already).  Here the signs of w are simply those of the diagonal A converges to.
// Storage: row-major A; the vectors are kept as rows of V = Z^T (not conjugated), so that a rotation of two eigenvectors combines
// two contiguous rows and lanes run along them.  In A, lane j of a wave touches column p_j = (r + j) mod (m - 1), ascending, and
// q_j = (r - j) mod (m - 1), descending: both contiguous.  A block below the diagonal is computed as the conjugate transpose of its
// mirror image, in the same order of operations, so A stays exactly Hermitian.
// Convergence: a sweep (m - 1 rounds) in which no pair was rotated; the host reads the counter once per sweep.  Then every
// off-diagonal entry is below thr, i.e. off(A) <= eps |A|_F.  The cap is EIGH_MAX_SWEEPS; reaching it is reported.
// Order: the eigenvalues are ranked on the device (ties by index) and the rows of V are written, permuted, over A, whose
// diagonal has been taken: on return A holds Z^T with ascending w, V is scratch.
#pragma once
#include "linalg.h"

namespace pepsgpu {

constexpr int EIGH_MAX_SWEEPS = 30;

// doubles of device workspace next to A and V: [0] thr, [1] |A|_F^2, [2] the rotation counter (an int), [8 ..) the round's
// rotations (c, Re sigma, Im sigma, t |a_pq|) per pair, the unsorted eigenvalues, their ranks (ints), 256 partial sums
inline size_t eigh_work_doubles(int n) { return 8 + 4 * (size_t)((n + 1) / 2) + 2 * (size_t)n + 256; }

// pair k of round r among m players (m even): player m - 1 stays, the others go round
__device__ __forceinline__ void eigh_pair(int k, int r, int m, int &p, int &q) {
  if (k == 0) { p = m - 1; q = r; return; }
  p = r + k; if (p >= m - 1) p -= m - 1;
  q = r - k; if (q < 0) q += m - 1;
}

// part[block] = the block's share of sum x^2 over len doubles (fixed order, no atomics)
__global__ __launch_bounds__(256) void eigh_sumsq_kernel(const double *__restrict__ x, long len, double *__restrict__ part) {
  __shared__ double s_red[4];
  double acc = 0.0;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < len; e += (long)gridDim.x * 256) acc += x[e] * x[e];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = s_red[0] + s_red[1] + s_red[2] + s_red[3];
}
// work[1] = |A|_F^2, work[0] = thr = eps |A|_F / n
__global__ __launch_bounds__(64) void eigh_thr_kernel(const double *__restrict__ part, int nblocks, int n, double *__restrict__ work) {
  double acc = 0.0;
  for (int e = threadIdx.x; e < nblocks; e += 64) acc += part[e];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) { work[1] = acc; work[0] = 2.220446049250313e-16 * sqrt(acc) / (double)n; }
}

// V = identity
template <int Z>
__global__ __launch_bounds__(256) void eigh_identity_kernel(double *__restrict__ v, int n) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)n * n) return;
  const int row = (int)(e / n), col = (int)(e - (long)row * n);
  v[Z * e] = row == col ? 1.0 : 0.0;
  if (Z == 2) v[2 * e + 1] = 0.0;
}

template <int Z>
__global__ __launch_bounds__(64) void eigh_rot_kernel(const double *__restrict__ a, int n, int m, int r, double *__restrict__ rot,
                                                      const double *__restrict__ thr, int *__restrict__ count) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= m / 2) return;
  int p, q;
  eigh_pair(k, r, m, p, q);
  double c = 1.0, sr = 0.0, si = 0.0, tb = 0.0;
  if (p < n && q < n) {
    const double app = a[Z * ((long)p * n + p)], aqq = a[Z * ((long)q * n + q)];
    const double br = a[Z * ((long)p * n + q)], bi = Z == 2 ? a[Z * ((long)p * n + q) + 1] : 0.0;
    const double ab = Z == 2 ? hypot(br, bi) : fabs(br);
    if (ab > *thr) {
      const double tau = (aqq - app) / (2.0 * ab);
      const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
      c = 1.0 / sqrt(1.0 + t * t);
      const double s = t * c;
      sr = s * (br / ab); si = s * (bi / ab);
      tb = t * ab;
      atomicAdd(count, 1);
    }
  }
  double *o = rot + 4 * (long)k;
  o[0] = c; o[1] = sr; o[2] = si; o[3] = tb;
}

struct EighRot { double c, sr, si; };

// x <- L^H x R for the 2 x 2 block x = (x00, x01, x10, x11) of Z doubles each, L = [[c, s], [-conj(s), c]]
template <int Z>
__device__ __forceinline__ void eigh_block(double (*x)[Z], const EighRot &L, const EighRot &R) {
#pragma clang fp contract(off)
  double y[4][Z];
  if constexpr (Z == 1) {
    y[0][0] = L.c * x[0][0] - L.sr * x[2][0];
    y[1][0] = L.c * x[1][0] - L.sr * x[3][0];
    y[2][0] = L.sr * x[0][0] + L.c * x[2][0];
    y[3][0] = L.sr * x[1][0] + L.c * x[3][0];
    x[0][0] = R.c * y[0][0] - R.sr * y[1][0];
    x[1][0] = R.sr * y[0][0] + R.c * y[1][0];
    x[2][0] = R.c * y[2][0] - R.sr * y[3][0];
    x[3][0] = R.sr * y[2][0] + R.c * y[3][0];
  } else {
    // rows: y_p = c x_p - s x_q, y_q = conj(s) x_p + c x_q
    for (int col = 0; col < 2; ++col) {
      const double pr = x[col][0], pi = x[col][1], qr = x[2 + col][0], qi = x[2 + col][1];
      y[col][0] = L.c * pr - (L.sr * qr - L.si * qi);
      y[col][1] = L.c * pi - (L.sr * qi + L.si * qr);
      y[2 + col][0] = (L.sr * pr + L.si * pi) + L.c * qr;
      y[2 + col][1] = (L.sr * pi - L.si * pr) + L.c * qi;
    }
    // columns: z_p = c y_p - conj(s) y_q, z_q = s y_p + c y_q
    for (int row = 0; row < 2; ++row) {
      const double pr = y[2 * row][0], pi = y[2 * row][1], qr = y[2 * row + 1][0], qi = y[2 * row + 1][1];
      x[2 * row][0] = R.c * pr - (R.sr * qr + R.si * qi);
      x[2 * row][1] = R.c * pi - (R.sr * qi - R.si * qr);
      x[2 * row + 1][0] = (R.sr * pr - R.si * pi) + R.c * qr;
      x[2 * row + 1][1] = (R.sr * pi + R.si * pr) + R.c * qi;
    }
  }
}

// grid (ceil((m / 2 + n) / 64), ceil((m / 2) / 4)), block (64, 4): lane x < m / 2 of pair-row i owns the block (i, x) of A, lane
// x >= m / 2 the column x - m / 2 of the rows p_i, q_i of V
template <int Z>
__global__ __launch_bounds__(256) void eigh_apply_kernel(double *__restrict__ a, double *__restrict__ v, int n, int m, int r,
                                                         const double *__restrict__ rot) {
#pragma clang fp contract(off)
  const int h = m / 2;
  const int i = blockIdx.y * 4 + threadIdx.y, x = blockIdx.x * 64 + threadIdx.x;
  if (i >= h || x >= h + n) return;
  const double *ri = rot + 4 * (long)i;
  const EighRot Ji{ri[0], ri[1], ri[2]};
  const bool idle_i = Ji.sr == 0.0 && Ji.si == 0.0;      // identity (c = 1 then)
  int pi, qi;
  eigh_pair(i, r, m, pi, qi);
  if (x >= h) {                                           // V' = J^T V on the rows p_i, q_i:  v_p' = c v_p - conj(s) v_q, v_q' = s v_p + c v_q
    if (idle_i) return;                                   // (a pair with the bye is idle)
    const int col = x - h;
    double *vp = v + Z * ((long)pi * n + col), *vq = v + Z * ((long)qi * n + col);
    if constexpr (Z == 1) {
      const double a0 = vp[0], b0 = vq[0];
      vp[0] = Ji.c * a0 - Ji.sr * b0;
      vq[0] = Ji.sr * a0 + Ji.c * b0;
    } else {
      const double ar = vp[0], ai = vp[1], br = vq[0], bi = vq[1];
      vp[0] = Ji.c * ar - (Ji.sr * br + Ji.si * bi);
      vp[1] = Ji.c * ai - (Ji.sr * bi - Ji.si * br);
      vq[0] = (Ji.sr * ar - Ji.si * ai) + Ji.c * br;
      vq[1] = (Ji.sr * ai + Ji.si * ar) + Ji.c * bi;
    }
    return;
  }
  const int j = x;
  const double *rj = rot + 4 * (long)j;
  const EighRot Jj{rj[0], rj[1], rj[2]};
  if (idle_i && Jj.sr == 0.0 && Jj.si == 0.0) return;
  int pj, qj;
  eigh_pair(j, r, m, pj, qj);
  const int rows[2] = {pi, qi}, cols[2] = {pj, qj};
  if (i == j) {                                           // the rotated block itself: diagonal, exactly
    const long dp = Z * ((long)pi * n + pi), dq = Z * ((long)qi * n + qi), o1 = Z * ((long)pi * n + qi), o2 = Z * ((long)qi * n + pi);
    a[dp] = a[dp] - ri[3]; a[dq] = a[dq] + ri[3];
    a[o1] = 0.0; a[o2] = 0.0;
    if (Z == 2) { a[dp + 1] = 0.0; a[dq + 1] = 0.0; a[o1 + 1] = 0.0; a[o2 + 1] = 0.0; }
    return;
  }
  // i > j: the mirror image of block (j, i); computed as its conjugate transpose, same operations in the same order
  const bool mirror = i > j;
  double blk[4][Z];
  for (int u = 0; u < 2; ++u)
    for (int w = 0; w < 2; ++w) {
      const int slot = mirror ? 2 * w + u : 2 * u + w;
      const bool live = rows[u] < n && cols[w] < n;
      const long e = Z * ((long)rows[u] * n + cols[w]);
      blk[slot][0] = live ? a[e] : 0.0;
      if (Z == 2) blk[slot][1] = live ? (mirror ? -a[e + 1] : a[e + 1]) : 0.0;
    }
  if (mirror) eigh_block<Z>(blk, Jj, Ji); else eigh_block<Z>(blk, Ji, Jj);
  for (int u = 0; u < 2; ++u)
    for (int w = 0; w < 2; ++w) {
      const int slot = mirror ? 2 * w + u : 2 * u + w;
      if (!(rows[u] < n && cols[w] < n)) continue;
      const long e = Z * ((long)rows[u] * n + cols[w]);
      a[e] = blk[slot][0];
      if (Z == 2) a[e + 1] = mirror ? -blk[slot][1] : blk[slot][1];
    }
}

// wraw[i] = Re a_ii
template <int Z>
__global__ __launch_bounds__(256) void eigh_diag_kernel(const double *__restrict__ a, int n, double *__restrict__ wraw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) wraw[i] = a[Z * ((long)i * n + i)];
}
// rank[i] = the position of wraw[i] in ascending order, ties by index; w[rank[i]] = wraw[i]
__global__ __launch_bounds__(256) void eigh_rank_kernel(const double *__restrict__ wraw, int n, int *__restrict__ rank, double *__restrict__ w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double x = wraw[i];
  int k = 0;
  for (int j = 0; j < n; ++j) {
    const double y = wraw[j];
    k += (y < x || (y == x && j < i)) ? 1 : 0;
  }
  rank[i] = k;        // (k < n always: i itself is never counted)
  w[k] = x;
}
// out row rank[k] = v row k      (grid (ceil(n Z / 256), n))
template <int Z>
__global__ __launch_bounds__(256) void eigh_permute_kernel(const double *__restrict__ v, const int *__restrict__ rank, int n, double *__restrict__ out) {
  const int k = blockIdx.y;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)Z * n) return;
  out[(long)rank[k] * n * Z + e] = v[(long)k * n * Z + e];
}

// a: n x n row-major (interleaved pairs when cplx), overwritten with Z^T (row k = the eigenvector of w[k]); v: n x n scratch;
// w: n doubles; work: eigh_work_doubles(n) doubles -- all device buffers.  Returns true when converged, false at the sweep cap
// (a, w then hold the state reached).  *sweeps = sweeps run, the closing one that rotated nothing included.
template <int Z>
bool eigh_jacobi_t(hipStream_t stream, int n, double *a, double *v, double *w, double *work, int *sweeps) {
  const int m = n + (n & 1), h = m / 2;
  double *thr = work, *rot = work + 8, *wraw = rot + 4 * (size_t)h, *part = wraw + 2 * (size_t)n;
  int *count = reinterpret_cast<int *>(work + 2), *rank = reinterpret_cast<int *>(wraw + n);
  const long len = (long)n * n * Z;
  const int nb = (int)std::min<long>((len + 255) / 256, 256);
  hipLaunchKernelGGL(eigh_sumsq_kernel, dim3(nb), dim3(256), 0, stream, (const double *)a, len, part);
  hipLaunchKernelGGL(eigh_thr_kernel, dim3(1), dim3(64), 0, stream, (const double *)part, nb, n, work);
  hipLaunchKernelGGL(eigh_identity_kernel<Z>, dim3((unsigned)(((long)n * n + 255) / 256)), dim3(256), 0, stream, v, n);
  PG_CHECK_HIP(hipGetLastError());
  const dim3 ag((unsigned)((h + n + 63) / 64), (unsigned)((h + 3) / 4)), ab(64, 4);
  bool converged = false;
  int sw = 0;
  while (sw < EIGH_MAX_SWEEPS && !converged) {
    ++sw;
    PG_CHECK_HIP(hipMemsetAsync(count, 0, sizeof(int), stream));
    for (int r = 0; r < m - 1; ++r) {
      hipLaunchKernelGGL(eigh_rot_kernel<Z>, dim3((h + 63) / 64), dim3(64), 0, stream, (const double *)a, n, m, r, rot, (const double *)thr, count);
      hipLaunchKernelGGL(eigh_apply_kernel<Z>, ag, ab, 0, stream, a, v, n, m, r, (const double *)rot);
    }
    PG_CHECK_HIP(hipGetLastError());
    int rotated = 0;
    PG_CHECK_HIP(hipMemcpyAsync(&rotated, count, sizeof(int), hipMemcpyDeviceToHost, stream));
    PG_CHECK_HIP(hipStreamSynchronize(stream));
    converged = rotated == 0;
  }
  hipLaunchKernelGGL(eigh_diag_kernel<Z>, dim3((n + 255) / 256), dim3(256), 0, stream, (const double *)a, n, wraw);
  hipLaunchKernelGGL(eigh_rank_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const double *)wraw, n, rank, w);
  hipLaunchKernelGGL(eigh_permute_kernel<Z>, dim3((unsigned)(((long)Z * n + 255) / 256), n), dim3(256), 0, stream, (const double *)v,
                     (const int *)rank, n, a);
  PG_CHECK_HIP(hipGetLastError());
  if (sweeps) *sweeps = sw;
  return converged;
}

inline bool eigh_jacobi(hipStream_t stream, int n, bool cplx, double *a, double *v, double *w, double *work, int *sweeps) {
  return cplx ? eigh_jacobi_t<2>(stream, n, a, v, w, work, sweeps) : eigh_jacobi_t<1>(stream, n, a, v, w, work, sweeps);
}

}  // namespace pepsgpu

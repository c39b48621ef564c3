// Tensor-GEMM descriptors of the row absorption (engine_impl.h, engine_cplx.h): one builder per contraction, the
// dimensions of one site, and the rank hint of the row absorbed before.  Host code only.
//
// Live extents are per-walker device arrays (nullptr: the static dimension; the complex path passes nullptr throughout).
// `zero_fill`: the result is written in full, zeros beyond the live extents (mask bit of TgDyn), for results that are read
// as whole rows or normalised as a whole.
#pragma once
#include "tgemm.h"

namespace pepsgpu {

// One site of the absorbed row: A[a, p, a2] of the absorbing MPS, the site tensor W[l, p, l2, u] (position (r, c), leg
// dimensions dd and element strides st in storage order), the new bond k2 to its right, the carry rows m.
struct SiteDims {
  int r = 0, c = 0, dd[4] = {1, 1, 1, 1}, st[4] = {0, 0, 0, 0};
  int ll = 0, lp = 0, lr = 0, lu = 0;   // storage positions of the legs l, p, l2, u
  int a = 1, p = 1, a2 = 1, l = 1, l2 = 1, u = 1, k2 = 1, m = 1;
  int la = 1, uk = 1;                   // l * a, u * k2
};

// Largest live carry at site i of the absorption that built `in` (the row absorbed before), or -1 when there is no hint:
// fewer than three rows absorbed (the carry rank can still grow by the factor D per row), no entry, or value unknown.
template <typename BM>
static inline int carry_hint(const BM &in, int i) {
  return (in.depth >= 3 && i >= 0 && (int)in.mlmax.size() > i && in.mlmax[i] >= 0) ? in.mlmax[i] : -1;
}

// X[m,l,p,a2] = sum_a R[m,l,a] A[a,p,a2]                      (bmps_impl.h:806)
static inline TGemmDesc desc_x(const SiteDims &d, long wR, long wA, long wX, int nb, const int *mdyn, int mmul, const int *live_a,
                               const int *live_a2) {
  TGemmDesc g;
  g.I[1] = d.m; g.I[2] = d.l; g.sAi[1] = d.l * d.a; g.sAi[2] = d.a; g.sCi[1] = d.l * d.p * d.a2; g.sCi[2] = d.p * d.a2;
  g.K[2] = d.a; g.sAk[2] = 1; g.sBk[2] = d.p * d.a2;
  g.J[1] = d.p; g.J[2] = d.a2; g.sBj[1] = d.a2; g.sBj[2] = 1; g.sCj[1] = d.a2; g.sCj[2] = 1;
  g.wA = wR; g.wB = wA; g.wC = wX; g.nbatch = nb;
  g.dI[1].p = mdyn; g.dI[1].mul = mmul;   // live carry rows
  g.dK[2].p = live_a;                     // live part of the bond to the left of A
  g.dJ[2].p = live_a2;                    // ... and to its right
  return g;
}

// P[m,u,l2,a2] = sum_{l,p} X[m,l,p,a2] W[l,p,l2,u]           (bmps_impl.h:807 + :815-817)
// site tensor as the A operand (its batch stride and selector are set by launch_site_gemm_a): the lanes of a tile run
// along (m, a2), contiguous in X and in P
static inline TGemmDesc desc_p(const SiteDims &d, long wX, long wP, int nb, const int *mdyn, int mmul, const int *live_a2) {
  TGemmDesc g;
  g.I[1] = d.l2; g.I[2] = d.u; g.sAi[1] = d.st[d.lr]; g.sAi[2] = d.st[d.lu]; g.sCi[1] = d.a2; g.sCi[2] = d.l2 * d.a2;
  g.K[1] = d.l; g.K[2] = d.p; g.sAk[1] = d.st[d.ll]; g.sAk[2] = d.st[d.lp]; g.sBk[1] = d.p * d.a2; g.sBk[2] = d.a2;
  g.J[1] = d.m; g.J[2] = d.a2; g.sBj[1] = d.l * d.p * d.a2; g.sBj[2] = 1; g.sCj[1] = d.u * d.l2 * d.a2; g.sCj[2] = 1;
  g.wB = wX; g.wC = wP; g.nbatch = nb;
  g.dJ[1].p = mdyn; g.dJ[1].mul = mmul;
  g.dJ[2].p = live_a2;
  return g;
}

// Z1[a,p,l2,k2] = sum_{a2} A[a,p,a2] Y[l2,a2,k2]
static inline TGemmDesc desc_z1(const SiteDims &d, long wA, long wY, long wZ1, int nb, const int *live_a, const int *live_a2,
                                const int *live_k2) {
  TGemmDesc g;
  g.I[1] = d.a; g.I[2] = d.p; g.sAi[1] = d.p * d.a2; g.sAi[2] = d.a2; g.sCi[1] = d.p * d.l2 * d.k2; g.sCi[2] = d.l2 * d.k2;
  g.K[2] = d.a2; g.sAk[2] = 1; g.sBk[2] = d.k2;
  g.J[1] = d.l2; g.J[2] = d.k2; g.sBj[1] = d.a2 * d.k2; g.sBj[2] = 1; g.sCj[1] = d.k2; g.sCj[2] = 1;
  g.wA = wA; g.wB = wY; g.wC = wZ1; g.nbatch = nb;
  g.dI[1].p = live_a;                    // live bonds: a (rows of A), a2 (contracted), k2 (new bond to the right)
  g.dK[2].p = live_a2;
  g.dJ[2].p = live_k2;
  return g;
}

// Tt[l,a,u,k2] = sum_{p,l2} Z1[a,p,l2,k2] W[l,p,l2,u]
// site tensor as the A operand: the lanes of a tile run along (a, k2), contiguous in Z1 and in Tt.
// tsw: Tt[l, a, k2, u], the fully live leg u innermost (see Engine::backward_pair)
static inline TGemmDesc desc_tt(const SiteDims &d, bool tsw, long wZ1, long wTt, int nb, const int *live_a, const int *live_k2,
                                bool zero_fill) {
  TGemmDesc g;
  g.I[1] = d.l; g.I[2] = d.u; g.sAi[1] = d.st[d.ll]; g.sAi[2] = d.st[d.lu]; g.sCi[1] = d.a * d.u * d.k2; g.sCi[2] = d.k2;
  g.K[1] = d.p; g.K[2] = d.l2; g.sAk[1] = d.st[d.lp]; g.sAk[2] = d.st[d.lr]; g.sBk[1] = d.l2 * d.k2; g.sBk[2] = d.k2;
  g.J[1] = d.a; g.J[2] = d.k2; g.sBj[1] = d.p * d.l2 * d.k2; g.sBj[2] = 1; g.sCj[1] = d.u * d.k2; g.sCj[2] = 1;
  if (tsw) { g.sCi[2] = 1; g.sCj[2] = d.u; }
  g.wB = wZ1; g.wC = wTt; g.nbatch = nb;
  g.dJ[1].p = live_a;
  g.dJ[2].p = live_k2; g.dJ[2].mask = zero_fill;
  return g;
}

// M[m,(u,k2)] = sum_{(l,a)} R_i[m,(l,a)] Tt[(l,a),(u,k2)]
// k2_outer (with tsw, wave-per-tile route): the columns are enumerated as (k2, u), the memory order of Tt[l,a,k2,u] -- the 32
// lanes of a column tile read 32 consecutive floats of Tt, and the tiles of k2 beyond the live bond are dead as a whole.  M keeps
// its layout [m,(u,k2)].
static inline TGemmDesc desc_m(const SiteDims &d, bool tsw, long wR, long wTt, long wM, int nb, const int *mdyn, int mmul,
                               const int *live_a, const int *live_k2, bool zero_fill, bool k2_outer = false) {
  TGemmDesc g;
  g.I[2] = d.m; g.sAi[2] = d.la; g.sCi[2] = d.uk;
  g.K[1] = d.l; g.K[2] = d.a; g.sAk[1] = d.a; g.sAk[2] = 1; g.sBk[1] = d.a * d.uk; g.sBk[2] = d.uk;
  g.J[1] = d.u; g.J[2] = d.k2; g.sBj[1] = d.k2; g.sBj[2] = 1; g.sCj[1] = d.k2; g.sCj[2] = 1;
  if (tsw) { g.sBj[1] = 1; g.sBj[2] = d.u; }
  g.wA = wR; g.wB = wTt; g.wC = wM; g.nbatch = nb;
  g.dynI = mdyn; g.dynI_mul = mmul;
  g.dK[2].p = live_a;
  g.dJ[2].p = live_k2; g.dJ[2].mask = zero_fill;   // the Jacobi reads whole rows of M: dead columns are written as zeros
  if (tsw && k2_outer) {
    g.J[1] = d.k2; g.J[2] = d.u; g.sBj[1] = d.u; g.sBj[2] = 1; g.sCj[1] = 1; g.sCj[2] = d.k2;
    g.dJ[1] = g.dJ[2]; g.dJ[2] = TgDyn();
  }
  return g;
}

// Ynew[(l,a),q] = sum_{(u,k2)} Tt[(l,a),(u,k2)] V[q,(u,k2)]   (k rows of V; conj: V enters conjugated)
static inline TGemmDesc desc_y(const SiteDims &d, int k, bool tsw, long wTt, long wV, long wY, int nb, const int *live_a,
                               const int *live_k2, const int *live_k, bool zero_fill, bool conj) {
  TGemmDesc g;
  g.I[1] = d.l; g.I[2] = d.a; g.sAi[1] = d.a * d.uk; g.sAi[2] = d.uk; g.sCi[1] = d.a * k; g.sCi[2] = k;
  g.K[1] = d.u; g.K[2] = d.k2; g.sAk[1] = d.k2; g.sAk[2] = 1; g.sBk[1] = d.k2; g.sBk[2] = 1;
  g.J[2] = k; g.sBj[2] = d.uk; g.sCj[2] = 1;
  g.wA = wTt; g.wB = wV; g.wC = wY; g.nbatch = nb;
  g.dI[2].p = live_a; g.dI[2].mask = zero_fill;    // Yn is normalised as a whole: written in full, zeros beyond the live bonds
  g.dK[2].p = live_k2;
  if (tsw) {   // K = (k2, u): u contiguous in Tt (vector loads), k2 contiguous in V
    g.K[1] = d.k2; g.K[2] = d.u; g.sAk[1] = d.u; g.sAk[2] = 1; g.sBk[1] = 1; g.sBk[2] = d.k2;
    g.dK[2].p = nullptr; g.dK[1].p = live_k2;
  }
  g.dJ[2].p = live_k; g.dJ[2].mask = zero_fill;
  g.conjB = conj;
  return g;
}

// G = P^T P (conj: P^H P) of the rows x cols block P, upper triangle unless `full`; the first dynK[b] * dynK_mul rows are live
static inline TGemmDesc desc_cols_gram(int rows, int cols, long wP, int nb, const int *dynK, int dynK_mul, bool full, const int *flag,
                                       bool conj) {
  TGemmDesc g;
  g.I[2] = cols; g.sAi[2] = 1; g.sCi[2] = cols;
  g.K[2] = rows; g.sAk[2] = cols; g.sBk[2] = cols;
  g.J[2] = cols; g.sBj[2] = 1; g.sCj[2] = 1;
  g.wA = wP; g.wB = wP; g.wC = (long)cols * cols; g.nbatch = nb;
  g.dynK = dynK; g.dynK_mul = dynK_mul;
  g.upper_only = full ? 0 : 1;            // (the real Cholesky reads the upper triangle only)
  g.conjA = conj;
  g.batch_flag = flag;
  return g;
}

// S = X X^T (conj: X X^H) over the live rows of X: `rows` rows of `len` elements, row_live / len_live of them alive;
// S has the leading dimension ld (batch stride ld * ld); upper triangle unless `full`; flag: batch_flag
static inline TGemmDesc desc_rows_gram(int rows, int len, int ld, long wX, int nb, const int *row_live, const int *len_live, bool full,
                                       const int *flag, bool conj) {
  TGemmDesc g;
  g.I[2] = rows; g.sAi[2] = len; g.sCi[2] = ld;
  g.K[2] = len; g.sAk[2] = 1; g.sBk[2] = 1;
  g.J[2] = rows; g.sBj[2] = len; g.sCj[2] = 1;
  g.wA = wX; g.wB = wX; g.wC = (long)ld * ld; g.nbatch = nb;
  g.dI[2].p = row_live; g.dJ[2].p = row_live;
  g.dK[2].p = len_live;
  g.upper_only = full ? 0 : 1;
  g.conjB = conj;
  g.batch_flag = flag;
  return g;
}

// C = Q B: nq rows of Q (leading dimension ldq, q_live of them alive) times the kdim x cols block B (k_live rows alive)
static inline TGemmDesc desc_rows_times(int nq, int ldq, int kdim, int cols, long wQ, long wB, long wC, int nb, const int *q_live,
                                        const int *k_live, const int *flag) {
  TGemmDesc g;
  g.I[2] = nq; g.sAi[2] = ldq; g.sCi[2] = cols;
  g.K[2] = kdim; g.sAk[2] = 1; g.sBk[2] = cols;
  g.J[2] = cols; g.sBj[2] = 1; g.sCj[2] = 1;
  g.wA = wQ; g.wB = wB; g.wC = wC; g.nbatch = nb;
  g.dI[2].p = q_live;
  g.dK[2].p = k_live;
  g.batch_flag = flag;
  return g;
}

// C = Q B^T (conj: Q B^H): nq rows of Q, `len` long, times the brows rows of B; C has the leading dimension ldc and is
// written as zeros beyond the b_live rows of B when zero_fill
static inline TGemmDesc desc_rows_times_t(int nq, int len, int brows, int ldc, long wQ, long wB, long wC, int nb, const int *q_live,
                                          const int *b_live, bool zero_fill, const int *flag, bool conj) {
  TGemmDesc g;
  g.I[2] = nq; g.sAi[2] = len; g.sCi[2] = ldc;
  g.K[2] = len; g.sAk[2] = 1; g.sBk[2] = 1;
  g.J[2] = brows; g.sBj[2] = len; g.sCj[2] = 1;
  g.wA = wQ; g.wB = wB; g.wC = wC; g.nbatch = nb;
  g.dI[2].p = q_live;
  g.dJ[2].p = b_live; g.dJ[2].mask = zero_fill;
  g.conjB = conj;
  g.batch_flag = flag;
  return g;
}

}  // namespace pepsgpu

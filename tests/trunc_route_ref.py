"""NumPy restatement of the dense-site truncation routes of the float64 and complex engines (engine_impl.h trunc_f64_pivot,
engine_cplx.h trunc_c128_rangefinder), of the pieces they launch (rows_qr.h, chol_pivot.h, the guard of linalg.h), the metrics the
site-level tests judge a delivered row space by, and the constructed matrices they run on.  Float64 / complex128 throughout, no
device: tests/test_cpu_trunc_route_ref.py pins what this file computes, tests/test_gpu_trunc_routes.py compares the kernels with it.

Conventions: M is m x len (len = u * k2), its rows are what the truncation rotates; V is k x len with orthonormal rows; k = chi,
kq = min(2 k, 3 min(m, len) / 4) the oversampled subspace dimension of the routes."""
import numpy as np
import scipy.linalg

EPS = 2.0 ** -52
SPECTRA = ("graded", "flat_tail", "steps", "rank_kq_minus", "rank_below_k", "cliff_out", "slow")
GUARD_TOL = 3e-2          # f64_pivot_guard_kernel's tolerance in trunc_f64_pivot
C128_GUARD_TOL = 1e-11    # c128_rangefinder_guard_kernel's tolerance in trunc_c128_rangefinder
# Seeds of the walkers of a launch (make_case).  The tests assert a route membership only where the restated guard value is a factor
# of ten from its tolerance; flat_tail at (256, 256, 32) sits at 2.3e-3 .. 3.5e-3 against 3e-2 depending on the draw, so the walkers
# are the first four seeds whose draw is on the decisive side (seeds 0 and 4 give 3.2e-3 .. 3.5e-3, nine times under, and are left out).
WALKER_SEEDS = (1, 2, 3, 5)


def kq_of(m, ln, k):
    return min(2 * k, (3 * min(m, ln)) // 4)


# ---- ported kernel pieces ----------------------------------------------------------------------------------------------------
def sign_table(rows, cols):
    """sign_table_kernel, element for element: +1 / -1 from a 32-bit integer hash of the flat index"""
    mask = np.uint64(0xFFFFFFFF)
    h = (np.arange(rows * cols, dtype=np.uint64) * np.uint64(2654435761)) & mask
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & mask
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(3266489917)) & mask
    h ^= h >> np.uint64(16)
    return np.where((h & np.uint64(1)) == 1, 1.0, -1.0).reshape(rows, cols)


def pivot_select(M, kq, block=4):
    """Diagonally pivoted Cholesky of G = M M^H, stopped after kq slots or when no positive diagonal is left.  block = 4 is
    chol_pivot_kernel's order: the `block` largest remaining diagonals are chosen together and taken in that order, each corrected
    for the ones before it (one whose pivot is gone by its turn burns its slot); block = 1 is the plain greedy order.
    Returns (pivot rows in the order taken, largest remaining diagonal of the Schur complement / max diag(G))."""
    G = M @ M.conj().T
    d = np.real(np.diag(G)).copy()
    maxd = float(d.max())
    m = G.shape[0]
    L = np.zeros((m, kq), dtype=G.dtype)
    piv = []
    taken = np.zeros(m, dtype=bool)
    j = 0
    while j < kq:
        dm = np.where(taken, -1.0, d)
        cand = [int(p) for p in np.argsort(-dm, kind="stable")[:block] if dm[p] > 0.0]
        if not cand:
            break
        for p in cand:
            if j >= kq:
                break
            taken[p] = True
            if d[p] > 0.0:
                col = (G[:, p] - L[:, :j] @ L[p, :j].conj()) / np.sqrt(d[p])
                L[:, j] = col
                d = d - np.abs(col) ** 2
                piv.append(p)
            j += 1
    rest = np.where(taken, 0.0, d)
    resid = max(float(rest.max()), 0.0) / maxd if maxd > 0 else 0.0
    return piv, resid


def chol_drop(G, scale=1.0):
    """chol_upper_kernel's factor R^H R = G in the natural order: a row whose pivot is below n 2^-52 max diag(G) x scale is dropped"""
    n = G.shape[0]
    thresh = n * EPS * float(np.max(np.real(np.diag(G)))) * scale
    rows = []
    for j in range(n):
        v = G[j].copy()
        for r in rows:
            v -= np.conj(r[j]) * r
        p = float(np.real(v[j]))
        if p > 0.0 and p >= thresh:
            r = v / np.sqrt(p)
            r[:j] = 0
            rows.append(r)
    return np.array(rows, dtype=G.dtype).reshape(len(rows), n)


def orthrows(X):
    """rows of X made orthonormal: Householder QR of X^H, transposed back"""
    q, _ = np.linalg.qr(X.conj().T)
    return q.conj().T


def cholqr_pass(S, X):
    """one Cholesky-QR pass as chol_solve_rows_kernel states it: L L^H = S, X <- L^-1 X"""
    L = np.linalg.cholesky(S)
    return scipy.linalg.solve_triangular(L, X, lower=True)


# ---- the two routes ----------------------------------------------------------------------------------------------------------
def _top_rows(Z, k):
    return np.linalg.svd(Z, full_matrices=False)[2][:k]


def route_f64(M, k, kq, steps=1, block=4):
    """trunc_f64_pivot: kq pivot rows of M, orthonormalised, B = orth(Q M^H), Z = B M, `steps` steps of subspace iteration, the top-k
    right singular vectors of Z"""
    piv, _ = pivot_select(M, kq, block)
    Q = orthrows(M[piv])
    B = orthrows(Q @ M.conj().T)
    Z = B @ M
    for _ in range(steps):
        Q = orthrows(Z)
        B = orthrows(Q @ M.conj().T)
        Z = B @ M
    return _top_rows(Z, k)


def route_c128(M, k, kq, iters=3):
    """trunc_c128_rangefinder: Z = signs M, `iters` re-orthonormalised steps of subspace iteration, the top-k right singular vectors"""
    Z = sign_table(kq, M.shape[0]) @ M
    for _ in range(iters):
        Q = orthrows(Z)
        U = orthrows(Q @ M.conj().T)
        Z = U @ M
    return _top_rows(Z, k)


def route_two_chol(M, k, kq):
    """trunc_f64_two_chol / trunc_c128_two_chol (the round-5 form) up to its guard: B^H B = M M^H (a factor that keeps more than 128
    rows is redone with the pivot threshold x 64, x 64^2), B2^H B2 = B B^H, the kq leading right singular vectors w of B2, u = w^H B
    normalised, the top-k right singular vectors of Z = U M.  None: the walker leaves the route at a row-count check."""
    G = M @ M.conj().T
    for scale in (1.0, 64.0, 64.0 ** 2):
        B1 = chol_drop(G, scale)
        if len(B1) <= 128:
            break
    lo = min(kq, k + 4)
    if len(B1) > 128 or len(B1) < lo:
        return None
    B2 = chol_drop(B1 @ B1.conj().T)
    if len(B2) < lo:
        return None
    T1 = np.linalg.svd(B2, full_matrices=False)[2][:kq] @ B1
    return _top_rows((T1 / np.linalg.norm(T1, axis=1, keepdims=True)) @ M, k)


def route_c128_spectrum(M, kq, iters=3):
    """singular values of the range finder's Z (the norms of its rotated rows on the device), descending"""
    Z = sign_table(kq, M.shape[0]) @ M
    for _ in range(iters):
        Q = orthrows(Z)
        U = orthrows(Q @ M.conj().T)
        Z = U @ M
    return np.linalg.svd(Z, compute_uv=False)


def rangefinder_guard_value(M, k, kq, iters=3):
    """what c128_rangefinder_guard_kernel compares with its tolerance, from the singular values z of the range finder's Z:
    (z_k / z_1) (z_kq / z_k)^(2 iters + 1), the leakage bound of `iters` steps weighted as `loss` weights direction k
    (0 when z_kq = 0: the subspace holds all of M)"""
    z = route_c128_spectrum(M, kq, iters)
    if len(z) < kq or not z[kq - 1] > 0.0:
        return 0.0
    return float((z[k - 1] / z[0]) * (z[kq - 1] / z[k - 1]) ** (2 * iters + 1))


def pivot_guard_value(M, k, kq, block=4):
    """what f64_pivot_guard_kernel compares with its tolerance: residual pivot x (sigma_1 / sigma_k)^2 (0 for a factor that took
    every direction; inf when fewer than k directions are there)"""
    _, resid = pivot_select(M, kq, block)
    if resid == 0.0:
        return 0.0
    s = np.linalg.svd(M, compute_uv=False)
    if len(s) < k or not s[k - 1] > 0.0:
        return np.inf
    return resid * (s[0] / s[k - 1]) ** 2


# ---- metrics -----------------------------------------------------------------------------------------------------------------
def loss(M, V, k, svd=None):
    """|| diag(sigma_1 .. sigma_k) V_k^H (I - V^H V) ||_F / sigma_1: the part of the kept sigma_j v_j the delivered rows V miss"""
    _, s, vh = svd if svd is not None else np.linalg.svd(M, full_matrices=False)
    A = s[:k, None] * vh[:k]
    return float(np.linalg.norm(A - (A @ V.conj().T) @ V) / s[0])


def captured(M, V, k, svd=None):
    """|| M V^H ||_F^2 / sum_{j < k} sigma_j^2 - 1: the weight the delivered rows capture against the optimal truncation"""
    s = svd[1] if svd is not None else np.linalg.svd(M, compute_uv=False)
    return float(np.linalg.norm(M @ V.conj().T) ** 2 / np.sum(s[:k] ** 2) - 1.0)


def numerical_rank(s):
    return int(np.sum(s > len(s) * EPS * s[0]))


# ---- constructed matrices ----------------------------------------------------------------------------------------------------
def spectrum(name, m, ln, k):
    r = min(m, ln)
    kq = kq_of(m, ln, k)
    j = np.arange(r, dtype=np.float64)
    if name == "graded":         # five decades over the kept directions, one more to kq, two more to r (the real state's shape)
        return np.where(j < k, 10.0 ** (-5.0 * j / k),
                        np.where(j < kq, 10.0 ** (-5.0 - (j - k) / max(kq - k, 1)), 10.0 ** (-6.0 - 2.0 * (j - kq) / max(r - kq, 1))))
    if name == "flat_tail":
        return np.where(j < k, 10.0 ** (-2.0 * j / k), 1e-4)
    if name == "steps":
        return np.where(j < k, 1.0 / (1.0 + j / k), np.where(j < kq, 1e-3, 1e-6))
    if name == "rank_kq_minus":
        return np.where(j < kq - 3, 10.0 ** (-3.0 * j / kq), 0.0)
    if name == "rank_below_k":
        return np.where(j < k - 2, 10.0 ** (-2.0 * j / k), 0.0)
    if name == "cliff_out":
        return np.where(j < k, 10.0 ** (-4.0 * j / k), 10.0 ** -4.2)
    if name == "slow":
        return 10.0 ** (-2.0 * j / r)
    raise ValueError(name)


def _haar(rng, n, r, cplx):
    a = rng.standard_normal((n, r))
    if cplx:
        a = a + 1j * rng.standard_normal((n, r))
    q, t = np.linalg.qr(a)
    d = np.diag(t)
    return q * (d / np.abs(d))


def make_case(name, m, ln, k, seed, cplx=False):
    """M = U diag(sigma) V^H, U (m x r) and V (len x r) Haar distributed from a seeded generator"""
    rng = np.random.default_rng([seed, SPECTRA.index(name), m, ln, k, int(cplx)])
    r = min(m, ln)
    s = spectrum(name, m, ln, k)
    U, V = _haar(rng, m, r, cplx), _haar(rng, ln, r, cplx)
    return (U * s) @ V.conj().T

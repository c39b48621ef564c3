"""Site-level reference tests of the dense truncation routes of the float64 and complex engines and of the kernels only they launch,
each against NumPy or the restatement of tests/trunc_route_ref.py (pinned by tests/test_cpu_trunc_route_ref.py); no subprocesses.

(a) Context.diag_truncate_site -- truncate_site itself (float64), truncate_site_simple (complex) -- on constructed matrices
    M = U diag(sigma) V^H of seven spectra, four walkers with different seeds per launch, at (m, u, k2, chi) = (64, 8, 8, 8) the
    smallest block a route takes, (256, 8, 32, 32) the production shape, (200, 4, 32, 32) a non-square block; float64 also with live
    rows [256, 200, 129, 64] in one launch and at (63, 8, 8, 8), which no route takes.  Per walker, on its live rows: orthonormality
    (|V V^H - I|_max <= 8 len 2^-52: the inner products of len-long rows the Jacobi rotates to 2 sqrt(len) eps), the loss of
    trunc_route_ref.loss against 8 x max(reference, len 2^-52), the captured weight against -8 x max(|reference|, len 2^-52), dead
    rows exactly zero, live rows >= the numerical rank.  Reference of a walker a route delivered (flag < 0): the restatement of that
    route on the same matrix; of a walker the general kernels took: NumPy's top-k right singular vectors.
(b) the complex range finder on `slow` and `cliff_out` against NumPy's top-k: it must deliver that or eject the walker.
(c) chol_solve_rows_kernel / chol_solve_rows_cplx_kernel: one pass and a second one (Gram matrices from the host in longdouble).
(d) sign_table_kernel and gather_rows_kernel, exactly.    (e) jacobi_rows_cplx_kernel with the float64 tolerances of test_jacobi_rows.

Reference of a round-5 walker: trunc_route_ref.route_two_chol.  The complex path keeps static shapes and reports no live count: a
direction that is not there comes back as a zero row behind the live ones, which is what its `dead rows` are.

Measured on the MI355X (largest device / bound ratio over every walker; the bound is 8 x the reference, so 0.125 means the device
reproduces the restatement's figure):
  route                          loss    captured   orthonormality
  f64 pivoted (round 6)          0.125   0.009      0.016      (device loss / restatement loss = 1.000 on every walker it kept)
  f64 two-Cholesky (round 5)     0.125   0.004      0.011      (1.000 x the restatement on graded at 256 x 256: 5.6e-10 .. 9.4e-10)
  c128 range finder (round 6)    0.268   0.010      0.016      (1.000 x the restatement on graded: 1.0e-13 .. 2.5e-13)
  c128 two-Cholesky (round 5)    0.268   0.006      0.011      (the maximum is a walker it handed to the general kernels)
  general kernels (route 3)      0.024   0.002      0.008
  Cholesky-QR pass, f64 / c128   0.44 / 0.64 (orthonormality), 0.003 / 0.005 (upper part of X_in X_out^H)
  complex Jacobi: 0 sweeps at one row, 3 at 2 x 2, 8 at 9 x 33, 15 .. 18 at 37 .. 64 rows, 23 at 256 x 256
On-route share per spectrum, walkers on the route / walkers, the three shapes of (a):
  f64 round 6:  graded 4/12 (on at chi = 8, off at the two chi = 32 shapes, where its guard value 4e-2 .. 8e-2 is borderline),
                flat_tail, steps, rank_kq_minus, rank_below_k 12/12, cliff_out 0/12, slow 0/12
  c128 round 6: graded, flat_tail, steps, rank_kq_minus, rank_below_k 12/12, cliff_out 0/12, slow 0/12
                (before the guard: 12/12 on every spectrum -- graded is untouched by it)
  round 5 (both types): graded, steps, rank_kq_minus 4/4 at (256, 8, 32), the other four spectra 0/4; 0/4 on every spectrum at
                (200, 4, 32), which has more rows than columns

What the device showed (the figures from before a fix were taken with walker seeds 0 .. 3).
(b) Before the guard the range finder kept every walker and delivered `slow` with a loss of 3.07e-2 at (256, 8, 32) (1.4e-2 at chi = 8,
    2.0e-4 at (200, 4, 32)), capturing 2.5e-5 less than the optimal truncation, and `cliff_out` with 1.80e-6 (1.0e-8, 1.1e-6): the
    restatement's figures to three digits.  With rangefinder_guard_kernel (tolerance 1e-11, trunc_route_ref.C128_GUARD_TOL) all 24 of
    those walkers take the general kernel and sit at 0.27 of the bound or below.
(a) f64, chi = 8: the guard priced the residual pivot behind 48 rows (the smallest instantiation of chol_pivot_kernel) for a route
    that goes on with 16, and kept 3 of 4 `slow` walkers with a loss of 2e-2; fixed, test_site_f64_guard_prices_the_rows_the_route_uses.
    The kernel takes its pivots four at a time, not greedily: on one graded walker at chi = 8 that costs a factor 23 in loss
    (2.5e-12 against 1.1e-13), which is why the restatement carries the kernel's order (pivot_select, block = 4).
Round 5 on (200, 4, 32), fixed: the block has rank 128 < m = 200 by shape, so the unpivoted factor of M M^H meets dependent rows while
    directions of weight are still open and decides at the rounding level which rows it keeps.  On `cliff_out` one walker in four
    lost 6.25e-8 (f64) / 1.69e-11 (c128) against 2.9e-11 / 1.5e-12 restated, on `slow` one sat at 1.33 of the bound; perturbing the
    restated Gram matrices by 2 x 2^-52 sqrt(G_ii G_jj) -- another summation order -- moves that walker's restated loss between
    2e-12 and 6e-8.  No guard of the form prices this: it no longer takes blocks with more rows than columns (asserted)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trunc_route_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
MARGIN = 8.0
SITE_SHAPES = ((64, 8, 8, 8), (256, 8, 32, 32), (200, 4, 32, 32))      # (m, u, k2, chi)
ROWS_CASE = (256, 200, 129, 64)
NB = 4
STATS = {}         # (dtype, route) -> largest device / bound ratios; (dtype, route, spectrum) -> [on route, walkers]


def _capi():
    from peps_amd import capi
    return capi


_CTX = {}


@pytest.fixture(scope="module")
def contexts():
    """one small context per element type and chi"""
    capi = _capi()

    def get(cplx, chi):
        key = (cplx, chi)
        if key not in _CTX:
            _CTX[key] = capi.Context(2, 2, 2, 2, chi, capi.C128 if cplx else capi.F64, max_walkers=NB)
        return _CTX[key]

    yield get
    for c in _CTX.values():
        c.close()
    _CTX.clear()
    for key in sorted(STATS, key=str):
        print("trunc-route stats %s: %s" % (key, STATS[key]))


@functools.lru_cache(maxsize=None)
def reference(name, rows, ln, k, seed, cplx):
    """(M [rows x ln], its SVD, the loss and the captured weight of NumPy's own top-k right singular vectors), computed once"""
    M = R.make_case(name, rows, ln, k, seed, cplx)
    svd = np.linalg.svd(M, full_matrices=False)
    Vn = svd[2][:k]
    for a in (M,) + tuple(svd):
        a.setflags(write=False)
    return M, svd, R.loss(M, Vn, k, svd), R.captured(M, Vn, k, svd)


@functools.lru_cache(maxsize=None)
def restatement(name, rows, ln, k, kq, seed, cplx, two_chol):
    """(loss, captured weight) of the restatement of the route on the same matrix; None where the restated route hands the walker on"""
    M, svd = reference(name, rows, ln, k, seed, cplx)[:2]
    V = R.route_two_chol(M, k, kq) if two_chol else (R.route_c128(M, k, kq) if cplx else R.route_f64(M, k, kq))
    return None if V is None else (R.loss(M, V, k, svd), R.captured(M, V, k, svd))


def _stat_max(key, **vals):
    d = STATS.setdefault(key, {})
    for n, v in vals.items():
        d[n] = max(d.get(n, 0.0), float(v))


def check_site(ctx, name, m, u, k2, chi, cplx, route, rows=None, numpy_reference=False, expect_on=None):
    """runs one launch of NB walkers through the site truncation and applies the assertions of (a) to every walker"""
    ln = u * k2
    k = min(chi, m, ln)
    kq = R.kq_of(m, ln, k)                      # (the device sizes the subspace by the static shape)
    live = list(rows) if rows is not None else [m] * NB
    refs = [reference(name, live[b], ln, k, R.WALKER_SEEDS[b], cplx) for b in range(NB)]
    M = np.zeros((NB, m, ln), dtype=np.complex128 if cplx else np.float64)
    for b in range(NB):
        M[b, :live[b]] = refs[b][0]
    V, klive, flag = ctx.diag_truncate_site(M, u, k2, rows=None if rows is None else np.array(rows, dtype=np.int32), route=route)
    assert V.shape == (NB, k, ln) and np.all(np.isfinite(V))
    tag = ("c128" if cplx else "f64", route)
    on = STATS.setdefault(tag + (name,), [0, 0])
    floor = ln * EPS
    failures = []
    for b in range(NB):
        Mb, svd, nl, nc = refs[b]
        s = svd[1]
        rank = R.numerical_rank(s)
        on_route = flag[b] < 0
        on[0] += int(on_route)
        on[1] += 1
        if cplx:
            # static shapes, no live count: a direction that is not there comes back as a zero row behind the live ones (select_rows_kernel)
            assert klive[b] == -1
            kl = int(np.sum(np.any(V[b] != 0, axis=1)))
            if not kl >= min(k, rank):
                failures.append("walker %d: %d non-zero rows, numerical rank %d" % (b, kl, rank))
        else:
            kl = int(klive[b])
            assert 0 <= kl <= k
        Vb = V[b, :kl]
        ref_l, ref_c = nl, nc
        if on_route and not numpy_reference:
            rs = restatement(name, live[b], ln, k, min(kq, live[b]), R.WALKER_SEEDS[b], cplx, route == 2)
            if rs is not None:           # (a walker the restated route hands on is held to NumPy's vectors)
                ref_l, ref_c = rs
        ortho = float(np.max(np.abs(Vb @ Vb.conj().T - np.eye(kl)))) if kl else 0.0
        ls = R.loss(Mb, Vb, k, svd)
        cp = R.captured(Mb, Vb, k, svd)
        b_l, b_c = MARGIN * max(ref_l, floor), MARGIN * max(abs(ref_c), floor)
        print("%s route %d %s (%d, %d, %d) chi %d walker %d rows %d: flag %d klive %d rank %d ortho %.2e loss %.2e / bound %.2e = %.3f "
              "captured %.2e / bound %.2e = %.3f" % (tag[0], route, name, m, u, k2, chi, b, live[b], flag[b], klive[b], rank, ortho, ls,
                                                     b_l, ls / b_l, cp, -b_c, max(-cp, 0.0) / b_c))
        _stat_max(tag, ortho_over_bound=ortho / (MARGIN * floor), loss_over_bound=ls / b_l, captured_over_bound=max(-cp, 0.0) / b_c)
        if not ortho <= MARGIN * floor:
            failures.append("walker %d: orthonormality %.2e above %.2e" % (b, ortho, MARGIN * floor))
        if not ls <= b_l:
            failures.append("walker %d (flag %d): loss %.2e above %.2e" % (b, flag[b], ls, b_l))
        if not cp >= -b_c:
            failures.append("walker %d (flag %d): captured %.2e below %.2e" % (b, flag[b], cp, -b_c))
        if not np.all(V[b, kl:] == 0):
            failures.append("walker %d: rows beyond klive = %d are not zero" % (b, kl))
        if name in ("rank_kq_minus", "rank_below_k") and not kl >= min(k, rank):
            failures.append("walker %d: klive %d below the numerical rank %d" % (b, kl, rank))
        if expect_on is not None and on_route != expect_on:
            failures.append("walker %d: flag %d, expected %s the route" % (b, flag[b], "on" if expect_on else "off"))
    assert not failures, "; ".join(failures)
    return V, klive, flag


# membership the restatement's guard values decide by a factor of ten or more (tests/test_cpu_trunc_route_ref.py)
F64_ON = ("flat_tail", "steps", "rank_kq_minus")
F64_OFF = ("cliff_out",)
C128_ON = ("graded", "flat_tail", "steps", "rank_kq_minus", "rank_below_k")
C128_OFF = ("cliff_out", "slow")


def _expect(cplx, name):
    on, off = (C128_ON, C128_OFF) if cplx else (F64_ON, F64_OFF)
    return True if name in on else (False if name in off else None)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.SPECTRA)
@pytest.mark.parametrize("shape", SITE_SHAPES)
@pytest.mark.parametrize("cplx", (False, True), ids=("f64", "c128"))
def test_site_round6_route(contexts, cplx, shape, name):
    m, u, k2, chi = shape
    check_site(contexts(cplx, chi), name, m, u, k2, chi, cplx, 1, expect_on=_expect(cplx, name))


@pytest.mark.parametrize("name", R.SPECTRA)
@pytest.mark.parametrize("shape", SITE_SHAPES[1:])
@pytest.mark.parametrize("cplx", (False, True), ids=("f64", "c128"))
def test_site_round5_two_cholesky_route(contexts, cplx, shape, name):
    """(200, 4, 32): more rows than columns -- the form must hand every walker to the general kernels (module docstring)."""
    m, u, k2, chi = shape
    _, _, flag = check_site(contexts(cplx, chi), name, m, u, k2, chi, cplx, 2)
    if m > u * k2:
        assert np.all(flag >= 0)


@pytest.mark.parametrize("name", R.SPECTRA)
def test_site_f64_mixed_live_rows(contexts, name):
    check_site(contexts(False, 32), name, 256, 8, 32, 32, False, 1, rows=ROWS_CASE)


@pytest.mark.parametrize("name", R.SPECTRA)
def test_site_f64_63_rows_take_no_route(contexts, name):
    _, _, flag = check_site(contexts(False, 8), name, 63, 8, 8, 8, False, 1)
    assert np.all(flag >= 0)


@pytest.mark.parametrize("cplx", (False, True), ids=("f64", "c128"))
def test_site_general_kernels_only(contexts, cplx):
    _, _, flag = check_site(contexts(cplx, 32), "graded", 256, 8, 32, 32, cplx, 3)
    assert np.all(flag >= 0)


@pytest.mark.parametrize("cplx", (False, True), ids=("f64", "c128"))
def test_site_default_dispatch_is_the_round6_form(contexts, cplx):
    ctx = contexts(cplx, 32)
    V0, k0, f0 = check_site(ctx, "flat_tail", 256, 8, 32, 32, cplx, 0)
    V1, k1, f1 = check_site(ctx, "flat_tail", 256, 8, 32, 32, cplx, 1)
    assert np.array_equal(V0, V1) and np.array_equal(f0, f1) and np.array_equal(k0, k1)
    assert np.all(f1 < 0)


def test_site_f64_route_membership_is_not_vacuous(contexts):
    """at least the flat_tail, steps and rank_kq_minus walkers -- 3 of 7 spectra -- stay on the pivoted route at every shape"""
    for m, u, k2, chi in SITE_SHAPES:
        on = 0
        for name in R.SPECTRA:
            _, _, flag = check_site(contexts(False, chi), name, m, u, k2, chi, False, 1, expect_on=_expect(False, name))
            on += int(np.sum(flag < 0))
        assert on >= 3 * NB


def test_site_f64_guard_prices_the_rows_the_route_uses(contexts):
    """chi = 8: the route asks for kq = 16 pivot rows, the smallest instantiation of chol_pivot_kernel holds 48.  The factorisation
    must stop at 16, so that the residual pivot the guard prices is the one behind the rows the route goes on with: the restatement's
    guard value of `slow` here is 0.57 .. 0.62, twenty times the tolerance, and every walker has to leave (left on the route they
    lose 2e-2 of sigma_1: the kernel ran on to 48 rows and reported the residual behind those)."""
    _, _, flag = check_site(contexts(False, 8), "slow", 64, 8, 8, 8, False, 1)
    assert np.all(flag >= 0)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("slow", "cliff_out"))
@pytest.mark.parametrize("shape", SITE_SHAPES)
def test_complex_rangefinder_delivers_the_top_k_or_ejects(contexts, shape, name):
    m, u, k2, chi = shape
    check_site(contexts(True, chi), name, m, u, k2, chi, True, 1, numpy_reference=True)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
CONDS = (1.0, 1e3, 1e6)


def _rows_with_condition(rng, r, ln, cond, cplx):
    """X = L0 Q: Q with orthonormal rows, L0 lower triangular with singular values from 1 down to 1 / cond"""
    def gauss(*shape):
        a = rng.standard_normal(shape)
        return a + 1j * rng.standard_normal(shape) if cplx else a

    Q = np.linalg.qr(gauss(ln, r))[0].conj().T
    A = (np.linalg.qr(gauss(r, r))[0] * np.logspace(0, -np.log10(cond), r)) @ np.linalg.qr(gauss(r, r))[0]
    L0 = np.linalg.qr(A.conj().T)[1].conj().T
    return L0 @ Q


def _gram_longdouble(X):
    t = np.clongdouble if np.iscomplexobj(X) else np.longdouble
    Xl = X.astype(t)
    return (Xl @ Xl.conj().T).astype(X.dtype)


def _pad_gram(S, fill=777.0):
    """[nb][64][64] with S in the upper triangle of the leading block and a sentinel everywhere the kernel must not read"""
    nb, r, _ = S.shape
    out = np.full((nb, 64, 64), fill, dtype=S.dtype)
    iu = np.triu_indices(r)
    for b in range(nb):
        out[b][iu] = S[b][iu]
    return out


# r: the chunk edges of CS_CH = 8 and CSC_CH = 16 and of the 16 x 16 trailing update; (r rows of ln < r elements are dependent: no factor)
CHOLQR_SIZES = [(r, ln) for ln in (4, 64, 200, 256) for r in (1, 7, 8, 9, 16, 17, 63, 64) if r <= ln]


@pytest.mark.parametrize("r,ln", CHOLQR_SIZES)
@pytest.mark.parametrize("cplx", (False, True), ids=("f64", "c128"))
def test_cholesky_qr_passes(cplx, r, ln):
    capi = _capi()
    rng = np.random.default_rng([r, ln, int(cplx)])
    X0 = np.stack([_rows_with_condition(rng, r, ln, c, cplx) for c in CONDS])
    nb = len(CONDS)
    X = X0
    for npass in (1, 2):
        S = np.stack([_gram_longdouble(X[b]) for b in range(nb)])
        rows = np.full(nb, r, dtype=np.int32)
        Y = capi.diag_chol_solve_rows(_pad_gram(S), X, r if cplx else rows)
        assert Y.shape == X.shape and np.all(np.isfinite(Y))
        for b in range(nb):
            Yr = R.cholqr_pass(S[b], X[b])
            ref = float(np.linalg.norm(Yr @ Yr.conj().T - np.eye(r)))
            bound = MARGIN * max(ref, r * EPS)
            got = float(np.linalg.norm(Y[b] @ Y[b].conj().T - np.eye(r)))
            tri = float(np.linalg.norm(np.triu(X[b] @ Y[b].conj().T, 1)))
            xn = float(np.linalg.norm(X[b]))
            print("cholqr %s r %d len %d cond %.0e pass %d: |Y Y^H - I| %.2e / bound %.2e = %.3f, upper part of X Y^H %.2e / %.2e = %.3f"
                  % ("c128" if cplx else "f64", r, ln, CONDS[b], npass, got, bound, got / bound, tri, bound * xn, tri / (bound * xn)))
            _stat_max(("cholqr", "c128" if cplx else "f64"), ortho_over_bound=got / bound, upper_over_bound=tri / (bound * xn))
            assert got <= bound
            assert tri <= bound * xn
        X = Y


def test_cholesky_qr_bookkeeping_real():
    capi = _capi()
    rng = np.random.default_rng(11)
    rows = np.array([0, 5, 64, 33], dtype=np.int32)
    ln = 200
    X = rng.standard_normal((4, 64, ln))
    S = np.stack([_gram_longdouble(X[b]) for b in range(4)])
    Y = capi.diag_chol_solve_rows(_pad_gram(S), X, rows)
    for b, r in enumerate(rows):
        assert np.array_equal(Y[b, r:], X[b, r:])                       # rows beyond r untouched (rows = 0: the whole entry)
        if r:
            Yr = R.cholqr_pass(S[b][:r, :r], X[b, :r])
            bound = MARGIN * max(float(np.linalg.norm(Yr @ Yr.T - np.eye(r))), r * EPS)
            assert np.linalg.norm(Y[b, :r] @ Y[b, :r].T - np.eye(r)) <= bound
    flag = np.array([-1, 0, 3, -1], dtype=np.int32)
    Y = capi.diag_chol_solve_rows(_pad_gram(S), X, np.array([5, 5, 64, 33], dtype=np.int32), run_flag=flag)
    assert np.array_equal(Y[1], X[1]) and np.array_equal(Y[2], X[2])
    assert not np.array_equal(Y[0, :5], X[0, :5]) and not np.array_equal(Y[3, :33], X[3, :33])


def test_cholesky_qr_bookkeeping_complex():
    capi = _capi()
    rng = np.random.default_rng(12)
    r, r_max, ln = 17, 20, 64
    X = rng.standard_normal((3, r_max, ln)) + 1j * rng.standard_normal((3, r_max, ln))
    S = np.stack([_gram_longdouble(X[b, :r]) for b in range(3)])
    flag = np.array([-1, 0, -1], dtype=np.int32)
    Y = capi.diag_chol_solve_rows(_pad_gram(S), X, r, run_flag=flag)
    assert np.array_equal(Y[1], X[1])
    for b in (0, 2):
        assert np.array_equal(Y[b, r:], X[b, r:])
        Yr = R.cholqr_pass(S[b], X[b, :r])
        bound = MARGIN * max(float(np.linalg.norm(Yr @ Yr.conj().T - np.eye(r))), r * EPS)
        assert np.linalg.norm(Y[b, :r] @ Y[b, :r].conj().T - np.eye(r)) <= bound
    assert np.array_equal(capi.diag_chol_solve_rows(_pad_gram(S), X, 0), X)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((16, 64), (64, 256)))
@pytest.mark.parametrize("cplx", (False, True), ids=("f64", "c128"))
def test_sign_table_matches_the_restatement(cplx, shape):
    t = _capi().diag_sign_table(shape[0], shape[1], complex=cplx)
    assert t.dtype == (np.complex128 if cplx else np.float64)
    assert np.array_equal(t, R.sign_table(*shape).astype(t.dtype))


@pytest.mark.parametrize("cplx", (False, True), ids=("f64", "c128"))
def test_gather_rows_copies_in_pivot_order(cplx):
    capi = _capi()
    rng = np.random.default_rng(13)
    nb, m, ln, slots = 4, 200, 130, 64
    M = rng.standard_normal((nb, m, ln))
    if cplx:
        M = M + 1j * rng.standard_normal((nb, m, ln))
    piv = np.stack([rng.permutation(m)[:slots] for _ in range(nb)]).astype(np.int32)
    piv[0, 3] = -1
    piv[2, 0] = -1
    rows = np.array([64, 17, 40, 64], dtype=np.int32)
    flag = np.array([-1, -1, -1, 0], dtype=np.int32)
    fill = -5.0
    Q = capi.diag_gather_rows(M, piv, rows, run_flag=flag, fill=fill)
    for b in range(nb):
        for j in range(64):
            if flag[b] >= 0 or j >= rows[b] or piv[b, j] < 0:
                assert np.all(Q[b, j] == fill), (b, j)
            else:
                assert np.array_equal(Q[b, j], M[b, piv[b, j]]), (b, j)
    Q = capi.diag_gather_rows(M, piv, rows, fill=fill)                     # no flag: every entry runs
    assert np.array_equal(Q[3, 5], M[3, piv[3, 5]])


# ---- (e) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 5), (2, 2), (9, 33), (64, 64), (37, 200), (64, 256), (256, 256)])
def test_jacobi_rows_complex(shape):
    """complex twins of test_jacobi_rows' matrices (tests/test_gpu_kernels.py), its float64 tolerances"""
    capi = _capi()
    m, ln = shape
    rng = np.random.default_rng(m * 1000 + ln)
    r = min(m, ln)
    U = np.linalg.qr(rng.standard_normal((m, r)) + 1j * rng.standard_normal((m, r)))[0]
    V = np.linalg.qr(rng.standard_normal((ln, r)) + 1j * rng.standard_normal((ln, r)))[0]
    s = np.logspace(0, -5, r)
    M = np.stack([(U * s) @ V.conj().T, (U * s[::-1]) @ V.conj().T])
    k = max(1, r // 2)
    Mo, Vt, S, sw = capi.diag_jacobi(capi.C128, M, k)
    eps = 1e-12
    assert S.dtype == np.float64
    for b in range(2):
        sref = np.linalg.svd(M[b], compute_uv=False)
        assert np.max(np.abs(S[b] - sref[:k])) < eps * sref[0]
        Vb = Vt[b]
        assert np.max(np.abs(Vb @ Vb.conj().T - np.eye(k))) < 20 * eps
        Pref = np.linalg.svd(M[b])[2][:k]
        if k < r and sref[k] < 0.5 * sref[k - 1]:
            gap_tol = 50 * eps * sref[0] / (sref[k - 1] - sref[k])
            assert np.max(np.abs(Vb.conj().T @ Vb - Pref.conj().T @ Pref)) < max(gap_tol, 50 * eps)
        print("complex jacobi %s entry %d: %d sweeps" % (shape, b, sw[b]))
        assert sw[b] < 60

"""Pins tests/trunc_route_ref.py, the NumPy restatement the site-level GPU tests (tests/test_gpu_trunc_routes.py) take their bounds
from, so that those bounds cannot drift: the routes sit at their measured level, the mutants (a missing half step of subspace
iteration) are visible by orders of magnitude, and the guard values of the constructed spectra are decisively on one side of the
tolerance where the GPU tests assert a route membership.  CPU only.

Shapes (m, len, chi): the three GPU-test shapes that have weight beyond kq.  Measured with this file (the four walker seeds of trunc_route_ref.WALKER_SEEDS per case):
  loss(route_f64)   6e-14 .. 2.6e-11 (largest: `graded` at (256, 256)),   loss(route_c128) <= 2.6e-13
  route_f64(steps=0) / route_f64(steps=1):   170 x .. 3e4 x, in the greedy pivot order and in the kernel's (four pivots at a time)
  route_c128(iters=2) / route_c128(iters=3): 100 x .. 640 x at the two chi = 32 shapes ((64, 64, 8) is at the rounding floor with two)
  pivot_guard_value: flat_tail 3e-4 .. 2.9e-3, steps 7e-11 .. 3e-6, rank_kq_minus 0 .. 1e-11, cliff_out 0.43 .. 9.4
  rangefinder_guard_value (tolerance 1e-11): graded <= 1.7e-13, flat_tail / steps / rank_* <= 4.2e-17, cliff_out >= 4.0e-9,
  slow >= 4.3e-5; loss(route_c128) <= 6.1 x the guard value wherever the loss is above the rounding floor."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trunc_route_ref as R  # noqa: E402

SHAPES = ((64, 64, 8), (256, 256, 32), (200, 128, 32))
SEEDS = R.WALKER_SEEDS


@pytest.fixture(scope="module")
def cases():
    """(spectrum, shape, seed, complex) -> (M, svd), built once"""
    out = {}
    for name in R.SPECTRA:
        for shp in SHAPES:
            for seed in SEEDS:
                for cplx in (False, True):
                    M = R.make_case(name, *shp, seed, cplx)
                    out[(name, shp, seed, cplx)] = (M, np.linalg.svd(M, full_matrices=False))
    return out


def test_sign_table_is_signs_and_balanced():
    t = R.sign_table(64, 256)
    assert t.shape == (64, 256) and set(np.unique(t)) == {-1.0, 1.0}
    assert abs(t.mean()) < 4.0 / np.sqrt(t.size)                 # a fair coin: the mean is within four standard errors
    assert np.linalg.matrix_rank(t) == 64
    assert np.array_equal(R.sign_table(16, 64).ravel(), R.sign_table(64, 16).ravel())     # a hash of the flat index only
    # the first entries by hand: h(0) = 0 -> -1; h(1) from the three multiplications
    h = 2654435761
    h ^= h >> 15
    h = (h * 2246822519) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 3266489917) & 0xFFFFFFFF
    h ^= h >> 16
    assert t[0, 0] == -1.0 and t[0, 1] == (1.0 if h & 1 else -1.0)


def test_pivot_select_is_a_greedy_pivoted_cholesky():
    rng = np.random.default_rng(3)
    M = rng.standard_normal((40, 24)) * np.logspace(0, -3, 40)[:, None]
    piv, resid = R.pivot_select(M, 12, block=1)
    assert len(piv) == 12 and len(set(piv)) == 12
    G = M @ M.T
    # the residual is the largest diagonal of the Schur complement of the pivot block
    rest = [i for i in range(40) if i not in piv]
    S = G[np.ix_(rest, rest)] - G[np.ix_(rest, piv)] @ np.linalg.solve(G[np.ix_(piv, piv)], G[np.ix_(piv, rest)])
    assert abs(resid - np.max(np.diag(S)) / np.max(np.diag(G))) < 1e-12
    assert piv[0] == int(np.argmax(np.diag(G)))
    # four at a time (the kernel's order): the first four are the four largest diagonals, the residual is again the Schur complement's
    piv4, resid4 = R.pivot_select(M, 12, block=4)
    assert len(set(piv4)) == 12 and piv4[:4] == [int(p) for p in np.argsort(-np.diag(G), kind="stable")[:4]]
    rest = [i for i in range(40) if i not in piv4]
    S = G[np.ix_(rest, rest)] - G[np.ix_(rest, piv4)] @ np.linalg.solve(G[np.ix_(piv4, piv4)], G[np.ix_(piv4, rest)])
    assert abs(resid4 - np.max(np.diag(S)) / np.max(np.diag(G))) < 1e-12
    # rank 5: the factorisation stops at the rank, nothing is left
    X = rng.standard_normal((30, 5)) @ rng.standard_normal((5, 20))
    piv, resid = R.pivot_select(X, 12)
    assert 5 <= len(piv) <= 12 and resid < 1e-13


def test_cholqr_pass_orthonormalises():
    rng = np.random.default_rng(4)
    X = rng.standard_normal((9, 40)) + 1j * rng.standard_normal((9, 40))
    Y = R.cholqr_pass(X @ X.conj().T, X)
    assert np.linalg.norm(Y @ Y.conj().T - np.eye(9)) < 1e-13
    assert np.allclose(np.triu(X @ Y.conj().T, 1), 0, atol=1e-12)


@pytest.mark.parametrize("shp", SHAPES)
@pytest.mark.parametrize("name", ("graded", "flat_tail"))
def test_routes_at_the_measured_level_and_mutants_visible(cases, name, shp):
    m, ln, k = shp
    kq = R.kq_of(m, ln, k)
    for seed in SEEDS:
        M, svd = cases[(name, shp, seed, False)]
        for block in (1, 4):         # the plain greedy pivot order, and the kernel's four at a time
            l1 = R.loss(M, R.route_f64(M, k, kq, block=block), k, svd)
            l0 = R.loss(M, R.route_f64(M, k, kq, steps=0, block=block), k, svd)
            print("f64 %s %s seed %d block %d: loss %.2e, without the iteration step %.2e (x %.0f)"
                  % (name, shp, seed, block, l1, l0, l0 / l1))
            assert l1 <= 1e-10
            assert l0 >= 100 * l1
        M, svd = cases[(name, shp, seed, True)]
        l3 = R.loss(M, R.route_c128(M, k, kq), k, svd)
        l2 = R.loss(M, R.route_c128(M, k, kq, iters=2), k, svd)
        print("c128 %s %s seed %d: loss %.2e, with two iterations %.2e (x %.0f)" % (name, shp, seed, l3, l2, l2 / l3))
        assert l3 <= 1e-11
        if k == 32:
            assert l2 >= 16 * l3


@pytest.mark.parametrize("shp", SHAPES)
def test_pivot_guard_values_are_decisive(cases, shp):
    """The spectra whose membership of the pivoted route the GPU tests assert are a factor of ten or more away from the guard's
    tolerance 3e-2, in the plain greedy pivot order and in the kernel's.
    Measured over the walkers' seeds (trunc_route_ref.WALKER_SEEDS, chosen by this very criterion): flat_tail 2.3e-3 .. 2.9e-3 at
    (256, 256, 32) and <= 1.3e-3 at the other two shapes, steps <= 3e-6, rank_kq_minus <= 1e-11, cliff_out >= 0.43, slow at
    (64, 64, 8) >= 0.48."""
    m, ln, k = shp
    kq = R.kq_of(m, ln, k)
    misses = []
    for seed in SEEDS:
        for block in (1, 4):
            for name in ("flat_tail", "steps", "rank_kq_minus"):
                g = R.pivot_guard_value(cases[(name, shp, seed, False)][0], k, kq, block)
                print("guard %s %s seed %d block %d: %.2e" % (name, shp, seed, block, g))
                if not g <= R.GUARD_TOL / 10:
                    misses.append("%s seed %d block %d: %.3e is not ten times below %.0e" % (name, seed, block, g, R.GUARD_TOL))
            out = ("cliff_out", "slow") if shp == (64, 64, 8) else ("cliff_out",)     # (slow: the GPU test of the factorisation's cap)
            for name in out:
                g = R.pivot_guard_value(cases[(name, shp, seed, False)][0], k, kq, block)
                print("guard %s %s seed %d block %d: %.2e" % (name, shp, seed, block, g))
                if not g >= R.GUARD_TOL * 10:
                    misses.append("%s seed %d block %d: %.3e is not ten times above %.0e" % (name, seed, block, g, R.GUARD_TOL))
    assert not misses, "; ".join(misses)


@pytest.mark.parametrize("shp", SHAPES)
def test_rangefinder_guard_separates_and_bounds_the_loss(cases, shp):
    """The tolerance of the complex range finder's guard, 1e-11: every spectrum the iteration resolves is at least 10 x below it
    (graded, the real state's shape, 60 x), cliff_out and slow are at least 100 x above it, and the loss of a matrix is at most 8 x
    its guard value (measured: 6.1 x) once it is above the rounding floor -- a walker the guard keeps loses at most 8e-11, the level
    of the float64 route's own algorithmic loss (2.2e-11 on graded)."""
    m, ln, k = shp
    kq = R.kq_of(m, ln, k)
    floor = ln * R.EPS
    for seed in SEEDS:
        for name in R.SPECTRA:
            M, svd = cases[(name, shp, seed, True)]
            g = R.rangefinder_guard_value(M, k, kq)
            ls = R.loss(M, R.route_c128(M, k, kq), k, svd)
            print("rangefinder guard %s %s seed %d: %.2e, loss %.2e" % (name, shp, seed, g, ls))
            if name in ("cliff_out", "slow"):
                assert g >= 100 * R.C128_GUARD_TOL
            else:
                assert g <= R.C128_GUARD_TOL / 10
            assert ls <= max(8 * g, 8 * floor)


def test_metrics_on_the_exact_answer(cases):
    M, svd = cases[("cliff_out", (200, 128, 32), SEEDS[0], True)]
    V = svd[2][:32]
    assert R.loss(M, V, 32, svd) < 1e-14
    assert abs(R.captured(M, V, 32, svd)) < 1e-14
    # one kept direction swapped for a discarded one: the loss is that direction's weight
    W = V.copy()
    W[5] = svd[2][40]
    assert abs(R.loss(M, W, 32, svd) - svd[1][5] / svd[1][0]) < 1e-12
    assert R.captured(M, W, 32, svd) < 0
    assert R.numerical_rank(np.linalg.svd(cases[("rank_below_k", (64, 64, 8), SEEDS[0], False)][0], compute_uv=False)) == 6

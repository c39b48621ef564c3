"""The device eigensolver (peps_amd/csrc/eigh_jacobi.h, two-sided parallel Jacobi in HBM) through ctx.diag_eigh against
numpy.linalg.eigh, float64.

Sizes: the trivial ones (1, 2), odd ones (3, 17, 65: the round-robin bye), a wave boundary and the size above it (64, 65), and more
pairs than one workgroup row holds (200).  Kinds: random symmetric indefinite; a Gram matrix of rank min(5, n) (many zero eigenvalues,
the shape of the MinSR T matrix); 2 I plus one off-diagonal pair (degenerate eigenvalues); a centred Gram matrix with the exact null
vector of ones; random complex Hermitian.  Eigenvectors are never compared directly (degenerate cases make them non-unique).

Checked with eps = 2^-52:  max|w - w_np| <= C n eps |A|_2,  |A Z - Z diag(w)|_F <= C n eps |A|_F,  |Z^H Z - I|_F <= C n eps.
Largest ratios to n eps (times the norm) observed over all 35 cases on the MI355X: device 0.339 (eigenvalues, n = 2 hermitian), 0.816
(residual, n = 3 gram_rank5), 11.600 (orthogonality, n = 200 centred_gram; it grows with n: 0.7, 1.5, 3.0, 5.5, 5.5, 11.6 at n = 2, 3,
17, 64, 65, 200); numpy.linalg.eigh on the same matrices 0.915, 0.956, 2.552.  C = 8 x the largest of all (11.600) = 92.8, rounded up
to a power of two = 128.  (A C above 1024 would mean the solver has not converged.)  Sweeps: 1 at n = 1, 2 at n = 2 and for the
degenerate kind, 5 at n = 3, 7-8 at n = 17, 9-10 at n = 64 and 65, 11-15 at n = 200."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
C = 128.0
SIZES = (1, 2, 3, 17, 64, 65, 200)
KINDS = ("indefinite", "gram_rank5", "degenerate", "centred_gram", "hermitian")


def make_matrix(n, kind):
    rng = np.random.default_rng(1000 * SIZES.index(n) + KINDS.index(kind))
    if kind == "indefinite":
        a = rng.standard_normal((n, n))
        return (a + a.T) / 2
    if kind == "gram_rank5":
        x = rng.standard_normal((n, min(5, n)))
        return x @ x.T
    if kind == "degenerate":
        a = 2.0 * np.eye(n)
        if n > 1:
            a[0, n - 1] = a[n - 1, 0] = 0.5
        return a
    if kind == "centred_gram":
        x = rng.standard_normal((n, 3 * n))
        g = x @ x.T
        m = g.sum(axis=1) / n
        t = (g - m[:, None] - m[None, :] + m.sum() / n) / n
        return (t + t.T) / 2
    a = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return (a + a.conj().T) / 2


def ratios(a, w, z):
    """the three checked quantities over n eps (times the norm of A)"""
    n = a.shape[0]
    n2, nf = np.linalg.norm(a, 2), np.linalg.norm(a)
    w_np = np.linalg.eigvalsh(a)
    def over(x, bound):           # the zero matrix (n = 1, centred): the bound is 0 and must be met exactly
        return float(x / bound) if bound > 0 else (0.0 if x == 0 else np.inf)

    return (over(np.max(np.abs(w - w_np)), n * EPS * n2), over(np.linalg.norm(a @ z - z * w), n * EPS * nf),
            over(np.linalg.norm(z.conj().T @ z - np.eye(n)), n * EPS))


@pytest.fixture(scope="module")
def ctx():
    from peps_amd import capi
    c = capi.Context(2, 2, 2, 2, 4, dtype=capi.F64, max_walkers=1)
    yield c
    c.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_eigh_against_numpy(ctx, n, kind):
    a = make_matrix(n, kind)
    w, z, sweeps = ctx.diag_eigh(a)
    assert w.shape == (n,) and z.shape == (n, n) and z.dtype == a.dtype
    assert np.all(np.diff(w) >= 0)
    assert 1 <= sweeps <= 30
    got = ratios(a, w, z)
    w_np, z_np = np.linalg.eigh(a)
    print("n %d %s: sweeps %d, ratios device %.3f %.3f %.3f  numpy %.3f %.3f %.3f" % ((n, kind, sweeps) + got + ratios(a, w_np, z_np)))
    assert got[0] <= C and got[1] <= C and got[2] <= C
    if n == 1:
        assert w[0] == a[0, 0].real and z[0, 0] == 1


def test_signs_of_an_indefinite_spectrum(ctx):
    """eigenvalues +x and -x share a singular value: the solver must still separate their vectors and keep the signs"""
    a = np.array([[0.0, 1.0], [1.0, 0.0]])
    w, z, _ = ctx.diag_eigh(a)
    assert np.max(np.abs(w - np.array([-1.0, 1.0]))) <= C * 2 * EPS
    assert np.linalg.norm(a @ z - z * w) <= C * 2 * EPS * np.linalg.norm(a)


def test_bad_arguments(ctx):
    with pytest.raises(ValueError):
        ctx.diag_eigh(np.zeros((0, 0)))
    a = np.eye(3)
    a[1, 2] = a[2, 1] = np.nan
    with pytest.raises(ValueError):
        ctx.diag_eigh(a)

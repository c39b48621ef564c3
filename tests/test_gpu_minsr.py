"""pepsgpu_minsr_direction: the MinSR direction of the resident O* store computed on the device (Gram, four-term centering, Jacobi
eigensolve, pseudo-inverse cutoff, back-substitution into the optimizer's direction buffer) against the oracle restatement of
Optimizer::CalculateMinSRDirection_ (oracle/sr.py), against the Python orchestration peps_amd/sr.py::minsr_direction (host eigh), and
the reference's own check MinSR == SR at zero shift (test_sr_vs_minsr_equivalence.cpp).  Sample store as in tests/test_gpu_sr.py:
4 x 4, D = 3, chi = 9, 48 samples (f64, f32), and the complex store of test_sr_matvec_complex_vs_oracle (32 samples)."""
import os

import numpy as np
import pytest

from oracle import sr as osr
from peps_amd import synthetic

pytestmark = pytest.mark.gpu

L, D, CHI = 4, 3, 9
SETTINGS = ({"r_pinv": 1e-12, "a_pinv": 0.0, "soft_cutoff": True}, {"r_pinv": 1e-6, "a_pinv": 1e-9, "soft_cutoff": False})
TOL = {"f64": 1e-10, "f32": 2e-5, "c128": 1e-10}


def _collect(ctx, cfgs, cplx=False):
    """punch every hole of every walker: once to the host (reference O* samples) and once into the device store"""
    from peps_amd.capi import LEFT, RIGHT, UP, DOWN, HORIZONTAL
    n = len(cfgs)
    ctx.set_configs(cfgs)
    psi = ctx.evaluate_amplitude()
    ctx.set_configs(cfgs)
    ctx.generate_bmps_approach(UP)
    ostar = np.zeros((n, L, L, 2, D, D, D, D), dtype=np.complex128 if cplx else np.float64)
    for row in range(L):
        ctx.init_bten(LEFT, row)
        ctx.grow_full_bten(RIGHT, row, 1, True)
        for col in range(L):
            h = ctx.punch_hole(row, col, HORIZONTAL)
            ctx.punch_hole_store(row, col, HORIZONTAL)
            for w in range(n):
                ostar[w, row, col, cfgs[w, row, col]] = np.conj(h[w]) / np.conj(psi[w]) if cplx else h[w] / psi[w]
            if col < L - 1:
                ctx.shift_bten_window(RIGHT)
        if row < L - 1:
            ctx.shift_bmps_window(DOWN)
    return psi, ostar


def _state(dt):
    flat = synthetic.sitps_to_flat(synthetic.make_sitps(L, D), D)
    if dt == "c128":
        rng = np.random.default_rng(12)
        flat = flat.astype(np.complex128)
        flat = flat * np.exp(2j * np.pi * rng.random(flat.shape)) * (np.abs(flat) > 0)
    return flat


def _store(dt):
    from peps_amd import capi
    cplx = dt == "c128"
    nb, seed0, step = (16, 300, 40) if cplx else (24, 300, 50)
    ctx = capi.Context(L, L, D, 2, CHI, dtype={"f32": capi.F32, "f64": capi.F64, "c128": capi.C128}[dt], max_walkers=nb)
    ctx.state_upload(_state(dt))
    ctx.sr_begin(2 * nb)
    samples = []
    for batch in range(2):
        cfgs = synthetic.make_configs(L, nb, "heisenberg", seed0=seed0 + step * batch)
        psi, ostar = _collect(ctx, cfgs, cplx)
        ctx.sr_append(psi)
        samples += list(ostar)
    return ctx, samples


def _mask():
    """1 where the zero padded state layout holds a tensor element (boundary legs have dimension 1)"""
    return synthetic.sitps_to_flat(synthetic.make_sitps(L, D), D).reshape(L, L, 2, D, D, D, D) != 0


class Case:
    def __init__(self, dt):
        self.dt = dt
        self.ctx, self.samples = _store(dt)
        self.ctx.opt_begin()
        n = len(self.samples)
        rng = np.random.default_rng(2)
        self.e_loc = rng.standard_normal(n) + (1j * rng.standard_normal(n) if dt == "c128" else 0.0)
        self.e_mean = complex(self.e_loc.mean()) if dt == "c128" else float(self.e_loc.mean())
        self.mean = np.mean(self.samples, axis=0)
        self.ev = np.linalg.eigvalsh(osr.minsr_tmatrix(self.samples))      # the oracle's eigenvalues of T
        self.oracle = {}

    def settings(self):
        for kw in SETTINGS:
            if self.dt == "f32" and kw["soft_cutoff"]:
                kw = dict(kw, r_pinv=1e-5)          # keep the cutoff above the f32 rounding of the Gram entries
            yield kw

    def want(self, kw):
        key = tuple(sorted(kw.items()))
        if key not in self.oracle:
            self.oracle[key] = osr.minsr_direction(self.samples, self.mean, self.e_loc, self.e_mean, **kw)
        return self.oracle[key]

    def cutoff(self, kw):
        return kw["r_pinv"] * float(np.max(np.abs(self.ev))) + kw["a_pinv"]


_CASES = {}


def _case(dt):
    """one store, one set of local energies and one oracle result per dtype, shared by the tests of this module"""
    if dt not in _CASES:
        _CASES[dt] = Case(dt)
    return _CASES[dt]


@pytest.fixture(params=["f64", "f32", "c128"])
def case(request):
    return _case(request.param)


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _CASES.values():
        c.ctx.close()
    _CASES.clear()


def test_direction_against_the_oracle(case):
    bound = max(1e3 * TOL[case.dt], 1e-7)
    mask = _mask()
    for kw in case.settings():
        if not kw["soft_cutoff"]:      # a hard cutoff next to an eigenvalue would make the comparison a coin toss: refuse such a draw loudly
            c = case.cutoff(kw)
            near = case.ev[(np.abs(case.ev) > c / 4) & (np.abs(case.ev) < 4 * c)]
            assert near.size == 0, "eigenvalues %s within a factor 4 of the cutoff %.3e" % (near, c)
        nrm, info = case.ctx.minsr_direction(case.e_loc, case.e_mean, **kw)
        g = case.ctx.opt_get_gradient()
        do, nrmo = case.want(kw)
        do = do.reshape(g.shape)
        err = float(np.linalg.norm((g - do)[mask]) / nrmo)
        print("%s %s: |g - oracle| / |oracle| = %.3e, norm rel %.3e, info %s" % (case.dt, kw, err, abs(nrm / nrmo - 1), info))
        assert err < bound, kw
        assert abs(nrm / nrmo - 1) < bound, kw
        assert np.all(g[~mask] == 0)
        assert 1 <= info["sweeps"] <= 30
        assert abs(info["lambda_max"] / np.max(np.abs(case.ev)) - 1) < bound and abs(info["cutoff"] / case.cutoff(kw) - 1) < bound


def test_direction_against_the_python_path(case):
    from peps_amd import sr
    bound = max(1e3 * TOL[case.dt], 1e-7)
    batch = sr.DeviceSampleBatch(case.ctx)
    for kw in case.settings():
        dp, nrmp = sr.minsr_direction(batch, case.e_loc, case.e_mean, **kw)
        nrm, info = case.ctx.minsr_direction(case.e_loc, case.e_mean, **kw)
        g = case.ctx.opt_get_gradient()
        err = float(np.linalg.norm(g.ravel() - np.asarray(dp).ravel()) / nrmp)
        print("%s %s: |g - python path| / |python path| = %.3e, norm rel %.3e" % (case.dt, kw, err, abs(nrm / nrmp - 1)))
        assert err < bound and abs(nrm / nrmp - 1) < bound, kw
        assert info["n_kept"] == int(np.count_nonzero(np.abs(case.ev) > case.cutoff(kw))), kw


def test_minsr_equals_sr_at_zero_shift():
    """test_sr_vs_minsr_equivalence.cpp: MinSR with r_pinv = 0, a_pinv = 1e-11, hard cutoff == (S + 0) x = g solved by CG to 1e-13"""
    from peps_amd import sr
    case = _case("f64")
    flat = np.stack([s.ravel() for s in case.samples])
    grad = ((case.e_loc - case.e_mean)[:, None] * flat).mean(axis=0).reshape(case.mean.shape)
    x, res, it, why = sr.natural_gradient(case.ctx, grad, 0.0, max_iter=500, relative_tolerance=1e-13)
    nrm, info = case.ctx.minsr_direction(case.e_loc, case.e_mean, r_pinv=0.0, a_pinv=1e-11, soft_cutoff=False)
    d = case.ctx.opt_get_gradient()
    err = float(np.linalg.norm(x.ravel() - d.ravel()) / np.linalg.norm(d.ravel()))
    print("MinSR vs SR: rel %.3e (CG iterations %d, kept %d)" % (err, it, info["n_kept"]))
    assert why == sr.K_CONVERGED
    assert err < 1e-7


@pytest.mark.parametrize("dt", ["f64", "c128"])
def test_step_applies_the_direction(dt):
    case = _case(dt)
    ctx, lr = case.ctx, 0.05
    theta0 = ctx.opt_read_state()
    ctx.minsr_direction(case.e_loc, case.e_mean, **SETTINGS[0])
    g = ctx.opt_get_gradient()
    ctx.opt_step(0, lr, (0.0, 0.0, 0.0))
    theta1 = ctx.opt_read_state()
    ctx.state_upload(_state(dt))         # leave the shared context as the other tests expect it
    ctx.opt_begin()
    mask = _mask()
    err = float(np.max(np.abs(theta1 - (theta0 - lr * g))))
    print("%s step: max |theta_1 - (theta_0 - lr g)| = %.3e (bound %.3e)" % (dt, err, 1e-15 * np.max(np.abs(theta0))))
    assert err <= 1e-15 * float(np.max(np.abs(theta0)))
    assert np.all(theta1[~mask] == 0) and np.count_nonzero(g) > 0


def test_refusals_leave_the_direction_untouched(fixtures_dir):
    from peps_amd import capi, fermion
    case = _case("f64")
    ctx = case.ctx
    ctx.minsr_direction(case.e_loc, case.e_mean, **SETTINGS[0])
    before = ctx.opt_get_gradient().tobytes()
    with pytest.raises(ValueError):
        ctx.minsr_direction(case.e_loc, case.e_mean, a_pinv=-1.0)
    assert ctx.opt_get_gradient().tobytes() == before
    with pytest.raises(ValueError):
        ctx.minsr_direction(case.e_loc, float("nan"))
    assert ctx.opt_get_gradient().tobytes() == before
    with pytest.raises(ValueError):
        ctx.minsr_direction(case.e_loc, case.e_mean, r_pinv=float("inf"))
    assert ctx.opt_get_gradient().tobytes() == before
    # a context of its own: before opt_begin, then with an empty store
    fresh = capi.Context(L, L, D, 2, CHI, dtype=capi.F64, max_walkers=4)
    fresh.state_upload(_state("f64"))
    with pytest.raises(RuntimeError):
        fresh.minsr_direction(np.zeros(4), 0.0)
    fresh.opt_begin()
    x = np.random.default_rng(5).standard_normal(_mask().shape) * _mask()
    fresh.opt_set_gradient(x)
    before = fresh.opt_get_gradient().tobytes()
    with pytest.raises(RuntimeError):
        fresh.minsr_direction(np.zeros(4), 0.0)
    fresh.sr_begin(4)                        # a store with no sample appended is still empty
    with pytest.raises(RuntimeError):
        fresh.minsr_direction(np.zeros(4), 0.0)
    assert fresh.opt_get_gradient().tobytes() == before
    fresh.close()
    # a fermionic decoration: the T matrix in the stored parameters is not built
    st = fermion.FermionState.load(os.path.join(fixtures_dir, "spinless_fermion_tps_t2_0.000000_double_from_simple_update"), False)
    fctx = capi.Context(st.rows, st.cols, st.D, 4 * st.d, 8, dtype=capi.F64, max_walkers=1)
    fctx.state_upload(st.extended_flat())
    fctx.fermion_decoration_set(st)
    fctx.opt_begin()
    fctx.opt_set_gradient(np.random.default_rng(6).standard_normal(st.extended_flat().shape))
    before = fctx.opt_get_gradient().tobytes()
    with pytest.raises(ValueError):
        fctx.minsr_direction(np.zeros(1), 0.0)
    assert fctx.opt_get_gradient().tobytes() == before
    fctx.close()

"""The device-resident optimizer on fermionic states (pepsgpu_fermion_decoration_set, hostapi.fermion_optimize_exact_sum /
fermion_sr_step_samples): theta, g and the rule state hold the 4 d decorated components, the gradient is finished, folded and projected
in HBM, norms and the SR solve are those of the stored parameters.  Checked against the reference's exact-summation golden values
(test_fermion_exact_optimizer_integration_golden.cpp), its Adam convergence criteria (test_optimizer_adam_exact_sum.cpp:146-169) and,
step for step, against the existing host path: hostapi.fermion_exact_sum (gradient read back and folded in NumPy) + tests/opt_ref.py."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import opt_fermion_ref as fref  # noqa: E402
import opt_ref  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = 0, 1
EPS64 = 2.220446049250313e-16
EPS32 = 1.1920929e-07
GOLDEN_ENERGY = -1.9821805385446198           # test_fermion_exact_optimizer_integration_golden.cpp, real and complex fixture
GOLDEN_NORM_SQ = 0.064616411237561233
GOLDEN_PROBE = 0.021610150065783196
GOLDEN_NORM_SQ_COMPLEX = 0.064616411237560373
SGD0 = (0.0, 0.0, 0.0)


def _load(fixtures_dir, name, complex_data=False):
    from peps_amd import fermion
    return fermion.FermionState.load(os.path.join(fixtures_dir, name), complex_data)


def _half_filling():
    return np.array([np.array(p).reshape(2, 2) for p in sorted(set(itertools.permutations([0, 0, 1, 1])))], dtype=np.int32)


def _energy_kwargs(model, params):
    if model == "spinless":
        t, V, t2 = params
        return dict(t=t, V=V, model="spinless", t2=t2)
    t, J, V, mu = params
    return dict(t=t, V=V, model="tj", J=J, mu=mu)


def _accumulated_context(st, cfgs, chi, model, params, dtype=F64, exact_sum=True, sr=False):
    """a capi context holding the decorated state with S_O / S_EO of `cfgs` accumulated (row pass of hole punches, as
    test_sr_step_of_the_optimizer_equals_the_host_vector_solve drives it) and, with sr, the O* samples; returns (ctx, e_loc_sum, weight_sum)"""
    from peps_amd import capi, fermion, hostapi
    from peps_amd.capi import LEFT, RIGHT, UP, DOWN, HORIZONTAL
    amps, en, _ = hostapi.fermion_energy(st, cfgs, chi, dtype=dtype, **_energy_kwargs(model, params))
    dense = st.sigma(cfgs) * amps
    ext = st.ext_config(cfgs, fermion.ROW)
    ctx = capi.Context(st.rows, st.cols, st.D, 4 * st.d, chi, dtype=dtype, max_walkers=len(cfgs))
    ctx.state_upload(st.extended_flat())
    ctx.set_configs(ext)
    ctx.generate_bmps_approach(UP)
    for row in range(st.rows):
        ctx.init_bten(LEFT, row)
        ctx.grow_full_bten(RIGHT, row, 1, True)
        for col in range(st.cols):
            ctx.punch_hole_store(row, col, HORIZONTAL)
            if col < st.cols - 1:
                ctx.shift_bten_window(RIGHT)
        if row < st.rows - 1:
            ctx.shift_bmps_window(DOWN)
    ctx.grad_reset()
    ctx.grad_accumulate(dense, en, exact_sum=exact_sum, states=ext)
    if sr:
        ctx.sr_begin(len(cfgs))
        ctx.sr_append(dense)
    w = amps ** 2 if exact_sum else np.ones(len(cfgs))
    return ctx, float(np.sum(w * en)), float(np.sum(w))


def test_reference_golden_through_the_device_loop(fixtures_dir):
    """SGD with lr = 0, one iteration: the energy, the NormSquare of the gradient and the weighted probe of the reference's golden, each
    at the reference's 1e-10; the state comes back bit for bit."""
    from peps_amd import hostapi
    st = _load(fixtures_dir, "spinless_fermion_tps_t2_0.000000_double_from_simple_update")
    cfgs = _half_filling()
    energies, stored, norms = hostapi.fermion_optimize_exact_sum(st, cfgs, 16, "spinless", (1.0, 0.0, 0.0), "sgd", 0.0, SGD0, 1, dtype=F64,
                                                                 return_grad_norms=True)
    print("golden: E - ref = %.3e  |g|^2 - ref = %.3e" % (energies[0] - GOLDEN_ENERGY, norms[0] ** 2 - GOLDEN_NORM_SQ))
    assert abs(energies[0] - GOLDEN_ENERGY) < 1e-10
    assert abs(norms[0] ** 2 - GOLDEN_NORM_SQ) < 1e-10
    assert np.array_equal(stored, fref.stored_flat(st))
    assert abs(energies[1] - energies[0]) < 1e-13 and abs(norms[1] - norms[0]) < 1e-13
    # the stored gradient itself, through the C ABI
    ctx, es, ws = _accumulated_context(st, cfgs, 16, "spinless", (1.0, 0.0, 0.0))
    ctx.fermion_decoration_set(st)
    ctx.opt_begin()
    e, nrm = ctx.opt_gradient_from_accumulators(es, ws)
    g_ext = ctx.opt_get_gradient()
    ctx.close()
    g = g_ext[:, :, :st.d]
    probe = sum(0.01 * ((r + 1) * 13 + (c + 1) * 7 + (s + 1) * 3) * float(np.sum(g[r, c, s] ** 2))
                for r in range(2) for c in range(2) for s in range(st.d))
    print("golden: probe - ref = %.3e  |g|^2 (C ABI) - ref = %.3e" % (probe - GOLDEN_PROBE, nrm ** 2 - GOLDEN_NORM_SQ))
    assert abs(e - GOLDEN_ENERGY) < 1e-10 and abs(nrm ** 2 - GOLDEN_NORM_SQ) < 1e-10
    assert abs(probe - GOLDEN_PROBE) < 1e-10
    assert np.array_equal(g_ext, fref.decorate(st, g))                       # the gradient is in the range of the decoration
    assert np.all(g[~fref.allowed_flat(st)] == 0)


def test_reference_golden_complex_fixture(fixtures_dir):
    from peps_amd import hostapi
    st = _load(fixtures_dir, "spinless_fermion_tps_t2_0.000000_complex_from_simple_update", True)
    energies, stored, norms = hostapi.fermion_optimize_exact_sum(st, _half_filling(), 16, "spinless", (1.0, 0.0, 0.0), "sgd", 0.0, SGD0, 1,
                                                                 return_grad_norms=True)
    print("golden (complex): E - ref = %.3e %+.3ej  |g|^2 - ref = %.3e"
          % (energies[0].real - GOLDEN_ENERGY, energies[0].imag, norms[0] ** 2 - GOLDEN_NORM_SQ_COMPLEX))
    assert abs(energies[0] - GOLDEN_ENERGY) < 1e-10
    assert np.array_equal(stored, fref.stored_flat(st))
    assert abs(norms[0] ** 2 - GOLDEN_NORM_SQ_COMPLEX) < 1e-10


def test_adam_converges_by_the_reference_criteria(fixtures_dir):
    """test_optimizer_adam_exact_sum.cpp:146-169: Adam (0.9, 0.999, 1e-8, 0), lr 0.01, 300 iterations, E0 = -2"""
    from peps_amd import fermion, hostapi
    st = _load(fixtures_dir, "spinless_fermion_tps_t2_0.000000_double_from_simple_update")
    cfgs = _half_filling()
    energies, stored = hostapi.fermion_optimize_exact_sum(st, cfgs, 8, "spinless", (1.0, 0.0, 0.0), "adam", 0.01, (0.9, 0.999, 1e-8, 0.0), 300,
                                                          dtype=F64)
    e = float(energies[300])
    print("adam: E[0] = %.12f  E[100] + 2 = %.3e  E[300] + 2 = %.3e" % (energies[0], energies[100] + 2, e + 2))
    assert e >= -2.0 - 1e-10 and abs(e + 2.0) < 1e-5
    final = fermion.FermionState.from_stored(st, stored)
    e_again, _ = hostapi.fermion_exact_sum(final, cfgs, 8, 1.0, 0.0, dtype=F64)
    print("adam: |E(re-uploaded state) - E[300]| = %.3e" % abs(e_again - e))
    assert abs(e_again - e) < 1e-12
    assert np.all(stored[~fref.allowed_flat(st)] == 0)


# Trajectory of the device loop against the existing host path, five iterations.  Measured on the MI355X; asserted
# at ten times the largest measured value, never looser than 1e-10 on the energy (the reference's tolerance on these energies) and
# 1e-9 per element on the state (the suite's gradient parity).
# Measured: 0 on both, in all fourteen cases -- the two paths run the same kernels on the same inputs and the rules commute with the
# decoration bit for bit (tests/test_cpu_opt_fermion.py), so the assertion is equality.
MEASURED_TRAJ_E = 0.0
MEASURED_TRAJ_STATE = 0.0
TOL_TRAJ_E = min(10 * MEASURED_TRAJ_E, 1e-10)
TOL_TRAJ_STATE = min(10 * MEASURED_TRAJ_STATE, 1e-9)

_TRAJ_CASES = {
    "spinless": ("spinless_fermion_tps_t2_2.100000_double_from_simple_update", "spinless", (1.0, 0.0, 2.1), 8, _half_filling),
    "tj": ("tj_model_tps_double_from_simple_update", "tj", (1.0, 0.3, 0.075, 0.0), 4,
           lambda: np.array([np.array(p).reshape(2, 2) for p in sorted(set(itertools.permutations([2, 2, 0, 1])))], dtype=np.int32)),
}


def _host_path_trajectory(st, cfgs, chi, model, params, rule, lr, rule_params, iterations, clip_value=0.0, clip_norm=0.0):
    """the existing path: per iteration hostapi.fermion_exact_sum (read-back, NumPy finish and fold) -> opt_ref.clip / step -> new state"""
    from peps_amd import fermion, hostapi
    kw = _energy_kwargs(model, params)
    t, V = kw.pop("t"), kw.pop("V")
    theta = [fref.stored_flat(st)]
    rs = opt_ref.RuleState(theta)
    energies, norms = [], []
    cur = st
    for it in range(iterations + 1):
        e, g = hostapi.fermion_exact_sum(cur, cfgs, chi, t, V, dtype=F64, **kw)
        energies.append(float(np.real(e)))
        norms.append(opt_ref.norm([g]))
        if it == iterations:
            break
        theta = opt_ref.step(rule, theta, opt_ref.clip([g], clip_value, clip_norm), rs, lr, rule_params)
        cur = fermion.FermionState.from_stored(st, theta[0])
    return np.array(energies), np.array(norms), theta[0]


def _trajectory_case(fixtures_dir, which, rule, lr, rule_params, clip_value=0.0, clip_norm=0.0, label=""):
    from peps_amd import hostapi
    name, model, params, chi, configs = _TRAJ_CASES[which]
    st = _load(fixtures_dir, name)
    cfgs = configs()
    if clip_norm < 0.0:                                   # half the initial norm
        _, g0 = hostapi.fermion_exact_sum(st, cfgs, chi, params[0], dtype=F64,
                                          **{k: v for k, v in _energy_kwargs(model, params).items() if k != "t"})
        clip_norm = 0.5 * opt_ref.norm([g0])
    e_ref, n_ref, th_ref = _host_path_trajectory(st, cfgs, chi, model, params, rule, lr, rule_params, 5, clip_value, clip_norm)
    energies, stored, norms = hostapi.fermion_optimize_exact_sum(st, cfgs, chi, model, params, rule, lr, rule_params, 5, clip_value, clip_norm,
                                                                 dtype=F64, return_grad_norms=True)
    de = float(np.max(np.abs(energies - e_ref)))
    dth = float(np.max(np.abs(stored - th_ref)))
    dn = float(np.max(np.abs(norms - n_ref)))
    print("trajectory %s %s: max |E - E_ref| = %.3e  max |theta_5 - ref| = %.3e  max | |g| - ref | = %.3e  E[0] = %.10f  E[5] = %.10f"
          % (which, label, de, dth, dn, energies[0], energies[5]))
    assert abs(e_ref[5] - e_ref[0]) > 1e-6                # the steps moved the state
    assert de <= TOL_TRAJ_E and dth <= TOL_TRAJ_STATE
    assert dn <= 1e-9
    assert np.all(stored[~fref.allowed_flat(st)] == 0)


@pytest.mark.parametrize("which", ["spinless", "tj"])
@pytest.mark.parametrize("name,rule,lr,params", opt_ref.SETTINGS, ids=[x[0] for x in opt_ref.SETTINGS])
def test_device_loop_follows_the_host_path(fixtures_dir, which, name, rule, lr, params):
    _trajectory_case(fixtures_dir, which, rule, lr, params, label=name)


@pytest.mark.parametrize("which", ["spinless", "tj"])
def test_device_loop_follows_the_host_path_with_clips(fixtures_dir, which):
    _, rule, lr, params = opt_ref.SETTINGS[4]                                # plain SGD: the clip is what moves
    _trajectory_case(fixtures_dir, which, rule, lr, params, clip_norm=-1.0, label="clip_norm")
    _, rule, lr, params = opt_ref.SETTINGS[0]
    _trajectory_case(fixtures_dir, which, rule, lr, params, clip_value=0.01, label="clip_value")


def _seeded_configs(rows, cols, n_occ, n, seed):
    """n seeded configurations with n_occ occupied sites (state 0); n_occ even: the random states have even total parity.  A
    configuration may repeat (2x3 has 15 with two particles): the exact sum is then a weighted one, on both sides alike."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        c = np.ones(rows * cols, dtype=np.int32)
        c[rng.permutation(rows * cols)[:n_occ]] = 0
        out.append(c.reshape(rows, cols))
    return np.array(out, dtype=np.int32)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(3, 3, 5), (2, 3, 3)], ids=["3x3D5", "2x3D3"])
def test_shapes_where_the_kernels_can_go_wrong(shape, dt):
    """(3, 3, 5): the interior site has 625 elements (three 256-thread blocks per slot), edge and corner legs have dimension 1, both
    parities occur on every bond.  One plain-SGD step of the device loop equals theta - lr fold(g) with g from the existing host path on
    the same context type.  float64: both sides finish the same accumulators with the same arithmetic, so the difference is the rounding
    of theta - lr g: 4 eps64 max|theta|.  float32 context: opt_begin adopts the device state, so theta is float(theta) there (as for
    bosons); the accumulators are float64 sums of float32 contractions, evaluated twice by the same kernels; allowing for a different
    summation order of the 16 float32 terms per element, 16 eps32 lr max|g| is added."""
    from peps_amd import capi, fermion, hostapi
    rows, cols, D = shape
    dtype = F64 if dt == "f64" else F32
    st = fermion.random_even_state(rows, cols, D, seed=7)
    cfgs = _seeded_configs(rows, cols, 2 * ((rows * cols) // 4), 16, 3)
    lr = 0.05
    theta = fref.stored_flat(st)
    if dt == "f32":
        theta = theta.astype(np.float32).astype(np.float64)                  # what the device holds, and opt_begin adopts
    e_ref, g = hostapi.fermion_exact_sum(st, cfgs, 16, 1.0, 0.0, batch=16, dtype=dtype)
    energies, stored = hostapi.fermion_optimize_exact_sum(st, cfgs, 16, "spinless", (1.0, 0.0, 0.0), "sgd", lr, SGD0, 1, dtype=dtype, batch=16)
    tol = 4 * EPS64 * float(np.max(np.abs(theta))) + (16 * EPS32 * lr * float(np.max(np.abs(g))) if dt == "f32" else 0.0)
    err = float(np.max(np.abs(stored - (theta - lr * g))))
    print("shape %s %s: max |theta_1 - (theta - lr fold g)| = %.3e (tol %.3e)  |E - E_ref| = %.3e" % (shape, dt, err, tol, abs(energies[0] - e_ref)))
    assert err <= tol
    assert np.count_nonzero(g) > 0.9 * np.count_nonzero(fref.allowed_flat(st))
    assert np.all(stored[~fref.allowed_flat(st)] == 0)
    # the same step through the C ABI: set (projection), step, a second begin on the stepped context, amplitudes
    n = len(cfgs)
    ctx = capi.Context(rows, cols, D, 4 * st.d, 16, dtype=dtype, max_walkers=n)
    ctx.state_upload(st.extended_flat())
    ctx.fermion_decoration_set(st)
    ctx.opt_begin()
    x = np.random.default_rng(5).standard_normal(st.extended_flat().shape)
    ctx.opt_set_gradient(x)
    assert np.array_equal(ctx.opt_get_gradient(), fref.project(st, x))       # Pi, bit for bit, at every block of every slot
    ctx.opt_set_gradient(fref.decorate(st, g) / 4)                            # Pi (E g / 4) = E g
    assert np.array_equal(ctx.opt_get_gradient(), fref.decorate(st, g))
    nrm = ctx.opt_clip(0.0, 0.0)
    assert abs(nrm - opt_ref.norm([g])) <= 1e-13 * opt_ref.norm([g])        # the stored norm
    ctx.opt_step(0, lr, SGD0)
    stepped = ctx.opt_read_state()
    assert np.array_equal(stepped, fref.decorate(st, stepped[:, :, :st.d]))
    assert float(np.max(np.abs(stepped[:, :, :st.d] - (theta - lr * g)))) <= 4 * EPS64 * float(np.max(np.abs(theta)))
    ctx.opt_begin()                                                           # the device state (float32: float(E theta)) passes the check
    assert np.array_equal(ctx.opt_read_state(), stepped.astype(np.float32).astype(np.float64) if dt == "f32" else stepped)
    amp = fermion.evaluate_amplitude(ctx, st, cfgs)
    ctx.close()
    new = fermion.FermionState.from_stored(st, stepped[:, :, :st.d])
    fresh = capi.Context(rows, cols, D, 4 * st.d, 16, dtype=dtype, max_walkers=n)
    fresh.state_upload(new.extended_flat())
    amp_fresh = fermion.evaluate_amplitude(fresh, new, cfgs)
    fresh.close()
    rel = float(np.max(np.abs(amp - amp_fresh) / np.abs(amp_fresh)))
    print("shape %s %s: amplitudes of the stepped context against a fresh upload: rel %.3e" % (shape, dt, rel))
    assert rel <= (1e-12 if dt == "f64" else 1e-5)


def test_sr_solves_in_the_stored_parameters(fixtures_dir):
    """(E^T S_ext E + shift) x = g on vectors in the range of E: Pi(S_ext x^) + shift x^ = g^, checked with the entry points that exist
    without the decoration (sr_sum, sr_matvec) and the NumPy projection; then the SR step of the host layer."""
    from peps_amd import hostapi
    st = _load(fixtures_dir, "spinless_fermion_tps_t2_0.000000_double_from_simple_update")
    cfgs = _half_filling()
    n, shift = len(cfgs), 1e-3
    ctx, es, ws = _accumulated_context(st, cfgs, 8, "spinless", (1.0, 0.0, 0.0), exact_sum=False, sr=True)
    ctx.fermion_decoration_set(st)
    ctx.opt_begin()
    e0, g_norm = ctx.opt_gradient_from_accumulators(es, ws)
    g_hat = ctx.opt_get_gradient()
    res, it, why, x_norm = ctx.opt_natural_gradient(shift, 200, 1e-10, 0.0, 20, 0.5)
    x_hat = ctx.opt_get_gradient()
    mean = ctx.sr_sum() / n
    s_x = ctx.sr_matvec(x_hat, float(np.sum(mean * x_hat)), 1.0 / n)
    # the host-vector solve ignores the decoration: same bytes with it set (here) and cleared (below)
    b = np.random.default_rng(2).standard_normal(g_hat.shape) * (g_hat != 0)
    with_dec = ctx.sr_cg_solve(b, None, shift, 50, 1e-8, 0.0, 20, 0.5)
    ctx.opt_end()
    ctx.fermion_decoration_set(None)
    without_dec = ctx.sr_cg_solve(b, None, shift, 50, 1e-8, 0.0, 20, 0.5)
    ctx.close()
    assert with_dec[0].tobytes() == without_dec[0].tobytes() and with_dec[1:] == without_dec[1:]
    resid = fref.project(st, s_x) + shift * x_hat - g_hat
    gn = float(np.linalg.norm(g_hat.ravel()))
    print("SR: CG iterations %d reason %d, |Pi(S x) + shift x - g| / |g| = %.3e, reported residual %.3e, |x| %.6e"
          % (it, why, float(np.linalg.norm(resid.ravel())) / gn, res, x_norm))
    assert why == 0 and 0 < it <= 200
    assert float(np.linalg.norm(resid.ravel())) <= 1e-8 * gn
    assert float(np.max(np.abs(fref.project(st, x_hat) - 4 * x_hat))) <= 8 * EPS64 * float(np.max(np.abs(x_hat)))
    x = x_hat[:, :, :st.d]
    xn = float(np.linalg.norm(x.ravel()))
    assert abs(x_norm - xn) <= 1e-12 * xn and abs(g_norm - 0.5 * gn) <= 1e-12 * gn      # stored norms
    theta = fref.stored_flat(st)
    lr = 0.05
    for normalize in (False, True):
        stored, info = hostapi.fermion_sr_step_samples(st, cfgs, 8, "spinless", (1.0, 0.0, 0.0), lr, shift, 200, 1e-10, normalize, dtype=F64)
        step = lr / xn if normalize else lr
        err = float(np.max(np.abs(stored - (theta - step * x))))
        print("SR step (normalize %d): CG iterations %d, |x| %.12e / %.12e, max |theta - ref| = %.3e, E %.12f -> %.12f"
              % (normalize, info["cg_iterations"], info["direction_norm"], xn, err, info["energy_before"], info["energy_after"]))
        assert err <= 1e-9 * step * float(np.max(np.abs(x)))
        assert abs(info["energy_before"] - e0) < 1e-12
        assert np.isfinite(info["energy_after"]) and info["energy_after"] < info["energy_before"]
        assert np.all(stored[~fref.allowed_flat(st)] == 0)


def test_bosonic_cg_solve_is_untouched(fixtures_dir):
    """pepsgpu_sr_cg_solve on the transverse-field Ising fixture: the same bytes before and after a decoration was offered to the context
    (refused there: phys_dim = 2 is no 4 d) and cleared"""
    from oracle import qlten_io, vmc
    from peps_amd import capi, fermion, hostapi, synthetic
    from peps_amd.capi import LEFT, RIGHT, UP, DOWN, HORIZONTAL
    s = qlten_io.load_sitps(os.path.join(fixtures_dir, "transverse_ising_tps_double_from_simple_update"))
    flat, cfgs = synthetic.sitps_to_flat(s, 4), np.array(vmc.generate_all_binary_configs(2, 2), dtype=np.int32)
    amps, en, _, _ = hostapi.energy_and_holes(flat, cfgs, 8, "tfim", (1.0,), False, F64)
    ctx = capi.Context(2, 2, 4, 2, 8, dtype=capi.F64, max_walkers=16)
    ctx.state_upload(flat)
    ctx.set_configs(cfgs)
    ctx.generate_bmps_approach(UP)
    for row in range(2):
        ctx.init_bten(LEFT, row)
        ctx.grow_full_bten(RIGHT, row, 1, True)
        for col in range(2):
            ctx.punch_hole_store(row, col, HORIZONTAL)
            if col < 1:
                ctx.shift_bten_window(RIGHT)
        if row < 1:
            ctx.shift_bmps_window(DOWN)
    ctx.sr_begin(16)
    ctx.sr_append(amps)
    b = np.random.default_rng(4).standard_normal(flat.shape) * (flat != 0)
    first = ctx.sr_cg_solve(b, None, 1e-3, 100, 1e-6, 0.0, 20, 0.5)
    with pytest.raises(ValueError):
        ctx.fermion_decoration_set(fermion.random_even_state(2, 2, 4, 1))
    ctx.fermion_decoration_set(None)
    second = ctx.sr_cg_solve(b, None, 1e-3, 100, 1e-6, 0.0, 20, 0.5)
    ctx.close()
    assert first[2] > 0 and first[0].tobytes() == second[0].tobytes() and first[1:] == second[1:]


def test_refusals_leave_the_context_usable(fixtures_dir):
    from peps_amd import capi, fermion
    st = fermion.random_even_state(2, 3, 3, seed=2)
    cfgs = _seeded_configs(2, 3, 2, 4, 1)
    ext = st.extended_flat()
    ctx = capi.Context(2, 3, 3, 4 * st.d, 9, dtype=capi.F64, max_walkers=4)
    ctx.state_upload(ext)
    ref = fermion.evaluate_amplitude(ctx, st, cfgs)

    def usable():
        assert np.allclose(fermion.evaluate_amplitude(ctx, st, cfgs), ref, rtol=1e-12, atol=0.0)

    wrong_d = fermion.FermionState([[t + t[:1] for t in row] for row in st.tensors], st.par, [1, 0, 1])     # d = 3: phys_dim != 4 d
    with pytest.raises(ValueError):
        ctx.fermion_decoration_set(wrong_d)
    usable()
    bad_par = fermion.FermionState.from_stored(st, fref.stored_flat(st))
    bad_par.par = [[tuple(np.array(p) for p in site) for site in row] for row in st.par]
    bad_par.par[0][1][0][1] = 2                                               # left leg of site (0, 1), a live entry
    with pytest.raises(ValueError):
        ctx.fermion_decoration_set(bad_par)
    usable()
    ctx.fermion_decoration_set(st)
    ctx.opt_begin()
    with pytest.raises(ValueError):                                           # optimizer buffers exist
        ctx.fermion_decoration_set(st)
    with pytest.raises(ValueError):
        ctx.fermion_decoration_set(None)
    ctx.opt_end()
    usable()
    # a state that is not a decoration: one variant's entry perturbed, then a forbidden entry non-zero
    allowed = fref.allowed_flat(st)
    k = tuple(np.argwhere(allowed[1, 1, 0])[3])
    perturbed = ext.copy()
    perturbed[(1, 1, 0 + st.d * 2) + k] *= 1.0 + 2 * EPS64
    forbidden = ext.copy()
    kf = tuple(np.argwhere(~allowed[0, 2, 1, :1, :3, :1, :1])[0])
    forbidden[(0, 2, 1) + kf] = 1e-300
    for bad, site in ((perturbed, "(1, 1)"), (forbidden, "(0, 2)")):
        ctx.state_upload(bad)
        with pytest.raises(ValueError, match=r"site \(%s\)" % site[1:-1]):
            ctx.opt_begin()
        with pytest.raises(RuntimeError):                                     # no buffer was kept
            ctx.opt_read_state()
    ctx.state_upload(ext)
    ctx.opt_begin()
    assert np.array_equal(ctx.opt_read_state(), ext)
    ctx.opt_end()
    ctx.fermion_decoration_set(None)
    usable()
    ctx.close()

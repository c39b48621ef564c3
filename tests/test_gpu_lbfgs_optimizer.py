"""L-BFGS in the Optimizer of the C++ host layer (LBFGSParams, peps_amd/host/qlpeps_gpu.h) on device buffers, driven through
hostapi.lbfgs_optimize_exact_sum / fermion_lbfgs_optimize_exact_sum: the whole loop, line searches included, in one C++ call.  Checked
against the reference's criteria on its 2x2 exact-summation fixtures (test_optimizer_lbfgs_exact_sum.cpp) and, step length by step
length, against the NumPy restatement tests/lbfgs_ref.py driven by the oracle's evaluator (bosons) or by the existing host path
hostapi.fermion_exact_sum (fermions)."""
import itertools
import os
import sys

import numpy as np
import pytest

from oracle import qlten_io, vmc
from peps_amd import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_ref as L  # noqa: E402
import opt_fermion_ref as fref  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = 1
EPS = 2.0 ** -52
# The suite's measured float64 energy deviation of the device against the oracle (tests/test_gpu_optimizer.py), amplified by the
# line search as measured on the CPU from the restatement alone (lbfgs_ref.AMPLIFICATION = 2.85: seeded relative noise of 1e-10 on every
# evaluated energy and gradient element moves the first eight energies of settings A and B by at most 2.85e-10 |E|), times ten; the
# floor is the rounding of E itself; never looser than 1e-7.
MEASURED_ENERGY_DEV = 1.776e-15


def energy_tolerance(e):
    return min(max(10 * L.AMPLIFICATION * MEASURED_ENERGY_DEV, 8 * EPS * abs(e)), 1e-7)


@pytest.fixture(scope="module")
def tfim(fixtures_dir):
    s = qlten_io.load_sitps(os.path.join(fixtures_dir, "transverse_ising_tps_double_from_simple_update"))
    return s, synthetic.sitps_to_flat(s, 4), np.array(vmc.generate_all_binary_configs(2, 2), dtype=np.int32)


@pytest.fixture(scope="module")
def heisenberg(fixtures_dir):
    s = qlten_io.load_sitps(os.path.join(fixtures_dir, "heisenberg_tps_double_from_simple_update"))
    return s, synthetic.sitps_to_flat(s, 4), np.array(vmc.generate_all_permutation_configs([2, 2], 2, 2), dtype=np.int32)


_REF = {}


def _ref(s, key, p, lr, iterations, **stop):
    """the restatement on the oracle's TFIM evaluator, once per setting"""
    if key not in _REF:
        evaluate, theta0, _ = L.oracle_evaluator(s, "tfim")
        _REF[key] = L.optimize(evaluate, theta0, p, lr, iterations, **stop)
    return _REF[key]


@pytest.mark.parametrize("which", ["tfim", "xxz"])
def test_reference_setting_meets_the_reference_criteria(request, which):
    """CreateStrongWolfeLBFGSParams with lr 0.05 / 140 iterations / patience 80 (TFIM, :341-342) and lr 0.1 / 80 / 60 (Heisenberg, :274-275)"""
    from peps_amd import hostapi
    s, flat, cfgs = request.getfixturevalue("tfim" if which == "tfim" else "heisenberg")
    params, lr, iters, patience, e0 = ((1.0,), 0.05, 140, 80, L.TFIM_E0) if which == "tfim" else ((1.0, 1.0, 0.0), 0.1, 80, 60, L.HEISENBERG_E0)
    r = hostapi.lbfgs_optimize_exact_sum(flat, cfgs, 8, which, params, lr, L.reference_setting(), iters, plateau_patience=patience,
                                         dtype=F64, batch=16, **L.REFERENCE_STOP)
    e = float(r["energies"][-1])
    print("%s: %d iterations, %d line-search evaluations, E - E0 = %.3e, counters %d %d %d" % (
        which, len(r["steps"]), r["line_search_evaluations"], e - e0, r["skip_curvature"], r["damping"], r["descent_reset"]))
    assert len(r["energies"]) == len(r["steps"]) + 1 == len(r["grad_norms"])
    assert e >= e0 - 1e-10 and abs(e - e0) < 1e-5
    state = r["state"]
    e_again, _ = hostapi.exact_sum_finish(hostapi.exact_sum_partial(state, cfgs, 8, which, params, 0, 1, 16, F64), flat.shape)
    print("%s: |E(re-uploaded state) - E[-1]| = %.3e" % (which, abs(e_again - e)))
    assert abs(e_again - e) < 1e-12
    assert np.all(state[flat == 0] == 0)


@pytest.mark.parametrize("name", ["A", "B"])
def test_step_lengths_and_energies_follow_the_restatement(tfim, name):
    """A: zoom; B: zoom, bracket doubling and history eviction.  The first eight step lengths equal the restatement's exactly."""
    from peps_amd import hostapi
    s, flat, cfgs = tfim
    (p, lr), steps = (L.SETTING_A, L.STEPS_A) if name == "A" else (L.SETTING_B, L.STEPS_B)
    ref = _ref(s, name, p, lr, 8, **L.REFERENCE_STOP)
    r = hostapi.lbfgs_optimize_exact_sum(flat, cfgs, 8, "tfim", (1.0,), lr, p, 8, dtype=F64, batch=16, **L.REFERENCE_STOP)
    de = np.abs(r["energies"][:8] - np.array(ref["energies"][:8]))
    tol = energy_tolerance(ref["energies"][0])
    print("setting %s: steps %s, max |E - ref| over the first eight = %.3e (tolerance %.3e), line-search evaluations %d (ref %d)"
          % (name, list(r["steps"]), float(de.max()), tol, r["line_search_evaluations"], ref["line_search_evaluations"]))
    assert ref["steps"][:8] == steps
    assert list(r["steps"][:8]) == steps
    assert r["line_search_evaluations"] == ref["line_search_evaluations"]
    assert float(de.max()) <= tol


def test_failed_search_raises_and_restores_or_falls_back(tfim):
    from peps_amd import hostapi
    s, flat, cfgs = tfim
    p, lr = L.SETTING_FAIL
    with pytest.raises(RuntimeError) as err:
        hostapi.lbfgs_optimize_exact_sum(flat, cfgs, 8, "tfim", (1.0,), lr, p, 3, dtype=F64, batch=16)
    assert isinstance(err.value, hostapi.LineSearchError)
    assert err.value.state.tobytes() == flat.tobytes()                       # theta_base bit for bit: the start
    r = hostapi.lbfgs_optimize_exact_sum(flat, cfgs, 8, "tfim", (1.0,), lr, p.replace(allow_fallback_to_fixed_step=True), 1, dtype=F64, batch=16)
    assert list(r["steps"]) == [max(p.min_step, lr * p.fallback_fixed_step_scale)] and r["line_search_evaluations"] == 2
    assert r["energies"][1] < r["energies"][0]


def test_fixed_step_mode_follows_the_restatement(tfim):
    from peps_amd import hostapi
    s, flat, cfgs = tfim
    p = L.LBFGSParams()
    ref = _ref(s, "fixed", p, 0.05, 5)
    r = hostapi.lbfgs_optimize_exact_sum(flat, cfgs, 8, "tfim", (1.0,), 0.05, p, 5, dtype=F64, batch=16)
    de = float(np.max(np.abs(r["energies"] - np.array(ref["energies"]))))
    dth = float(np.max(np.abs(r["state"] - synthetic.sitps_to_flat(L.oracle_evaluator(s, "tfim")[2](ref["theta"]), 4))))
    print("fixed step: max |E - ref| = %.3e, max |theta_5 - ref| = %.3e, E = %s" % (de, dth, r["energies"]))
    assert list(r["steps"]) == [0.05] * 5 and r["line_search_evaluations"] == 0
    assert de <= energy_tolerance(ref["energies"][0])
    assert dth <= 1e-9                                                     # the suite's gradient parity per element
    assert r["energies"][5] < r["energies"][0] - 1e-3


def test_parameter_checks(tfim):
    from peps_amd import hostapi
    s, flat, cfgs = tfim
    ok = L.reference_setting()
    for bad in (dict(wolfe_c1=0.0), dict(wolfe_c2=1e-4), dict(wolfe_c2=1.0), dict(max_eval=0), dict(tolerance_grad=-1.0), dict(history_size=0),
                dict(history_size=33)):
        with pytest.raises(ValueError):
            hostapi.lbfgs_optimize_exact_sum(flat, cfgs, 8, "tfim", (1.0,), 0.05, ok.replace(**bad), 1, dtype=F64, batch=16)
    with pytest.raises(ValueError):
        hostapi.lbfgs_optimize_exact_sum(flat, cfgs, 8, "tfim", (1.0,), 0.05, {"no_such_field": 1}, 1)


def test_complex_twin_follows_the_real_run(tfim):
    """the QLTEN_Complex instantiation on the same (real-valued) state through setting A's zoom: same energies, no imaginary part"""
    from peps_amd import hostapi
    s, flat, cfgs = tfim
    p, lr = L.SETTING_A
    rr = hostapi.lbfgs_optimize_exact_sum(flat, cfgs, 8, "tfim", (1.0,), lr, p, 4, dtype=F64, batch=16)
    rc = hostapi.lbfgs_optimize_exact_sum(flat.astype(np.complex128), cfgs, 8, "tfim", (1.0,), lr, p, 4, batch=16)
    ec, sc = rc["energies"], rc["state"]
    print("complex twin: max |Re E - E_real| = %.3e, max |Im E| = %.3e, steps %s" % (
        float(np.max(np.abs(ec.real - rr["energies"]))), float(np.max(np.abs(ec.imag))), list(rc["steps"])))
    assert ec.dtype == np.complex128 and sc.dtype == np.complex128
    assert list(rc["steps"]) == list(rr["steps"])
    assert np.max(np.abs(ec.real - rr["energies"])) < 1e-10 and np.max(np.abs(ec.imag)) < 1e-10 and np.max(np.abs(sc.imag)) < 1e-10


# ---- fermions: the spinless t2 = 0 fixture at half filling, E0 = -2 (test_optimizer_lbfgs_exact_sum.cpp:203-218) ----
def _half_filling():
    return np.array([np.array(p).reshape(2, 2) for p in sorted(set(itertools.permutations([0, 0, 1, 1])))], dtype=np.int32)


@pytest.fixture(scope="module")
def spinless(fixtures_dir):
    from peps_amd import fermion
    return fermion.FermionState.load(os.path.join(fixtures_dir, "spinless_fermion_tps_t2_0.000000_double_from_simple_update"), False)


def test_fermionic_run_meets_the_reference_criteria(spinless):
    from peps_amd import fermion, hostapi
    cfgs = _half_filling()
    r = hostapi.fermion_lbfgs_optimize_exact_sum(spinless, cfgs, 8, "spinless", (1.0, 0.0, 0.0), 0.05, L.reference_setting(), 140,
                                                 plateau_patience=80, dtype=F64, **L.REFERENCE_STOP)
    e = float(r["energies"][-1])
    print("fermions: %d iterations, %d line-search evaluations, E + 2 = %.3e" % (len(r["steps"]), r["line_search_evaluations"], e + 2))
    assert abs(e + 2.0) < 1e-5 and e >= -2.0 - 1e-10
    final = fermion.FermionState.from_stored(spinless, r["state"])
    e_again, _ = hostapi.fermion_exact_sum(final, cfgs, 8, 1.0, 0.0, dtype=F64)
    assert abs(e_again - e) < 1e-12
    assert np.all(r["state"][~fref.allowed_flat(spinless)] == 0)


def test_fermionic_first_iterations_follow_the_host_path(spinless):
    """five iterations against lbfgs_ref driven by hostapi.fermion_exact_sum (gradient read back and folded in NumPy): 1e-9 per
    element on the stored tensors, the bound of the existing fermionic trajectory tests"""
    from peps_amd import fermion, hostapi
    cfgs = _half_filling()

    def evaluate(theta):
        e, g = hostapi.fermion_exact_sum(fermion.FermionState.from_stored(spinless, theta[0]), cfgs, 8, 1.0, 0.0, dtype=F64)
        return float(np.real(e)), [np.asarray(g)]

    p, lr = L.reference_setting(), 0.05
    ref = L.optimize(evaluate, [fref.stored_flat(spinless)], p, lr, 5, **L.REFERENCE_STOP)
    r = hostapi.fermion_lbfgs_optimize_exact_sum(spinless, cfgs, 8, "spinless", (1.0, 0.0, 0.0), lr, p, 5, dtype=F64, **L.REFERENCE_STOP)
    dth = float(np.max(np.abs(r["state"] - ref["theta"][0])))
    de = float(np.max(np.abs(r["energies"] - np.array(ref["energies"]))))
    dn = float(np.max(np.abs(r["grad_norms"] - np.array(ref["grad_norms"]))))
    print("fermions, five iterations: steps %s (ref %s), max |theta - ref| = %.3e, max |E - ref| = %.3e, max ||g| - ref| = %.3e"
          % (list(r["steps"]), ref["steps"], dth, de, dn))
    assert list(r["steps"]) == ref["steps"]
    assert dth <= 1e-9 and dn <= 1e-9
    assert abs(ref["energies"][5] - ref["energies"][0]) > 1e-6

"""The NumPy restatement of the reference's L-BFGS (tests/lbfgs_ref.py) on its own: the three scalar behaviour tests of the reference
(test_optimizer_lbfgs_exact_sum.cpp:413-578) case by case, the exact-summation runs on the reference's 2x2 fixtures driven by the
oracle's evaluator, the step-length sequences that exercise the zoom, the bracket doubling and the history eviction, and the agreement
of the coefficient-space two-loop recursion (what the device runs) with the sequential one.  Nothing of the product is involved."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_ref as L  # noqa: E402

TFIM = "transverse_ising_tps_double_from_simple_update"
HEISENBERG = "heisenberg_tps_double_from_simple_update"


def scalar_evaluator(f, df):
    def evaluate(theta):
        x = float(theta[0][0])
        return f(x), [np.array([df(x)])]
    return evaluate


def test_strong_wolfe_conditions_hold_on_a_convex_quadratic():
    """SatisfiesStrongWolfeOnConvexQuadratic (:413-474)"""
    p = L.LBFGSParams(5, 1e-12, 1e-14, 64, L.STRONG_WOLFE, 1e-4, 0.9, 1e-8, 1.0, 1e-12, True, 1e3, False, 0.2)
    seen = []

    def evaluate(theta):
        x = float(theta[0][0])
        seen.append(x)
        return 0.5 * (x - 2.0) ** 2, [np.array([x - 2.0])]

    r = L.optimize(evaluate, [np.array([1.0])], p, 0.5, 2)
    assert len(r["energies"]) == 3 and len(r["steps"]) == 2
    x0, alpha = 1.0, r["steps"][0]
    g0 = x0 - 2.0
    d0 = -g0
    assert abs(d0 - 1.0) < 1e-12                  # the first L-BFGS step is steepest descent
    x1 = x0 + alpha * d0
    assert x1 in seen
    phi0, dphi0 = 0.5 * (x0 - 2.0) ** 2, g0 * d0
    phi_alpha, dphi_alpha = 0.5 * (x1 - 2.0) ** 2, (x1 - 2.0) * d0
    assert phi_alpha <= phi0 + p.wolfe_c1 * alpha * dphi0 + 1e-12
    assert abs(dphi_alpha) <= -p.wolfe_c2 * dphi0 + 1e-12


def test_tolerance_grad_floor_can_relax_the_curvature_acceptance():
    """ToleranceGradFloorCanRelaxCurvatureAcceptance (:476-528): tolerance_grad 0 fails the one allowed trial, 1e-16 accepts it"""
    evaluate = scalar_evaluator(lambda x: 0.5 * (x - 2.0) ** 2, lambda x: x - 2.0)

    def params(tol_grad):
        return L.LBFGSParams(5, tol_grad, 1e-14, 1, L.STRONG_WOLFE, 1e-4, 0.9, 0.05, 0.05, 1e-12, True, 1e3, False, 0.2)

    with pytest.raises(L.LineSearchFailed):
        L.optimize(evaluate, [np.array([2.0 + 1e-8])], params(0.0), 0.05, 1)
    r = L.optimize(evaluate, [np.array([2.0 + 1e-8])], params(1e-16), 0.05, 1)
    assert len(r["energies"]) == 2 and np.isfinite(r["energies"][-1]) and r["steps"] == [0.05]


def test_failure_throws_unless_the_fallback_is_enabled():
    """FailureThrowsUnlessFallbackEnabled (:530-578): the fallback step is max(min_step, lr * fallback_fixed_step_scale)"""
    evaluate = scalar_evaluator(lambda x: x * x, lambda x: 2.0 * x)
    strict = L.LBFGSParams(5, 1e-12, 1e-14, 1, L.STRONG_WOLFE, 1e-4, 0.9, 0.1, 10.0, 1e-12, True, 1e3, False, 0.05)
    with pytest.raises(L.LineSearchFailed) as err:
        L.optimize(evaluate, [np.array([1.0])], strict, 10.0, 1)
    assert err.value.theta[0][0] == 1.0
    r = L.optimize(evaluate, [np.array([1.0])], strict.replace(allow_fallback_to_fixed_step=True), 10.0, 2)
    assert r["energies"] and np.isfinite(r["energies"][-1])
    assert r["steps"][0] == max(0.1, 10.0 * 0.05)


def test_parameter_checks():
    """:1559-1568 and history_size == 0"""
    evaluate = scalar_evaluator(lambda x: x * x, lambda x: 2.0 * x)
    ok = L.reference_setting()
    for bad in (dict(wolfe_c1=0.0), dict(wolfe_c1=1.0), dict(wolfe_c2=1e-4), dict(wolfe_c2=1.0), dict(max_eval=0), dict(tolerance_grad=-1.0),
                dict(history_size=0)):
        with pytest.raises(ValueError):
            L.optimize(evaluate, [np.array([1.0])], ok.replace(**bad), 0.1, 1)


def test_damping_skip_descent_reset_and_norm_cap_branches():
    rng = np.random.default_rng(3)
    p = L.LBFGSParams(history_size=2, min_curvature=1e-3)
    st = L.State()
    th0, g0 = [rng.standard_normal(7)], [rng.standard_normal(7)]
    st.anchor_theta, st.anchor_g = th0, g0
    s = rng.standard_normal(7)
    # <s, y> < 0: damping lifts it above min_curvature only when delta / <y,y> |s|^2 does; here y = -0.5 s / |s|^2 ...
    y = -0.5 * s / np.dot(s, s)
    oc, cv = L.update_history(st, [th0[0] + s], [g0[0] + y], p)
    assert oc == L.PUSHED_DAMPED and cv > p.min_curvature and st.damping == 1 and len(st.history) == 1
    # ... without damping the same pair is skipped
    st2 = L.State()
    st2.anchor_theta, st2.anchor_g = th0, g0
    oc, cv = L.update_history(st2, [th0[0] + s], [g0[0] + y], p.replace(use_damping=False))
    assert oc == L.SKIPPED and cv < 0 and st2.skip_curvature == 1 and not st2.history
    # a gradient along -H g of a history with negative-definite action gives <g, d> >= 0: reset to -g
    st3 = L.State()
    st3.history = [(s, -s, 1.0 / -np.dot(s, s), -np.dot(s, s), np.dot(s, s))]        # (forced: such a pair is never pushed)
    st3.anchor_theta, st3.anchor_g = th0, g0
    d, dphi0, reset = L.search_direction(st3, [s], p.replace(min_curvature=-1e9))
    assert reset and st3.descent_reset == 1 and not st3.history and st3.anchor_theta is None
    assert np.array_equal(d[0], -s) and dphi0 == -np.dot(s, s)
    # the cap
    d = L.direction_sequential(L.State(), [s], p.replace(max_direction_norm=0.25))
    assert abs(np.linalg.norm(d[0]) - 0.25) < 1e-15


@pytest.fixture(scope="module")
def runs(fixtures_dir):
    """the four exact-summation runs, each once: name -> (result, largest relative deviation of the coefficient-space direction)"""
    from oracle import qlten_io
    out = {}
    for name, fixture, model, (p, lr), iters, patience in (
            ("tfim", TFIM, "tfim", (L.reference_setting(), 0.05), 140, 80),
            ("heisenberg", HEISENBERG, "xxz", (L.reference_setting(), 0.1), 80, 60),
            ("A", TFIM, "tfim", L.SETTING_A, 140, 80),
            ("B", TFIM, "tfim", L.SETTING_B, 140, 80)):
        evaluate, theta0, _ = L.oracle_evaluator(qlten_io.load_sitps(os.path.join(fixtures_dir, fixture)), model)
        dev = [0.0]

        def compare(st, g, p=p, dev=dev):
            a, b = L.direction_sequential(st, g, p), L.direction_coefficient(st, g, p)
            diff = [x - y for x, y in zip(a, b)]
            dev[0] = max(dev[0], np.sqrt(L.real_inner(diff, diff)) / np.sqrt(L.real_inner(a, a)))

        out[name] = (L.optimize(evaluate, theta0, p, lr, iters, plateau_patience=patience, on_direction=compare, **L.REFERENCE_STOP), dev[0])
    return out


@pytest.mark.parametrize("name,e0", [("tfim", L.TFIM_E0), ("heisenberg", L.HEISENBERG_E0)])
def test_reference_setting_reaches_the_exact_energy(runs, name, e0):
    """the two criteria of the reference's RunTestCase (:142-145)"""
    r, _ = runs[name]
    e = r["energies"][-1]
    print("%s: E - E0 = %.3e after %d evaluations, %d zoom entries" % (name, e - e0, len(r["energies"]) + r["line_search_evaluations"],
                                                                         r["zoom_entries"]))
    assert e >= e0 - 1e-10
    assert abs(e - e0) < 1e-5
    assert r["zoom_entries"] == 0 and r["doublings"] == 0        # c2 = 0.99 accepts every first trial: the search paths stay untouched


def test_setting_a_exercises_the_zoom(runs):
    r, _ = runs["A"]
    assert r["steps"][:8] == L.STEPS_A
    assert r["zoom_entries"] == 13 and r["converged"] and len(r["steps"]) == 14
    assert abs(r["energies"][-1] - L.TFIM_E0) < 1e-10


def test_setting_b_exercises_zoom_doubling_and_eviction(runs):
    r, _ = runs["B"]
    assert r["steps"][:8] == L.STEPS_B
    assert r["zoom_entries"] == 4 and r["doublings"] == 1 and r["converged"] and len(r["steps"]) == 22
    assert r["history"] == 3                                      # full from iteration 4 on: every later push evicts
    assert abs(r["energies"][-1] - L.TFIM_E0) < 1e-10


def test_failing_setting_fails_at_iteration_zero_after_two_trials(fixtures_dir):
    from oracle import qlten_io
    evaluate, theta0, _ = L.oracle_evaluator(qlten_io.load_sitps(os.path.join(fixtures_dir, TFIM)), "tfim")
    p, lr = L.SETTING_FAIL
    with pytest.raises(L.LineSearchFailed) as err:
        L.optimize(evaluate, theta0, p, lr, 3, **L.REFERENCE_STOP)
    assert err.value.iteration == 0 and err.value.trials == 2
    assert all(np.array_equal(a, b) for a, b in zip(err.value.theta, theta0))
    r = L.optimize(evaluate, theta0, p.replace(allow_fallback_to_fixed_step=True), lr, 1, **L.REFERENCE_STOP)
    assert r["steps"] == [max(p.min_step, lr * p.fallback_fixed_step_scale)]


def test_coefficient_space_direction_equals_the_sequential_one(runs):
    worst = max(dev for _, dev in runs.values())
    print("largest relative deviation of the coefficient-space direction: %.3e (recorded %.3e, gate %.3e)"
          % (worst, L.COEF_DEVIATION_MEASURED, L.COEF_GATE))
    assert worst <= L.COEF_GATE

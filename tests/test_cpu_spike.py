"""Spike recovery and the step selectors of the C++ host layer on the CPU (no device call): EMATracker, the SpikeGuard that
Optimizer::IterativeOptimize drives, the selection rules and the refusals, against the plain-Python restatement tests/spike_ref.py."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spike_ref  # noqa: E402

from peps_amd import hostapi  # noqa: E402

SGD0 = (0.0, 0.0, 0.0)
ADAM = (0.9, 0.999, 1e-8, 0.0)
SR = (1e-3, 50, 1e-5, 0)
MINSR = (1e-12, 0.0, 1)
LBFGS = None


def _rec(energy, error=0.01, gnorm=1.0, ngnorm=1.0, cg=10):
    return (energy, error, gnorm, ngnorm, cg)


def _smooth(n, start=-1.0, step=-0.01):
    return [_rec(start + step * k, 0.01 + 0.0001 * k, 1.0 + 0.01 * k, 2.0 + 0.01 * k, 10 + k) for k in range(n)]


def _check(records, algo, **cfg):
    """replay through the host layer and through the restatement; every discrete outcome equal, tracker values to 1e-14"""
    got = hostapi.spike_replay(records, algo, cfg)
    g, actions, iters, accepted, ema = spike_ref.replay(records, algo, **cfg)
    assert got["actions"] == actions
    assert list(got["iterations"]) == iters
    assert [(e["step"], e["attempt"], e["signal"], e["action"]) for e in got["events"]] == \
           [(e["step"], e["attempt"], e["signal"], e["action"]) for e in g.events]
    for a, b in zip(got["events"], g.events):
        for key in ("value", "threshold"):
            assert a[key] == pytest.approx(b[key], rel=1e-14, abs=0.0)
    assert (got["total_resamples"], got["total_rollbacks"], got["total_forced_accepts"]) == (g.resamples, g.rollbacks, g.forced)
    # the counters are the counts of the log
    for key, action in (("total_resamples", "RESAMPLE"), ("total_rollbacks", "ROLLBACK"), ("total_forced_accepts", "ACCEPT_WARN")):
        assert got[key] == sum(e["action"] == action for e in got["events"])
    np.testing.assert_allclose(got["ema"], np.array(ema), rtol=1e-14, atol=0.0)
    return got, accepted


@pytest.mark.parametrize("window", [1, 5, 50])
def test_ema_tracker(window):
    x = np.random.default_rng(window).standard_normal(200) * 3.0 - 1.0
    mean, var = hostapi.ema_track(x, window)
    ref = np.array(spike_ref.ema_series(list(x), window))
    np.testing.assert_allclose(mean, ref[:, 0], rtol=1e-14, atol=0.0)
    np.testing.assert_allclose(var, ref[:, 1], rtol=1e-14, atol=0.0)
    assert mean[0] == x[0] and var[0] == 0.0               # the first observation
    if window == 1:
        # alpha = 1: the tracker follows the series (mean + (x - mean) rounds twice) and 1 - alpha = 0 wipes the variance
        np.testing.assert_allclose(mean, x, rtol=0.0, atol=4 * 2.0 ** -52 * float(np.max(np.abs(x))))
        assert np.all(var == 0.0)
    # Reset: the series after it is tracked as a new one
    m2, v2 = hostapi.ema_track(x, window, reset_at=120)
    assert np.array_equal(m2[:120], mean[:120]) and m2[120] == x[120] and v2[120] == 0.0
    ref2 = np.array(spike_ref.ema_series(list(x[120:]), window))
    np.testing.assert_allclose(m2[120:], ref2[:, 0], rtol=1e-14, atol=0.0)
    np.testing.assert_allclose(v2[120:], ref2[:, 1], rtol=1e-14, atol=0.0)


def test_nothing_fires_at_iteration_zero_or_on_a_smooth_series():
    wild = [_rec(100.0, 1e9, 1e30, 1e30, 0)] + _smooth(5)
    got, _ = _check(wild, "sr", enable_rollback=True, factor_grad=2.0)
    assert got["actions"][0] == "ACCEPT" and not [e for e in got["events"] if e["step"] == 0]
    got, accepted = _check(_smooth(30), "sr", enable_rollback=True, factor_grad=2.0)
    assert got["events"] == [] and accepted == list(range(30))


def test_s1_needs_a_positive_error_average():
    zero = [_rec(-1.0 - 0.01 * k, 0.0) for k in range(3)] + [_rec(-1.1, 5.0)] + [_rec(-1.2, 0.0)]
    got, _ = _check(zero, "sgd")
    assert got["events"] == []                              # EMA(error) == 0: S1 is silent however large the error
    fire = _smooth(4) + [_rec(-1.05, 2.0)] + _smooth(2, -1.06)
    got, accepted = _check(fire, "sgd")
    assert [(e["signal"], e["action"]) for e in got["events"]] == [("S1_ERRORBAR", "RESAMPLE")]
    assert accepted == [0, 1, 2, 3, 5, 6] and got["actions"][4] == "RESAMPLE"
    just_below = _smooth(4) + [_rec(-1.05, 0.9)]            # 100 x EMA(error) is about 1.0
    got, _ = _check(just_below, "sgd")
    assert got["events"] == []


def test_s2_at_factor_grad():
    rec = _smooth(4) + [_rec(-1.05, 0.01, 3.5)] + [_rec(-1.05, 0.01, 1.04)]
    got, accepted = _check(rec, "adam", factor_grad=3.0)
    assert [(e["signal"], e["action"]) for e in got["events"]] == [("S2_GRAD_NORM", "RESAMPLE")] and accepted == [0, 1, 2, 3, 5]
    got, _ = _check(rec, "adam")                            # the default factor of 1e10 never fires here
    assert got["events"] == []


def test_s3_by_norm_by_iterations_and_never_on_iterations_for_minsr():
    by_norm = _smooth(4) + [_rec(-1.05, 0.01, 1.0, 40.0, 12)] + _smooth(1, -1.06)
    got, _ = _check(by_norm, "sr")
    assert [(e["signal"], e["action"]) for e in got["events"]] == [("S3_NGRAD_ANOMALY", "RESAMPLE")]
    by_iters = _smooth(4) + [_rec(-1.05, 0.01, 1.0, 2.0, 1)] + _smooth(1, -1.06)
    got, _ = _check(by_iters, "sr")
    assert [(e["signal"], e["action"]) for e in got["events"]] == [("S3_NGRAD_ANOMALY", "RESAMPLE")]
    got, _ = _check(by_iters, "sr", sr_min_iters_suspicious=0)
    assert got["events"] == []
    got, _ = _check(by_iters, "minsr")                      # no iterative solve: the count is not read
    assert got["events"] == []
    got, _ = _check(by_norm, "minsr")
    assert len(got["events"]) == 1
    got, _ = _check(by_norm, "sgd")                         # S3 belongs to SR and MinSR
    assert got["events"] == []


def test_s4_only_upward_and_only_with_a_spread():
    flat = [_rec(-1.0)] * 4 + [_rec(5.0)]
    got, _ = _check(flat, "sgd", enable_rollback=True, sigma_k=1.0)
    assert got["events"] == []                              # Std == 0
    down = _smooth(6) + [_rec(-50.0)]
    got, _ = _check(down, "sgd", enable_rollback=True, sigma_k=1.0)
    assert got["events"] == []
    up = _smooth(6) + [_rec(3.0)] + _smooth(3, -1.05)
    got, accepted = _check(up, "sgd", enable_rollback=True, sigma_k=3.0)
    assert [(e["signal"], e["action"], e["step"]) for e in got["events"]] == [("S4_ENERGY_SPIKE", "ROLLBACK", 6)]
    assert accepted == [0, 1, 2, 3, 4, 5, 7, 8, 9]
    got, _ = _check(up, "sgd", enable_rollback=False, sigma_k=3.0)
    assert got["events"] == []                              # S4 is opt-in


def test_retries_then_rollback_or_forced_accept():
    bad = _rec(-1.05, 9.0)
    rec = _smooth(4) + [bad, bad, bad] + _smooth(2, -1.06)
    got, accepted = _check(rec, "sgd")                      # no rollback: the third bad evaluation is accepted with a warning
    assert [e["action"] for e in got["events"]] == ["RESAMPLE", "RESAMPLE", "ACCEPT_WARN"]
    assert [e["attempt"] for e in got["events"]] == [0, 1, 2] and accepted == [0, 1, 2, 3, 6, 7, 8]
    assert got["actions"][6] == "ACCEPT_WARN"
    got, accepted = _check(rec + [_rec(-1.07)], "sgd", enable_rollback=True)
    assert [e["action"] for e in got["events"]] == ["RESAMPLE", "RESAMPLE", "ROLLBACK"]      # a base is saved: roll back instead
    # ... which consumes the base: three more bad evaluations right after it end in a forced accept
    again = _smooth(4) + [bad] * 6 + _smooth(1, -1.06)
    got, _ = _check(again, "sgd", enable_rollback=True)
    assert [e["action"] for e in got["events"]] == ["RESAMPLE", "RESAMPLE", "ROLLBACK", "RESAMPLE", "RESAMPLE", "ACCEPT_WARN"]
    got, _ = _check(rec, "sgd", redo_mc_max_retries=0)
    assert [e["action"] for e in got["events"]][:1] == ["ACCEPT_WARN"]
    got, _ = _check(rec, "sgd", enable_auto_recover=False)
    assert got["events"] == []


def test_rejected_evaluations_never_reach_the_trackers():
    clean = _smooth(8)
    dirty = clean[:4] + [_rec(7.0, 50.0, 1e3, 1e3, 0)] + clean[4:]
    a = hostapi.spike_replay(clean, "sr", {})
    b = hostapi.spike_replay(dirty, "sr", {})
    assert b["actions"][4] == "RESAMPLE"
    assert np.array_equal(b["ema"][4], b["ema"][3])         # untouched by the rejected record
    assert np.array_equal(np.delete(b["ema"], 4, axis=0), a["ema"])


def test_trigger_csv_byte_for_byte():
    rec = _smooth(4) + [_rec(-1.05, 2.0)] + _smooth(2, -1.06)
    got = hostapi.spike_replay(rec, "sgd", {})
    g, *_ = spike_ref.replay(rec, "sgd")
    assert got["csv"] == spike_ref.trigger_csv(g.events)
    lines = got["csv"].split("\n")
    assert lines[0] == "step,attempt,signal,action,value,threshold"
    thr = 100.0 * spike_ref.ema_series([r[1] for r in rec[:4]], 50)[-1][0]
    assert lines[1] == "4,0,S1_ERRORBAR,RESAMPLE,2.000000e+00,%.6e" % thr and lines[2] == ""


def test_selection_rules():
    # initial: the lowest energy, the first of equal ones
    assert hostapi.step_select("initial", [(0.1, -1.0, 0), (0.2, -1.5, 0), (0.3, -1.5, 0)], 0, 10, 0.1) == (0.2, 0.2)
    assert hostapi.step_select("initial", [(0.1, -1.0, 0), (0.2, -1.0, 0), (0.3, -0.5, 0)], 0, 10, 0.1) == (0.1, 0.1)
    assert hostapi.step_select("initial", [(0.1, -1.0, 0), (0.2, -0.9, 0), (0.3, -1.2, 0)], 0, 10, 0.1) == (0.3, 0.3)
    # periodic: early phase below ratio * max_iterations, late phase from it on
    small, large = [(0.1, -1.0, 0.05), (0.05, -1.01, 0.02)], [(0.1, -1.0, 0.05), (0.05, -1.2, 0.02)]
    rng = np.random.default_rng(0)
    cases = [(small, 2), (small, 3), (small, 9), (large, 2), (large, 3), (large, 9), ([(0.1, -1.0, 0.05), (0.05, -0.9, 0.02)], 1)]
    cases += [([(0.1, float(rng.normal()), abs(float(rng.normal()))), (0.05, float(rng.normal()), abs(float(rng.normal())))], int(rng.integers(1, 10)))
              for _ in range(40)]
    for res, it in cases:
        want = spike_ref.select_periodic(res, it, 10, 0.3)
        assert hostapi.step_select("periodic", res, it, 10, 0.1, 0.3) == (want, min(0.1, want))
    assert hostapi.step_select("periodic", small, 2, 10, 0.1, 0.3)[0] == 0.05        # early: any improvement halves
    assert hostapi.step_select("periodic", small, 3, 10, 0.1, 0.3)[0] == 0.1         # late (3 >= 0.3 * 10): 0.01 is below the error bar
    assert hostapi.step_select("periodic", large, 3, 10, 0.1, 0.3)[0] == 0.05
    # the base learning rate never grows under the periodic rule, whatever is selected
    base = 0.1
    for k in range(30):
        res = [(base, float(rng.normal()), 0.1), (base / 2, float(rng.normal()), 0.1)]
        sel, new = hostapi.step_select("periodic", res, k + 1, 40, base, 0.3)
        assert new <= base and new == spike_ref.next_base_lr("periodic", base, sel)
        base = new
    assert base < 0.1
    assert hostapi.step_select("periodic", [(0.1, -1.0, 0.0), (0.2, -2.0, 0.0)], 1, 10, 0.1, 0.3)[1] == 0.1     # (a larger eta cannot raise it)
    # the candidates
    assert list(hostapi.step_candidates("initial", 0.1, 3)) == spike_ref.candidates("initial", 0.1, 3) == [0.1, 0.2, 0.1 * 3.0]
    assert list(hostapi.step_candidates("periodic", 0.1)) == [0.1, 0.05]
    with pytest.raises(ValueError, match="Auto step selector requires positive candidate step sizes"):
        hostapi.step_candidates("periodic", 0.0)
    # non-finite trials
    for res, msg in (([(0.1, math.nan, 0.0)], "non-finite energy$"), ([(0.1, -1.0, math.inf)], "non-finite energy error$"),
                     ([(0.1, math.inf, math.nan)], "non-finite energy and energy error$")):
        with pytest.raises(RuntimeError, match="Step selector candidate evaluation produced " + msg):
            hostapi.step_select("initial", res, 0, 10, 0.1)


def test_acceptance_check():
    rates = [0.40, 0.19, 0.21, 0.0, 0.20, 0.41]
    assert hostapi.acceptance_rate_check(rates) == spike_ref.acceptance_flags(rates) == [1, 3, 4]
    assert hostapi.acceptance_rate_check([0.3, 0.3, 0.3]) == [] and hostapi.acceptance_rate_check([]) == []
    assert hostapi.acceptance_rate_check([0.0, 0.0]) == []


INITIAL = dict(initial=dict(enable_in_deterministic=True))
PERIODIC = dict(periodic=dict(every_n_steps=2))


@pytest.mark.parametrize("vmc", [False, True])
def test_refusals_need_no_device(vmc):
    kw = dict(n_walkers=4) if vmc else {}
    ok = [("sgd", SGD0, INITIAL), ("sr", SR, PERIODIC), ("minsr", MINSR, INITIAL), ("adam", ADAM, None)]
    for algo, rp, sel in ok:
        hostapi.validate_guards(algo, 0.1, rp, selectors=sel, **kw)
    for algo, rp in (("adam", ADAM), ("adagrad", (1e-8, 0.0)), ("lbfgs", LBFGS)):
        with pytest.raises(ValueError, match="Step selectors only support SGD, SR, and MinSR in IterativeOptimize"):
            hostapi.validate_guards(algo, 0.1, rp, selectors=INITIAL, **kw)
    with pytest.raises(ValueError, match="Step selectors cannot be used together with lr_scheduler in v1"):
        hostapi.validate_guards("sgd", 0.1, SGD0, selectors=PERIODIC, scheduler=True, **kw)
    hostapi.validate_guards("sgd", 0.1, SGD0, scheduler=True, **kw)          # a scheduler alone is fine
    with pytest.raises(ValueError, match="Initial step selector max_line_search_steps must be > 0"):
        hostapi.validate_guards("sgd", 0.1, SGD0, selectors=dict(initial=dict(max_line_search_steps=0)), **kw)
    with pytest.raises(ValueError, match="Auto step selector every_n_steps must be > 0"):
        hostapi.validate_guards("sgd", 0.1, SGD0, selectors=dict(periodic=dict(every_n_steps=0)), **kw)
    for ratio in (-0.1, 1.5):
        with pytest.raises(ValueError, match=r"Auto step selector phase_switch_ratio must be within \[0, 1\]"):
            hostapi.validate_guards("sgd", 0.1, SGD0, selectors=dict(periodic=dict(phase_switch_ratio=ratio)), **kw)
    with pytest.raises(ValueError, match="Step selectors require a positive base learning_rate"):
        hostapi.validate_guards("sgd", 0.0, SGD0, selectors=INITIAL, **kw)
    with pytest.raises(ValueError, match="rollback is not available with L-BFGS"):
        hostapi.validate_guards("lbfgs", 0.1, LBFGS, spike=dict(enable_rollback=True), **kw)
    hostapi.validate_guards("lbfgs", 0.1, LBFGS, spike=dict(), **kw)          # S1 / S2 resampling is


def test_guarded_entries_refuse_before_any_device_call():
    """the same refusals through the entries that would build a contractor next: they return before doing so (this test has no GPU)"""
    flat = np.zeros((2, 2, 2, 4, 4, 4, 4))
    cfgs = np.zeros((4, 2, 2), dtype=np.int32)
    with pytest.raises(ValueError, match="Step selectors only support"):
        hostapi.guarded_vmc_optimize(flat, cfgs, [1, 2, 3, 4], 8, "tfim", (1.0,), "fullspace", "adam", 0.1, ADAM, 2, selectors=INITIAL)
    with pytest.raises(ValueError, match="lr_scheduler"):
        hostapi.guarded_vmc_optimize(flat, cfgs, [1, 2, 3, 4], 8, "tfim", (1.0,), "fullspace", "sgd", 0.1, SGD0, 2, selectors=INITIAL, scheduler=True)
    with pytest.raises(ValueError, match="rollback is not available with L-BFGS"):
        hostapi.guarded_vmc_optimize(flat, cfgs, [1, 2, 3, 4], 8, "tfim", (1.0,), "fullspace", "lbfgs", 0.1, None, 2,
                                     spike=dict(enable_rollback=True))
    with pytest.raises(ValueError, match="Step selectors only support"):
        hostapi.guarded_optimize_exact_sum(flat, cfgs, 8, "tfim", (1.0,), "adam", 0.1, ADAM, 2, selectors=PERIODIC)
    with pytest.raises(ValueError, match="rollback is not available with L-BFGS"):
        hostapi.guarded_optimize_exact_sum(flat, cfgs, 8, "tfim", (1.0,), "lbfgs", 0.1, None, 2, spike=dict(enable_rollback=True))

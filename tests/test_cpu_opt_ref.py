"""The update rules of the device optimizer as restated in tests/opt_ref.py, driven by the oracle's exact-sum evaluator on the
reference's 2x2 transverse-field Ising state: each of the five rule settings meets the reference's own convergence criteria
(test_optimizer_adam_exact_sum.cpp:90-92) after 100 iterations; the learning-rate schedules against their closed forms."""
import os
import sys

import numpy as np
import pytest

from oracle import qlten_io

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import opt_ref  # noqa: E402

# energies after 100 iterations as first measured (the start is -5.19991995228, E0 = -5.2262518595)
MEASURED = {"adam": -5.2262513776, "adagrad": -5.2262504943, "sgd_momentum": -5.2262515260, "sgd_nesterov": -5.2262518118,
            "sgd_plain": -5.2262517923}


@pytest.mark.parametrize("name,rule,lr,params", opt_ref.SETTINGS, ids=[s[0] for s in opt_ref.SETTINGS])
def test_rule_converges_on_the_tfim_fixture(fixtures_dir, name, rule, lr, params):
    s = qlten_io.load_sitps(os.path.join(fixtures_dir, "transverse_ising_tps_double_from_simple_update"))
    energies, norms, _ = opt_ref.oracle_tfim_trajectory(s, rule, lr, params, 100)
    print(name, "E[0] = %.11f  E[100] = %.10f (first measured %.10f)  |g|[100] = %.3e" % (energies[0], energies[-1], MEASURED[name], norms[-1]))
    assert abs(energies[0] - (-5.19991995228)) < 1e-10
    e, e0 = energies[-1], opt_ref.TFIM_E0
    assert e >= e0 - 1e-10                      # variational
    assert abs(e - e0) < 1e-5


def test_clip_and_finish_identities():
    rng = np.random.default_rng(5)
    for cplx in (False, True):
        g = [rng.standard_normal((3, 4)) + (1j * rng.standard_normal((3, 4)) if cplx else 0) for _ in range(3)]
        assert opt_ref.clip(g)[0] is not g[0] and all(np.array_equal(a, b) for a, b in zip(opt_ref.clip(g), g))
        c = opt_ref.clip(g, clip_value=0.5)
        assert max(np.max(np.abs(x)) for x in c) <= 0.5 * (1 + 4e-16)
        for a, b in zip(c, g):          # the phase / sign is kept, small elements untouched
            small = np.abs(b) <= 0.5
            assert np.array_equal(a[small], b[small])
            assert np.allclose(a[~small] / np.abs(a[~small]), b[~small] / np.abs(b[~small]), rtol=0, atol=1e-15)
        r = opt_ref.norm(g)
        assert abs(opt_ref.norm(opt_ref.clip(g, clip_norm=r / 2)) - r / 2) < 1e-14 * r
        assert all(np.array_equal(a, b) for a, b in zip(opt_ref.clip(g, clip_norm=2 * r), g))
        so, seo = g, [x[::-1].copy() for x in g]
        es = (0.3 - 0.2j) if cplx else 0.3
        e, fin = opt_ref.finish(so, seo, es, 0.7)
        assert e == es / 0.7
        assert all(np.allclose(f, (b - np.conj(e) * a) / 0.7, rtol=0, atol=1e-15) for f, a, b in zip(fin, so, seo))


def test_first_steps_in_closed_form():
    """one step of each rule from a cleared state: Adam and AdaGrad (acc0 = 0) move every element by lr g / (|g| + eps)"""
    rng = np.random.default_rng(6)
    th, g = [rng.standard_normal(7)], [rng.standard_normal(7)]
    lr, eps = 0.03, 1e-8
    got = opt_ref.adam(th, g, opt_ref.RuleState(th), lr, 0.9, 0.999, eps)[0]
    assert np.max(np.abs(got - (th[0] - lr * g[0] / (np.abs(g[0]) + eps)))) < 1e-15
    got = opt_ref.adagrad(th, g, opt_ref.RuleState(th), lr, eps, 0.0)[0]
    assert np.max(np.abs(got - (th[0] - lr * g[0] / (np.abs(g[0]) + eps)))) < 1e-15
    st = opt_ref.RuleState(th)
    one = opt_ref.sgd(th, g, st, lr, momentum=0.9, nesterov=True, weight_decay=0.1)[0]
    assert np.max(np.abs(one - (th[0] * (1 - lr * 0.1) - lr * (0.9 * g[0] + g[0])))) < 1e-15
    two = opt_ref.sgd([one], g, st, lr, momentum=0.9)[0]
    assert np.max(np.abs(two - (one - lr * 1.9 * g[0]))) < 1e-15
    assert np.array_equal(opt_ref.sgd(th, g, opt_ref.RuleState(th), lr)[0], th[0] + (-lr) * g[0])


def test_lr_schedules_against_closed_forms():
    for it in (0, 1, 7, 100, 250):
        assert opt_ref.constant_lr(0.05, it) == 0.05
        assert opt_ref.exponential_decay_lr(0.1, 0.95, 100, it) == 0.1 * 0.95 ** (it / 100.0)
        assert opt_ref.step_lr(0.1, 100, 0.1, it) == 0.1 * 0.1 ** (it // 100)
    assert abs(opt_ref.exponential_decay_lr(0.1, 0.5, 10, 20) - 0.025) < 1e-17
    assert abs(opt_ref.step_lr(1.0, 3, 0.5, 7) - 0.25) < 1e-17


def test_host_layer_schedulers_against_closed_forms():
    """ConstantLR / ExponentialDecayLR / StepLR of the C++ host layer (peps_amd/host/qlpeps_gpu.h) through hostapi.lr_schedule; no device"""
    from peps_amd import hostapi
    if not os.path.exists(hostapi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    for it in (0, 1, 7, 99, 100, 250):
        assert hostapi.lr_schedule("constant", (0.05,), it) == 0.05
        assert abs(hostapi.lr_schedule("exponential", (0.1, 0.95, 100), it) - opt_ref.exponential_decay_lr(0.1, 0.95, 100, it)) < 1e-16
        assert abs(hostapi.lr_schedule("step", (0.1, 100, 0.1), it) - opt_ref.step_lr(0.1, 100, 0.1, it)) < 1e-16
    with pytest.raises(ValueError):
        hostapi.lr_schedule("step", (0.1, 100), 3)
    with pytest.raises(ValueError):
        hostapi.lr_schedule("exponential", (0.1, 0.9, 0), 3)

"""The initial and the periodic step selector of the device-resident Optimizer (optimizer_impl.h:320-542 of the reference) through
hostapi.guarded_optimize_exact_sum / fermion_guarded_optimize_exact_sum.  A trial is formed from the base of the step on the device
(pepsgpu_guard_preview), evaluated, and the base is put back (pepsgpu_guard_base_restore); the real step then starts from it.

Plain SGD and the exact-summation evaluator are stateless and a float64 state survives a host round trip unchanged, so every trial
and every step can be reproduced by a separate one-step run of existing code (hostapi.optimize_exact_sum, sr_step_samples) from the
same state: selections follow from those runs' energies through the restatement tests/spike_ref.py, and energies and states are
compared as bytes."""
import itertools
import os
import sys

import numpy as np
import pytest

from oracle import qlten_io, vmc
from peps_amd import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spike_ref  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = 1
TFIM = ("tfim", (1.0,))
SGD0 = (0.0, 0.0, 0.0)
INITIAL = dict(initial=dict(enable_in_deterministic=True))


def _host():
    from peps_amd import hostapi
    return hostapi


@pytest.fixture(scope="module")
def tfim(fixtures_dir):
    s = qlten_io.load_sitps(os.path.join(fixtures_dir, "transverse_ising_tps_double_from_simple_update"))
    return synthetic.sitps_to_flat(s, 4), np.array(vmc.generate_all_binary_configs(2, 2), dtype=np.int32)


def _one_step(flat, cfgs, lr, rp=SGD0):
    """(energy before, energy after, state after) of one unguarded step"""
    e, state = _host().optimize_exact_sum(flat, cfgs, 8, *TFIM, "sgd", lr, rp, 1, dtype=F64, batch=16)
    return e[0], e[1], state


@pytest.mark.parametrize("eta,rp", [(0.2, SGD0), (0.6, SGD0), (0.3, (0.9, 1.0, 1e-3))], ids=["eta0.2", "eta0.6", "nesterov_decay"])
def test_initial_selector_takes_the_argmin_of_three_separate_runs(tfim, eta, rp):
    flat, cfgs = tfim
    host = _host()
    etas = list(host.step_candidates("initial", eta, 3))
    runs = [_one_step(flat, cfgs, x, rp) for x in etas]
    want = spike_ref.select_initial([(x, r[1], 0.0) for x, r in zip(etas, runs)])
    chosen = runs[etas.index(want)]
    got = host.guarded_optimize_exact_sum(flat, cfgs, 8, *TFIM, "sgd", eta, rp, 1, selectors=INITIAL, dtype=F64, batch=16)
    print("initial selector from eta = %g: trial energies %s -> %g" % (eta, [float(r[1]) for r in runs], want))
    assert list(got["selected_eta"]) == [want]
    assert got["state"].tobytes() == chosen[2].tobytes()               # the state after iteration 0 is the chosen run's
    assert got["energies"].tobytes() == np.array([chosen[0], chosen[1]]).tobytes()      # no trial energy in the trajectory
    assert got["evaluator_calls"] == 1 + 3 + 1 and got["energy_only_calls"] == 0
    # in Monte-Carlo mode an evaluator without an error bar is refused, with the reference's words
    with pytest.raises(ValueError, match="Initial step selector requires positive energy error in MC mode"):
        host.guarded_optimize_exact_sum(flat, cfgs, 8, *TFIM, "sgd", eta, rp, 1, selectors=dict(initial={}), dtype=F64, batch=16)


@pytest.mark.parametrize("eta,err", [(0.2, 1e-3), (1.5, 1e-3), (1.5, 10.0)], ids=["eta0.2", "eta1.5", "eta1.5_wide_error"])
def test_periodic_selector_follows_the_restatement(tfim, eta, err):
    """every 2 iterations of 5, phase switch at 0.5 * 5: iteration 2 is judged by the early rule, iteration 4 by the late one with the
    scheduled error bar.  The expected run is put together from one-step runs of existing code."""
    flat, cfgs = tfim
    host = _host()
    its, every, ratio = 5, 2, 0.5
    state, lr = flat, eta
    energies, selected, calls = [], [], 0
    for it in range(its):
        sel = 0.0
        if it > 0 and it % every == 0:
            cands = spike_ref.candidates("periodic", lr)
            trials = [(x, float(_one_step(state, cfgs, x)[1]), err) for x in cands]
            sel = spike_ref.select_periodic(trials, it, its, ratio)
            lr = spike_ref.next_base_lr("periodic", lr, sel)
            sel = lr
            calls += 2
        before, after, state = _one_step(state, cfgs, lr)
        energies.append(before)
        selected.append(sel)
        calls += 1
    energies.append(after)
    calls += 1
    got = host.guarded_optimize_exact_sum(flat, cfgs, 8, *TFIM, "sgd", eta, SGD0, its, dtype=F64, batch=16,
                                          selectors=dict(periodic=dict(every_n_steps=every, phase_switch_ratio=ratio)),
                                          schedule=dict(error_override=np.full(calls, err)))
    print("periodic selector from eta = %g, error %g: selected %s" % (eta, err, selected))
    assert list(got["selected_eta"]) == selected
    assert got["evaluator_calls"] == calls == its + 1 + 2 * 2
    assert got["energies"].tobytes() == np.array(energies).tobytes()
    assert got["state"].tobytes() == state.tobytes()
    assert all(s == 0.0 or s <= eta for s in selected)


def test_sr_normalized_update_is_applied_once(tfim):
    flat, cfgs = tfim
    host = _host()
    eta, sr = 0.05, (1e-3, 100, 1e-4, 1)
    etas = list(host.step_candidates("initial", eta, 3))
    runs = [host.sr_step_samples(flat, cfgs, 8, *TFIM, x, sr[0], sr[1], sr[2], True, dtype=F64) for x in etas]
    want = spike_ref.select_initial([(x, r[1]["energy_after"], 0.0) for x, r in zip(etas, runs)])
    state, info = runs[etas.index(want)]
    got = host.guarded_optimize_exact_sum(flat, cfgs, 8, *TFIM, "sr", eta, sr, 1, selectors=INITIAL, dtype=F64)
    print("SR initial selector: |x| = %.6e, trial energies %s -> %g" % (info["direction_norm"], [r[1]["energy_after"] for r in runs], want))
    assert list(got["selected_eta"]) == [want]
    assert got["state"].tobytes() == state.tobytes()                   # eta / |x| once: twice would be another state
    assert (got["energies"][0], got["energies"][1]) == (info["energy_before"], info["energy_after"])
    assert (got["sr_iterations"], got["sr_natural_grad_norm"]) == (info["cg_iterations"], info["direction_norm"])
    assert info["direction_norm"] != 1.0


def test_fermionic_state(fixtures_dir):
    from peps_amd import fermion
    host = _host()
    st = fermion.FermionState.load(os.path.join(fixtures_dir, "spinless_fermion_tps_t2_0.000000_double_from_simple_update"))
    cfgs = np.array([np.array(p).reshape(2, 2) for p in sorted(set(itertools.permutations([0, 0, 1, 1])))], dtype=np.int32)
    model, eta = ("spinless", (1.0, 0.0, 0.0)), 0.1
    etas = list(host.step_candidates("initial", eta, 3))
    runs = [host.fermion_optimize_exact_sum(st, cfgs, 16, *model, "sgd", x, SGD0, 1, dtype=F64, batch=6) for x in etas]
    want = spike_ref.select_initial([(x, float(r[0][1]), 0.0) for x, r in zip(etas, runs)])
    e, stored = runs[etas.index(want)]
    got = host.fermion_guarded_optimize_exact_sum(st, cfgs, 16, *model, "sgd", eta, SGD0, 1, selectors=INITIAL, dtype=F64, batch=6)
    assert list(got["selected_eta"]) == [want]
    assert got["energies"].tobytes() == e.tobytes() and got["state"].tobytes() == stored.tobytes()


def test_monte_carlo_trials_use_the_energy_only_evaluator(tfim):
    """VMCPEPSOptimizer hands the optimizer MCEnergyGradEvaluator::EvaluateEnergyOnly: the trials cost no gradient evaluation, leave
    the accumulators alone and are no entries of the trajectory.  With the initial selector off at lr = 0 the same chains give the
    same first evaluation, which the trials (they come after it) cannot have touched."""
    host = _host()
    flat, all_cfgs = tfim
    n, S, its = 16, 4, 3
    cfgs = np.stack([all_cfgs[i % len(all_cfgs)] for i in range(n)])
    seeds = np.arange(n, dtype=np.uint64) + 81
    kw = dict(warmup_sweeps=2, samples_per_walker=S)
    got = host.guarded_vmc_optimize(flat, cfgs, seeds, 8, *TFIM, "fullspace", "sgd", 0.05, SGD0, its,
                                    selectors=dict(initial={}, periodic=dict(every_n_steps=2)), **kw)
    first = host.guarded_vmc_optimize(flat, cfgs, seeds, 8, *TFIM, "fullspace", "sgd", 0.0, SGD0, 0, **kw)
    assert got["energy_only_calls"] == 3 + 2 and got["evaluator_calls"] == its + 1
    assert got["energies"].shape == (its + 1,) and np.all(np.isfinite(got["energies"])) and np.all(got["energy_errors"] > 0)
    assert got["energies"][0] == first["energies"][0] and got["energy_errors"][0] == first["energy_errors"][0]
    eta0 = got["selected_eta"][0]
    assert eta0 in list(host.step_candidates("initial", 0.05, 3))
    assert list(got["selected_eta"][[1]]) == [0.0] and got["selected_eta"][2] in (eta0, eta0 * 0.5)
    assert float(np.max(np.abs(got["state"] - flat))) > 1e-6


def test_a_non_finite_trial_raises_and_leaves_the_base(tfim):
    flat, cfgs = tfim
    host = _host()
    _, base = host.optimize_exact_sum(flat, cfgs, 8, *TFIM, "sgd", 0.2, SGD0, 2, dtype=F64, batch=16)
    shift = np.zeros(8)
    shift[4] = np.nan                                       # calls 0, 1, 2: iterations; 3, 4: the trials at iteration 2
    with pytest.raises(host.GuardedRunError, match="Step selector candidate evaluation produced non-finite energy$") as info:
        host.guarded_optimize_exact_sum(flat, cfgs, 8, *TFIM, "sgd", 0.2, SGD0, 4, dtype=F64, batch=16,
                                        selectors=dict(periodic=dict(every_n_steps=2, enable_in_deterministic=True)),
                                        schedule=dict(energy_shift=shift))
    assert info.value.evaluator_calls == 5
    assert info.value.state.tobytes() == base.tobytes()

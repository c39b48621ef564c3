"""Spike recovery of the device-resident Optimizer (peps_amd/host/qlpeps_gpu.h: SpikeGuard, Optimizer::IterativeOptimize; the base of a
step in HBM, pepsgpu_guard_*) through hostapi.guarded_optimize_exact_sum / guarded_vmc_optimize on the reference's 2x2
transverse-field Ising state (D = 4, chi = 8, the 16 configurations in one batch).

The exact-summation evaluator and every update rule are deterministic, and a restored state is the saved one bit for bit, so a run
with scripted spikes must reproduce the energies and states of the unguarded run (hostapi.optimize_exact_sum, existing code) exactly:
every comparison below is equality of bytes.  The schedule raises when the evaluator is called more often than it is long, so no
scripted run can loop."""
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
ADAM = (0.9, 0.999, 1e-8, 0.0)
SR = (1e-3, 100, 1e-4, 0)
MINSR = (1e-12, 0.0, 1)
LR = 0.2
N = 6                                      # iterations of the scripted SGD runs


def _host():
    from peps_amd import hostapi
    return hostapi


@pytest.fixture(scope="module")
def tfim(fixtures_dir):
    s = qlten_io.load_sitps(os.path.join(fixtures_dir, "transverse_ising_tps_double_from_simple_update"))
    return synthetic.sitps_to_flat(s, 4), np.array(vmc.generate_all_binary_configs(2, 2), dtype=np.int32)


@pytest.fixture(scope="module")
def plain(tfim):
    """the unguarded plain-SGD run, computed once: energies and gradient norms of N + 1 evaluations, the state after N and N - 1 steps"""
    flat, cfgs = tfim
    host = _host()
    e, state, norms = host.optimize_exact_sum(flat, cfgs, 8, *TFIM, "sgd", LR, SGD0, N, dtype=F64, batch=16, return_grad_norms=True)
    _, before = host.optimize_exact_sum(flat, cfgs, 8, *TFIM, "sgd", LR, SGD0, N - 1, dtype=F64, batch=16)
    assert np.all(np.diff(e) < 0)
    return e, norms, state, before


def _guarded(tfim, algo, lr, rp, iterations, **kw):
    flat, cfgs = tfim
    return _host().guarded_optimize_exact_sum(flat, cfgs, 8, *TFIM, algo, lr, rp, iterations, dtype=F64, batch=16, **kw)


# ---- everything off: the loop is the one that was there ----
@pytest.mark.parametrize("algo,lr,rp", [("sgd", 0.05, (0.9, 1.0, 1e-3)), ("adam", 0.02, ADAM), ("adagrad", 0.1, (1e-8, 0.0))],
                         ids=["sgd", "adam", "adagrad"])
def test_everything_off_first_order(tfim, algo, lr, rp):
    flat, cfgs = tfim
    e, state, norms = _host().optimize_exact_sum(flat, cfgs, 8, *TFIM, algo, lr, rp, 5, dtype=F64, batch=16, return_grad_norms=True)
    got = _guarded(tfim, algo, lr, rp, 5)
    assert got["energies"].tobytes() == e.tobytes() and got["grad_norms"].tobytes() == norms.tobytes()
    assert got["state"].tobytes() == state.tobytes()
    assert got["events"] == [] and got["evaluator_calls"] == 6 and not np.any(got["selected_eta"])
    assert got["min_energy"] == e.min() and np.all(got["energy_errors"] == 0)


def test_everything_off_sr_minsr_and_complex(tfim):
    flat, cfgs = tfim
    host = _host()
    for normalize in (0, 1):
        rp = SR[:3] + (normalize,)
        state, info = host.sr_step_samples(flat, cfgs, 8, *TFIM, 0.1, rp[0], rp[1], rp[2], bool(normalize), dtype=F64)
        got = _guarded(tfim, "sr", 0.1, rp, 1)
        assert got["state"].tobytes() == state.tobytes()
        assert (got["energies"][0], got["energies"][1]) == (info["energy_before"], info["energy_after"])
        assert (got["sr_iterations"], got["sr_natural_grad_norm"], got["sr_residual_norm"]) == \
               (info["cg_iterations"], info["direction_norm"], info["cg_residual_norm"])
    state, info = host.minsr_step_samples(flat, cfgs, 8, *TFIM, 0.1, *MINSR[:2], bool(MINSR[2]), dtype=F64)
    got = _guarded(tfim, "minsr", 0.1, MINSR, 1)
    assert got["state"].tobytes() == state.tobytes() and got["sr_natural_grad_norm"] == info["direction_norm"]
    cflat = flat.astype(np.complex128) * np.exp(0.3j)
    e, state = host.optimize_exact_sum(cflat, cfgs, 8, *TFIM, "adam", 0.02, ADAM, 3, batch=16)
    got = host.guarded_optimize_exact_sum(cflat, cfgs, 8, *TFIM, "adam", 0.02, ADAM, 3, batch=16)
    assert got["energies"].tobytes() == e.tobytes() and got["state"].tobytes() == state.tobytes()


# ---- S4: the rollback is exact ----
K, SHIFT, SIGMA_K = 3, 50.0, 3.0


def test_rollback_script_crosses_the_threshold_by_a_factor_of_ten(plain):
    """the CPU check of the script below: fed with the unguarded trajectory, the restatement fires S4 at evaluation K and nothing else,
    with (E - EMA) at least ten times sigma_k * Std"""
    e, norms, _, _ = plain
    rec = [(float(e[k]) + (SHIFT if k == K else 0.0), 0.0, float(norms[k]), 0.0, 0) for k in range(K + 1)]
    g, actions, *_ = spike_ref.replay(rec, "sgd", enable_rollback=True, sigma_k=SIGMA_K)
    assert actions == ["ACCEPT"] * K + ["ROLLBACK"] and len(g.events) == 1
    ev = g.events[0]
    assert ev["signal"] == "S4_ENERGY_SPIKE"
    margin = (ev["value"] - g.energy.mean) / (ev["threshold"] - g.energy.mean)
    print("S4 script: E + shift - EMA = %.3f, sigma_k Std = %.3e: crossed by a factor %.1f" % (ev["value"] - g.energy.mean,
                                                                                                 ev["threshold"] - g.energy.mean, margin))
    assert margin >= 10.0


def test_rollback_is_exact(tfim, plain):
    e, norms, state, before = plain
    shift = np.zeros(N + 2)
    shift[K] = SHIFT
    got = _guarded(tfim, "sgd", LR, SGD0, N, spike=dict(enable_rollback=True, sigma_k=SIGMA_K), schedule=dict(energy_shift=shift))
    want = np.concatenate([e[:K], e[K - 1:N]])             # E_0 .. E_{K-1}, E_{K-1}, E_K, ...
    assert got["energies"].tobytes() == want.tobytes()
    assert got["state"].tobytes() == before.tobytes()      # one iteration was spent on the rollback
    assert (got["total_rollbacks"], got["total_resamples"], got["total_forced_accepts"]) == (1, 0, 0)
    (ev,) = got["events"]
    assert (ev["step"], ev["attempt"], ev["signal"], ev["action"]) == (K, 0, "S4_ENERGY_SPIKE", "ROLLBACK")
    assert abs(ev["value"] - (float(e[K]) + SHIFT)) <= 1e-12        # (e_loc_sum + shift W) / W
    assert got["evaluator_calls"] == N + 2
    assert got["min_energy"] == want.min()


def test_schedule_is_a_hard_limit(tfim):
    host = _host()
    with pytest.raises(host.GuardedRunError, match="beyond the schedule") as info:
        _guarded(tfim, "sgd", LR, SGD0, 3, schedule=dict(energy_shift=np.zeros(2)))
    assert info.value.evaluator_calls == 3


# ---- S1 / S2: resample ----
def test_s1_resample_and_forced_accept(tfim, plain):
    e, norms, state, _ = plain
    err = np.full(N + 4, 0.01)
    err[K] = 100.0
    got = _guarded(tfim, "sgd", LR, SGD0, N, spike={}, schedule=dict(error_override=err))
    assert got["energies"].tobytes() == e.tobytes() and got["state"].tobytes() == state.tobytes()
    assert got["evaluator_calls"] == N + 2 and got["total_resamples"] == 1
    (ev,) = got["events"]
    assert (ev["step"], ev["signal"], ev["action"], ev["value"]) == (K, "S1_ERRORBAR", "RESAMPLE", 100.0)
    assert ev["threshold"] == pytest.approx(1.0, rel=1e-12)
    assert np.all(got["energy_errors"] == 0.01)            # the rejected error bar is not in the trajectory
    # redo_mc_max_retries + 1 bad evaluations in a row, no rollback: two resamples, then the third is accepted with a warning
    err[K:K + 3] = 100.0
    got = _guarded(tfim, "sgd", LR, SGD0, N, spike={}, schedule=dict(error_override=err))
    assert [(x["attempt"], x["action"]) for x in got["events"]] == [(0, "RESAMPLE"), (1, "RESAMPLE"), (2, "ACCEPT_WARN")]
    assert (got["total_resamples"], got["total_forced_accepts"], got["total_rollbacks"]) == (2, 1, 0)
    assert got["energies"].tobytes() == e.tobytes() and got["state"].tobytes() == state.tobytes()
    assert got["energy_errors"][K] == 100.0 and got["evaluator_calls"] == N + 3


def test_s2_through_the_energy_shift(tfim, plain):
    e, norms, state, _ = plain
    shift = np.zeros(N + 2)
    shift[K] = SHIFT                                        # g = (S_EO - E S_O) / W: the shifted energy inflates the gradient
    got = _guarded(tfim, "sgd", LR, SGD0, N, spike=dict(factor_grad=3.0), schedule=dict(energy_shift=shift))
    (ev,) = got["events"]
    assert (ev["step"], ev["signal"], ev["action"]) == (K, "S2_GRAD_NORM", "RESAMPLE") and ev["value"] > 3.0 * float(norms[:K].max())
    assert got["energies"].tobytes() == e.tobytes() and got["grad_norms"].tobytes() == norms.tobytes()
    assert got["state"].tobytes() == state.tobytes()


def test_adam_moments_see_no_rejected_evaluation(tfim):
    flat, cfgs = tfim
    e, state = _host().optimize_exact_sum(flat, cfgs, 8, *TFIM, "adam", 0.02, ADAM, 5, dtype=F64, batch=16)
    err, shift = np.full(8, 0.01), np.zeros(8)
    err[2], shift[2] = 100.0, 7.0                           # the rejected evaluation carries another gradient as well
    got = _guarded(tfim, "adam", 0.02, ADAM, 5, spike={}, schedule=dict(error_override=err, energy_shift=shift))
    assert got["total_resamples"] == 1
    assert got["energies"].tobytes() == e.tobytes() and got["state"].tobytes() == state.tobytes()


def test_s3_forced_by_the_iteration_count(tfim):
    """sr_min_iters_suspicious above every CG iteration count: S3 at every iteration after the first, two resamples and a forced accept
    each, and the states those accepts step from are the unguarded ones"""
    its = 3
    base = _guarded(tfim, "sr", 0.1, SR, its)
    assert 0 < base["sr_iterations"] < 1000
    got = _guarded(tfim, "sr", 0.1, SR, its, spike=dict(sr_min_iters_suspicious=1000))
    assert got["energies"].tobytes() == base["energies"].tobytes() and got["state"].tobytes() == base["state"].tobytes()
    assert got["sr_iterations"] == base["sr_iterations"]
    want = [(it, a, "S3_NGRAD_ANOMALY", act) for it in range(1, its) for a, act in ((0, "RESAMPLE"), (1, "RESAMPLE"), (2, "ACCEPT_WARN"))]
    assert [(x["step"], x["attempt"], x["signal"], x["action"]) for x in got["events"]] == want
    assert got["evaluator_calls"] == 1 + 3 * (its - 1) + 1
    minsr = _guarded(tfim, "minsr", 0.1, MINSR, its, spike=dict(sr_min_iters_suspicious=1000))
    assert minsr["events"] == []                            # no iterative solve: the count is not read


# ---- Monte-Carlo ----
def _walkers(all_cfgs, n):
    return np.stack([all_cfgs[i % len(all_cfgs)] for i in range(n)])


def test_chains_persist_through_a_rejected_evaluation(tfim):
    """lr = 0: the state never moves, so the run's evaluator calls are the consecutive evaluations of one engine
    (hostapi.mc_evaluate_resident, n_evaluates = 4).  The second is rejected (S1 override): the accepted ones are calls 0, 2 and 3."""
    host = _host()
    flat, all_cfgs = tfim
    n, S = 16, 4
    cfgs, seeds = _walkers(all_cfgs, n), np.arange(n, dtype=np.uint64) + 61
    ref = host.mc_evaluate_resident(flat, cfgs, seeds, 8, *TFIM, "fullspace", warmup_sweeps=2, n_samples=S, n_evaluates=4, normalize=True)
    e_ref = ref["e_loc_sum"] / ref["weight_sum"]
    assert np.all(ref["energy_error"] > 0) and np.all(np.isfinite(ref["energy_error"]))
    err = np.full(4, np.nan)
    err[1] = 1e6
    got = host.guarded_vmc_optimize(flat, cfgs, seeds, 8, *TFIM, "fullspace", "sgd", 0.0, SGD0, 2, warmup_sweeps=2, samples_per_walker=S,
                                    spike={}, schedule=dict(error_override=err))
    assert got["energies"].tobytes() == e_ref[[0, 2, 3]].tobytes()
    assert got["energy_errors"].tobytes() == ref["energy_error"][[0, 2, 3]].tobytes()
    assert np.array_equal(got["accept_rates"], ref["accept_rates"][[0, 2, 3]])
    assert got["total_resamples"] == 1 and got["evaluator_calls"] == 4
    assert (got["events"][0]["step"], got["events"][0]["signal"], got["events"][0]["value"]) == (1, "S1_ERRORBAR", 1e6)
    assert np.array_equal(got["configs"], ref["configs"])


def test_a_rejected_evaluation_is_never_the_lowest(tfim):
    host = _host()
    flat, all_cfgs = tfim
    n, S = 16, 4
    cfgs, seeds = _walkers(all_cfgs, n), np.arange(n, dtype=np.uint64) + 71
    err, shift = np.full(5, np.nan), np.zeros(5)
    err[1] = 1e6
    kw = dict(warmup_sweeps=2, samples_per_walker=S, spike={})
    b = host.guarded_vmc_optimize(flat, cfgs, seeds, 8, *TFIM, "fullspace", "sgd", 0.1, SGD0, 3, schedule=dict(error_override=err), **kw)
    shift[1] = -100.0                                       # far below anything the state can reach
    a = host.guarded_vmc_optimize(flat, cfgs, seeds, 8, *TFIM, "fullspace", "sgd", 0.1, SGD0, 3,
                                  schedule=dict(error_override=err, energy_shift=shift), **kw)
    assert a["total_resamples"] == b["total_resamples"] == 1
    assert a["energies"].tobytes() == b["energies"].tobytes() and a["state"].tobytes() == b["state"].tobytes()
    assert a["min_energy"] == b["min_energy"] == a["energies"].min() > -50.0
    assert a["lowest_state"].tobytes() == b["lowest_state"].tobytes()
    assert float(np.max(np.abs(a["state"] - flat))) > 1e-6


def test_refusals_come_before_the_device(tfim):
    host = _host()
    flat, all_cfgs = tfim
    cfgs, seeds = _walkers(all_cfgs, 4), np.arange(4, dtype=np.uint64)
    ini = dict(initial=dict(enable_in_deterministic=True))
    with pytest.raises(ValueError, match="Step selectors only support SGD, SR, and MinSR"):
        host.guarded_vmc_optimize(flat, cfgs, seeds, 8, *TFIM, "fullspace", "adam", 0.1, ADAM, 2, selectors=ini)
    with pytest.raises(ValueError, match="cannot be used together with lr_scheduler"):
        host.guarded_vmc_optimize(flat, cfgs, seeds, 8, *TFIM, "fullspace", "sgd", 0.1, SGD0, 2, selectors=ini, scheduler=True)
    with pytest.raises(ValueError, match="rollback is not available with L-BFGS"):
        host.guarded_vmc_optimize(flat, cfgs, seeds, 8, *TFIM, "fullspace", "lbfgs", 0.1, None, 2, spike=dict(enable_rollback=True))

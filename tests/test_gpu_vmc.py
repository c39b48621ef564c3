"""Monte-Carlo VMC on the resident state: MCEnergyGradEvaluator and VMCPEPSOptimizer of the C++ host layer (peps_amd/host/qlpeps_gpu.h)
through hostapi.mc_evaluate_resident / vmc_optimize / fermion_vmc_optimize, and the snapshot calls of the C ABI.

Shapes: the reference's 2x2 fixtures (D = 4: Heisenberg, transverse-field Ising, spinless fermions) and a synthetic 3x3, D = 2.  chi is
large enough that no boundary MPS is truncated (8 / 16 >= D^2 resp. D on these lattices), so a freshly contracted amplitude and a
chain-carried one differ by rounding only.  8 - 64 walkers, except the two statistical comparisons with their 10 000 samples."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

from oracle import qlten_io, statistics, vmc
from peps_amd import synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import opt_fermion_ref as fref  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = 0, 1
EINVAL, ESTATE = 1, 3                     # PEPSGPU_EINVAL, PEPSGPU_ESTATE (include/pepsgpu.h)
XXZ = (1.0, 1.0, 0.0)
ADAM = (0.9, 0.999, 1e-8, 0.0)
SR = (1e-3, 100, 1e-4, 0)
# device-against-host gradients in float64: tests/test_gpu_optimizer.py (1e-9 per element)
TOL64 = 1e-9
# float32 contexts: the suite's device parity in float32 is 2e-5 relative (tests/test_gpu_host.py, (F32, 2e-5)); the evaluator's fresh
# amplitude after RefreshWavefunctionComponent and the chain-carried one of the existing loop differ by float32 rounding of two
# contraction orders, which enters O* = hole / psi relatively: the bound is 2e-5 of the largest element of the compared array
RTOL32 = 2e-5


def _host():
    from peps_amd import hostapi
    return hostapi


def binned(samples):
    """the restated statistic (tests/test_cpu_vmc.py): samples[sample][walker]"""
    samples = np.asarray(samples)
    S, n = samples.shape
    bs = max(1, int(np.floor(np.sqrt(S))))
    bins = np.array([samples[i * bs:(i + 1) * bs, w].sum() / bs for w in range(n) for i in range(S // bs)])
    mu = statistics.mean(bins)
    return mu, statistics.standard_error(bins, mu)


@pytest.fixture(scope="module")
def heis(fixtures_dir):
    s = qlten_io.load_sitps(os.path.join(fixtures_dir, "heisenberg_tps_double_from_simple_update"))
    return synthetic.sitps_to_flat(s, 4), np.array(vmc.generate_all_permutation_configs([2, 2], 2, 2), dtype=np.int32)


@pytest.fixture(scope="module")
def tfim(fixtures_dir):
    s = qlten_io.load_sitps(os.path.join(fixtures_dir, "transverse_ising_tps_double_from_simple_update"))
    return synthetic.sitps_to_flat(s, 4), np.array(vmc.generate_all_binary_configs(2, 2), dtype=np.int32)


@pytest.fixture(scope="module")
def spinless(fixtures_dir):
    from peps_amd import fermion
    st = fermion.FermionState.load(os.path.join(fixtures_dir, "spinless_fermion_tps_t2_0.000000_double_from_simple_update"))
    cfgs = np.array([np.array(p).reshape(2, 2) for p in sorted(set(itertools.permutations([0, 0, 1, 1])))], dtype=np.int32)
    return st, cfgs


def _walkers(all_cfgs, n):
    return np.stack([all_cfgs[i % len(all_cfgs)] for i in range(n)])


def _case(name, heis):
    if name == "heis2x2":
        flat, all_cfgs = heis
        return flat, _walkers(all_cfgs, 8), 8
    return synthetic.sitps_to_flat(synthetic.make_sitps(3, 2), 2), synthetic.make_configs(3, 8, "heisenberg"), 16


# ---- 1. one Evaluate equals the existing loop ----
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["heis2x2", "synth3x3"])
def test_one_evaluate_equals_the_existing_loop(heis, name, dt):
    """warm-up 2, S = 5, 8 walkers, the same seeds: energy samples, S_O / S_EO and acceptance rates of one Evaluate against
    mc_energy_grad_partial on a context of the same dtype; and gradient = (S_EO - conj(E_binned) S_O) / W with E_binned from the restated
    statistic -- S = 5 drops the fifth sample of every walker, which the plain mean would not."""
    host = _host()
    flat, cfgs, chi = _case(name, heis)
    n, S = 8, 5
    seeds = np.arange(n, dtype=np.uint64) + 11
    step = dict(algo="sgd", lr=0.0, rule_params=(0.0, 0.0, 0.0))
    ev = host.mc_evaluate_resident(flat, cfgs, seeds, chi, "xxz", XXZ, "exchange", warmup_sweeps=2, n_samples=S, dtype=dt, step=step)
    packed, cfg_ref, acc_ref = host.mc_energy_grad_partial(flat, cfgs, seeds, chi, "exchange", "xxz", XXZ, 2, S, dt)
    m = flat.size
    so_ref, seo_ref = packed[:m].reshape(flat.shape), packed[m:2 * m].reshape(flat.shape)
    w_ref, esum_ref, esq_ref, ns_ref = packed[2 * m:2 * m + 4]
    es = ev["energy_samples"][0]
    tol = (lambda a: TOL64) if dt == F64 else (lambda a: RTOL32 * float(np.max(np.abs(a))))
    d_so, d_seo = float(np.max(np.abs(ev["S_O"][0] - so_ref))), float(np.max(np.abs(ev["S_EO"][0] - seo_ref)))
    d_e, d_e2 = abs(float(es.sum()) - esum_ref), abs(float((es ** 2).sum()) - esq_ref)
    print("%s dtype %d: max |S_O - ref| = %.3e (max |S_O| %.3e)  max |S_EO - ref| = %.3e  |sum E - ref| = %.3e  |sum E^2 - ref| = %.3e  "
          "max |accept - ref| = %.3e" % (name, dt, d_so, float(np.max(np.abs(so_ref))), d_seo, d_e, d_e2,
                                         float(np.max(np.abs(ev["accept_rates"][0] - acc_ref)))))
    assert ns_ref == n * S and ev["weight_sum"][0] == w_ref == n * S
    assert np.array_equal(ev["configs"], cfg_ref)                       # the same chain
    assert np.array_equal(ev["accept_rates"][0], acc_ref)
    assert d_so <= tol(so_ref) and d_seo <= tol(seo_ref)
    assert d_e <= tol(es) * n * S and d_e2 <= tol(es ** 2) * n * S
    # the local energies sample by sample: the configurations after k samples of the existing loop, evaluated afresh
    for k in range(1, S + 1):
        _, cfg_k, _ = host.mc_energy_grad_partial(flat, cfgs, seeds, chi, "exchange", "xxz", XXZ, 2, k, dt)
        _, en_k, _, _ = host.energy_and_holes(flat, cfg_k, chi, "xxz", XXZ, False, dt)
        d_k = float(np.max(np.abs(es[k - 1] - en_k)))
        print("  sample %d: max |E_loc - fresh| = %.3e" % (k, d_k))
        assert d_k <= tol(en_k)
    # E_binned, and the gradient the optimizer finishes from it
    e_binned, err = binned(es)
    assert abs(ev["e_loc_sum"][0] / (n * S) - e_binned) <= 1e-13 * max(1.0, abs(e_binned))
    assert abs(ev["energy_error"][0] - err) <= 1e-13 * max(1.0, err)
    assert abs(e_binned - es.mean()) > 1e-6                            # the dropped sample matters on this chain
    assert abs(ev["step_energy"] - e_binned) <= 1e-13 * max(1.0, abs(e_binned))
    g = (ev["S_EO"][0] - np.conj(e_binned) * ev["S_O"][0]) / (n * S)
    gn = float(np.linalg.norm(g.ravel()))
    print("  E_binned = %.12f  plain mean = %.12f  |g| device %.12e restated %.12e" % (e_binned, es.mean(), ev["step_grad_norm"], gn))
    assert abs(ev["step_grad_norm"] - gn) <= 1e-9 * max(1.0, gn)
    assert np.array_equal(ev["state"], flat if dt == F64 else flat.astype(np.float32).astype(np.float64))   # lr = 0


# ---- 2. chains persist ----
@pytest.mark.parametrize("name", ["heis2x2", "synth3x3"])
def test_chains_persist_across_evaluations(heis, name):
    host = _host()
    flat, cfgs, chi = _case(name, heis)
    S = 3
    seeds = np.arange(8, dtype=np.uint64) + 5
    two = host.mc_evaluate_resident(flat, cfgs, seeds, chi, "xxz", XXZ, "exchange", warmup_sweeps=1, n_samples=S, n_evaluates=2, dtype=F64)
    one = host.mc_evaluate_resident(flat, cfgs, seeds, chi, "xxz", XXZ, "exchange", warmup_sweeps=1, n_samples=2 * S, dtype=F64)
    es2 = two["energy_samples"].reshape(2 * S, 8)
    d_e = float(np.max(np.abs(es2 - one["energy_samples"][0])))
    d_so = float(np.max(np.abs(two["S_O"].sum(axis=0) - one["S_O"][0])))
    d_seo = float(np.max(np.abs(two["S_EO"].sum(axis=0) - one["S_EO"][0])))
    print("%s: max |E_loc| diff %.3e  |S_O| diff %.3e  |S_EO| diff %.3e" % (name, d_e, d_so, d_seo))
    assert np.array_equal(two["configs"], one["configs"])
    assert d_e < 1e-10 and d_so < 1e-10 and d_seo < 1e-10
    assert np.max(np.abs(two["accept_rates"].mean(axis=0) - one["accept_rates"][0])) < 1e-14
    assert not np.array_equal(two["energy_samples"][0], two["energy_samples"][1])      # the second call went on, it did not restart


# ---- 3. Monte Carlo against exact summation by the reference's criteria ----
def _direction_error(g_mc, g_ex):
    a, b = g_mc.ravel() / np.linalg.norm(g_mc.ravel()), g_ex.ravel() / np.linalg.norm(g_ex.ravel())
    return float(np.linalg.norm(a - b))


def test_mc_against_exact_summation_heisenberg(heis):
    """test_mc_energy_grad_evaluator.cpp:287-336: 10 000 samples (500 walkers x 20), |E_mc - E_ex| <= 3 x the reported error and the
    error of the unit gradient direction < 0.3.  Seeds 1 .. 500 (the float64 chain is deterministic: one std::mt19937 per walker, the
    deviates of oracle/vmc.py's updater); measured on the MI355X with them: |E_mc - E_ex| = 9.1e-4 at a reported error of 1.0e-3,
    direction error 0.009; spinless fermions below: 2.4e-4 at 9.2e-4, direction error 0.053."""
    host = _host()
    flat, all_cfgs = heis
    e_ex, g_ex = host.exact_sum_finish(host.exact_sum_partial(flat, all_cfgs, 8, "xxz", XXZ, 0, 1, 8, F64), flat.shape)
    n, S = 500, 20
    ev = host.mc_evaluate_resident(flat, _walkers(all_cfgs, n), np.arange(n, dtype=np.uint64) + 1, 8, "xxz", XXZ, "exchange",
                                   warmup_sweeps=5, n_samples=S, dtype=F64)
    e_mc, err = ev["e_loc_sum"][0] / ev["weight_sum"][0], ev["energy_error"][0]
    g_mc = (ev["S_EO"][0] - e_mc * ev["S_O"][0]) / (n * S)
    de = _direction_error(g_mc, g_ex)
    print("heisenberg: E_mc = %.8f  E_ex = %.8f  |diff| = %.3e  reported error = %.3e  direction error = %.4f"
          % (e_mc, e_ex, abs(e_mc - e_ex), err, de))
    assert np.isfinite(err) and err > 0
    assert abs(e_mc - e_ex) <= 3 * err
    assert de < 0.3


def test_mc_against_exact_summation_spinless_fermions(spinless):
    host = _host()
    from peps_amd import fermion
    st, all_cfgs = spinless
    e_ex, g_ex = host.fermion_exact_sum(st, all_cfgs, 16, 1.0, 0.0, batch=8, dtype=F64)
    n, S = 500, 20
    ev = host.mc_evaluate_resident(st, _walkers(all_cfgs, n), np.arange(n, dtype=np.uint64) + 1, 16, "spinless", (1.0, 0.0, 0.0), "exchange",
                                   warmup_sweeps=5, n_samples=S, dtype=F64)
    e_mc, err = ev["e_loc_sum"][0] / ev["weight_sum"][0], ev["energy_error"][0]
    g_mc = fermion.fold_gradient(st, (ev["S_EO"][0] - e_mc * ev["S_O"][0]) / (n * S))
    de = _direction_error(np.asarray(g_mc), np.asarray(g_ex))
    print("spinless fermions: E_mc = %.8f  E_ex = %.8f  |diff| = %.3e  reported error = %.3e  direction error = %.4f"
          % (e_mc, e_ex, abs(e_mc - e_ex), err, de))
    assert np.isfinite(err) and err > 0
    assert abs(e_mc - e_ex) <= 3 * err
    assert de < 0.3


# ---- 4. one VMCPEPSOptimizer iteration equals the hand-composed sequence ----
RULES = [("sgd", "sgd", 0.05, (0.9, 1.0, 1e-3), 0.0), ("adam", "adam", 0.02, ADAM, 0.5), ("sr", "sr", 0.1, SR, 0.0),
         ("minsr", "minsr", 0.1, (1e-12, 0.0, 1), 0.0)]


@pytest.mark.parametrize("name,algo,lr,rp,clip", RULES, ids=[r[0] for r in RULES])
def test_one_iteration_equals_the_hand_composed_sequence(heis, name, algo, lr, rp, clip):
    """Execute with one iteration (stopped before the closing normalisation) against warm-up -> Evaluate -> finish -> clip -> step put
    together from the contractor's calls; Adam runs with a global-norm clip of half the gradient norm."""
    host = _host()
    flat, all_cfgs = heis
    n, S = 16, 4
    cfgs, seeds = _walkers(all_cfgs, n), np.arange(n, dtype=np.uint64) + 21
    clip_norm = 0.0
    if clip:
        probe = host.mc_evaluate_resident(flat, cfgs, seeds, 8, "xxz", XXZ, "exchange", warmup_sweeps=2, n_samples=S, normalize=True,
                                          step=dict(algo=algo, lr=0.0, rule_params=rp))
        clip_norm = clip * probe["step_grad_norm"]
    hand = host.mc_evaluate_resident(flat, cfgs, seeds, 8, "xxz", XXZ, "exchange", warmup_sweeps=2, n_samples=S, normalize=True,
                                     step=dict(algo=algo, lr=lr, rule_params=rp, clip_norm=clip_norm))
    run = host.vmc_optimize(flat, cfgs, seeds, 8, "xxz", XXZ, "exchange", algo, lr, rp, 1, warmup_sweeps=2, samples_per_walker=S,
                            clip_norm=clip_norm, finalize=False)
    moved = float(np.max(np.abs(run["state"] - flat)))
    print("%s: max |theta_1 - theta_0| = %.3e  E[0] = %.10f (hand %.10f)  |g| = %.6e (hand %.6e)"
          % (name, moved, run["energies"][0], hand["step_energy"], run["grad_norms"][0], hand["step_grad_norm"]))
    assert run["energies"].shape == (2,) and moved > 1e-6
    assert run["energies"][0] == hand["step_energy"] and run["grad_norms"][0] == hand["step_grad_norm"]
    assert run["energy_errors"][0] == hand["energy_error"][0]
    assert np.array_equal(run["accept_rates"][0], hand["accept_rates"][0])
    assert np.array_equal(run["state"], hand["state"])                   # bit for bit
    assert np.all(run["state"][flat == 0] == 0)


def test_one_sr_iteration_on_a_fermionic_state(spinless):
    host = _host()
    st, all_cfgs = spinless
    n, S = 16, 4
    cfgs, seeds = _walkers(all_cfgs, n), np.arange(n, dtype=np.uint64) + 31
    hand = host.mc_evaluate_resident(st, cfgs, seeds, 16, "spinless", (1.0, 0.0, 0.0), "exchange", warmup_sweeps=2, n_samples=S,
                                     normalize=True, step=dict(algo="sr", lr=0.1, rule_params=SR))
    run = host.fermion_vmc_optimize(st, cfgs, seeds, 16, "spinless", (1.0, 0.0, 0.0), "exchange", "sr", 0.1, SR, 1, warmup_sweeps=2,
                                    samples_per_walker=S, finalize=False)
    stored0 = fref.stored_flat(st)
    moved = float(np.max(np.abs(run["state"] - stored0)))
    print("fermionic SR: max |theta_1 - theta_0| = %.3e  E[0] = %.10f  |g| = %.6e" % (moved, run["energies"][0], run["grad_norms"][0]))
    assert moved > 1e-6
    assert run["energies"][0] == hand["step_energy"] and run["grad_norms"][0] == hand["step_grad_norm"]
    assert np.array_equal(run["state"], hand["state"])
    assert np.all(run["state"][~fref.allowed_flat(st)] == 0)             # the step stays in the parameters of the state


# ---- 5. a ten-iteration SR run, the lowest state ----
def _perturbed(flat):
    rng = np.random.default_rng(2024)
    return flat * (1.0 + 0.3 * rng.normal(size=flat.shape))


def _exact_energy(host, flat, cfgs, model, params):
    return host.exact_sum_finish(host.exact_sum_partial(flat, cfgs, 8, model, params, 0, 1, 16, F64), flat.shape)[0]


@pytest.fixture(scope="module")
def sr_run(tfim):
    host = _host()
    flat, all_cfgs = tfim
    start = _perturbed(flat)
    n = 64
    cfgs, seeds = _walkers(all_cfgs, n), np.arange(n, dtype=np.uint64) + 41
    kw = dict(warmup_sweeps=3, samples_per_walker=4)
    run = host.vmc_optimize(start, cfgs, seeds, 8, "tfim", (1.0,), "fullspace", "sr", 0.1, SR, 10, **kw)
    return start, cfgs, seeds, kw, run


def test_sr_run_lowers_the_energy_and_keeps_the_lowest_state(tfim, sr_run):
    host = _host()
    flat, all_cfgs = tfim
    start, cfgs, seeds, kw, run = sr_run
    e0, e1 = _exact_energy(host, start, all_cfgs, "tfim", (1.0,)), _exact_energy(host, run["state"], all_cfgs, "tfim", (1.0,))
    k = int(np.argmin(run["energies"]))
    print("SR run: exact-sum energy %.8f -> %.8f; trajectory %s; argmin %d" % (e0, e1, np.array2string(run["energies"], precision=6), k))
    assert run["energies"].shape == (11,) and run["grad_norms"].shape == (11,) and run["accept_rates"].shape == (11, 64)
    assert e1 < e0
    assert run["min_energy"] == run["energies"].min()
    assert run["current_energy"] == run["energies"][-1]
    # a second run on the same chains stopped at the argmin iteration: theta after k steps, before any closing normalisation
    again = host.vmc_optimize(start, cfgs, seeds, 8, "tfim", (1.0,), "fullspace", "sr", 0.1, SR, k, finalize=False, **kw)
    assert np.array_equal(again["energies"], run["energies"][:k + 1])
    assert run["lowest_state"].tobytes() == again["state"].tobytes()
    if k < 10:           # an OptimizationCallback sees the same parameters at that iteration of the first run's schedule
        probe = host.vmc_optimize(start, cfgs, seeds, 8, "tfim", (1.0,), "fullspace", "sr", 0.1, SR, k + 1, finalize=False,
                                  probe_iteration=k, **kw)
        assert probe["probe_state"].tobytes() == run["lowest_state"].tobytes()


# ---- 6. normalisation and dumps ----
def test_normalisation_and_dumps(tfim, sr_run, tmp_path):
    host = _host()
    start, cfgs, seeds, kw, _ = sr_run
    base, edir, cdir = str(tmp_path / "tps_"), str(tmp_path / "energy"), str(tmp_path / "configs")
    run = host.vmc_optimize(start, cfgs, seeds, 8, "tfim", (1.0,), "fullspace", "sr", 0.1, SR, 3, tps_dump_base_name=base, energy_dir=edir,
                            config_dump_path=cdir, **kw)
    print("after Execute: max |psi| - 1 = %.3e" % (run["max_abs_psi"] - 1.0))
    assert abs(run["max_abs_psi"] - 1.0) < 1e-10
    lines = open(os.path.join(edir, "energy_trajectory.csv")).read().splitlines()
    assert lines[0] == "iteration,energy,energy_error,gradient_norm"
    assert len(lines) == 1 + 3 + 1
    rows = np.array([[float(x) for x in ln.split(",")] for ln in lines[1:]])
    assert np.array_equal(rows[:, 0], np.arange(4))
    assert np.array_equal(rows[:, 1], run["energies"]) and np.array_equal(rows[:, 2], run["energy_errors"])
    assert np.array_equal(rows[:, 3], run["grad_norms"])
    assert np.array_equal(host.load_sitps(base + "final", 4), run["state"])
    assert np.array_equal(host.load_sitps(base + "lowest", 4), run["lowest_state"])
    for w in (0, 63):
        assert np.array_equal(host.load_configuration(cdir, w, 2, 2), run["configs"][w])


# ---- 7. the complex twin ----
@pytest.mark.parametrize("algo,lr,rp", [("sgd", 0.05, (0.9, 1.0, 0.0)), ("sr", 0.1, SR)], ids=["sgd", "sr"])
def test_complex_twin_follows_the_real_run(heis, algo, lr, rp):
    """the QLTEN_Complex instantiation on the same (real-valued) state, three iterations.  The rules are those whose update is
    continuous in the gradient.  Adam is left out on purpose: this fixture holds entries of magnitude 1e-15 whose gradient is rounding
    noise of the same size, and m1 / (sqrt(m2) + 1e-8) turns a noise of 1e-15 into a step of 1e-7 lr per iteration with the sign of
    the noise -- measured on the MI355X: the two Adam runs agree to 4.8e-13 after one step and drift to 3.5e-5 at exactly such an
    entry after three, while SGD and SR agree to 4.4e-16."""
    host = _host()
    flat, all_cfgs = heis
    n = 16
    cfgs, seeds = _walkers(all_cfgs, n), np.arange(n, dtype=np.uint64) + 51
    args = (cfgs, seeds, 8, "xxz", XXZ, "exchange", algo, lr, rp, 3)
    kw = dict(warmup_sweeps=2, samples_per_walker=4)
    r = host.vmc_optimize(flat, *args, **kw)
    c = host.vmc_optimize(flat.astype(np.complex128), *args, **kw)
    d_e, d_s = float(np.max(np.abs(c["energies"] - r["energies"]))), float(np.max(np.abs(c["state"] - r["state"])))
    print("complex twin (%s): max |E - E_real| = %.3e  max |theta - theta_real| = %.3e  max |lowest - lowest_real| = %.3e"
          % (algo, d_e, d_s, float(np.max(np.abs(c["lowest_state"] - r["lowest_state"])))))
    assert c["energies"].dtype == np.complex128 and c["state"].dtype == np.complex128
    assert np.array_equal(c["configs"], r["configs"])
    assert float(np.max(np.abs(r["state"] - flat))) > 1e-3               # the run moved
    assert d_e < 1e-10 and d_s < 1e-10
    assert np.max(np.abs(c["energy_errors"] - r["energy_errors"])) < 1e-10 and np.max(np.abs(c["grad_norms"] - r["grad_norms"])) < 1e-10
    assert np.max(np.abs(c["lowest_state"] - r["lowest_state"])) < 1e-10


# ---- 8. the snapshot ABI ----
def _accumulate_one(ctx, flat, cfgs, amps, en, rows, cols):
    from peps_amd.capi import LEFT, RIGHT, UP, DOWN, HORIZONTAL
    ctx.set_configs(cfgs)
    ctx.generate_bmps_approach(UP)
    for row in range(rows):
        ctx.init_bten(LEFT, row)
        ctx.grow_full_bten(RIGHT, row, 1, True)
        for col in range(cols):
            ctx.punch_hole_store(row, col, HORIZONTAL)
            if col < cols - 1:
                ctx.shift_bten_window(RIGHT)
        if row < rows - 1:
            ctx.shift_bmps_window(DOWN)
    ctx.grad_reset()
    ctx.grad_accumulate(amps, en, exact_sum=False)


@pytest.mark.parametrize("dt", ["f64", "f32", "c128"])
def test_snapshot_save_step_read(tfim, dt):
    from peps_amd import capi
    host = _host()
    flat, cfgs = tfim
    cplx = dt == "c128"
    state = flat.astype(np.complex128) * (1.0 + 0.25j) if cplx else flat
    ctx = capi.Context(2, 2, 4, 2, 8, dtype={"f64": capi.F64, "f32": capi.F32, "c128": capi.C128}[dt], max_walkers=16)
    ctx.state_upload(state)
    # before opt_begin every call is refused with PEPSGPU_ESTATE and the context stays usable
    buf = np.zeros(state.shape, dtype=np.complex128 if cplx else np.float64)
    bp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert ctx._l.pepsgpu_vmc_snapshot_save(ctx._h) == ESTATE
    assert ctx._l.pepsgpu_vmc_snapshot_read(ctx._h, bp) == ESTATE
    assert ctx._l.pepsgpu_vmc_snapshot_clear(ctx._h) == ESTATE
    with pytest.raises(RuntimeError, match="pepsgpu_opt_begin"):
        ctx.vmc_snapshot_save()
    ctx.opt_begin()
    assert ctx._l.pepsgpu_vmc_snapshot_read(ctx._h, bp) == ESTATE       # read before save
    assert ctx._l.pepsgpu_vmc_snapshot_read(ctx._h, None) == EINVAL
    theta0 = ctx.opt_read_state()
    ctx.vmc_snapshot_save()
    g = np.where(state != 0, 0.5, 0.0).astype(state.dtype)
    ctx.opt_set_gradient(g)
    ctx.opt_step(capi.Context.OPT_SGD, 0.1, (0.0, 0.0, 0.0))
    theta1 = ctx.opt_read_state()
    snap = ctx.vmc_snapshot_read()
    assert not np.array_equal(theta1, theta0)
    assert snap.tobytes() == theta0.tobytes()                # the pre-step theta, bit for bit
    ctx.vmc_snapshot_save()                                  # a later save overwrites
    assert ctx.vmc_snapshot_read().tobytes() == theta1.tobytes()
    ctx.vmc_snapshot_clear()
    ctx.vmc_snapshot_clear()
    with pytest.raises(RuntimeError, match="no snapshot"):
        ctx.vmc_snapshot_read()
    ctx.vmc_snapshot_save()
    ctx.opt_end()                                            # frees the snapshot with the optimizer buffers
    ctx.opt_begin()
    assert ctx._l.pepsgpu_vmc_snapshot_read(ctx._h, bp) == ESTATE
    ctx.set_configs(cfgs)                                    # the context is still usable
    assert np.all(np.isfinite(ctx.evaluate_amplitude()))
    ctx.close()


def test_snapshot_under_a_fermionic_decoration(spinless):
    """the read-back obeys the opt_read_state contract: E theta in the extended layout, variant 0 = the stored arrays"""
    from peps_amd import capi
    st, _ = spinless
    ctx = capi.Context(st.rows, st.cols, st.D, 4 * st.d, 16, dtype=capi.F64, max_walkers=4)
    ctx.state_upload(st.extended_flat())
    ctx.fermion_decoration_set(st)
    ctx.opt_begin()
    theta0 = ctx.opt_read_state()
    ctx.vmc_snapshot_save()
    ctx.opt_scale_state(1.25)
    snap = ctx.vmc_snapshot_read()
    assert not np.array_equal(ctx.opt_read_state(), theta0)
    assert snap.tobytes() == theta0.tobytes()
    assert np.array_equal(snap[:, :, :st.d], fref.stored_flat(st))
    assert np.array_equal(snap, fref.decorate(st, snap[:, :, :st.d]))
    ctx.close()

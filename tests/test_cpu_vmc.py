"""CPU checks of the Monte-Carlo VMC layer (MCEnergyGradEvaluator / VMCPEPSOptimizer of peps_amd/host/qlpeps_gpu.h): the new entry
points are exported and bound, the binned energy statistic equals a NumPy restatement of MeanAndBinnedErrorSqrtNUniformBin
(vmc_basic/monte_carlo_tools/statistics.h:146-225) built on oracle.statistics, and VMCPEPSOptimizerParams refuses bad parameters
before any device call (these tests run without a GPU)."""
import ctypes
import math
import os

import numpy as np
import pytest

from oracle import statistics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_NEW = ("pepshost_vmc_optimize", "pepshost_vmc_optimize_c128", "pepshost_fermion_vmc_optimize", "pepshost_mc_evaluate_resident",
            "pepshost_binned_energy_stat")
SNAPSHOT = {"pepsgpu_vmc_snapshot_save": 1, "pepsgpu_vmc_snapshot_read": 2, "pepsgpu_vmc_snapshot_clear": 1}


def _built():
    from peps_amd import capi, hostapi
    if not (os.path.exists(capi.LIB_PATH) and os.path.exists(hostapi.LIB_PATH)):
        import __graft_entry__ as g
        g.build()
    return capi, hostapi


def binned_restatement(samples):
    """samples[sample][walker] -> (mean, error): per walker bins of max(1, floor(sqrt(S))) samples, the trailing samples dropped, the
    bin means gathered walker-major, then oracle.statistics.mean / standard_error of them"""
    samples = np.asarray(samples)
    S, n = samples.shape
    bs = max(1, int(math.floor(math.sqrt(S))))
    nb = S // bs
    bins = np.array([samples[i * bs:(i + 1) * bs, w].sum() / bs for w in range(n) for i in range(nb)])
    mu = statistics.mean(bins)
    return mu, statistics.standard_error(bins, mu)


def test_new_symbols_are_exported_and_bound():
    capi, hostapi = _built()
    header = open(os.path.join(ROOT, "include", "pepsgpu.h")).read()
    lib = ctypes.CDLL(capi.LIB_PATH)
    bound = capi.load_library()
    for name, nargs in SNAPSHOT.items():
        assert name + "(" in header, name
        assert hasattr(lib, name) and name in capi.SYMBOLS, name
        assert len(getattr(bound, name).argtypes) == nargs, name
        assert callable(getattr(capi.Context, name[len("pepsgpu_"):])), name
    host = ctypes.CDLL(hostapi.LIB_PATH)
    for name in HOST_NEW:
        assert hasattr(host, name) and name in hostapi.SYMBOLS, name
    for fn in ("vmc_optimize", "fermion_vmc_optimize", "mc_evaluate_resident", "binned_energy_stat"):
        assert callable(getattr(hostapi, fn)), fn


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("n_walkers", [1, 3])
@pytest.mark.parametrize("S", [1, 4, 5, 9, 10])
def test_binned_energy_stat_equals_the_restatement(S, n_walkers, cplx):
    _, hostapi = _built()
    rng = np.random.default_rng(1000 * S + 10 * n_walkers + cplx)
    x = rng.normal(size=(S, n_walkers)) - 2.0
    if cplx:
        x = x + 1j * rng.normal(size=(S, n_walkers))
    mean, err = hostapi.binned_energy_stat(x)
    want_mean, want_err = binned_restatement(x)
    # sums of at most 30 numbers of magnitude <= 10 in another order: a few units in the last place
    assert abs(mean - want_mean) <= 1e-13
    if math.isinf(want_err):
        assert math.isinf(err) and err > 0
    else:
        assert abs(err - want_err) <= 1e-13
    assert isinstance(mean, complex) == cplx


def test_one_bin_in_total_gives_an_infinite_error():
    _, hostapi = _built()
    mean, err = hostapi.binned_energy_stat(np.array([[1.5]]))            # one walker, one sample: a single bin
    assert mean == 1.5 and math.isinf(err) and err > 0
    mean, err = hostapi.binned_energy_stat(np.array([[1.5 + 2j]]))
    assert mean == 1.5 + 2j and math.isinf(err)
    mean, err = hostapi.binned_energy_stat(np.array([[2.0, 6.0]]))       # two walkers, one bin each: two bins in total
    assert mean == 4.0 and abs(err - 2.0) < 1e-15
    # S = 5: bins of two samples, the fifth sample of the walker is dropped
    mean, err = hostapi.binned_energy_stat(np.array([[1.0], [2.0], [3.0], [4.0], [100.0]]))
    assert mean == 2.5 and abs(err - 1.0) < 1e-15


def _tiny():
    flat = np.zeros((2, 2, 2, 2, 2, 2, 2))
    cfgs = np.array([[[0, 1], [1, 0]]] * 4, dtype=np.int32)
    return flat, cfgs


ADAM = (0.9, 0.999, 1e-8, 0.0)


def test_parameter_refusals_need_no_device():
    """zero walkers, zero samples, a seed count that differs from the walker count, a model / updater pair that does not belong
    together: std::invalid_argument (ValueError) before any contractor is built, so also on a machine without a GPU"""
    _, hostapi = _built()
    flat, cfgs = _tiny()
    seeds = np.arange(4) + 1
    with pytest.raises(ValueError, match="walker"):
        hostapi.vmc_optimize(flat, cfgs[:0], seeds[:0], 4, "xxz", (1.0, 1.0, 0.0), "exchange", "adam", 0.01, ADAM, 1)
    with pytest.raises(ValueError, match="samples_per_walker"):
        hostapi.vmc_optimize(flat, cfgs, seeds, 4, "xxz", (1.0, 1.0, 0.0), "exchange", "adam", 0.01, ADAM, 1, samples_per_walker=0)
    with pytest.raises(ValueError, match="seeds"):
        hostapi.vmc_optimize(flat, cfgs, seeds[:3], 4, "xxz", (1.0, 1.0, 0.0), "exchange", "adam", 0.01, ADAM, 1)
    with pytest.raises(ValueError, match="MCUpdateSquareNNFullSpaceUpdateOBC"):
        hostapi.vmc_optimize(flat, cfgs, seeds, 4, "tfim", (1.0,), "exchange", "adam", 0.01, ADAM, 1)
    with pytest.raises(ValueError, match="parameters"):
        hostapi.vmc_optimize(flat, cfgs, seeds, 4, "xxz", (1.0, 1.0, 0.0), "exchange", "adam", 0.01, ADAM[:2], 1)
    with pytest.raises(ValueError, match="strong-Wolfe"):
        hostapi.vmc_optimize(flat, cfgs, seeds, 4, "xxz", (1.0, 1.0, 0.0), "exchange", "lbfgs", 0.01, {"step_mode": "strong_wolfe"}, 1)


def test_fermionic_pair_refusals_need_no_device():
    _, hostapi = _built()
    from peps_amd import fermion
    st = fermion.FermionState.load(os.path.join(ROOT, "tests", "golden", "ref_fixtures",
                                                "spinless_fermion_tps_t2_0.000000_double_from_simple_update"))
    cfgs = np.array([[[0, 1], [1, 0]]] * 2, dtype=np.int32)
    with pytest.raises(ValueError, match="SquareHubbardModel"):
        hostapi.fermion_vmc_optimize(st, cfgs, [1, 2], 16, "spinless", (1.0, 0.0, 0.0), "hubbard_u1u1", "sgd", 0.1, (0.0, 0.0, 0.0), 1)
    with pytest.raises(ValueError, match="seeds"):
        hostapi.fermion_vmc_optimize(st, cfgs, [1, 2, 3], 16, "spinless", (1.0, 0.0, 0.0), "exchange", "sgd", 0.1, (0.0, 0.0, 0.0), 1)

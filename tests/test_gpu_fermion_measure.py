"""GPU tests of the measurement solvers of the fermionic models in the host layer (hostapi.fermion_observables,
fermion_exact_sum_measure, fermion_measure) and of the Python-driven registry fermion.tj_observables: slice path against hook path,
against the oracle's registry and the restated pairing estimator (tests/pair_ref.py), the exact sum against dense operators, and
MCPEPSMeasurer on the reference's 6 x 6 t-J fixture.

Setup of the per-walker tests: that of tests/test_gpu_pair_slice.py (3 x 4, D = 3 parity-even t-J state that does not conserve the
electron number, chi = 16 -- exact on this lattice --, 12 walkers)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_ref  # noqa: E402
import tj_nnn_ref as ref  # noqa: E402
import test_gpu_pair_slice as ps  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = ps.TOL
T, J, V, MU, T2 = 1.0, 0.4, 0.1, 0.3, 0.6
PRM = (T, J, V, MU, T2)
SC_KEYS = ("SC_bond_singlet_h", "SC_bond_singlet_v")
ALL_KEYS = {"energy", "spin_z", "charge", "bond_energy_h", "bond_energy_v", "bond_energy_dr", "bond_energy_ur"} | set(SC_KEYS)

_CACHE = {}


def _state(dtype):
    """the state of tests/test_gpu_pair_slice.py without a context"""
    from peps_amd import fermion
    st = ref.tj_state(ps.ROWS, ps.COLS, ps.D)
    if dtype == "c128":
        rng = np.random.default_rng(3)
        st = fermion.FermionState([[[t * np.exp(2j * np.pi * rng.uniform(size=t.shape)) for t in site] for site in row]
                                   for row in st.tensors], st.par, st.nf)
    return st


def _host(dtype, prm=PRM, model="tj"):
    """hostapi.fermion_observables of this process (the slice path), once per case"""
    key = ("host", dtype, prm, model)
    if key not in _CACHE:
        from peps_amd import capi, hostapi
        before = capi.diag_pair_slice_calls()
        obs, psi = hostapi.fermion_observables(_state(dtype), ps._configs(), ps.CHI, model, prm, dtype=0 if dtype == "f32" else 1)
        _CACHE[key] = (obs, psi, capi.diag_pair_slice_calls() - before)
    return _CACHE[key]


_HOOK = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_fermion_measure as m
from peps_amd import capi, hostapi
out = {}
for dt in ("f64", "f32", "c128"):
    obs, psi = hostapi.fermion_observables(m._state(dt), m.ps._configs(), m.ps.CHI, "tj", m.PRM, dtype=0 if dt == "f32" else 1)
    out[dt] = {k: [[float(x.real), float(x.imag)] for x in np.asarray(v, dtype=complex).ravel()] for k, v in obs.items()}
    out[dt]["psi_mean"] = [[float(x.real), float(x.imag)] for x in np.asarray(psi[0], dtype=complex)]
out["pair_slice_calls"] = capi.diag_pair_slice_calls()
print(json.dumps(out))
"""


def _hook():
    """the same through the per-bond hooks, PEPSHOST_NO_DEVICE_SWEEP=1 in ONE child process for the three element types"""
    if "hook" not in _CACHE:
        r = subprocess.run([sys.executable, "-c", _HOOK, ROOT], env=dict(os.environ, PEPSHOST_NO_DEVICE_SWEEP="1"), capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        raw = json.loads(r.stdout.strip().splitlines()[-1])
        assert raw.pop("pair_slice_calls") == 0              # the hook path never enters the slice
        _CACHE["hook"] = {dt: {k: np.array(v)[:, 0] + 1j * np.array(v)[:, 1] for k, v in d.items()} for dt, d in raw.items()}
    return _CACHE["hook"]


def _close(a, b, tol, what):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    assert a.shape == b.shape and a.size > 0, what
    scale = np.max(np.abs(b))
    err = np.max(np.abs(a - b))
    assert err <= tol * scale, (what, err / max(scale, 1e-300))


def _preconditions(psi_mean):
    ps._check_preconditions(ps._configs(), np.asarray(psi_mean))


@pytest.mark.parametrize("dtype", ["f64", "f32", "c128"])
def test_fermion_observables_slice_path_equals_hook_path_and_the_python_registry(dtype):
    from peps_amd import capi, fermion
    obs, psi, calls = _host(dtype)
    _preconditions(psi[0])
    assert set(obs) == ALL_KEYS and calls == ps.ROWS + ps.COLS      # one pair slice per row and per column
    assert obs["energy"].shape == (ps.NW, 1) and obs["SC_bond_singlet_h"].shape == (ps.NW, ps.ROWS * (ps.COLS - 1))
    assert obs["SC_bond_singlet_v"].shape == (ps.NW, (ps.ROWS - 1) * ps.COLS)
    for key in ("bond_energy_dr", "bond_energy_ur") + SC_KEYS:
        assert np.count_nonzero(obs[key]) > ps.NW, key              # dense: the state conserves nothing but parity
    hook = _hook()[dtype]
    tol = TOL[dtype]
    assert set(hook) == ALL_KEYS | {"psi_mean"}
    for key in ALL_KEYS:
        _close(obs[key], hook[key], tol, (dtype, "slice / hook", key))
    _close(np.abs(psi[0]), np.abs(hook["psi_mean"]), tol, (dtype, "psi"))
    st, ctx = ps._state(dtype)
    for path in ("slice", "calls"):
        py, psis = fermion.tj_observables(ctx, st, ps._configs(), T, J, V, MU, T2, pair=path)
        assert set(py) == ALL_KEYS and psis.shape == (ps.ROWS + ps.COLS, ps.NW)
        for key in ALL_KEYS:
            _close(py[key], obs[key], tol, (dtype, "python " + path + " / host slice", key))
            _close(py[key], hook[key], tol, (dtype, "python " + path + " / host hook", key))
    ctx.close()


def test_fermion_observables_nearest_neighbour_form_and_spinless_keys():
    """SquaretJNNModel reports the nearest-neighbour registry (no diagonal keys), with the numbers of SquaretJVModel at V = t2 = 0;
    SquareSpinlessFermion reports no spin_z and no pairing keys"""
    from peps_amd import capi, fermion, hostapi
    nn, _, _ = _host("f64", (T, J, MU), "tjnn")
    full, _, _ = _host("f64", (T, J, 0.0, MU, 0.0), "tj")
    assert set(nn) == ALL_KEYS - {"bond_energy_dr", "bond_energy_ur"}
    for key in nn:
        assert np.array_equal(nn[key], full[key]), key
    assert not np.any(full["bond_energy_dr"]) and not np.any(full["bond_energy_ur"])          # t2 = 0: zero-filled
    st = fermion.random_even_state(ps.ROWS, ps.COLS, ps.D, seed=31)
    cfgs = (ps._configs() == 2).astype(int)                        # (even electron number -> even number of occupied sites)
    obs, _ = hostapi.fermion_observables(st, cfgs, ps.CHI, "spinless", (1.0, 0.5, 0.7))
    assert set(obs) == {"energy", "charge", "bond_energy_h", "bond_energy_v", "bond_energy_dr", "bond_energy_ur"}
    ctx = capi.Context(ps.ROWS, ps.COLS, st.D, fermion.NVAR * st.d, ps.CHI, dtype=capi.F64, max_walkers=ps.NW)
    ctx.state_upload(st.extended_flat())
    py, _ = fermion.spinless_fermion_observables(ctx, st, cfgs, 1.0, 0.5, 0.7)
    ctx.close()
    for key in obs:
        _close(obs[key], py[key], 1e-9, ("spinless", key))


def _oracle():
    """the oracle's registry (t2 = 0) and the restated pairing estimator on the oracle's amplitudes, once"""
    if "oracle" not in _CACHE:
        from oracle import fermion as ofermion
        from oracle.bmps import BMPSTruncateParams
        fs = ref.oracle_view(ref.tj_state(ps.ROWS, ps.COLS, ps.D))
        tp = BMPSTruncateParams.SVD(ps.CHI, ps.CHI, 0.0)
        model = ofermion.SquaretJVModelOBC(T, 0.0, J, V, MU)
        memo = {}

        def amp(c):
            k = np.asarray(c).tobytes()
            if k not in memo:
                memo[k] = fs.amplitude(c, tp)
            return memo[k]
        regs, scs = [], []
        for cfg in ps._configs():
            regs.append(model.EvaluateObservables(fs, cfg, tp))
            scs.append(pair_ref.sc_from_amplitudes(cfg, amp)[0])
        _CACHE["oracle"] = (regs, scs)
    return _CACHE["oracle"]


def test_fermion_observables_against_the_oracle_registry_and_the_restated_pairing_estimator():
    """f64, t2 = 0: every non-SC key against oracle.fermion.SquaretJVModelOBC.EvaluateObservables at 1e-9 relative; SC per walker
    against the restatement on fresh oracle amplitudes at 1e-9"""
    obs, psi, _ = _host("f64", (T, J, V, MU, 0.0))
    _preconditions(psi[0])
    regs, scs = _oracle()
    for key in ALL_KEYS - set(SC_KEYS):
        want = np.array([np.asarray(r[key]).ravel() for r in regs])
        _close(obs[key], want, 1e-9, ("oracle", key))
    for key, short in zip(SC_KEYS, ("h", "v")):
        want = np.array([s[short].ravel() for s in scs])
        assert np.max(np.abs(want.imag)) == 0 and np.count_nonzero(want) > ps.NW
        _close(obs[key], want.real, 1e-9, ("restated SC", key))


def test_fermion_exact_sum_measure_equals_the_dense_operators():
    """the 2 x 3, D = 2 state, f64, chi = 64 (exact), summed over its 729 configurations -- handed over are the 365 parity-even ones: the
    others have amplitude zero by symmetry, weigh nothing in any sum, and a zero amplitude is refused by the solver.  SC_bond_singlet_h /
    _v equal the dense <Delta_ij> at 1e-9, the energy the Rayleigh quotient of the dense t-t'-J Hamiltonian at 1e-9, and the shares of 4
    ranks sum to the same values"""
    from oracle.bmps import BMPSTruncateParams
    from peps_amd import hostapi
    rows, cols = 2, 3
    st = ref.tj_state(rows, cols, 2)
    allc = ref.all_tj_configs(rows, cols)
    even = allc[np.sum(allc != ref.EMPTY, axis=(1, 2)) % 2 == 0]
    assert len(allc) == 729 and len(even) == 365
    fs = ref.oracle_view(st)
    tp = BMPSTruncateParams.SVD(64, 64, 0.0)
    psi = np.array([fs.amplitude(c, tp) if np.sum(c != ref.EMPTY) % 2 == 0 else 0.0 for c in allc])
    sums, weight = hostapi.fermion_exact_sum_measure(st, even, 64, "tj", PRM, batch=128)
    got = {k: v / weight for k, v in sums.items()}
    assert set(got) == ALL_KEYS
    want_e = ref.rayleigh(ref.dense_ttj_hamiltonian(rows, cols, T, T2, J, V, MU), psi)
    assert abs(got["energy"][0] - want_e) <= 1e-9 * abs(want_e), (got["energy"][0], want_e)
    dense = {"h": [], "v": []}
    for key, s1, s2 in pair_ref.nn_bonds(rows, cols):
        M = pair_ref.dense_delta(rows, cols, s1[0] * cols + s1[1], s2[0] * cols + s2[1])
        dense[key].append((np.conj(psi) @ (M @ psi)) / (np.conj(psi) @ psi))
    for key, short in zip(SC_KEYS, ("h", "v")):
        want = np.array(dense[short])
        assert np.min(np.abs(want)) > 1e-4
        assert np.max(np.abs(got[key] - want)) <= 1e-9, (key, got[key], want)
    parts = [hostapi.fermion_exact_sum_measure(st, even, 64, "tj", PRM, rank=r, size=4, batch=128) for r in range(4)]
    wsum = sum(p[1] for p in parts)
    assert abs(wsum - weight) <= 1e-12 * weight
    for key in ALL_KEYS:
        tot = sum(p[0][key] for p in parts)
        assert np.max(np.abs(tot - sums[key])) <= 1e-12 * max(np.max(np.abs(sums[key])), weight), key


@pytest.mark.parametrize("dtype", ["f64", "c128"])
def test_python_exact_sum_with_the_tj_keyword_equals_the_host_layer(dtype):
    """fermion.exact_sum_measure(.., tj=(J, mu)) -- the Python-driven registry summed with |psi|^2 -- against
    hostapi.fermion_exact_sum_measure on the 2 x 3 state (c128: random phases on the stored tensors), every key at 1e-9 of the
    largest sum; the spinless default of the keyword is untouched (tests/test_gpu_fermion.py)"""
    from peps_amd import capi, fermion, hostapi
    rows, cols = 2, 3
    st = ref.tj_state(rows, cols, 2)
    if dtype == "c128":
        rng = np.random.default_rng(5)
        st = fermion.FermionState([[[t * np.exp(2j * np.pi * rng.uniform(size=t.shape)) for t in site] for site in row]
                                   for row in st.tensors], st.par, st.nf)
    allc = ref.all_tj_configs(rows, cols)
    even = allc[np.sum(allc != ref.EMPTY, axis=(1, 2)) % 2 == 0]
    sums, weight = hostapi.fermion_exact_sum_measure(st, even, 64, "tj", PRM, batch=128)
    ctx = capi.Context(rows, cols, st.D, fermion.NVAR * st.d, 64, dtype=capi.C128 if dtype == "c128" else capi.F64, max_walkers=128)
    ctx.state_upload(st.extended_flat())
    acc, wsum = fermion.exact_sum_measure(ctx, st, even, T, V, batch=128, t2=T2, tj=(J, MU))
    ctx.close()
    assert set(acc) == set(sums) == ALL_KEYS and abs(wsum - weight) <= 1e-12 * weight
    if dtype == "c128":
        assert np.max(np.abs(np.imag(sums["SC_bond_singlet_h"]))) > 1e-6 * weight
    for key in ALL_KEYS:
        _close(acc[key], sums[key], 1e-9, (dtype, key))


def test_fermion_measure_on_a_complex_state_samples_the_energies_of_fermion_measure_energy():
    """the complex instantiation of MCPEPSMeasurer on the 3 x 4 state with random phases: the energy samples are those of
    fermion_measure_energy bit for bit (t2 != 0: the entry with a parameter count), the registry's energy is their mean over samples
    and walkers, and its pairing values are complex"""
    from peps_amd import hostapi
    st, cfgs = _state("c128"), ps._configs()
    seeds = np.arange(ps.NW, dtype=np.uint64) + 7
    reg, psi, en, cfg_m, rates = hostapi.fermion_measure(st, cfgs, seeds, ps.CHI, 1, 2, 1, "tj", PRM)
    en_e, cfg_e, _ = hostapi.fermion_measure_energy(st, cfgs, seeds, ps.CHI, 1, 2, 1, "tj", t=T, J=J, V=V, mu=MU, t2=T2)
    assert set(reg) == ALL_KEYS and en.dtype == np.complex128 and en.shape == (2, ps.NW)
    assert np.array_equal(en, en_e) and np.array_equal(cfg_m, cfg_e)
    assert abs(reg["energy"][0][0] - np.mean(en)) <= 1e-12 * abs(np.mean(en))
    assert reg["energy"][1].shape == (1,) and reg["energy"][1][0] > 0          # standard error across the 12 walkers
    assert np.max(np.abs(reg["SC_bond_singlet_h"][0].imag)) > 0 and np.all(np.isfinite(reg["SC_bond_singlet_v"][0]))
    assert np.all(np.abs(psi[0]) > 0) and np.all((rates >= 0) & (rates <= 1))


def test_fermion_measure_on_the_reference_tj_fixture(fixtures_dir):
    """MCPEPSMeasurer on the reference's 6 x 6 t-J state (two holes, fU1 tensors, D = 8) with the seed and sweep counts of
    tests/test_gpu_fermion.py::test_k9_reference_tj_measurer_regression_energy_on_the_device: the mean energy reproduces the
    reference's -14.74320489110316 at 1e-8, the energy samples are those of fermion_measure_energy bit for bit, and every pairing value
    is below 1e-10 -- the state conserves the electron number"""
    from peps_amd import fermion, hostapi
    d = os.path.join(fixtures_dir, "tps_tJ_6x6Hole2_J0.3_D8_fU1")
    st = fermion.FermionState.load(d)
    cfg = np.loadtxt(os.path.join(d, "configuration0"), dtype=int).reshape(1, 6, 6)
    hostapi.set_truncate_params(8, 1e-15, 0)                       # BMPSTruncateParams::SVD(8, 16, 1e-15)
    try:
        reg, psi, en, cfg_m, rates_m = hostapi.fermion_measure(st, cfg, [42], 16, 10, 10, 1, "tjnn", (1.0, 0.3, 0.0))
        en_e, cfg_e, rates_e = hostapi.fermion_measure_energy(st, cfg, [42], 16, 10, 10, 1, "tj", t=1.0, J=0.3, V=0.0, mu=0.0, dtype=1)
    finally:
        hostapi.set_truncate_params()
    assert set(reg) == ALL_KEYS - {"bond_energy_dr", "bond_energy_ur"}
    e = float(reg["energy"][0][0])
    print("fermion_measure on the K9 fixture: energy %.14f (reference -14.74320489110316, diff %.1e)" % (e, abs(e + 14.74320489110316)))
    assert abs(e - (-14.74320489110316)) < 1e-8
    assert en.shape == (10, 1) and np.array_equal(en, en_e)
    assert np.array_equal(cfg_m, cfg_e) and np.array_equal(rates_m, rates_e)
    assert abs(float(np.mean(en[:, 0])) - e) < 1e-12
    assert abs(reg["charge"][0].sum() - 34.0) < 1e-12              # two holes, and the exchange updater keeps them
    for key in SC_KEYS:
        assert np.max(np.abs(reg[key][0])) < 1e-10, (key, np.max(np.abs(reg[key][0])))
    assert np.isfinite(psi[0][0]) and abs(psi[0][0]) > 0

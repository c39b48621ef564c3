"""CPU checks of the Hubbard convention and of the new entry points.

1. The restated E_loc (tests/hubbard_ref.py: the hop rule s_up = (-1)^(n_down of site 1), s_down = (-1)^(n_up of site 2) on fresh
   oracle amplitudes, jw = (-1)^(odd sites strictly between the two sites in row-major order)) against a dense Jordan-Wigner Hubbard
   Hamiltonian built from mode operators: the |psi|^2-weighted mean over ALL parity-even configurations is the Rayleigh quotient.
2. The hop rule tabulated over the 16 pairs equals the coefficients transcribed from square_hubbard_model.h:200-262
   (tests/golden/hubbard_bond_coefficients.json), and fermion.hubbard_hop_table() states the same rule.
3. fermion.hubbard_sector_table() is EnumerateHubbardTwoSiteConfigsWithU1U1's order, conserves (N_up, N_down), sector sizes {1, 2, 4}.
4. The dense H is symmetric and conserves N_up and N_down.
5. Every new pepsgpu_* and pepshost_* symbol is declared, exported and bound (no compute call is made), and the host layer's tables
   equal the Python ones."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hubbard_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, U, MU = 1.0, 3.0, 0.4
NEW_GPU = ("pepsgpu_sweep_slice_sector", "pepsgpu_diag_sector_cand", "pepsgpu_diag_sector_slice_calls", "pepsgpu_nn_hop_slice_fermion",
           "pepsgpu_diag_hop_slice_calls", "pepsgpu_trace_scaling")

NEW_HOST = ("pepshost_fermion_measure_updater", "pepshost_hubbard_sector_table", "pepshost_hubbard_hop_table")

_CACHE = {}


def _amplitudes(shape):
    """psi(S) of all 4^N configurations of a random parity-even D = 2 state, zero for the parity-odd ones (computed once per lattice)"""
    if shape not in _CACHE:
        from oracle.bmps import BMPSTruncateParams
        rows, cols = shape
        fs = ref.oracle_view(ref.hubbard_state(rows, cols, 2))
        tp = BMPSTruncateParams.SVD(64, 64, 0.0)                  # exact on these lattices
        cfgs = ref.all_configs(rows, cols)
        even = ref.is_even(cfgs)
        psi = np.zeros(len(cfgs))
        for k in np.nonzero(even)[0]:
            psi[k] = fs.amplitude(cfgs[k], tp)
        _CACHE[shape] = (cfgs, even, psi)
    return _CACHE[shape]


@pytest.mark.parametrize("shape,n_even", [((2, 2), 128), ((2, 3), 2048), ((3, 2), 2048)])
def test_restated_hubbard_local_energy_equals_the_dense_hamiltonian(shape, n_even):
    """t = 1, U = 3, mu = 0.4: the weighted mean of the restated E_loc over all parity-even configurations equals the Rayleigh quotient
    of the dense H to 1e-12 relative (both are float64 sums of a few thousand terms of order 1), and flipping s_down alone moves the
    mean by more than 1e-6."""
    rows, cols = shape
    cfgs, even, psi = _amplitudes(shape)
    assert int(even.sum()) == n_even
    assert np.all(psi[even] != 0)

    def amp_of(c):
        return psi[ref.config_index(c)]

    e_loc, e_flip, terms = np.zeros(len(cfgs), complex), np.zeros(len(cfgs), complex), 0
    for k in np.nonzero(even)[0]:
        e_loc[k], n = ref.local_energy(amp_of, cfgs[k], T, U, MU)
        e_flip[k], _ = ref.local_energy(amp_of, cfgs[k], T, U, MU, sign_dn=-1)
        terms += n
    w = np.abs(psi) ** 2
    mean, flipped = np.sum(w * e_loc) / np.sum(w), np.sum(w * e_flip) / np.sum(w)
    quot = ref.rayleigh(ref.dense_hubbard_hamiltonian(rows, cols, T, U, MU), psi)
    print("Hubbard", shape, "even configurations %d, hop terms %d, E = %.15g, |mean - quotient| / |quotient| = %.2e, "
          "mean(s_down flipped) - mean = %.6e" % (n_even, terms, quot.real, abs(mean - quot) / abs(quot), (flipped - mean).real))
    assert terms >= 4 * n_even // 2
    assert abs(flipped - mean) > 1e-6
    assert abs(mean - quot) <= 1e-12 * abs(quot)


@pytest.mark.parametrize("shape", [(2, 3), (3, 2)])
def test_traversal_form_equals_the_fresh_amplitude_form(shape):
    """hubbard_ref.cal_energy (Trace + ReplaceNNSiteTrace inside the row and the column pass: what the device and the host layer
    compute) equals hubbard_ref.local_energy (fresh global amplitudes with the explicit string, pinned to the dense H above), bond by
    bond, on 24 parity-even configurations at exact chi: 1e-10 of the largest bond term of the configuration (a ratio of amplitudes
    reaches 1e3 where psi(S) is small; float64 contractions of a few hundred terms)."""
    from oracle.bmps import BMPSTruncateParams
    rows, cols = shape
    cfgs, even, psi = _amplitudes(shape)
    fs = ref.oracle_view(ref.hubbard_state(rows, cols, 2))
    tp = BMPSTruncateParams.SVD(64, 64, 0.0)
    pick = np.nonzero(even)[0][np.random.default_rng(1).permutation(int(even.sum()))[:24]]
    worst = 0.0
    for k in pick:
        b1, b2 = {}, {}
        e1, _ = ref.cal_energy(fs, cfgs[k], tp, T, U, MU, b1)
        e2, _ = ref.local_energy(lambda c: psi[ref.config_index(c)], cfgs[k], T, U, MU, bonds=b2)
        scale = max(1.0, float(np.max(np.abs(b2["h"]))), float(np.max(np.abs(b2["v"]))))
        worst = max(worst, max(abs(e1 - e2), float(np.max(np.abs(b1["h"] - b2["h"]))), float(np.max(np.abs(b1["v"] - b2["v"])))) / scale)
    print("Hubbard", shape, "traversal form - fresh form: max %.2e of the largest bond term" % worst)
    assert worst < 1e-10


def test_hop_rule_equals_the_transcribed_reference_table():
    with open(os.path.join(ROOT, "tests", "golden", "hubbard_bond_coefficients.json")) as f:
        golden = sorted(json.load(f)["coefficients"])
    assert len(golden) == 16
    assert ref.bond_coefficients() == golden
    from peps_amd import fermion
    table, sign = fermion.hubbard_hop_table()
    assert table.shape == (16, 2, 2) and sign.shape == (16, 2)
    mine = sorted([a, b, int(table[a * 4 + b, k, 0]), int(table[a * 4 + b, k, 1]), -int(sign[a * 4 + b, k])]
                  for a in range(4) for b in range(4) for k in range(2) if table[a * 4 + b, k, 0] >= 0)
    assert mine == golden
    assert np.all((table[:, :, 0] < 0) == (sign == 0)) and np.all((table[:, :, 0] < 0) == (table[:, :, 1] < 0))
    for a in range(4):
        assert np.all(table[a * 4 + a] == -1)                                 # equal states: nothing (:200-202)
    assert tuple(fermion.HUBBARD_NF) == ref.NF


def test_sector_table_is_the_enumeration_order_and_conserves_both_numbers():
    from peps_amd import fermion
    tab = fermion.hubbard_sector_table()
    assert tab.shape == (16, 10) and tab.dtype == np.int32
    sizes = set()
    for a in range(4):
        for b in range(4):
            row = tab[a * 4 + b]
            valid = ref.sector(a, b)
            m, init = int(row[0]), int(row[1])
            sizes.add(m)
            assert m == len(valid) and valid[init] == (a, b)
            assert [tuple(x) for x in row[2:2 + 2 * m].reshape(m, 2).tolist()] == valid
            assert np.all(row[2 + 2 * m:] == -1)
            for a2, b2 in valid:
                assert ref.N_UP[a2] + ref.N_UP[b2] == ref.N_UP[a] + ref.N_UP[b]
                assert ref.N_DN[a2] + ref.N_DN[b2] == ref.N_DN[a] + ref.N_DN[b]
    assert sizes == {1, 2, 4}
    # the order is a' in the outer loop, b' in the inner one
    assert ref.sector(1, 2) == [(0, 3), (1, 2), (2, 1), (3, 0)]


def test_dense_hamiltonian_is_symmetric_and_conserves_both_numbers():
    H = ref.dense_hubbard_hamiltonian(2, 2, T, U, MU)
    assert np.array_equal(H, H.T)
    cfgs = ref.all_configs(2, 2)
    nu, nd = np.sum(ref.N_UP[cfgs], axis=(1, 2)), np.sum(ref.N_DN[cfgs], axis=(1, 2))
    assert np.all(H[(nu[:, None] != nu[None, :]) | (nd[:, None] != nd[None, :])] == 0.0)
    assert np.count_nonzero(H - np.diag(np.diag(H))) > 0
    # the diagonal is U (#doublons) - mu (#electrons)
    assert np.allclose(np.diag(H), [ref.onsite_energy(c, U, MU) for c in cfgs], rtol=0, atol=1e-14)


def test_hubbard_entry_points_declared_exported_and_bound():
    from peps_amd import capi, fermion, hostapi
    if not (os.path.exists(capi.LIB_PATH) and os.path.exists(hostapi.LIB_PATH)):
        import __graft_entry__ as g
        g.build()
    header = open(os.path.join(ROOT, "include", "pepsgpu.h")).read()
    declared = set(re.findall(r"\b(pepsgpu_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW_GPU:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
    bound = capi.load_library()
    assert len(bound.pepsgpu_sweep_slice_sector.argtypes) == 13
    assert len(bound.pepsgpu_diag_sector_cand.argtypes) == 13
    assert len(bound.pepsgpu_nn_hop_slice_fermion.argtypes) == 9
    assert len(bound.pepsgpu_trace_scaling.argtypes) == 2 and callable(getattr(capi.Context, "trace_scaling"))
    for name in ("pepsgpu_diag_sector_slice_calls", "pepsgpu_diag_hop_slice_calls"):
        assert len(getattr(bound, name).argtypes) == 0 and getattr(bound, name).restype is ctypes.c_long
    assert callable(getattr(capi.Context, "sweep_slice_sector")) and callable(getattr(capi.Context, "nn_hop_slice_fermion"))
    assert callable(capi.diag_sector_cand)
    assert capi.diag_sector_slice_calls() >= 0 and capi.diag_hop_slice_calls() >= 0      # asking needs no device
    assert callable(fermion.hubbard_energy) and callable(fermion.hubbard_observables)
    capi.lib()
    host = ctypes.CDLL(hostapi.LIB_PATH)
    for name in NEW_HOST:
        assert hasattr(host, name), name
        assert name in hostapi.SYMBOLS, name
    assert hostapi.FERMION_UPDATER_ID["hubbard_u1u1"] == 3 and hostapi.FERMION_MODEL_ID["hubbard"] == 3
    assert hostapi.FERMION_MEASURE_MODEL_ID["hubbard"] == 3
    # the host layer's tables (HubbardSectorTable, SquareHubbardModel::HopTable) are the Python ones; no device is touched
    sec, hop = hostapi.hubbard_tables()
    assert np.array_equal(sec, fermion.hubbard_sector_table())
    assert np.array_equal(hop, fermion.hubbard_hop_table()[0])

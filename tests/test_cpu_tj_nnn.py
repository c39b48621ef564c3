"""CPU checks of the t-t'-J convention and of the new entry points.

1. The restated diagonal hop (tests/tj_nnn_ref.py: jw = (-1)^(electrons strictly between the two ends in row-major order), a hop only
   where exactly one end is empty) against a dense Jordan-Wigner t-t'-J Hamiltonian built independently: the |psi|^2-weighted mean of
   E_loc over ALL configurations is the Rayleigh quotient <psi|H|psi> / <psi|psi>.
2. pepsgpu_nnn_hop_slice_fermion, pepsgpu_diag_fermion_hop_cand, pepsgpu_diag_nnn_hop_slice_calls and the host shim's entry points
   with a parameter count are declared, exported and bound (no compute call is made)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tj_nnn_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, J, V, MU = 1.0, 0.4, 0.1, 0.3
NEW_GPU = ("pepsgpu_nnn_hop_slice_fermion", "pepsgpu_diag_fermion_hop_cand", "pepsgpu_diag_nnn_hop_slice_calls")
NEW_HOST = ("pepshost_fermion_energy_prm", "pepshost_fermion_measure_energy_prm")

_CACHE = {}


def _amplitudes_and_nn_energy(shape):
    """psi(S) and the nearest-neighbour E_loc(S) of all 3^N configurations (computed once per lattice, shared by the t2 cases)"""
    if shape not in _CACHE:
        from oracle import fermion as ofermion
        from oracle.bmps import BMPSTruncateParams
        rows, cols = shape
        fs = ref.oracle_view(ref.tj_state(rows, cols, 2))
        tp = BMPSTruncateParams.SVD(64, 64, 0.0)                  # exact on these lattices
        cfgs = ref.all_tj_configs(rows, cols)
        psi = np.array([fs.amplitude(c, tp) for c in cfgs])
        # a parity-odd configuration has amplitude zero by symmetry; the contraction returns rounding noise for some of them
        psi[np.abs(psi) < 1e-12 * np.max(np.abs(psi))] = 0.0
        model = ofermion.SquaretJVModelOBC(T, 0.0, J, V, MU)
        e_nn = np.array([model.CalEnergy(fs, c, tp)[0] if psi[k] != 0 else 0.0 for k, c in enumerate(cfgs)])
        _CACHE[shape] = (fs, tp, cfgs, psi, e_nn)
    return _CACHE[shape]


@pytest.mark.parametrize("t2", [0.7, -0.6])
@pytest.mark.parametrize("shape", [(2, 3), (3, 2)])
def test_restated_tj_diagonal_hop_equals_the_dense_hamiltonian(shape, t2):
    """All 729 configurations of a random parity-even D = 2 t-J state, t = 1, J = 0.4, V = 0.1, mu = 0.3: the weighted mean of the restated
    E_loc equals the Rayleigh quotient of the dense H to 1e-12 relative (both are float64 sums of a few thousand terms of order 1;
    measured <= 4e-16), over at least 600 allowed diagonal terms, and t2 moves the quotient by more than 1e-6."""
    rows, cols = shape
    fs, tp, cfgs, psi, e_nn = _amplitudes_and_nn_energy(shape)
    assert len(cfgs) == 729
    live = psi != 0
    assert np.array_equal(live, np.sum(cfgs != ref.EMPTY, axis=(1, 2)) % 2 == 0)      # exactly the parity-even configurations
    e_loc, terms = np.zeros(len(cfgs), complex), 0
    for k in np.nonzero(live)[0]:
        e_nnn, count = ref.nnn_energy(fs, cfgs[k], tp, t2, "tj", psi0=psi[k])
        e_loc[k] = e_nn[k] + e_nnn
        terms += count
    w = np.abs(psi) ** 2
    mean = np.sum(w * e_loc) / np.sum(w)
    quot = ref.rayleigh(ref.dense_ttj_hamiltonian(rows, cols, T, t2, J, V, MU), psi)
    quot0 = ref.rayleigh(ref.dense_ttj_hamiltonian(rows, cols, T, 0.0, J, V, MU), psi)
    print("t-t'-J", shape, "t2 = %g: non-zero amplitudes %d, diagonal terms %d, E = %.15g, |mean - quotient| / |quotient| = %.2e, "
          "quotient - quotient(t2 = 0) = %.6e" % (t2, int(live.sum()), terms, quot.real, abs(mean - quot) / abs(quot), (quot - quot0).real))
    assert terms >= 600
    assert abs(quot - quot0) > 1e-6
    assert abs(mean - quot) <= 1e-12 * abs(quot)


def test_dense_hamiltonian_is_symmetric_and_conserves_the_electron_number():
    H = ref.dense_ttj_hamiltonian(2, 3, T, 0.7, J, V, MU)
    assert np.array_equal(H, H.T)
    ne = np.sum(ref.all_tj_configs(2, 3) != ref.EMPTY, axis=(1, 2))
    assert np.all(H[ne[:, None] != ne[None, :]] == 0.0)


def test_hop_slice_entry_points_declared_exported_and_bound():
    from peps_amd import capi, hostapi
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
    assert len(bound.pepsgpu_nnn_hop_slice_fermion.argtypes) == 7
    assert len(bound.pepsgpu_diag_fermion_hop_cand.argtypes) == 11
    assert len(bound.pepsgpu_diag_nnn_hop_slice_calls.argtypes) == 0 and bound.pepsgpu_diag_nnn_hop_slice_calls.restype is ctypes.c_long
    assert callable(getattr(capi.Context, "nnn_hop_slice_fermion"))
    assert callable(capi.diag_fermion_hop_cand) and callable(capi.diag_nnn_hop_slice_calls)
    assert capi.diag_nnn_hop_slice_calls() == 0                  # no slice has run in this process; asking needs no device
    capi.lib()
    host = ctypes.CDLL(hostapi.LIB_PATH)
    for name in NEW_HOST:
        assert hasattr(host, name), name
        assert name in hostapi.SYMBOLS, name

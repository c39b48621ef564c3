"""CPU checks of the bond-singlet pairing convention and of the pair slice's entry points.

1. The restated estimator (tests/pair_ref.py) on the oracle's amplitudes against an independently built dense Delta_ij: the
   |psi|^2-weighted mean over ALL configurations is <Psi|Delta_ij|Psi> / <Psi|Psi>.  The states do not conserve the electron number
   (on a U(1)-symmetric state every pair amplitude is exactly zero and no sign error would show).
2. The local path: -ReplaceNNSiteTrace / Trace of the oracle's row and column pass equals jw x the ratio of fresh amplitudes; the
   unsigned ratio fails the dense pin.
3. pepsgpu_nn_pair_slice_fermion, pepsgpu_diag_pair_slice_calls and pepsgpu_diag_pair_cand are declared, exported and bound; the three
   pepshost_fermion_* measurement entries are exported and listed.
4. The candidate rule as a pure function against FermionState.ext_config of the changed configuration."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_ref  # noqa: E402
import tj_nnn_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_GPU = ("pepsgpu_nn_pair_slice_fermion", "pepsgpu_diag_pair_slice_calls", "pepsgpu_diag_pair_cand")
NEW_HOST = ("pepshost_fermion_observables", "pepshost_fermion_exact_sum_measure_partial", "pepshost_fermion_measure")
SHAPES = [(2, 3), (3, 2)]

_CACHE = {}


def _lattice(shape):
    """per lattice, computed once: the oracle state, psi of all 3^N configurations, the fresh-amplitude registry values and the local
    path's raw ratios of every parity-even configuration"""
    if shape not in _CACHE:
        from oracle.bmps import BMPSTruncateParams
        rows, cols = shape
        fs = ref.oracle_view(ref.tj_state(rows, cols, 2))
        tp = BMPSTruncateParams.SVD(64, 64, 0.0)                  # exact on these lattices
        cfgs = ref.all_tj_configs(rows, cols)
        psi = np.array([fs.amplitude(c, tp) for c in cfgs])
        psi[np.abs(psi) < 1e-12 * np.max(np.abs(psi))] = 0.0      # parity-odd configurations: zero by symmetry
        pw = 3 ** np.arange(rows * cols - 1, -1, -1)
        amp = lambda c: psi[int(np.asarray(c).ravel() @ pw)]
        live = np.nonzero(psi != 0)[0]
        fresh, terms = {}, 0
        for k in live:
            fresh[k], t = pair_ref.sc_from_amplitudes(cfgs[k], amp)
            terms += t
        local = {k: pair_ref.local_pair_ratios(fs, cfgs[k], tp) for k in live}
        _CACHE[shape] = dict(fs=fs, cfgs=cfgs, psi=psi, amp=amp, live=live, fresh=fresh, terms=terms, local=local)
    return _CACHE[shape]


def _weighted_mean(lat, per_config):
    w = np.abs(lat["psi"]) ** 2
    out = {}
    for key in ("h", "v"):
        out[key] = sum(w[k] * per_config[k][key] for k in lat["live"]) / np.sum(w)
    return out


def _dense_expectation(shape, psi):
    rows, cols = shape
    out = {"h": np.zeros((rows, cols - 1), complex), "v": np.zeros((rows - 1, cols), complex)}
    for key, s1, s2 in pair_ref.nn_bonds(rows, cols):
        M = pair_ref.dense_delta(rows, cols, s1[0] * cols + s1[1], s2[0] * cols + s2[1])
        out[key][s1] = (np.conj(psi) @ (M @ psi)) / (np.conj(psi) @ psi)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_restated_sc_estimator_equals_the_dense_pair_operator(shape):
    """All 729 configurations of a random parity-even D = 2 t-J state: the weighted mean of the restated estimator equals <Delta_ij> of
    the dense operator to 1e-12 absolute on each of the 7 bonds (float64 sums of a few hundred terms of order <= 1), over at least 500
    non-zero pair terms, with |<Delta_ij>| > 1e-4 on every bond.  The local path with Sigma(S') / Sigma(S) = -1 gives the same means (1e-9:
    the tolerance of the local path, see the next test); without that sign it misses the dense value by more than 1e-4 on some bond."""
    lat = _lattice(shape)
    assert len(lat["cfgs"]) == 729
    assert np.array_equal(lat["psi"] != 0, np.sum(lat["cfgs"] != ref.EMPTY, axis=(1, 2)) % 2 == 0)
    dense = _dense_expectation(shape, lat["psi"])
    mean = _weighted_mean(lat, lat["fresh"])
    signed = _weighted_mean(lat, {k: pair_ref.sc_from_local_ratios(lat["cfgs"][k], lat["local"][k]) for k in lat["live"]})
    unsigned = _weighted_mean(lat, {k: pair_ref.sc_from_local_ratios(lat["cfgs"][k], lat["local"][k], sign=1.0) for k in lat["live"]})
    nbonds, worst, worst_signed, smallest, miss = 0, 0.0, 0.0, np.inf, 0.0
    for key in ("h", "v"):
        nbonds += dense[key].size
        worst = max(worst, float(np.max(np.abs(mean[key] - dense[key]))))
        worst_signed = max(worst_signed, float(np.max(np.abs(signed[key] - dense[key]))))
        smallest = min(smallest, float(np.min(np.abs(dense[key]))))
        miss = max(miss, float(np.max(np.abs(unsigned[key] - dense[key]))))
    print("pair", shape, "terms %d, max |mean - dense| = %.2e, local path %.2e, min |<Delta>| = %.3e, unsigned local path misses by %.3e"
          % (lat["terms"], worst, worst_signed, smallest, miss))
    assert nbonds == 7
    assert lat["terms"] >= 500
    assert smallest > 1e-4
    assert worst <= 1e-12
    assert worst_signed <= 1e-9
    assert miss > 1e-4


@pytest.mark.parametrize("shape", SHAPES)
def test_local_path_with_the_sign_rule_equals_fresh_amplitudes(shape):
    """every pair term of the lattice, row pass (horizontal bonds) and column pass (vertical bonds): -ReplaceNNSiteTrace / Trace equals
    jw x the ratio of fresh amplitudes at 1e-9 relative; no Kappa factor enters"""
    lat = _lattice(shape)
    rows, cols = shape
    count = {"h": 0, "v": 0}
    unsigned_match = 0
    for k in lat["live"]:
        cfg = lat["cfgs"][k]
        for key, s1, s2 in pair_ref.nn_bonds(rows, cols):
            for slot, cand in enumerate(pair_ref.pair_candidates(int(cfg[s1]), int(cfg[s2]))):
                if cand is None:
                    continue
                new = cfg.copy()
                new[s1], new[s2] = cand
                want = pair_ref.jw_between(cfg, s1, s2) * lat["amp"](new) / lat["amp"](cfg)
                raw = lat["local"][k][(key, s1, slot)]
                assert abs(-raw - want) <= 1e-9 * abs(want), (shape, k, key, s1, slot, raw, want)
                unsigned_match += abs(raw - want) <= 1e-9 * abs(want)
                count[key] += 1
    print("local path", shape, count)
    assert count["h"] >= 200 and count["v"] >= 200 and count["h"] + count["v"] == lat["terms"]
    assert unsigned_match == 0


def test_pair_slice_entry_points_declared_exported_and_bound():
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
    assert len(bound.pepsgpu_nn_pair_slice_fermion.argtypes) == 10
    assert len(bound.pepsgpu_diag_pair_cand.argtypes) == 12
    assert len(bound.pepsgpu_diag_pair_slice_calls.argtypes) == 0 and bound.pepsgpu_diag_pair_slice_calls.restype is ctypes.c_long
    assert callable(getattr(capi.Context, "nn_pair_slice_fermion"))
    assert callable(capi.diag_pair_cand) and callable(capi.diag_pair_slice_calls)
    assert capi.diag_pair_slice_calls() == 0                     # no slice has run in this process; asking needs no device
    capi.lib()
    host = ctypes.CDLL(hostapi.LIB_PATH)
    for name in NEW_HOST:
        assert hasattr(host, name), name
        assert name in hostapi.SYMBOLS, name
    for name in ("fermion_observables", "fermion_exact_sum_measure", "fermion_measure"):
        assert callable(getattr(hostapi, name)), name


@pytest.mark.parametrize("order", [0, 1])
def test_candidate_rule_equals_ext_config_of_the_changed_configuration(order):
    """a four-site chain along the mode order (1 x 4 row-major, 4 x 1 column-major): a site that sets the parity before the bond, the
    bond, a site behind it.  Every (a, b, variant) of d = 3 and both candidate slots of the t-J pair table, plus a table with
    number-conserving candidates (the exchange written as a pair move): the rule's extended states equal ext_config of the changed
    configuration, the site behind the bond keeps its state, and the sign is -1 exactly where the electron number changes by 2."""
    from peps_amd import fermion
    shape = (1, 4) if order == 0 else (4, 1)
    st = ref.tj_state(shape[0], shape[1], 2)
    swap = -np.ones((9, 2, 2), dtype=np.int32)
    for a, b in itertools.product(range(3), repeat=2):
        swap[a * 3 + b, 0] = (b, a)                                # (keeps the parity of the pair)
    seen = set()
    for table in (pair_ref.tj_pair_table(), swap):
        for first, a, b, last in itertools.product(range(3), repeat=4):
            cfg = np.array([first, a, b, last]).reshape(shape)
            ext = st.ext_config(cfg, order).ravel()
            cand, sign = pair_ref.pair_cand_rule(int(ext[1]), int(ext[2]), order, st.nf, table)
            seen.add((a, b, int(ext[1]) // 3))
            for k in range(2):
                pa, pb = table[a * 3 + b, k]
                if pa < 0:
                    assert tuple(cand[k]) == (ext[1], ext[2]) and sign[k] == 0
                    continue
                new = cfg.copy().ravel()
                new[1], new[2] = pa, pb
                ne = st.ext_config(new.reshape(shape), order).ravel()
                assert tuple(cand[k]) == (ne[1], ne[2]), (order, cfg.ravel(), k)
                assert ne[3] == ext[3] and ne[0] == ext[0]
                dn = int(np.sum(st.nf[new])) - int(np.sum(st.nf[cfg.ravel()]))
                assert dn in (-2, 0, 2) and sign[k] == (1 if dn == 0 else -1)
                assert sign[k] == st.sigma(new.reshape(shape)) * st.sigma(cfg)
    assert len(seen) == 18                                         # every (a, b) with both variants of the mode order

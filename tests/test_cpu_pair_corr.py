"""CPU checks of the singlet-pair correlation SC_singlet_pair_corr: its convention, its walker path, its index mapping and its entry
points.

1. The restated estimator (tests/pair_corr_ref.py) from fresh brute-force amplitudes of the oracle against the dense operator
   Delta+_ref Delta_tgt built from single c / c+: the |psi|^2-weighted mean over ALL 729 configurations is <Psi|Delta+_ref Delta_tgt|Psi>
   / <Psi|Psi>, for every bond pair of 2 x 3 (x1 != x2, occupied sites between the bonds) and 3 x 2 (y2 = y1 + 2).  The states do not
   conserve the electron number.  The estimator with the (down, up) sign flipped misses, and so does the one without the conj (shown
   on the same state with random phases: on a real state the conj changes nothing).
2. The excited-state propagation on the oracle's BMPSWalker, extended states from pair_ref.pair_cand_rule and raw two-site traces,
   reproduces the fresh-amplitude estimator term by term.
3. Mapping, count and coordinate string against values recorded from the formulas of
   singlet_pair_correlation_measurement_mixin.h:136-245.
4. The new symbols are declared, exported and bound."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_corr_ref as pc  # noqa: E402
import pair_ref  # noqa: E402
import tj_nnn_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 3), (3, 2)]
NEW_GPU = ("pepsgpu_walker_set_mpo_excited_pair", "pepsgpu_walker_pair_trace_slice", "pepsgpu_diag_walker_pair_slice_calls",
           "pepsgpu_diag_walker_pair_cand")
NEW_HOST = ("pepshost_fermion_observables_sc", "pepshost_fermion_exact_sum_measure_partial_sc", "pepshost_fermion_measure_sc",
            "pepshost_sc_pair_corr_mapping")

_CACHE = {}


def _lattice(shape, cplx=False):
    """per lattice and element type, computed once: the oracle state, psi of all 3^N configurations and the estimator of every
    configuration with a non-zero amplitude"""
    key = (shape, cplx)
    if key not in _CACHE:
        from oracle.bmps import BMPSTruncateParams
        from peps_amd import fermion
        rows, cols = shape
        st = ref.tj_state(rows, cols, 2)
        if cplx:                                                  # the same state with random phases on the stored tensors
            rng = np.random.default_rng(3)
            st = fermion.FermionState([[[t * np.exp(2j * np.pi * rng.uniform(size=t.shape)) for t in site] for site in row]
                                       for row in st.tensors], st.par, st.nf)
        fs = ref.oracle_view(st)
        tp = BMPSTruncateParams.SVD(64, 64, 0.0)                  # exact on these lattices
        cfgs = ref.all_tj_configs(rows, cols)
        psi = np.array([fs.amplitude(c, tp) for c in cfgs])
        psi[np.abs(psi) < 1e-12 * np.max(np.abs(psi))] = 0.0      # parity-odd configurations: zero by symmetry
        pw = 3 ** np.arange(rows * cols - 1, -1, -1)
        amp = lambda c: psi[int(np.asarray(c).ravel() @ pw)]
        live = np.nonzero(psi != 0)[0]
        fresh, terms = {}, 0
        for k in live:
            fresh[k], t = pc.estimator_from_amplitudes(cfgs[k], amp)
            terms += t
        _CACHE[key] = dict(fs=fs, tp=tp, cfgs=cfgs, psi=psi, amp=amp, live=live, fresh=fresh, terms=terms)
    return _CACHE[key]


def _weighted_mean(lat, per_config):
    w = np.abs(lat["psi"]) ** 2
    return sum(w[k] * per_config[k] for k in lat["live"]) / np.sum(w)


def _dense_expectation(shape, psi):
    rows, cols = shape
    cache, out = {}, []
    for y1, x1, _, y2, x2, _ in pc.index_mapping(rows, cols):
        M = pc.dense_pair_corr(rows, cols, (y1, x1), (y2, x2), cache)
        out.append((np.conj(psi) @ (M @ psi)) / (np.conj(psi) @ psi))
    return np.array(out)


@pytest.mark.parametrize("shape", SHAPES)
def test_restated_estimator_equals_the_dense_pair_pair_operator(shape):
    """All 729 configurations of a random parity-even D = 2 t-J state: the weighted mean of the restated estimator equals
    <Delta+_ref Delta_tgt> of the dense operator to 1e-12 absolute on every bond pair (the gate of tests/test_cpu_pair.py: float64 sums
    of a few hundred terms of order <= 1), with |<..>| > 1e-6 on every pair; the estimator with the (down, up) sign flipped misses the
    dense value by more than 1e-4 on some pair.  The same on the state with random phases, where the estimator without the conj
    misses by more than 1e-4 too."""
    rows, cols = shape
    npairs = {(2, 3): 4, (3, 2): 3}[shape]
    for cplx in (False, True):
        lat = _lattice(shape, cplx)
        assert len(lat["cfgs"]) == 729
        assert np.array_equal(lat["psi"] != 0, np.sum(lat["cfgs"] != ref.EMPTY, axis=(1, 2)) % 2 == 0)
        dense = _dense_expectation(shape, lat["psi"])
        mean = _weighted_mean(lat, lat["fresh"])
        flipped = _weighted_mean(lat, {k: pc.estimator_from_amplitudes(lat["cfgs"][k], lat["amp"], du_sign=1.0)[0] for k in lat["live"]})
        noconj = _weighted_mean(lat, {k: pc.estimator_from_amplitudes(lat["cfgs"][k], lat["amp"], conj=False)[0] for k in lat["live"]})
        worst, smallest = float(np.max(np.abs(mean - dense))), float(np.min(np.abs(dense)))
        miss_flip, miss_conj = float(np.max(np.abs(flipped - dense))), float(np.max(np.abs(noconj - dense)))
        print("pair corr", shape, "complex" if cplx else "real", "terms %d, max |mean - dense| = %.2e, min |<..>| = %.3e, flipped (down, up) "
              "sign misses by %.3e, no conj by %.3e" % (lat["terms"], worst, smallest, miss_flip, miss_conj))
        assert dense.shape == (npairs,) == mean.shape
        # per bond pair: 2 target classes x the 5 even fillings of the other two sites (both empty, or both occupied)
        assert lat["terms"] == 10 * npairs
        assert smallest > 1e-6
        assert worst <= 1e-12
        assert miss_flip > 1e-4
        if cplx:
            assert miss_conj > 1e-4
            assert np.max(np.abs(dense.imag)) > 1e-4
        else:
            assert miss_conj <= 1e-12                             # (a real state cannot tell: hence the complex one)


def test_bond_pairs_cover_the_cases_of_the_issue():
    """2 x 3: a pair with x1 != x2; 3 x 2: a pair with y2 = y1 + 2 (rows in between are evolved through)"""
    assert any(m[1] != m[4] for m in pc.index_mapping(2, 3))
    assert any(m[3] == m[0] + 2 for m in pc.index_mapping(3, 2))


@pytest.mark.parametrize("shape", SHAPES)
def test_walker_path_reproduces_the_fresh_amplitude_estimator(shape):
    """every non-zero term of the lattice: two excited walkers and the original walker of the oracle, chi large enough to be exact,
    against the ratio of fresh amplitudes at 1e-9 relative (the gate of the local-path test of tests/test_cpu_pair.py); entries
    without a term are exactly zero.  Configurations without any term are checked on a sample (their walkers compute nothing)."""
    lat = _lattice(shape)
    with_terms = [k for k in lat["live"] if np.any(lat["fresh"][k] != 0)]
    without = [k for k in lat["live"] if not np.any(lat["fresh"][k] != 0)][::40]
    count = 0
    for k in with_terms + without:
        got, terms = pc.walker_estimator(lat["fs"], lat["cfgs"][k], lat["tp"])
        want = lat["fresh"][k]
        nz = want != 0
        assert terms == int(nz.sum()) and got.shape == want.shape
        assert np.all(got[~nz] == 0)
        assert np.all(np.abs(got - want)[nz] <= 1e-9 * np.abs(want[nz])), (shape, k, got, want)
        count += terms
    print("walker path", shape, "terms", count, "configurations", len(with_terms), "+", len(without))
    assert count == lat["terms"] and len(without) >= 3


def test_walker_path_with_a_selection_returns_the_sub_vector():
    lat = _lattice((2, 3))
    k = next(k for k in lat["live"] if np.count_nonzero(lat["fresh"][k]) >= 2)
    full, _ = pc.walker_estimator(lat["fs"], lat["cfgs"][k], lat["tp"])
    sel, _ = pc.walker_estimator(lat["fs"], lat["cfgs"][k], lat["tp"], ref_bonds=[(0, 1), (5, 5)])
    idx = [i for i, m in enumerate(pc.index_mapping(2, 3)) if (m[0], m[1]) == (0, 1)]
    assert len(idx) == 2 and np.array_equal(sel, full[idx])


# values written down from the formulas of singlet_pair_correlation_measurement_mixin.h:136-245
RECORDED = [
    # (Ly, Lx, selection, count, mapping)
    (2, 2, (), 1, [(0, 0, 0, 1, 0, 0)]),
    (3, 4, (), 27, None),
    (3, 4, ((1, 2), (7, 0), (0, 3), (0, 1)), 9,              # (7, 0): row outside; (0, 3): x + 1 outside the row; the rest sorted
     [(0, 1, 0, 1, 0, 0), (0, 1, 0, 1, 1, 0), (0, 1, 0, 1, 2, 0), (0, 1, 0, 2, 0, 0), (0, 1, 0, 2, 1, 0), (0, 1, 0, 2, 2, 0),
      (1, 2, 0, 2, 0, 0), (1, 2, 0, 2, 1, 0), (1, 2, 0, 2, 2, 0)]),
    (3, 3, ((1, 1), (0, 1), (1, 0), (0, 0)), 12,             # unsorted: the output is ordered by (y, x)
     [(0, 0, 0, 1, 0, 0), (0, 0, 0, 1, 1, 0), (0, 0, 0, 2, 0, 0), (0, 0, 0, 2, 1, 0), (0, 1, 0, 1, 0, 0), (0, 1, 0, 1, 1, 0),
      (0, 1, 0, 2, 0, 0), (0, 1, 0, 2, 1, 0), (1, 0, 0, 2, 0, 0), (1, 0, 0, 2, 1, 0), (1, 1, 0, 2, 0, 0), (1, 1, 0, 2, 1, 0)]),
    (1, 4, (), 0, []),
    (4, 1, (), 0, []),
]


@pytest.mark.parametrize("case", RECORDED, ids=lambda c: "%dx%d-%d" % (c[0], c[1], len(c[2])))
def test_mapping_count_and_coordinate_string(case):
    Ly, Lx, sel, count, mapping = case
    got = pc.index_mapping(Ly, Lx, sel)
    assert pc.num_sc_pairs(Ly, Lx, sel) == count == len(got)
    if mapping is not None:
        assert got == mapping
    else:                                                      # 3 x 4, all: 2 rows x 3 reference bonds, 2 + 1 target rows x 3 bonds
        assert got[0] == (0, 0, 0, 1, 0, 0) and got[5] == (0, 0, 0, 2, 2, 0) and got[6] == (0, 1, 0, 1, 0, 0)
        assert got[18] == (1, 0, 0, 2, 0, 0) and got[26] == (1, 2, 0, 2, 2, 0)
        assert all(m[3] > m[0] and m[2] == m[5] == 0 for m in got) and len(set(got)) == 27
    text = pc.coord_string(Ly, Lx, sel)
    lines = text.split("\n")
    assert lines[0] == "# idx ref_y ref_x ref_orient tgt_y tgt_x tgt_orient" and lines[-1] == "" and len(lines) == count + 2
    if Ly == 2 and Lx == 2:
        assert text == "# idx ref_y ref_x ref_orient tgt_y tgt_x tgt_orient\n0 0 0 0 1 0 0\n"
    for i, m in enumerate(got):
        assert lines[1 + i] == " ".join(str(v) for v in (i,) + m)
    # the product's own mapping (the Python twin and the walker calls index by it)
    from peps_amd import fermion, hostapi
    assert [tuple(m) for m in fermion.sc_pair_corr_mapping(Ly, Lx, sel)] == got
    if not os.path.exists(hostapi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    # ... and GenerateSCPairCorrIndexMapping of the host layer's mixin (needs no device)
    assert [tuple(m) for m in hostapi.sc_pair_corr_mapping(Ly, Lx, sel).tolist()] == got


def test_pair_correlation_entry_points_declared_exported_and_bound():
    import inspect
    from peps_amd import capi, fermion, hostapi
    if not (os.path.exists(capi.LIB_PATH) and os.path.exists(hostapi.LIB_PATH)):
        import __graft_entry__ as g
        g.build()
    header = open(os.path.join(ROOT, "include", "pepsgpu.h")).read()
    declared = set(re.findall(r"\b(pepsgpu_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(capi.LIB_PATH)
    capi.lib()
    host = ctypes.CDLL(hostapi.LIB_PATH)
    for name in NEW_HOST:
        assert hasattr(host, name), name
        assert name in hostapi.SYMBOLS, name
    for name in ("fermion_observables", "fermion_exact_sum_measure", "fermion_measure"):
        prm = inspect.signature(getattr(hostapi, name)).parameters
        assert prm["sc_pair_corr"].default is False and prm["ref_bonds"].default == (), name
    host_header = open(os.path.join(ROOT, "peps_amd", "host", "qlpeps_gpu.h")).read()
    for name in ("SetMPOExcitedPair", "PairTraceSlice", "class SingletPairCorrelationMixin", "SetEnableSingletPairCorrelation",
                 "IsSingletPairCorrelationEnabled", "SetSelectedRefBonds", "GetSelectedRefBonds", "ComputeNumSCPairs",
                 "GenerateSCPairCorrIndexMapping", "GenerateSCPairCorrCoordString", "MeasureSingletPairCorrelation"):
        assert name in host_header, name
    for name in NEW_GPU:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
    bound = capi.load_library()
    assert len(bound.pepsgpu_walker_set_mpo_excited_pair.argtypes) == 10
    assert len(bound.pepsgpu_walker_pair_trace_slice.argtypes) == 8
    assert len(bound.pepsgpu_diag_walker_pair_cand.argtypes) == 13
    assert len(bound.pepsgpu_diag_walker_pair_slice_calls.argtypes) == 0
    assert bound.pepsgpu_diag_walker_pair_slice_calls.restype is ctypes.c_long
    assert callable(getattr(capi.Walker, "set_mpo_excited_pair")) and callable(getattr(capi.Walker, "pair_trace_slice"))
    assert callable(capi.diag_walker_pair_cand) and callable(capi.diag_walker_pair_slice_calls)
    calls = capi.diag_walker_pair_slice_calls()                  # asking needs no device
    assert isinstance(calls, int) and calls >= 0
    assert callable(fermion.tj_pair_correlation) and callable(fermion.sc_pair_corr_mapping)

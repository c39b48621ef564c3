"""CPU checks of the three-site exchange updater's surface: pepsgpu_sweep_slice_tnn3 is declared, exported and bound (no compute call),
and the host layer's triple table (pepshost_tnn3_table, no device) matches a Python restatement of square_3site_updater.h:118-127 for
bosonic states and, over the extended states, for fermionic states in both mode orders."""
import ctypes
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _built():
    from peps_amd import capi, hostapi
    if not (os.path.exists(capi.LIB_PATH) and os.path.exists(hostapi.LIB_PATH)):
        import __graft_entry__ as g
        g.build()


def _perms(t):
    """the distinct permutations of the sorted triple in lexicographic (std::next_permutation) order, and the slot of t"""
    perms = sorted(set(itertools.permutations(sorted(t))))
    return perms, perms.index(tuple(t))


def _entry(m, init, slots):
    row = [m, init]
    for k in range(6):
        row += list(slots[k if k < m else 0])
    return row


def test_tnn3_entry_point_declared_exported_and_bound():
    from peps_amd import capi, hostapi
    _built()
    header = open(os.path.join(ROOT, "include", "pepsgpu.h")).read()
    declared = set(re.findall(r"\b(pepsgpu_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert "pepsgpu_sweep_slice_tnn3" in declared
    assert hasattr(lib, "pepsgpu_sweep_slice_tnn3")
    assert "pepsgpu_sweep_slice_tnn3" in capi.SYMBOLS
    for name in ("pepsgpu_diag_tnn3_table",):
        assert name in declared and hasattr(lib, name) and name in capi.SYMBOLS, name
    # (ctx, orientation, slice, triple_table, n_words, engine_words, amplitude, consumed, accepted, slice_states)
    assert len(capi.load_library().pepsgpu_sweep_slice_tnn3.argtypes) == 10
    assert callable(getattr(capi.Context, "sweep_slice_tnn3"))
    host = ctypes.CDLL(hostapi.LIB_PATH)
    for name in ("pepshost_tnn3_table", "pepshost_fermion_mc_sweeps_updater"):
        assert hasattr(host, name) and name in hostapi.SYMBOLS, name
    assert hostapi.UPDATER_ID == {"exchange": 0, "fullspace": 1, "tnn3": 2}


@pytest.mark.parametrize("d", [2, 3])
def test_bosonic_triple_table_matches_restatement(d):
    from peps_amd import hostapi
    _built()
    got = hostapi.tnn3_table(d)
    assert got.shape == (d ** 3, 20)
    for e, t in enumerate(itertools.product(range(d), repeat=3)):
        perms, init = _perms(t)
        assert len(perms) in (1, 3, 6)
        assert got[e].tolist() == _entry(len(perms), init, perms), (t, got[e])
    # d = 2 never needs more than 3 slots (the slot count of the slice for phys_dim 2)
    if d == 2:
        assert got[:, 0].max() == 3


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_engine_bosonic_table_equals_host_table(d):
    """the engine builds the bosonic table itself for a NULL table (engine_sweep.h); the host layer states the same rule
    (qlpeps_gpu.h): both copies must agree"""
    from peps_amd import capi, hostapi
    _built()
    assert capi.diag_tnn3_table(d).tolist() == hostapi.tnn3_table(d).tolist()


def _ext_run(phys, before, order, nf, d):
    """extended states of three sites consecutive in the mode order, given the parity of the fermions before the first one
    (FermionState.ext_config: row-major variant = inclusive parity, column-major = 2 + parity before the site)"""
    occ = [nf[s] % 2 for s in phys]
    out, par = [], before
    for s, o in zip(phys, occ):
        if order == 0:
            par ^= o
            out.append(s + d * par)
        else:
            out.append(s + d * (2 + par))
            par ^= o
    return tuple(out)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("nf", [[1, 1, 0], [1, 0]])
def test_fermionic_triple_table_matches_restatement(order, nf):
    """t-J-like (up, down, hole) and spinless (occupied, empty) parities: over every triple of extended states"""
    from peps_amd import hostapi
    _built()
    d = len(nf)
    dp = 4 * d
    got = hostapi.tnn3_table(d, nf=nf, order=order)
    assert got.shape == (dp ** 3, 20)
    moved = 0
    for e, ex in enumerate(itertools.product(range(dp), repeat=3)):
        phys = tuple(x % d for x in ex)
        var = [x // d for x in ex]
        ok = all(v < 2 for v in var) if order == 0 else all(v >= 2 for v in var)
        if not ok or len(set(phys)) == 1:
            assert got[e].tolist() == _entry(1, 0, [ex]), (ex, got[e])
            continue
        before = ((var[0] & 1) ^ (nf[phys[0]] % 2)) if order == 0 else (var[0] & 1)
        perms, init = _perms(phys)
        slots = [_ext_run(p, before, order, nf, d) for p in perms]
        assert got[e].tolist() == _entry(len(perms), init, slots), (ex, got[e])
        # a consistent triple (its own variants follow from `before`) finds itself at init, and every slot conserves the parity
        if _ext_run(phys, before, order, nf, d) == ex:
            assert slots[init] == ex
            moved += 1
        for s in slots:
            assert sum(nf[x % d] for x in s) % 2 == sum(nf[x] for x in phys) % 2
    assert moved > 0


def test_triple_table_rejects_bad_arguments():
    from peps_amd import hostapi
    _built()
    with pytest.raises(ValueError):
        hostapi.tnn3_table(2, nf=[1, 0], order=2)
    with pytest.raises(ValueError):
        hostapi.tnn3_table(0)

"""GPU tests of the pair slice of a fermionic context (pepsgpu_nn_pair_slice_fermion): its candidate kernel against the NumPy rule,
every slice of both passes against per-bond Trace + ReplaceNNSiteTrace calls whose candidates are built independently from
FermionState.ext_config of the changed configuration, and its refusals.

Setup: a 3 x 4 lattice (rows != cols), a D = 3 parity-even t-J state that does not conserve the electron number (tj_nnn_ref.tj_state),
chi = 16, 12 walkers drawn from {up, down, empty} with an even electron number."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_ref  # noqa: E402
import tj_nnn_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, COLS, D, CHI, NW = 3, 4, 3, 16, 12
TOL = {"f64": 1e-12, "f32": 1e-5, "c128": 1e-12}           # tests/test_gpu_energy_slices.py
CLASSES = {(2, 2): "ee", (0, 1): "ud", (1, 0): "du"}


def _configs():
    """12 walkers, even electron number; the first two are laid out so that every bond class occurs on a horizontal and on a
    vertical bond whatever the generator draws, the rest is random"""
    rng = np.random.default_rng(21)
    out = [np.array([[2, 2, 0, 1], [2, 0, 1, 0], [0, 1, 2, 0]]), np.array([[0, 1, 0, 2], [1, 0, 2, 2], [2, 2, 1, 2]])]
    while len(out) < NW:
        c = rng.integers(0, 3, size=(ROWS, COLS))
        if np.sum(c != 2) % 2 == 0:
            out.append(c)
    return np.array(out)


def _bond_class(c1, c2):
    return CLASSES.get((int(c1), int(c2)), "none")


def _state(dtype):
    from peps_amd import capi, fermion
    st = ref.tj_state(ROWS, COLS, D)
    if dtype == "c128":                                    # the same state with random phases on the stored tensors
        rng = np.random.default_rng(3)
        st = fermion.FermionState([[[t * np.exp(2j * np.pi * rng.uniform(size=t.shape)) for t in site] for site in row]
                                   for row in st.tensors], st.par, st.nf)
    ctx = capi.Context(ROWS, COLS, st.D, fermion.NVAR * st.d, CHI, dtype={"f64": capi.F64, "f32": capi.F32, "c128": capi.C128}[dtype],
                       max_walkers=NW)
    ctx.state_upload(st.extended_flat())
    return st, ctx


def _passes():
    """(orientation, mode order, BMPS approach, BMPS window shift, BTen low / high side, slices, slice length)"""
    from peps_amd import capi, fermion
    return ((capi.HORIZONTAL, fermion.ROW, capi.UP, capi.DOWN, capi.LEFT, capi.RIGHT, ROWS, COLS),
            (capi.VERTICAL, fermion.COL, capi.LEFT, capi.RIGHT, capi.UP, capi.DOWN, COLS, ROWS))


def _site(orient, s, j):
    from peps_amd import capi
    return (s, j) if orient == capi.HORIZONTAL else (j, s)


def _exchange_table(st, order):
    import test_gpu_energy_slices as es
    return es._fermion_exchange_table(st, order)


def _check_preconditions(cfgs, psi0):
    """each bond class on a horizontal and on a vertical bond; no walker with a negligible amplitude; all walkers present"""
    assert cfgs.shape == (NW, ROWS, COLS) and np.all(np.sum(cfgs != 2, axis=(1, 2)) % 2 == 0)
    seen = {"h": set(), "v": set()}
    for c in cfgs:
        for key, s1, s2 in pair_ref.nn_bonds(ROWS, COLS):
            seen[key].add(_bond_class(c[s1], c[s2]))
    assert seen["h"] == seen["v"] == {"ee", "ud", "du", "none"}, seen
    a = np.abs(psi0)
    assert a.shape == (NW,) and np.min(a) > 1e-6 * np.median(a), a


def test_pair_cand_kernel_equals_the_numpy_rule():
    from peps_amd import capi
    cfgs = _configs()
    table = pair_ref.tj_pair_table()
    st, ctx = _state("f64")
    ctx.set_configs(st.ext_config(cfgs, 0))
    _check_preconditions(cfgs, ctx.evaluate_amplitude())
    ctx.close()
    checked = 0
    for orient, order, *_ in _passes():
        ext = st.ext_config(cfgs, order)
        for key, s1, s2 in pair_ref.nn_bonds(ROWS, COLS):
            if (key == "h") != (orient == capi.HORIZONTAL):
                continue
            cand, sign = capi.diag_pair_cand(ext, st.nf % 2, table, orient, s1[0] * COLS + s1[1], s2[0] * COLS + s2[1])
            for w in range(NW):
                want_c, want_s = pair_ref.pair_cand_rule(int(ext[w][s1]), int(ext[w][s2]), order, st.nf, table)
                assert np.array_equal(cand[w], want_c) and np.array_equal(sign[w], want_s), (orient, s1, w)
                # ... and the rule is ext_config of the changed configuration
                for k, pc in enumerate(pair_ref.pair_candidates(int(cfgs[w][s1]), int(cfgs[w][s2]))):
                    if pc is None:
                        assert sign[w, k] == 0 and tuple(cand[w, k]) == (ext[w][s1], ext[w][s2])
                        continue
                    new = cfgs[w].copy()
                    new[s1], new[s2] = pc
                    ne = st.ext_config(new, order)
                    assert tuple(cand[w, k]) == (ne[s1], ne[s2]) and sign[w, k] == -1
                    assert np.array_equal(np.delete(ne.ravel(), [s1[0] * COLS + s1[1], s2[0] * COLS + s2[1]]),
                                          np.delete(ext[w].ravel(), [s1[0] * COLS + s1[1], s2[0] * COLS + s2[1]]))
                    checked += 1
    assert checked > 50
    with pytest.raises(ValueError):                        # (0, 1) - (1, 1) is no horizontal bond
        capi.diag_pair_cand(st.ext_config(cfgs, 0), st.nf % 2, table, capi.HORIZONTAL, 1, 1 + COLS)
    with pytest.raises(ValueError):                        # row-major states handed to the column pass
        capi.diag_pair_cand(st.ext_config(cfgs, 0), st.nf % 2, table, capi.VERTICAL, 0, COLS)


def _reference_slice(ctx, st, cfgs, orient, order, lo, hi, s, N, xtab):
    """the per-bond sequence of the fermionic hooks: InitBTen, GrowFullBTen(.., 2), per bond Trace and ONE ReplaceNNSiteTrace over
    [exchange, pair slot 0, pair slot 1] built from ext_config of the changed configurations, ShiftBTenWindow while j + 2 < N"""
    ctx.init_bten(lo, s)
    ctx.grow_full_bten(hi, s, 2, True)
    ext = st.ext_config(cfgs, order)
    psi, ex, pair, has, differ = [], [], [], [], []
    for j in range(N - 1):
        s1, s2 = _site(orient, s, j), _site(orient, s, j + 1)
        psi.append(ctx.trace(s1[0], s1[1], orient))
        cands = np.zeros((NW, 3, 2), dtype=np.int32)
        h = np.zeros((NW, 2), dtype=bool)
        for w in range(NW):
            new = cfgs[w].copy()
            new[s1], new[s2] = cfgs[w][s2], cfgs[w][s1]
            ne = st.ext_config(new, order)
            cands[w, 0] = (ne[s1], ne[s2])
            for k, pc in enumerate(pair_ref.pair_candidates(int(cfgs[w][s1]), int(cfgs[w][s2]))):
                cands[w, 1 + k] = (ext[w][s1], ext[w][s2])
                if pc is not None:
                    new = cfgs[w].copy()
                    new[s1], new[s2] = pc
                    ne = st.ext_config(new, order)
                    cands[w, 1 + k] = (ne[s1], ne[s2])
                    h[w, k] = True
        # (the exchange table and the independently built exchange candidate must agree, or the comparison below means nothing)
        assert np.array_equal(cands[:, 0], xtab[ext[:, s1[0], s1[1]] * 4 * st.d + ext[:, s2[0], s2[1]]])
        r = ctx.replace_nn_trace(s1[0], s1[1], orient, cands)
        ex.append(r[:, 0])
        pair.append(-r[:, 1:])                             # Sigma(S') / Sigma(S) = -1: every candidate of this table changes nf by 2
        has.append(h)
        differ.append(cfgs[:, s1[0], s1[1]] != cfgs[:, s2[0], s2[1]])
        if j + 2 < N:
            ctx.shift_bten_window(hi)
    return np.stack(psi, 1), np.stack(ex, 1), np.stack(pair, 1), np.stack(has, 1), np.stack(differ, 1)


def _stack_sizes(ctx):
    return [ctx.bten_stack_size(p) for p in range(4)] + [ctx.bmps_stack_size(p) for p in range(4)]


@pytest.mark.parametrize("dtype", ["f64", "f32", "c128"])
def test_pair_slice_matches_the_per_bond_calls(dtype):
    from peps_amd import capi
    st, ctx = _state(dtype)
    cfgs = _configs()
    table = pair_ref.tj_pair_table()
    tol = TOL[dtype]
    ctx.set_configs(st.ext_config(cfgs, 0))
    _check_preconditions(cfgs, ctx.evaluate_amplitude())
    before = capi.diag_pair_slice_calls()
    nslices = 0
    for orient, order, approach, step, lo, hi, S, N in _passes():
        ctx.set_configs(st.ext_config(cfgs, order))
        xtab = _exchange_table(st, order)
        ctx.generate_bmps_approach(approach)
        for s in range(S):
            psi, ex, pair = ctx.nn_pair_slice_fermion(orient, s, st.nf % 2, table, xtab)
            sizes = _stack_sizes(ctx)
            psi2, none_ex, pair2 = ctx.nn_pair_slice_fermion(orient, s, st.nf % 2, table)        # without the exchange slot
            assert none_ex is None and sizes == _stack_sizes(ctx)
            nslices += 2
            # psi and the exchanged amplitude are bit for bit those of the energy slice (the host layer's measured energy is the energy
            # solver's number)
            psi_e, ex_e = ctx.nn_exchange_slice_tab(orient, s, False, xtab, psi_per_bond=True)
            assert np.array_equal(psi, psi_e) and np.array_equal(ex, ex_e) and sizes == _stack_sizes(ctx), (orient, s)
            psi_r, ex_r, pair_r, has, differ = _reference_slice(ctx, st, cfgs, orient, order, lo, hi, s, N, xtab)
            assert sizes == _stack_sizes(ctx), (orient, s)
            assert psi.shape == (NW, N - 1) and ex.shape == (NW, N - 1) and pair.shape == (NW, N - 1, 2)
            if dtype == "c128":
                assert psi.dtype == np.complex128 and np.max(np.abs(psi.imag)) > 0
            scale = np.max(np.abs(psi_r))
            assert np.max(np.abs(psi - psi_r)) < tol * scale, (orient, s)
            assert np.max(np.abs(ex - ex_r)[differ]) < tol * np.max(np.abs(ex_r[differ])), (orient, s)
            assert np.array_equal(ex[~differ], psi[~differ])                   # identity exchanges: exactly psi of the bond
            assert has.any() and (~has).any()
            assert np.max(np.abs(pair - pair_r)[has]) < tol * np.max(np.abs(pair_r[has])), (orient, s)
            assert np.all(pair[~has] == 0.0)                                   # "no candidate": exactly zero
            assert np.all(pair[has] != 0.0)
            # the exchange slot changes nothing in the other outputs
            assert np.max(np.abs(psi2 - psi)) < tol * scale and np.max(np.abs(pair2 - pair)) < tol * np.max(np.abs(pair_r[has]))
            assert np.all(pair2[~has] == 0.0)
            if s + 1 < S:
                ctx.shift_bmps_window(step)
    assert capi.diag_pair_slice_calls() == before + nslices
    ctx.close()


def test_pair_slice_refusals_leave_the_context_usable():
    from peps_amd import capi
    st, ctx = _state("f64")
    cfgs = _configs()
    table = pair_ref.tj_pair_table()
    occ = np.ascontiguousarray(st.nf % 2, dtype=np.int32)
    d, dp = st.d, 4 * st.d
    ctx.set_configs(st.ext_config(cfgs, 0))
    _check_preconditions(cfgs, ctx.evaluate_amplitude())
    xtab = np.ascontiguousarray(_exchange_table(st, 0), dtype=np.int32)
    psi, ex, pair = np.zeros((NW, COLS - 1)), np.zeros((NW, COLS - 1)), np.zeros((NW, COLS - 1, 2))
    lib, h = ctx._l, ctx._h

    def call(orient=capi.HORIZONTAL, s=0, dd=d, o=occ, t=table, x=xtab, p=psi, e=ex, q=pair):
        ip = lambda a: None if a is None else capi._ip(np.ascontiguousarray(a, dtype=np.int32))
        dp_ = lambda a: None if a is None else capi._dp(a)
        return lib.pepsgpu_nn_pair_slice_fermion(h, orient, s, dd, ip(o), ip(t), ip(x), dp_(p), dp_(e), dp_(q))

    ctx.set_configs(st.ext_config(cfgs, 0))                # (drops the boundary MPS the amplitude evaluation grew)
    assert call() == 3                                     # no boundary MPS yet: PEPSGPU_ESTATE
    ctx.generate_bmps_approach(capi.UP)
    good = ctx.nn_pair_slice_fermion(capi.HORIZONTAL, 0, occ, table, xtab)
    calls = capi.diag_pair_slice_calls()
    # PEPSGPU_EINVAL
    assert call(orient=2) == 1 and call(s=-1) == 1 and call(s=ROWS) == 1
    assert call(o=None) == 1 and call(t=None) == 1 and call(p=None) == 1 and call(q=None) == 1
    assert call(e=None) == 1                               # ex_out is required with an exchange table
    assert call(dd=2) == 1                                 # 4 d != the context's physical dimension
    assert call(o=np.array([1, 2, 0], dtype=np.int32)) == 1
    bad = table.copy(); bad[0, 0] = (3, 0)
    assert call(t=bad) == 1                                # entry outside [-1, d)
    bad = table.copy(); bad[0, 0] = (-2, -2)
    assert call(t=bad) == 1
    bad = table.copy(); bad[0, 0] = (-1, 0)
    assert call(t=bad) == 1                                # only one -1
    bad = table.copy(); bad[0 * 3 + 1, 1] = (2, 0)         # (up, down) -> (empty, up): the pair's parity changes
    assert call(t=bad) == 1
    # PEPSGPU_ERANGE
    badx = xtab.copy(); badx[5, 1] = dp
    assert call(x=badx) == 4
    badx = xtab.copy(); badx[0, 0] = -1
    assert call(x=badx) == 4
    # PEPSGPU_ESTATE
    assert call(s=1) == 3                                  # the UP boundary MPS of row 1 is not there yet
    assert call(orient=capi.VERTICAL) == 3                 # the column pass's boundary MPS are missing (and the states are row-major)
    ctx.cfg_override_slice(capi.HORIZONTAL, 0, st.ext_config(cfgs, 0)[:, 0, :])
    assert call() == 3                                     # a configuration override is active
    ctx.cfg_override_slice(capi.HORIZONTAL, 0, None)
    assert capi.diag_pair_slice_calls() == calls           # a refused call is no completed call
    again = ctx.nn_pair_slice_fermion(capi.HORIZONTAL, 0, occ, table, xtab)
    for a, b in zip(good, again):
        assert np.array_equal(a, b)
    # column-major states in a row slice, with the boundary MPS in place: the variant test itself
    ctx.set_configs(st.ext_config(cfgs, 1))
    ctx.generate_bmps_approach(capi.UP)
    assert call() == 3
    ctx.set_configs(st.ext_config(cfgs, 0))
    ctx.generate_bmps_approach(capi.UP)
    again = ctx.nn_pair_slice_fermion(capi.HORIZONTAL, 0, occ, table, xtab)
    for a, b in zip(good, again):
        assert np.array_equal(a, b)
    ctx.close()

"""GPU tests of the singlet-pair correlation SC_singlet_pair_corr on the device: pepsgpu_walker_set_mpo_excited_pair and
pepsgpu_walker_pair_trace_slice against the NumPy rule, against set_mpo with host-built states and against the per-call sequence of the
same BMPSWalker; the assembled estimator against fresh amplitudes of the changed configurations; the host layer's mixin against the
Python twin, its hook path and the dense operator; the refusals.

Setup (tests/test_gpu_pair_slice.py): a 3 x 4 lattice, a D = 3 parity-even t-J state that does not conserve the electron number
(tj_nnn_ref.tj_state), chi = 16 (exact: every boundary bond of this lattice is <= D^2 = 9), 12 walkers.  The first walkers are laid
out by hand so that an (empty, empty) reference bond in rows 0 and 1 stands above (up, down) and (down, up) targets in rows 1 and 2,
and one has no (empty, empty) bond at all; the rest is random with an even electron number."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_corr_ref as pc  # noqa: E402
import pair_ref  # noqa: E402
import tj_nnn_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS, D, CHI, NW = 3, 4, 3, 16, 12
TOL = {"f64": 1e-12, "f32": 1e-5, "c128": 1e-12}           # tests/test_gpu_energy_slices.py
UD, DU, EE = (0, 1), (1, 0), (2, 2)


def _configs():
    rng = np.random.default_rng(21)
    out = [np.array([[2, 2, 2, 2], [0, 1, 1, 0], [1, 0, 2, 2]]),       # row 0 all empty; row 1 (up, down) . (down, up); row 2 (down, up)
           np.array([[0, 2, 2, 1], [2, 2, 0, 1], [0, 1, 1, 0]]),       # refs (0, 1) and (1, 0); targets (1, 2) ud, (2, 0) ud, (2, 2) du
           np.array([[1, 0, 2, 2], [0, 1, 2, 2], [2, 1, 0, 2]]),       # refs (0, 2) and (1, 2); targets (1, 0) ud, (2, 1) du
           np.array([[0, 1, 0, 1], [1, 0, 1, 0], [2, 2, 2, 2]])]       # no (empty, empty) bond in rows 0 and 1: closed everywhere
    while len(out) < NW:
        c = rng.integers(0, 3, size=(ROWS, COLS))
        if np.sum(c != 2) % 2 == 0:
            out.append(c)
    return np.array(out)


def _pair(c, y, x):
    return (int(c[y, x]), int(c[y, x + 1]))


def _check_preconditions(cfgs, psi0):
    """each class occurs: for (ref row, target row) in (0, 1), (0, 2), (1, 2) an (empty, empty) reference above an (up, down) and
    above a (down, up) target; a walker that is closed for every reference bond; a reference bond that is open for some walkers and
    closed for others; no walker with a negligible amplitude"""
    assert cfgs.shape == (NW, ROWS, COLS) and np.all(np.sum(cfgs != 2, axis=(1, 2)) % 2 == 0)
    seen = set()
    for c in cfgs:
        for y1, x1, _, y2, x2, _ in pc.index_mapping(ROWS, COLS):
            if _pair(c, y1, x1) == EE and _pair(c, y2, x2) in (UD, DU):
                seen.add((y1, y2, _pair(c, y2, x2)))
    assert seen == {(y1, y2, t) for y1, y2 in ((0, 1), (0, 2), (1, 2)) for t in (UD, DU)}, seen
    ref_open = np.array([[[_pair(c, y, x) == EE for x in range(COLS - 1)] for y in range(ROWS - 1)] for c in cfgs])
    assert (~ref_open.any(axis=(1, 2))).any()
    assert (ref_open.any(axis=0) & ~ref_open.all(axis=0)).any()
    a = np.abs(psi0)
    assert a.shape == (NW,) and np.min(a) > 1e-6 * np.median(a), a


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


def _ready(dtype):
    """context with the row-major extended configurations, UP and DOWN stacks full (what the measurement starts from)"""
    from peps_amd import capi
    st, ctx = _state(dtype)
    cfgs = _configs()
    ctx.set_configs(st.ext_config(cfgs, 0))
    _check_preconditions(cfgs, ctx.evaluate_amplitude())
    ctx.set_configs(st.ext_config(cfgs, 0))
    ctx.generate_bmps_approach(capi.UP)
    ctx.grow_full_bmps(capi.UP)
    assert ctx.bmps_stack_size(capi.UP) == ROWS and ctx.bmps_stack_size(capi.DOWN) == ROWS
    return st, ctx, cfgs


def _rule_rows(st, ext_rows, col, table):
    """pair_cand_rule per walker on [n][cols] extended rows: cand [n][2][2], sign [n][2]"""
    cand, sign = np.zeros((len(ext_rows), 2, 2), dtype=np.int32), np.zeros((len(ext_rows), 2), dtype=np.int32)
    for w, row in enumerate(ext_rows):
        cand[w], sign[w] = pair_ref.pair_cand_rule(int(row[col]), int(row[col + 1]), 0, st.nf, table)
    return cand, sign


# ---- 1. the kernels against the rule, the excited row against set_mpo with host-built states ----
def test_candidate_and_patch_kernels_equal_the_numpy_rule():
    from peps_amd import capi, fermion
    st = ref.tj_state(ROWS, COLS, D)
    cfgs = _configs()
    ext = st.ext_config(cfgs, 0)
    swap = -np.ones((9, 2, 2), dtype=np.int32)             # number-conserving candidates: both signs of the rule occur
    for a in range(3):
        for b in range(3):
            swap[a * 3 + b, 1] = (b, a)
    mask = np.arange(NW) % 3 != 1
    checked = 0
    for table in (pair_ref.tj_pair_table(), fermion.tj_pair_identity_table(), swap):
        for y in range(ROWS):
            rows = ext[:, y, :]
            for col in range(COLS - 1):
                want_c, want_s = _rule_rows(st, rows, col, table)
                for slot in (0, 1):
                    for mk in (None, mask):
                        cand, skip, sign, patched = capi.diag_walker_pair_cand(rows, st.nf % 2, table, col, slot, mk)
                        assert np.array_equal(cand, want_c) and np.array_equal(sign, want_s), (y, col)
                        closed = (want_s == 0) | (False if mk is None else ~mk[:, None])
                        assert np.array_equal(skip, closed.T.astype(np.int32)), (y, col)
                        want_p = rows.copy()
                        want_p[:, col:col + 2] = want_c[:, slot]
                        assert np.array_equal(patched, want_p), (y, col, slot)
                        checked += int((want_s[:, slot] != 0).sum())
                # ... and the rule is ext_config of the changed configuration: nothing else of the lattice changes
                for w in range(NW):
                    for k in range(2):
                        pa, pb = table[cfgs[w, y, col] * 3 + cfgs[w, y, col + 1], k]
                        if pa < 0:
                            continue
                        new = cfgs[w].copy()
                        new[y, col], new[y, col + 1] = pa, pb
                        ne = st.ext_config(new, 0)
                        assert tuple(want_c[w, k]) == (ne[y, col], ne[y, col + 1])
                        others = np.ones((ROWS, COLS), dtype=bool)
                        others[y, col:col + 2] = False
                        assert np.array_equal(ne[others], ext[w][others])
                        assert want_s[w, k] == st.sigma(new) * st.sigma(cfgs[w])
    assert checked > 200
    rows = ext[:, 0, :]
    with pytest.raises(ValueError):                        # the pair (3, 4) is outside a row of 4
        capi.diag_walker_pair_cand(rows, st.nf % 2, pair_ref.tj_pair_table(), COLS - 1)
    with pytest.raises(ValueError):                        # column-major states
        capi.diag_walker_pair_cand(st.ext_config(cfgs, 1)[:, 0, :], st.nf % 2, pair_ref.tj_pair_table(), 0)
    with pytest.raises(ValueError):
        capi.diag_walker_pair_cand(rows, st.nf % 2, pair_ref.tj_pair_table(), 0, slot=2)


@pytest.mark.parametrize("dtype", ["f64", "f32", "c128"])
def test_excited_pair_row_matches_set_mpo_with_host_states(dtype):
    """set_mpo_excited_pair against set_mpo_states with the row built in NumPy from ext_config of the changed configurations: open
    mask, sign, and every tensor and log-scale of the boundary MPS after Evolve, byte for byte; for every reference bond and slot"""
    from peps_amd import capi, fermion
    st, ctx, cfgs = _ready(dtype)
    inject = fermion.tj_pair_inject_table()
    ext = st.ext_config(cfgs, 0)
    for y1, x1 in pc.valid_ref_bonds(ROWS, COLS):
        valid = np.array([_pair(c, y1, x1) == EE for c in cfgs])
        for slot in (0, 1):
            new = cfgs.copy()
            new[valid, y1, x1], new[valid, y1, x1 + 1] = inject[8, slot]
            ne = st.ext_config(new, 0)
            assert np.array_equal(np.delete(ne, y1, axis=1), np.delete(ext, y1, axis=1))       # the rows below need no change
            a, b = ctx.get_walker(capi.UP, level=y1), ctx.get_walker(capi.UP, level=y1)
            opened, sign = a.set_mpo_excited_pair(y1, x1, st.nf % 2, inject, slot)
            assert opened.dtype == bool and np.array_equal(opened, valid) and np.array_equal(sign, np.where(valid, -1, 0))
            b.set_mpo_states(y1, ne[:, y1, :])
            a.Evolve()
            b.Evolve()
            for idx in range(COLS):
                (ta, la), (tb, lb) = a.GetBMPSTensor(idx), b.GetBMPSTensor(idx)
                assert ta.shape == tb.shape and ta.tobytes() == tb.tobytes() and la.tobytes() == lb.tobytes(), (y1, x1, slot, idx)
            a.destroy()
            b.destroy()
    ctx.close()


# ---- 2. the slice against the per-call sequence ----
def _per_call_scan(w, bottom, ext_row, st, table):
    """InitBTenLeft(0), InitBTenRight(1), per position TraceWithTwoSiteBTen with the candidates of pair_cand_rule for every walker and
    slot, ShiftBTenWindow(RIGHT): sign * trace [n][cols - 1][2], has [n][cols - 1][2], the cache columns"""
    from peps_amd import capi
    n = len(ext_row)
    out = np.zeros((n, COLS - 1, 2), dtype=w.ctx._ot)
    has = np.zeros((n, COLS - 1, 2), dtype=bool)
    w.InitBTenLeft(bottom, 0)
    w.InitBTenRight(bottom, 1)
    for x in range(COLS - 1):
        cand, sign = _rule_rows(st, ext_row, x, table)
        for k in range(2):
            out[:, x, k] = sign[:, k] * w.TraceWithTwoSiteBTen(bottom, x, states=cand[:, k])
            has[:, x, k] = sign[:, k] != 0
        if x < COLS - 2:
            w.ShiftBTenWindow(bottom, capi.RIGHT)
    return out, has, (w.GetBTenLeftCol(), w.GetBTenRightCol())


@pytest.mark.parametrize("dtype", ["f64", "f32", "c128"])
def test_pair_trace_slice_matches_the_per_call_sequence(dtype):
    """an excited walker (reference bond (0, 1), slot 0) and the original walker, both target rows with one Evolve between their
    scans; the t-J pair table (both slots on (empty, empty) bonds), the removal table and the identity table; with and without a
    mask.  The per-call sequence runs on a clone."""
    from peps_amd import capi, fermion
    st, ctx, cfgs = _ready(dtype)
    tol = TOL[dtype]
    nf = st.nf % 2
    ext = st.ext_config(cfgs, 0)
    tables = {"tj": pair_ref.tj_pair_table(), "remove": fermion.tj_pair_remove_table(), "identity": fermion.tj_pair_identity_table()}
    y1, x1 = 0, 1
    ex = ctx.get_walker(capi.UP, level=y1)
    opened, _ = ex.set_mpo_excited_pair(y1, x1, nf, fermion.tj_pair_inject_table(), 0)
    assert opened.any() and (~opened).any()
    ex.Evolve()
    orig = ctx.get_walker(capi.UP, level=y1)
    orig.set_mpo(y1)
    orig.Evolve()
    calls0 = capi.diag_walker_pair_slice_calls()
    done = 0
    for y2 in (1, 2):
        bottom = ROWS - 1 - y2
        for w in (ex, orig):
            if y2 == 2:
                w.set_mpo(1)
                w.Evolve()
            w.set_mpo(y2)
            twin = w.clone()
            twin.set_mpo(y2)
            for name, table in tables.items():
                want, has, cols_ref = _per_call_scan(twin, bottom, ext[:, y2, :], st, table)
                twin.ClearBTen()
                for mask in (None, opened):
                    got = w.pair_trace_slice(bottom, nf, table, mask)
                    done += 1
                    entry = has if mask is None else has & mask[:, None, None]
                    assert got.shape == want.shape == (NW, COLS - 1, 2) and got.dtype == want.dtype
                    assert entry.any() and (~entry).any()
                    assert np.all(got[~entry] == 0.0), (y2, name)                   # closed and masked entries: exactly zero
                    assert np.all(got[entry] != 0.0)
                    scale = np.max(np.abs(want[entry]))
                    err = np.max(np.abs(got - want)[entry]) / scale
                    print("pair trace slice", dtype, "row", y2, name, "masked" if mask is not None else "all", "open", int(entry.sum()),
                          "rel err", err)
                    assert err < tol, (y2, name, err)
                    assert (w.GetBTenLeftCol(), w.GetBTenRightCol()) == cols_ref == (COLS - 2, COLS)
                    if dtype == "c128":
                        assert np.max(np.abs(got.imag)) > 0
                    w.ClearBTen()
            # the identity slot is the walker's own two-site trace
            w.InitBTenLeft(bottom, 0)
            w.InitBTenRight(bottom, 1)
            own = w.TraceWithTwoSiteBTen(bottom, 0)
            w.ClearBTen()
            ident = w.pair_trace_slice(bottom, nf, tables["identity"])[:, 0, 0]
            done += 1
            is_pair = np.array([_pair(c, y2, 0) in (UD, DU) for c in cfgs])
            assert is_pair.any() and np.max(np.abs(ident - own)[is_pair]) < tol * np.max(np.abs(own[is_pair]))
            w.ClearBTen()
            twin.destroy()
    assert capi.diag_walker_pair_slice_calls() - calls0 == done
    ctx.close()


# ---- 3. the assembled estimator against fresh amplitudes ----
@functools.lru_cache(maxsize=None)
def _fresh(dtype):
    """the estimator of every walker and bond pair from fresh amplitudes of the changed configurations, evaluated on a second context"""
    from peps_amd import fermion
    st, ctx = _state(dtype)
    cfgs = _configs()
    need, index = [], {}
    for c in cfgs:
        index[c.tobytes()] = len(need)
        need.append(c)
        for y1, x1, _, y2, x2, _ in pc.index_mapping(ROWS, COLS):
            if _pair(c, y1, x1) == EE and _pair(c, y2, x2) in (UD, DU):
                for p in (UD, DU):
                    new = c.copy()
                    new[y1, x1], new[y1, x1 + 1] = p
                    new[y2, x2], new[y2, x2 + 1] = EE
                    if new.tobytes() not in index:
                        index[new.tobytes()] = len(need)
                        need.append(new)
    need = np.array(need)
    psi = np.concatenate([fermion.evaluate_amplitude(ctx, st, need[i:i + NW]) for i in range(0, len(need), NW)])
    ctx.close()
    amp = lambda c: psi[index[np.asarray(c, dtype=cfgs.dtype).tobytes()]]
    out = np.array([pc.estimator_from_amplitudes(c, amp)[0] for c in cfgs])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("dtype", ["f64", "c128"])
@pytest.mark.parametrize("scan", ["slice", "calls"])
def test_assembled_estimator_equals_fresh_amplitudes(dtype, scan):
    """fermion.tj_pair_correlation for every walker and bond pair against the ratio of fresh amplitudes (Sigma applied) at 1e-9
    relative per term; entries without a term exactly zero.  float32 is covered by the slice-against-per-call test only: its
    distance to a differently ordered contraction has not been measured."""
    from peps_amd import capi, fermion
    st, ctx = _state(dtype)
    cfgs = _configs()
    want = _fresh(dtype)
    calls0 = capi.diag_walker_pair_slice_calls()
    got = fermion.tj_pair_correlation(ctx, st, cfgs, scan=scan)
    nz = want != 0
    assert got.shape == want.shape == (NW, pc.num_sc_pairs(ROWS, COLS)) and nz.sum() >= 12
    assert np.all(got[~nz] == 0)
    err = np.max(np.abs(got - want)[nz] / np.abs(want[nz]))
    print("pair correlation", dtype, scan, "terms", int(nz.sum()), "max rel err", err)
    assert err <= 1e-9
    assert (capi.diag_walker_pair_slice_calls() > calls0) == (scan == "slice")
    # a selection (unsorted, with an out-of-lattice bond) returns the sub-vector
    sel = [(1, 2), (0, 1), (2, 0)]
    idx = [i for i, m in enumerate(pc.index_mapping(ROWS, COLS)) if (m[0], m[1]) in ((0, 1), (1, 2))]
    sub = fermion.tj_pair_correlation(ctx, st, cfgs, ref_bonds=sel, scan=scan)
    assert sub.shape == (NW, 9) and np.array_equal(sub, got[:, idx])
    ctx.close()


# ---- 4. the host layer ----
_HOOK = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from peps_amd import capi, hostapi
import test_gpu_pair_corr as t

out = {}
for name in ("f64", "f32", "c128"):
    v = t._host_values(name)
    out[name] = [[float(x.real), float(x.imag)] for x in np.asarray(v, dtype=complex).ravel()]
out["pair_calls"] = capi.diag_walker_pair_slice_calls()
print(json.dumps(out))
"""
MODEL = dict(model="tj", params=(1.0, 0.3, 0.0, 0.0, 0.0))


def _host_state(dtype):
    from peps_amd import fermion
    st = ref.tj_state(ROWS, COLS, D)
    if dtype == "c128":
        rng = np.random.default_rng(3)
        st = fermion.FermionState([[[t * np.exp(2j * np.pi * rng.uniform(size=t.shape)) for t in site] for site in row]
                                   for row in st.tensors], st.par, st.nf)
    return st


def _host_values(dtype, ref_bonds=()):
    """SC_singlet_pair_corr [n][pairs] of the host layer's SquaretJVModel on the test's walkers"""
    from peps_amd import hostapi
    obs, _ = hostapi.fermion_observables(_host_state(dtype), _configs(), CHI, dtype=0 if dtype == "f32" else 1, sc_pair_corr=True,
                                         ref_bonds=ref_bonds, **MODEL)
    return obs["SC_singlet_pair_corr"]


def test_host_layer_pair_correlation():
    """hostapi.fermion_observables(sc_pair_corr=True): the mixin's values against the Python twin on capi (f64 / c128 at 1e-12, f32
    at 1e-5 of the largest value: the same launches, a different host arithmetic of the ratio), the slice path bit for bit against the
    per-call hooks (a child process with PEPSHOST_NO_DEVICE_SWEEP=1), a selection of two reference bonds against the sub-vector, and
    the default: no key, no call."""
    from peps_amd import capi, fermion, hostapi
    cfgs = _configs()
    calls0 = capi.diag_walker_pair_slice_calls()
    plain, _ = hostapi.fermion_observables(_host_state("f64"), cfgs, CHI, **MODEL)
    assert "SC_singlet_pair_corr" not in plain and "SC_bond_singlet_h" in plain
    assert capi.diag_walker_pair_slice_calls() == calls0                      # disabled: no extra call
    e = {k: v for k, v in os.environ.items() if k != "PEPSHOST_NO_DEVICE_SWEEP"}
    r = subprocess.run([sys.executable, "-c", _HOOK, ROOT], env=dict(e, PEPSHOST_NO_DEVICE_SWEEP="1"), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    hook = json.loads(r.stdout.strip().splitlines()[-1])
    assert hook["pair_calls"] == 0
    mapping = pc.index_mapping(ROWS, COLS)
    for dtype in ("f64", "f32", "c128"):
        before = capi.diag_walker_pair_slice_calls()
        got = _host_values(dtype)
        assert capi.diag_walker_pair_slice_calls() > before
        assert got.shape == (NW, len(mapping))
        # with the switch on, the other keys keep their bytes
        if dtype == "f64":
            full, _ = hostapi.fermion_observables(_host_state("f64"), cfgs, CHI, sc_pair_corr=True, **MODEL)
            assert set(full) == set(plain) | {"SC_singlet_pair_corr"}
            for key in plain:
                assert np.array_equal(full[key], plain[key]), key
        h = np.array(hook[dtype])
        h = (h[:, 0] + 1j * h[:, 1]).reshape(got.shape)
        assert np.array_equal(np.asarray(got, dtype=complex), h), dtype       # slice path == hook path, bit for bit
        st, ctx = _state(dtype)
        twin = fermion.tj_pair_correlation(ctx, st, cfgs)
        ctx.close()
        nz = twin != 0
        assert nz.sum() >= 12 and np.array_equal(got != 0, nz)
        err = np.max(np.abs(got - twin)) / np.max(np.abs(twin))
        print("host layer against the Python twin", dtype, "rel err", err)
        assert err < TOL[dtype]
        if dtype == "f64":
            assert np.max(np.abs(got - _fresh("f64"))[nz] / np.abs(_fresh("f64")[nz])) <= 1e-9
    # a selection of two reference bonds: the corresponding sub-vector, the mapping of the shim
    sel = [(1, 2), (0, 1)]
    full = _host_values("f64")
    sub = _host_values("f64", sel)
    idx = [i for i, m in enumerate(mapping) if (m[0], m[1]) in ((0, 1), (1, 2))]
    assert sub.shape == (NW, 9) and np.array_equal(sub, full[:, idx])
    assert [tuple(m) for m in hostapi.sc_pair_corr_mapping(ROWS, COLS, sel).tolist()] == [mapping[i] for i in idx]
    with pytest.raises(ValueError):                                           # not an observable of the spinless model
        hostapi.fermion_observables(_host_state("f64"), cfgs, CHI, model="spinless", params=(1.0, 0.0, 0.0), sc_pair_corr=True)


# ---- 5. the exact sum against the dense operator ----
@pytest.mark.parametrize("shape", [(2, 3), (3, 2)])
def test_exact_sum_reproduces_the_dense_pair_pair_operator(shape):
    """fermion_exact_sum_measure over the 365 parity-even configurations of the D = 2 state of tests/test_cpu_pair_corr.py, f64:
    SC_singlet_pair_corr equals <Delta+_ref Delta_tgt> of the dense operator on the device's own amplitudes at 1e-9"""
    from peps_amd import capi, fermion, hostapi
    rows, cols = shape
    st = ref.tj_state(rows, cols, 2)
    cfgs = ref.all_tj_configs(rows, cols)
    ctx = capi.Context(rows, cols, st.D, fermion.NVAR * st.d, 16, dtype=capi.F64, max_walkers=64)
    ctx.state_upload(st.extended_flat())
    psi = np.concatenate([fermion.evaluate_amplitude(ctx, st, cfgs[i:i + 64]) for i in range(0, len(cfgs), 64)])
    ctx.close()
    even = np.sum(cfgs != ref.EMPTY, axis=(1, 2)) % 2 == 0
    assert even.sum() == 365 and np.max(np.abs(psi[~even])) < 1e-12 * np.max(np.abs(psi))
    psi[~even] = 0.0
    cache, dense = {}, []
    for y1, x1, _, y2, x2, _ in pc.index_mapping(rows, cols):
        M = pc.dense_pair_corr(rows, cols, (y1, x1), (y2, x2), cache)
        dense.append((np.conj(psi) @ (M @ psi)) / (np.conj(psi) @ psi))
    dense = np.array(dense)
    sums, weight = hostapi.fermion_exact_sum_measure(st, cfgs[even], 16, batch=64, sc_pair_corr=True, **MODEL)
    got = sums["SC_singlet_pair_corr"] / weight
    print("exact sum", shape, "max |got - dense|", np.max(np.abs(got - dense)), "dense", dense)
    assert got.shape == dense.shape == (pc.num_sc_pairs(rows, cols),)
    assert np.min(np.abs(dense)) > 1e-6
    assert np.max(np.abs(got - dense)) <= 1e-9
    plain, w0 = hostapi.fermion_exact_sum_measure(st, cfgs[even], 16, batch=64, **MODEL)
    assert "SC_singlet_pair_corr" not in plain and w0 == weight
    for key in plain:
        assert np.array_equal(plain[key], sums[key]), key


# ---- 6. refusals ----
def test_refusals_leave_walker_and_context_usable():
    from peps_amd import capi, fermion
    st, ctx, cfgs = _ready("f64")
    nf = np.ascontiguousarray(st.nf % 2, dtype=np.int32)
    inject, remove = fermion.tj_pair_inject_table(), fermion.tj_pair_remove_table()
    lib, h = ctx._l, ctx._h
    ip = lambda a: None if a is None else capi._ip(np.ascontiguousarray(a, dtype=np.int32))
    u8 = lambda a: None if a is None else a.ctypes.data_as(capi.C.POINTER(capi.C.c_uint8))
    w = ctx.get_walker(capi.UP, level=0)
    dn = ctx.get_walker(capi.DOWN)
    op, sg = np.zeros(NW, dtype=np.uint8), np.zeros(NW, dtype=np.int32)
    out = np.zeros((NW, COLS - 1, 2))

    def excite(wk=w, num=0, col=1, d=3, o=nf, t=inject, slot=0):
        return lib.pepsgpu_walker_set_mpo_excited_pair(h, wk.wid, num, col, d, ip(o), ip(t), slot, u8(op), ip(sg))

    def scan(wk=w, lvl=ROWS - 2, d=3, o=nf, t=remove, m=None, q=out):
        return lib.pepsgpu_walker_pair_trace_slice(h, wk.wid, lvl, d, ip(o), ip(t), u8(m), None if q is None else capi._dp(q))

    def bad_tables():
        b = inject.copy(); b[8, 0] = (3, 0); yield b               # entry outside [-1, d)
        b = inject.copy(); b[8, 0] = (-2, -2); yield b
        b = inject.copy(); b[8, 0] = (-1, 0); yield b              # a half-empty candidate
        b = inject.copy(); b[8, 0] = (2, 0); yield b               # (empty, empty) -> (empty, up): the pair's parity changes

    assert scan() == 3                                             # no MPO set: PEPSGPU_ESTATE
    assert excite() == 0
    w.Evolve()
    w.set_mpo(1)
    good = w.pair_trace_slice(ROWS - 2, nf, remove)
    calls = capi.diag_walker_pair_slice_calls()
    # PEPSGPU_EINVAL
    assert excite(o=None) == 1 and excite(t=None) == 1 and scan(o=None) == 1 and scan(t=None) == 1 and scan(q=None) == 1
    assert excite(wk=dn) == 1                                      # a walker that is not UP
    assert excite(d=2) == 1 and scan(d=2) == 1                     # 4 d != the physical dimension
    assert excite(o=np.array([1, 2, 0])) == 1 and scan(o=np.array([1, 2, 0])) == 1
    assert excite(slot=2) == 1 and excite(slot=-1) == 1
    assert excite(col=COLS - 1) == 1 and excite(col=-1) == 1 and excite(num=ROWS) == 1 and excite(num=-1) == 1
    for b in bad_tables():
        assert excite(t=b) == 1 and scan(t=b) == 1
    dn.set_mpo(ROWS - 1)
    assert scan(wk=dn) == 1
    # PEPSGPU_ESTATE
    assert scan(lvl=ROWS) == 3 and scan(lvl=-1) == 3               # opp_level not in the DOWN stack
    t = ctx.get_walker(capi.UP, level=1)
    t.set_mpo_tensors(1, np.zeros((1, COLS, D, D, D, D)))
    assert scan(wk=t) == 3                                         # an MPO given as explicit tensors
    t.destroy()
    ctx.cfg_override_slice(capi.HORIZONTAL, 0, st.ext_config(cfgs, 0)[:, 0, :])
    assert scan() == 3                                             # a configuration override is active
    ctx.cfg_override_slice(capi.HORIZONTAL, 0, None)
    col_major = st.ext_config(cfgs, 1)[:, 1, :]
    w.set_mpo_states(1, col_major)
    assert scan() == 3                                             # a state of the row with a column-major variant
    w.set_mpo(1)
    assert capi.diag_walker_pair_slice_calls() == calls            # a refused call is no completed call
    assert (w.GetBTenLeftCol(), w.GetBTenRightCol()) == (COLS - 2, COLS)    # ... and released no cache
    again = w.pair_trace_slice(ROWS - 2, nf, remove)
    assert np.array_equal(good, again)
    # a refused set_mpo_excited_pair keeps the walker's MPO: the scan still runs on row 1
    assert excite(slot=2) == 1
    assert np.array_equal(w.pair_trace_slice(ROWS - 2, nf, remove), good)
    # column-major configurations: the excited row refuses, row-major ones serve again
    ctx.set_configs(st.ext_config(cfgs, 1))
    ctx.generate_bmps_approach(capi.UP)
    w2 = ctx.get_walker(capi.UP, level=0)
    assert excite(wk=w2) == 3
    ctx.set_configs(st.ext_config(cfgs, 0))
    ctx.generate_bmps_approach(capi.UP)
    w3 = ctx.get_walker(capi.UP, level=0)
    assert excite(wk=w3) == 0
    w3.Evolve()
    w3.set_mpo(1)
    assert np.array_equal(w3.pair_trace_slice(ROWS - 2, nf, remove), good)
    ctx.close()

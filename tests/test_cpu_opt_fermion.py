"""CPU checks of the fermionic mode of the device-resident optimizer: the NumPy restatement of the projection (tests/opt_fermion_ref.py)
against fermion.fold_gradient / extended_flat, the bitwise equivariance of the update rules under the decoration that lets the device
reuse its element-wise rule kernels on the extended layout, and the new entry points (no compute call is made)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import opt_fermion_ref as fref  # noqa: E402
import opt_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nonuniform_state(seed):
    """2x3 lattice, horizontal bonds of dimension 3 (parities 0, 1, 1) and 2 (0, 1), vertical bonds of dimension 2 (1, 0) and 1;
    three physical states of parities (1, 1, 0) as the t-J model has them"""
    from peps_amd import fermion
    rng = np.random.default_rng(seed)
    one = np.zeros(1, dtype=np.int64)
    hb = [np.array([0, 1, 1]), np.array([0, 1])]           # bond between columns 0-1, 1-2
    vb = [np.array([1, 0]), np.array([1, 0]), np.array([0])]   # bond between the rows, per column
    nf = [1, 1, 0]
    rows, cols = 2, 3
    tensors, par = [[None] * cols for _ in range(rows)], [[None] * cols for _ in range(rows)]
    for r in range(rows):
        for c in range(cols):
            p = (one if c == 0 else hb[c - 1], one if r == rows - 1 else vb[c], one if c == cols - 1 else hb[c], one if r == 0 else vb[c])
            par[r][c] = p
            tot = p[0][:, None, None, None] + p[1][None, :, None, None] + p[2][None, None, :, None] + p[3][None, None, None, :]
            tensors[r][c] = [rng.standard_normal(tot.shape) * ((tot + n) % 2 == 0) for n in nf]
    return fermion.FermionState(tensors, par, nf)


def _states():
    from peps_amd import fermion
    return [fermion.random_even_state(3, 3, 5, 11), _nonuniform_state(5)]


@pytest.mark.parametrize("which", [0, 1])
def test_projection_restatement_identities(which):
    from peps_amd import fermion
    st = _states()[which]
    ext = st.extended_flat()
    assert np.array_equal(fref.project(st, ext), 4 * ext)
    assert np.array_equal(fref.decorate(st, fref.stored_flat(st)), ext)
    x = np.random.default_rng(3).standard_normal(ext.shape)
    px = fref.project(st, x)
    fx = fermion.fold_gradient(st, x)
    assert np.array_equal(fermion.fold_gradient(st, px), 4 * fx)
    assert np.array_equal(px[:, :, :st.d], fx)
    assert np.array_equal(px, fref.decorate(st, fx))
    assert np.all(fx[~fref.allowed_flat(st)] == 0) and np.count_nonzero(fx) == np.count_nonzero(fref.allowed_flat(st))
    # stored norm = 1/2 extended norm on the range of the decoration
    assert abs(opt_ref.norm([px]) - 2 * opt_ref.norm([fx])) <= 4e-16 * opt_ref.norm([px])


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("setting", opt_ref.SETTINGS, ids=[s[0] for s in opt_ref.SETTINGS])
def test_rules_commute_with_the_decoration_bitwise(which, setting):
    """three successive steps on (E theta, Pi g_ext) == E of the steps on (theta, fold(g_ext)), bit for bit: the rules are element-wise,
    a sign flip of (theta, g, velocity, m1) flips their results exactly, m2 / acc see |g|^2"""
    from peps_amd import fermion
    _, rule, lr, params = setting
    st = _states()[which]
    rng = np.random.default_rng(17)
    theta = [fref.stored_flat(st)]
    theta_ext = [st.extended_flat()]
    rs, rs_ext = opt_ref.RuleState(theta), opt_ref.RuleState(theta_ext)
    for _ in range(3):
        g_ext = rng.standard_normal(theta_ext[0].shape)
        theta = opt_ref.step(rule, theta, [fermion.fold_gradient(st, g_ext)], rs, lr, params)
        theta_ext = opt_ref.step(rule, theta_ext, [fref.project(st, g_ext)], rs_ext, lr, params)
        assert np.array_equal(theta_ext[0], fref.decorate(st, theta[0]))
    assert not np.array_equal(theta[0], fref.stored_flat(st))
    back = fermion.FermionState.from_stored(st, theta[0])        # the result can be fed back: still parity even
    assert np.array_equal(back.extended_flat(), theta_ext[0])


def test_fermion_entry_points_declared_exported_and_bound():
    from peps_amd import capi, hostapi
    if not os.path.exists(capi.LIB_PATH) or not os.path.exists(hostapi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    header = open(os.path.join(ROOT, "include", "pepsgpu.h")).read()
    declared = set(re.findall(r"\b(pepsgpu_[a-z0-9_]+)\s*\(", header))
    name = "pepsgpu_fermion_decoration_set"
    assert name in declared and name in capi.SYMBOLS
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), name)
    assert len(getattr(capi.load_library(), name).argtypes) == 4
    assert callable(capi.Context.fermion_decoration_set)
    lib = ctypes.CDLL(hostapi.LIB_PATH)
    for shim in ("pepshost_fermion_optimize_exact_sum", "pepshost_fermion_optimize_exact_sum_c128", "pepshost_fermion_sr_step_samples",
                 "pepshost_fermion_sr_step_samples_c128"):
        assert hasattr(lib, shim), shim
        assert shim in hostapi.SYMBOLS, shim
    assert callable(hostapi.fermion_optimize_exact_sum) and callable(hostapi.fermion_sr_step_samples)

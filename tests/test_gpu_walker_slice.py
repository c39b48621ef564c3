"""GPU tests of the device-side row scan of the structure-factor measurement: pepsgpu_walker_set_mpo_excited and
pepsgpu_walker_trace_slice against the per-call sequence of the same BMPSWalker (InitBTenLeft / InitBTenRight / TraceWithBTen /
GrowBTenRightStep), set_mpo_excited against set_mpo_states, the error paths, and MeasureStructureFactor of the host layer on the
slice path against its per-call body (PEPSHOST_NO_DEVICE_SWEEP=1) and the oracle, end to end.

Lattice 3 x 4 (non-square: two target rows and one Evolve between their scans; a boundary, an interior and a last column), D = 3,
chi = 5 (truncating, no power of two), 5 walkers."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the project's tolerances for "slice against per-call" (tests/test_gpu_link_slice.py), relative to the largest reference magnitude
TOL = {"f64": 1e-12, "f32": 1e-5, "c128": 1e-12}
LY, LX, D, CHI, NW = 3, 4, 3, 5, 5
SRC = (0, 1)                                     # the source site (y1, x1) of the excited row
# walker 0: the source holds state 1 (closed); walker 1: every position of row 1 closed; column 2 of row 1: closed for every walker
CFGS = np.array([[[0, 1, 0, 1], [1, 0, 0, 1], [1, 1, 0, 0]],
                 [[1, 0, 1, 0], [0, 0, 0, 0], [1, 0, 1, 1]],
                 [[0, 0, 1, 1], [1, 1, 0, 0], [0, 1, 0, 1]],
                 [[1, 0, 0, 1], [0, 1, 0, 1], [1, 0, 0, 0]],
                 [[0, 0, 1, 0], [1, 0, 0, 1], [0, 0, 0, 1]]], dtype=np.int32)


def _dtype(name):
    from peps_amd import capi
    return {"f64": capi.F64, "f32": capi.F32, "c128": capi.C128}[name]


def _case(d):
    """(configurations, state_map of the source, site_map of the targets) for phys_dim d.  d = 2: S+ at the source, S- at the targets.
    d = 3: the same open / closed pattern with the closed target state 2 and open target states 0 and 1, one more state 2 on row 0."""
    if d == 2:
        return CFGS, np.array([1, 1], dtype=np.int32), np.array([0, 0], dtype=np.int32)
    cfg = CFGS.copy()
    w, x = np.arange(NW)[:, None, None], np.arange(LX)[None, None, :]
    cfg[:, 1:, :] = np.where(CFGS[:, 1:, :] == 1, (w + x) % 2, 2)
    cfg[2, 0, 3] = 2
    return cfg, np.array([1, 1, 1], dtype=np.int32), np.array([2, 2, 2], dtype=np.int32)


def _open_tables(cfg, smap, tmap):
    """src_open [n], tgt_open [n][Ly][Lx] (before the source mask)"""
    s = cfg[:, SRC[0], SRC[1]]
    return smap[s] != s, tmap[cfg] != cfg


def test_the_configurations_are_as_intended():
    for d in (2, 3):
        cfg, smap, tmap = _case(d)
        assert cfg.shape == (NW, LY, LX) and cfg.min() >= 0 and cfg.max() == d - 1
        src, tgt = _open_tables(cfg, smap, tmap)
        assert src.tolist() == [False, True, True, True, True]                 # one walker whose source is closed
        assert not tgt[1, 1].any()                                             # one walker whose target row is closed everywhere
        assert not tgt[:, 1, 2].any()                                          # one column at which every walker is closed
        entry = src[:, None, None] & tgt
        assert entry[:, 1, :].any(axis=0).tolist() == [True, True, False, True]
        for w in (2, 3, 4):                                                    # an open entry in each target row of the other walkers
            assert entry[w, 1].any() and entry[w, 2].any()
        assert entry[1, 2].any() and not entry[0].any()


def _state(d, cplx):
    rng = np.random.default_rng(5)
    flat = np.zeros((LY, LX, d, D, D, D, D), dtype=np.complex128 if cplx else np.float64)
    sitps = []
    for r in range(LY):
        sitps.append([])
        for c in range(LX):
            shp = (1 if c == 0 else D, 1 if r == LY - 1 else D, 1 if c == LX - 1 else D, 1 if r == 0 else D)
            sitps[r].append([])
            for k in range(d):
                t = rng.standard_normal(shp) + 0.3
                if cplx:
                    t = t * np.exp(2j * np.pi * rng.uniform(size=shp))
                sitps[r][c].append(t)
                flat[r, c, k, :shp[0], :shp[1], :shp[2], :shp[3]] = t
    return sitps, flat


def _context(dtype, d):
    from peps_amd import capi
    ctx = capi.Context(LY, LX, D, d, CHI, dtype=_dtype(dtype), max_walkers=NW)
    ctx.state_upload(_state(d, dtype == "c128")[1])
    ctx.set_configs(_case(d)[0])
    ctx.generate_bmps_approach(capi.UP)          # UP = the vacuum, DOWN fully grown: the state the mixin starts from
    assert ctx.bmps_stack_size(capi.DOWN) == LY
    return ctx


def _excited(ctx, d):
    """the mixin's excited walker after Evolve through the excited row (built on the device), and the open mask of the source"""
    from peps_amd import capi
    main = ctx.get_walker(capi.UP, level=0)
    ex = main.clone()
    opened = ex.set_mpo_excited(SRC[0], SRC[1], _case(d)[1])
    ex.Evolve()
    return ex, opened


def _per_call_scan(w, bottom, y2, cfg, tmap):
    """the target-row loop of MeasureStructureFactor through the per-call entries: [n][Lx] traces at every position, every walker"""
    w.set_mpo(y2)
    w.InitBTenLeft(bottom, LX)
    w.InitBTenRight(bottom, LX - 1)
    rows = np.zeros((cfg.shape[0], LX), dtype=w.ctx._ot)
    for x2 in range(LX - 1, -1, -1):
        rows[:, x2] = w.TraceWithBTen(bottom, x2, states=tmap[cfg[:, y2, x2]])
        if x2 > 0:
            w.GrowBTenRightStep(bottom)
    return rows, (w.GetBTenLeftCol(), w.GetBTenRightCol())


@functools.lru_cache(maxsize=None)
def _reference(dtype, d):
    """per-call traces {y2: [n][Lx]} of both target rows (every entry computed; the callers mask) and the cache columns they leave"""
    ctx = _context(dtype, d)
    cfg, _, tmap = _case(d)
    ex, _ = _excited(ctx, d)
    out = {}
    for y2 in (1, 2):
        out[y2] = _per_call_scan(ex, LY - 1 - y2, y2, cfg, tmap)
        ex.ClearBTen()
        if y2 + 1 < LY:
            ex.Evolve()
    ctx.close()
    for v, _ in out.values():
        v.setflags(write=False)
    return out


def _check_rows(dtype, d, y2, got, opened, what):
    cfg, smap, tmap = _case(d)
    src, tgt = _open_tables(cfg, smap, tmap)
    assert np.array_equal(opened, src)
    want, _ = _reference(dtype, d)[y2]
    entry = src[:, None] & tgt[:, y2, :]
    assert got.shape == want.shape == (NW, LX) and got.dtype == want.dtype
    assert np.all(got[~entry] == 0.0), (what, y2)                  # closed entries: exactly zero
    scale = np.max(np.abs(want[entry]))
    err = np.max(np.abs(got - want)[entry]) / scale
    print("walker slice", what, dtype, "d", d, "row", y2, "open", int(entry.sum()), "rel err", err)
    assert scale > 0 and err < TOL[dtype], (what, y2, err)


# ---- 1. the slice against the per-call scan ----
@pytest.mark.parametrize("dtype,d", [("f64", 2), ("f32", 2), ("c128", 2), ("f64", 3)])
def test_trace_slice_matches_the_per_call_scan(dtype, d):
    """set_mpo_excited, Evolve, the standard row, trace_slice for both target rows (one Evolve between them) against a walker driven
    through InitBTenLeft / InitBTenRight / TraceWithBTen / GrowBTenRightStep; d = 3 with site_map = [2, 2, 2] checks the stride of the
    state table."""
    from peps_amd import capi
    ctx = _context(dtype, d)
    tmap = _case(d)[2]
    ex, opened = _excited(ctx, d)
    calls0 = capi.diag_walker_slice_calls()
    for y2 in (1, 2):
        bottom = LY - 1 - y2
        ex.set_mpo(y2)
        got = ex.trace_slice(bottom, tmap, opened)
        _check_rows(dtype, d, y2, got, opened, "slice")
        assert (ex.GetBTenLeftCol(), ex.GetBTenRightCol()) == (LX, 1) == _reference(dtype, d)[y2][1]
        ex.ClearBTen()
        if y2 + 1 < LY:
            ex.Evolve()
    assert capi.diag_walker_slice_calls() - calls0 == 2
    # without a mask the walker whose source is closed is computed too: its row-2 entries are the per-call values
    ex.set_mpo(2)
    got = ex.trace_slice(0, tmap)
    want, _ = _reference(dtype, d)[2]
    tgt = _open_tables(*_case(d))[1][:, 2, :]
    assert tgt[0].any() and np.all(got[~tgt] == 0.0)
    assert np.max(np.abs(got - want)[tgt]) < TOL[dtype] * np.max(np.abs(want[tgt]))
    assert capi.diag_walker_slice_calls() - calls0 == 3
    ctx.close()


# ---- 2. set_mpo_excited against set_mpo_states ----
@pytest.mark.parametrize("dtype,d", [("f64", 2), ("f32", 2), ("c128", 2), ("f64", 3)])
def test_set_mpo_excited_matches_set_mpo_states(dtype, d):
    """the excited row built on the device against the same row built in NumPy and uploaded: the open mask, and ContractRow after
    Evolve against DOWN level 1 (MPO row 1) and, one Evolve later, DOWN level 0 (MPO row 2)"""
    from peps_amd import capi
    ctx = _context(dtype, d)
    cfg, smap, _ = _case(d)
    row = cfg[:, SRC[0], :].copy()
    row[:, SRC[1]] = smap[row[:, SRC[1]]]
    main = ctx.get_walker(capi.UP, level=0)
    a, b = main.clone(), main.clone()
    opened = a.set_mpo_excited(SRC[0], SRC[1], smap)
    assert opened.dtype == bool and np.array_equal(opened, row[:, SRC[1]] != cfg[:, SRC[0], SRC[1]])
    b.set_mpo_states(SRC[0], row)
    for w in (a, b):
        w.Evolve()
    for y2 in (1, 2):
        va, vb = [], []
        for w, v in ((a, va), (b, vb)):
            w.set_mpo(y2)
            v.append(w.ContractRow(LY - 1 - y2))
            if y2 + 1 < LY:
                w.Evolve()
        scale = np.max(np.abs(vb[0]))
        err = np.max(np.abs(va[0] - vb[0])) / scale
        print("set_mpo_excited", dtype, "d", d, "ContractRow level", LY - 1 - y2, "rel err", err)
        assert scale > 0 and err < TOL[dtype]
    ctx.close()


# ---- 3. the host layer, end to end ----
_E2E = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from peps_amd import capi, hostapi
import test_gpu_walker_slice as t

def cx(a):
    a = np.asarray(a)
    return [[float(x.real), float(x.imag)] for x in a.ravel()] if np.iscomplexobj(a) else [float(x) for x in a.ravel()]

params = (1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)          # params[7] = structure factor on
out = {}
for name, dt in (("f64", 1), ("f32", 0), ("c128", 1)):
    flat = t._state(2, name == "c128")[1]
    obs, _ = hostapi.measure(flat, t.CFGS, t.CHI, "xxz", params, dtype=dt)
    out[name] = {k: cx(v) for k, v in obs.items()}
out["walker_calls"] = capi.diag_walker_slice_calls()
print(json.dumps(out))
"""


def test_host_layer_structure_factor_on_the_slice_path():
    """host.measure with the structure factor on the 3 x 4 state in child processes with and without PEPSHOST_NO_DEVICE_SWEEP=1
    (f64, f32, c128): every registry key agrees, the process-wide counter proves which path ran, and the f64 SpSm_cross tuples are
    the oracle's per walker at the tolerance of tests/test_gpu_measure.py::test_structure_factor_cross_row_spsm."""
    from oracle import vmc
    from oracle.bmps import BMPSTruncateParams
    res = {}
    for name, env in (("device", {}), ("hook", {"PEPSHOST_NO_DEVICE_SWEEP": "1"})):
        e = {k: v for k, v in os.environ.items() if k != "PEPSHOST_NO_DEVICE_SWEEP"}
        r = subprocess.run([sys.executable, "-c", _E2E, ROOT], env=dict(e, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print("walker slice calls: device", res["device"]["walker_calls"], "hook", res["hook"]["walker_calls"])
    assert res["hook"]["walker_calls"] == 0
    # one slice per (y1, x1, y2), three element types
    assert res["device"]["walker_calls"] == 3 * LX * LY * (LY - 1) // 2
    for dt in ("f64", "f32", "c128"):
        assert set(res["hook"][dt]) == set(res["device"][dt]) and "SpSm_cross" in res["device"][dt]
        for key in res["hook"][dt]:
            a, b = np.array(res["device"][dt][key]), np.array(res["hook"][dt][key])
            if a.ndim == 2:
                a, b = a[:, 0] + 1j * a[:, 1], b[:, 0] + 1j * b[:, 1]
            assert a.shape == b.shape and a.size > 0, (dt, key)
            scale = max(np.max(np.abs(b)), 1e-300)
            print(dt, key, np.max(np.abs(a - b)) / scale)
            assert np.max(np.abs(a - b)) < TOL[dt] * scale, (dt, key, np.max(np.abs(a - b)) / scale)
    s = _state(2, False)[0]
    tp = BMPSTruncateParams.SVD(CHI, CHI, 0.0)
    have_all = np.array(res["device"]["f64"]["SpSm_cross"]).reshape(NW, -1, 5)
    for w, cfg in enumerate(CFGS):
        want = np.array(vmc.measure_structure_factor(s, vmc.TPSWaveFunctionComponent(s, cfg, tp))).reshape(-1, 5)
        have = have_all[w]
        assert have.shape == want.shape
        assert np.array_equal(have[:, :4], want[:, :4])
        scale = np.max(np.abs(want[:, 4]))
        print("SpSm_cross against the oracle, walker", w, np.max(np.abs(have[:, 4] - want[:, 4])) / scale)
        assert scale > 0 and np.max(np.abs(have[:, 4] - want[:, 4])) < 1e-9 * 10 * scale


# ---- 4. error paths ----
def test_walker_slice_error_paths():
    """every refusal of the two calls by status, on a walker that is in use; the same walker then computes the values of test 1"""
    import ctypes as C
    from peps_amd import capi
    d, dtype = 2, "f64"
    ctx = _context(dtype, d)
    cfg, smap, tmap = _case(d)
    lib, h = ctx._l, ctx._h
    ex, opened = _excited(ctx, d)
    ex.set_mpo(1)
    out = np.zeros((NW, LX))
    op = np.zeros(NW, dtype=np.uint8)
    u8 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))
    ip = lambda a: None if a is None else capi._ip(np.ascontiguousarray(a, dtype=np.int32))
    excite = lambda wk, num, col, m, o=op: lib.pepsgpu_walker_set_mpo_excited(h, wk.wid, num, col, ip(m), u8(o))
    scan = lambda wk, lvl, m, buf=out: lib.pepsgpu_walker_trace_slice(h, wk.wid, lvl, ip(m), None, None if buf is None else capi._dp(buf))
    calls0 = capi.diag_walker_slice_calls()
    # PEPSGPU_EINVAL: a null buffer, a site outside the lattice, a walker that is not UP
    assert scan(ex, 1, tmap, None) == 1 and scan(ex, 1, None) == 1 and excite(ex, 0, 1, None) == 1
    for num, col in ((-1, 1), (LY, 1), (0, -1), (0, LX)):
        assert excite(ex, num, col, smap) == 1, (num, col)
    down = ctx.get_walker(capi.DOWN)
    assert excite(down, 0, 1, smap) == 1
    down.set_mpo(1)
    assert scan(down, 1, tmap) == 1
    down.destroy()
    # PEPSGPU_ERANGE: a map entry outside [0, phys_dim)
    for bad in ([0, 2], [-1, 0]):
        assert excite(ex, 0, 1, bad) == 4 and scan(ex, 1, bad) == 4, bad
    with pytest.raises(IndexError):
        ex.trace_slice(1, [0, 2])
    # PEPSGPU_ESTATE: no MPO, an MPO of explicit tensors, an opposite level outside the DOWN stack, a configuration override
    fresh = ex.clone()
    assert scan(fresh, 1, tmap) == 3
    fresh.set_mpo_tensors(1, np.ones((1, LX, D, D, D, D)))
    assert scan(fresh, 1, tmap) == 3
    fresh.destroy()
    assert scan(ex, LY, tmap) == 3 and scan(ex, -1, tmap) == 3
    ctx.cfg_override_slice(capi.HORIZONTAL, 1, 1 - cfg[:, 1, :])
    assert scan(ex, 1, tmap) == 3
    ctx.cfg_override_slice(capi.HORIZONTAL, 1)
    assert capi.diag_walker_slice_calls() == calls0                # a refused call is not a completed one
    # the walker kept its MPO (row 1) and its boundary MPS through every refusal: the values of test 1, both rows
    _check_rows(dtype, d, 1, ex.trace_slice(1, tmap, opened), opened, "after the refusals")
    ex.ClearBTen()
    ex.Evolve()
    ex.set_mpo(2)
    _check_rows(dtype, d, 2, ex.trace_slice(0, tmap, opened), opened, "after the refusals")
    assert (ex.GetBTenLeftCol(), ex.GetBTenRightCol()) == (LX, 1)
    ctx.close()

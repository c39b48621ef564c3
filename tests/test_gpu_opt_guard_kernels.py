"""The base of a step through the C ABI (pepsgpu_guard_*, peps_amd/csrc/engine_guard.h): save, restore, clear and the SGD preview.
Every comparison is between two device results that the same arithmetic must produce, so every assertion is equality of bytes.
Layouts: 3x3, D = 5, d = 3 (slots of 25 / 125 / 625 live elements, three blocks per slot, rows of odd length: 8-byte accesses in
the real contexts, 16-byte ones in the complex context) and 2x3, D = 4, d = 2 (rows of 256 doubles, 16 or 64 of them live: 16-byte
accesses in the real contexts, most of every slot is padding)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ["f64", "f32", "c128"]
LAYOUTS = {"3x3D5": (3, 3, 5, 3), "2x3D4": (2, 3, 4, 2)}
# (momentum, nesterov, weight_decay) of pepsgpu_opt_step's SGD rule
SGD = {"plain": (0.0, 0.0, 0.0), "momentum": (0.9, 0.0, 0.0), "nesterov": (0.9, 1.0, 0.0), "decay": (0.0, 0.0, 0.1),
       "nesterov_decay": (0.7, 1.0, 0.05)}
LR = 0.05


def _mask(rows, cols, d, bond):
    m = np.zeros((rows, cols, d, bond, bond, bond, bond))
    for r in range(rows):
        for c in range(cols):
            m[r, c, :, :(1 if c == 0 else bond), :(1 if r == rows - 1 else bond), :(1 if c == cols - 1 else bond), :(1 if r == 0 else bond)] = 1.0
    return m


def _rand(rng, mask, cplx):
    x = rng.standard_normal(mask.shape)
    if cplx:
        x = x + 1j * rng.standard_normal(mask.shape)
    return x * mask


_CTX = {}


def _ctx(layout, dt):
    from peps_amd import capi
    key = (layout, dt)
    if key not in _CTX:
        rows, cols, bond, d = LAYOUTS[layout]
        _CTX[key] = capi.Context(rows, cols, bond, d, 8, dtype={"f64": capi.F64, "f32": capi.F32, "c128": capi.C128}[dt], max_walkers=4)
    return _CTX[key]


class _Run:
    """a context with a seeded state adopted, one SGD step taken (so that the velocity is not zero when momentum > 0) and a second
    gradient set: the point at which a step, or a preview of it, starts"""

    def __init__(self, layout, dt, params, seed=1):
        rows, cols, bond, d = LAYOUTS[layout]
        self.mask = _mask(rows, cols, d, bond)
        self.cplx = dt == "c128"
        rng = np.random.default_rng(seed)
        self.ctx = _ctx(layout, dt)
        self.ctx.state_upload(_rand(rng, self.mask, self.cplx))
        self.ctx.opt_begin()
        self.ctx.opt_set_gradient(_rand(rng, self.mask, self.cplx))
        self.ctx.opt_step(0, LR, params)
        self.g = _rand(rng, self.mask, self.cplx)
        self.ctx.opt_set_gradient(self.g)
        self.cfgs = np.random.default_rng(3).integers(0, d, size=(4, rows, cols)).astype(np.int32)

    def amplitudes(self):
        """what the device state gives: equal bytes here <=> equal sitps_ wherever these four configurations read it"""
        self.ctx.set_configs(self.cfgs)
        a = self.ctx.evaluate_amplitude()
        assert np.all(np.isfinite(a)) and np.all(a != 0)
        return a


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(SGD))
def test_preview_equals_the_step_and_leaves_the_velocity(layout, dt, name):
    p = SGD[name]
    # the step alone
    a = _Run(layout, dt, p)
    base = a.ctx.opt_read_state()
    a.ctx.opt_step(0, LR, p)
    want, want_amp = a.ctx.opt_read_state(), a.amplitudes()
    a.ctx.opt_set_gradient(a.g)
    a.ctx.opt_step(0, LR, p)                               # a second step: shows the velocity the first one left
    want2 = a.ctx.opt_read_state()
    assert not np.array_equal(want, base)
    # preview, a preview at another rate, the preview again: always from the base, never from theta
    b = _Run(layout, dt, p)
    b.ctx.opt_base_save()
    b.ctx.opt_preview(0, LR, p)
    got, got_amp = b.ctx.opt_read_state(), b.amplitudes()
    assert np.array_equal(got, want) and np.array_equal(got_amp, want_amp)
    b.ctx.opt_preview(0, 3 * LR, p)
    assert not np.array_equal(b.ctx.opt_read_state(), want)
    b.ctx.opt_preview(0, LR, p)
    assert np.array_equal(b.ctx.opt_read_state(), want)
    assert np.array_equal(b.ctx.opt_get_gradient(), b.g)          # g is read only
    assert np.all(got[b.mask == 0] == 0)                            # the padding stays exactly zero
    # restore, then the real step: the bytes of the step alone, now and one step later (theta and the velocity were untouched)
    b.ctx.opt_base_restore()
    assert np.array_equal(b.ctx.opt_read_state(), base)
    b.ctx.opt_step(0, LR, p)
    assert np.array_equal(b.ctx.opt_read_state(), want) and np.array_equal(b.amplitudes(), want_amp)
    b.ctx.opt_set_gradient(b.g)
    b.ctx.opt_step(0, LR, p)
    assert np.array_equal(b.ctx.opt_read_state(), want2)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dt", DTYPES)
def test_restore_ignores_a_poisoned_gradient_and_returns_the_saved_amplitudes(layout, dt):
    adam = (0.9, 0.999, 1e-8, 0.0)
    r = _Run(layout, dt, SGD["momentum"], seed=2)
    base, base_amp = r.ctx.opt_read_state(), r.amplitudes()
    r.ctx.opt_base_save()
    for k in range(3):                                     # several steps of another rule
        r.ctx.opt_set_gradient(_rand(np.random.default_rng(40 + k), r.mask, r.cplx))
        r.ctx.opt_step(2, 0.02, adam)
    assert not np.array_equal(r.ctx.opt_read_state(), base)
    for poison in (np.nan, np.inf):
        r.ctx.opt_set_gradient(np.full(r.mask.shape, complex(poison, poison) if r.cplx else poison))
        r.ctx.opt_step(0, LR, SGD["plain"])                # the spike: theta is destroyed
        assert not np.all(np.isfinite(r.ctx.opt_read_state()))
        r.ctx.opt_base_restore()
        got = r.ctx.opt_read_state()
        assert np.array_equal(got, base) and np.all(got[r.mask == 0] == 0)
        assert np.array_equal(r.amplitudes(), base_amp)
    # a second save overwrites the first
    r.ctx.opt_set_gradient(r.g)
    r.ctx.opt_step(0, LR, SGD["plain"])
    later = r.ctx.opt_read_state()
    r.ctx.opt_base_save()
    r.ctx.opt_step(0, LR, SGD["plain"])
    r.ctx.opt_base_restore()
    assert np.array_equal(r.ctx.opt_read_state(), later)


@pytest.mark.parametrize("dt", DTYPES)
def test_refusals(dt):
    from peps_amd import capi
    rows, cols, bond, d = LAYOUTS["2x3D4"]
    mask = _mask(rows, cols, d, bond)
    rng = np.random.default_rng(5)
    ctx = capi.Context(rows, cols, bond, d, 8, dtype={"f64": capi.F64, "f32": capi.F32, "c128": capi.C128}[dt], max_walkers=4)
    ctx.state_upload(_rand(rng, mask, dt == "c128"))
    p = SGD["plain"]
    # PEPSGPU_ESTATE before opt_begin
    for call in (ctx.opt_base_save, ctx.opt_base_restore, ctx.opt_base_clear, lambda: ctx.opt_preview(0, LR, p)):
        with pytest.raises(RuntimeError):
            call()
    ctx.opt_begin()
    theta = ctx.opt_read_state()
    g = _rand(rng, mask, dt == "c128")
    ctx.opt_set_gradient(g)
    # ... and for a restore / preview without a base
    for call in (ctx.opt_base_restore, lambda: ctx.opt_preview(0, LR, p)):
        with pytest.raises(RuntimeError):
            call()
    ctx.opt_base_clear()                                   # clearing nothing is fine
    ctx.opt_base_save()
    # PEPSGPU_EINVAL: a rule other than SGD, and the parameter errors of opt_step
    for rule, lr, params in ((1, LR, (1e-8, 0.0)), (2, LR, (0.9, 0.999, 1e-8, 0.0)), (3, LR, p), (-1, LR, p), (0, float("nan"), p),
                             (0, -LR, p), (0, LR, (0.9, 0.0)), (0, LR, (-0.1, 0.0, 0.0)), (0, LR, (0.0, 0.0, float("inf")))):
        with pytest.raises(ValueError):
            ctx.opt_preview(rule, lr, params)
    assert np.array_equal(ctx.opt_read_state(), theta) and np.array_equal(ctx.opt_get_gradient(), g)
    ctx.opt_preview(0, LR, p)                              # the refused calls left the base in place
    assert not np.array_equal(ctx.opt_read_state(), theta)
    ctx.opt_base_clear()
    for call in (ctx.opt_base_restore, lambda: ctx.opt_preview(0, LR, p)):
        with pytest.raises(RuntimeError):
            call()
    ctx.opt_base_save()                                    # the buffer is still there: theta after the preview is the new base
    stepped = ctx.opt_read_state()
    ctx.opt_step(0, LR, p)
    ctx.opt_base_restore()
    assert np.array_equal(ctx.opt_read_state(), stepped)
    ctx.opt_begin()                                        # a new begin drops the base
    with pytest.raises(RuntimeError):
        ctx.opt_base_restore()
    ctx.opt_end()
    with pytest.raises(RuntimeError):
        ctx.opt_base_save()
    ctx.close()


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_fermionic_decoration(dt):
    """2x3, D = 3, spinless fermions: theta, g and the velocity are decorated vectors; preview and restore keep them so."""
    from peps_amd import capi, fermion
    rows, cols, bond = 2, 3, 3
    st = fermion.random_even_state(rows, cols, bond, seed=7)
    cfgs = np.array([[[0, 1, 1], [1, 0, 1]], [[1, 1, 0], [0, 1, 1]], [[0, 0, 1], [1, 1, 1]], [[1, 1, 1], [1, 0, 0]]], dtype=np.int32)
    p = SGD["nesterov_decay"]

    def start():
        ctx = capi.Context(rows, cols, bond, 4 * st.d, 9, dtype=capi.F64 if dt == "f64" else capi.F32, max_walkers=4)
        ctx.state_upload(st.extended_flat())
        ctx.fermion_decoration_set(st)
        ctx.opt_begin()
        rng = np.random.default_rng(11)
        ctx.opt_set_gradient(rng.standard_normal(st.extended_flat().shape))      # (projected onto the range of the decoration)
        ctx.opt_step(0, LR, p)
        ctx.opt_set_gradient(rng.standard_normal(st.extended_flat().shape))
        return ctx

    a = start()
    base = a.opt_read_state()
    a.opt_step(0, LR, p)
    want, want_amp = a.opt_read_state(), fermion.evaluate_amplitude(a, st, cfgs)
    a.close()
    b = start()
    b.opt_base_save()
    b.opt_preview(0, LR, p)
    got = b.opt_read_state()
    assert np.array_equal(got, want) and np.array_equal(fermion.evaluate_amplitude(b, st, cfgs), want_amp)
    assert np.all(np.isfinite(want_amp)) and np.all(want_amp != 0)
    b.opt_set_gradient(np.full(st.extended_flat().shape, np.nan))
    b.opt_base_restore()
    assert np.array_equal(b.opt_read_state(), base)
    b.opt_begin()                                          # the restored device state passes the decoration check of opt_begin
    assert np.array_equal(b.opt_read_state(), base.astype(np.float32).astype(np.float64) if dt == "f32" else base)
    b.close()

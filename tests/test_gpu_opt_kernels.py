"""The device-resident optimisation step through the C ABI (pepsgpu_opt_*, peps_amd/csrc/engine_opt.h) against the NumPy
restatement tests/opt_ref.py.  Lattice 3x3, D = 5, d = 3: corner / edge / interior slots of 25 / 125 / 625 live elements (3 675 in
all): several blocks per slot, no extent a multiple of the wave, per-site extents differ.  float64, float32 and complex contexts."""
import os
import sys

import numpy as np
import pytest

from oracle import qlten_io, vmc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import opt_ref  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
L, D, DP, CHI = 3, 5, 3, 8
DTYPES = ["f64", "f32", "c128"]
# (id, rule, lr, params of pepsgpu_opt_step)
VARIANTS = [
    ("sgd_plain", 0, 0.05, (0.0, 0.0, 0.0)),
    ("sgd_decay", 0, 0.05, (0.0, 0.0, 0.1)),
    ("sgd_momentum", 0, 0.05, (0.9, 0.0, 0.0)),
    ("sgd_nesterov", 0, 0.05, (0.9, 1.0, 0.05)),
    ("adagrad_acc0", 1, 0.1, (1e-8, 0.0)),
    ("adagrad_acc0.1", 1, 0.1, (1e-8, 0.1)),
    ("adam", 2, 0.02, (0.9, 0.999, 1e-8, 0.0)),
    ("adam_decay", 2, 0.02, (0.9, 0.999, 1e-8, 0.01)),
]


def _mask(rows=L, cols=L, d=DP, bond=D):
    """1 where the padded state layout [row][col][s][L][D][R][U] holds a tensor element (boundary legs have dimension 1)"""
    m = np.zeros((rows, cols, d, bond, bond, bond, bond))
    for r in range(rows):
        for c in range(cols):
            m[r, c, :, :(1 if c == 0 else bond), :(1 if r == rows - 1 else bond), :(1 if c == cols - 1 else bond), :(1 if r == 0 else bond)] = 1.0
    return m


def _rand(rng, cplx, scale=1.0):
    m = _mask()
    x = rng.standard_normal(m.shape)
    if cplx:
        x = x + 1j * rng.standard_normal(m.shape)
    return scale * x * m


_CTX = {}


def _ctx(dt):
    from peps_amd import capi
    if dt not in _CTX:
        _CTX[dt] = capi.Context(L, L, D, DP, CHI, dtype={"f64": capi.F64, "f32": capi.F32, "c128": capi.C128}[dt], max_walkers=4)
    return _CTX[dt]


def _begin(dt, seed):
    """a fresh random state uploaded and adopted; returns (ctx, rng, the state as the device holds it in float64)"""
    rng = np.random.default_rng(seed)
    ctx = _ctx(dt)
    theta = _rand(rng, dt == "c128")
    ctx.state_upload(theta)
    ctx.opt_begin()
    if dt == "f32":
        theta = theta.astype(np.float32).astype(np.float64)
    return ctx, rng, theta


def test_mask_counts():
    m = _mask()
    per_slot = sorted(set(int(m[r, c, 0].sum()) for r in range(L) for c in range(L)))
    assert per_slot == [25, 125, 625] and int(m.sum()) == DP * 1225 == 3675


@pytest.mark.parametrize("dt", DTYPES)
def test_begin_reads_the_uploaded_state_and_gradient_round_trip(dt):
    ctx, rng, theta = _begin(dt, 1)
    got = ctx.opt_read_state()
    assert got.dtype == (np.complex128 if dt == "c128" else np.float64)
    assert np.array_equal(got, theta)                     # exact: float64 / complex128, or float32(input)
    g = _rand(rng, dt == "c128")
    ctx.opt_set_gradient(g)
    assert np.array_equal(ctx.opt_get_gradient(), g)
    junk = g + (1.0 - _mask()) * 7.0                       # what the caller puts into the padding never reaches the device
    ctx.opt_set_gradient(junk)
    back = ctx.opt_get_gradient()
    assert np.array_equal(back, g) and np.all(back[_mask() == 0] == 0)
    # scale: theta *= f, and the state follows
    ctx.opt_scale_state(0.75)
    assert np.array_equal(ctx.opt_read_state(), theta * 0.75)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name,rule,lr,params", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_three_steps_follow_the_restatement(dt, name, rule, lr, params):
    """Element-wise float64 arithmetic without reductions: 4 eps64 max|theta| per step covers the rounding of single operations
    (contraction into fused multiply-adds is off in the kernels; sqrt and the division are correctly rounded on both sides)."""
    ctx, rng, theta0 = _begin(dt, 10 + rule)
    mask = _mask()
    theta, st = [theta0], opt_ref.RuleState([theta0])
    for k in range(3):
        g = _rand(rng, dt == "c128")
        ctx.opt_set_gradient(g)
        ctx.opt_step(rule, lr, params)
        theta = opt_ref.step(rule, theta, [g], st, lr, params, mask=[mask])
        got = ctx.opt_read_state()
        err, bound = float(np.max(np.abs(got - theta[0]))), 4 * EPS * float(np.max(np.abs(theta[0])))
        print("%s %s step %d: max |theta - ref| = %.3e (bound %.3e)" % (dt, name, k + 1, err, bound))
        assert err <= bound
        assert np.array_equal(ctx.opt_get_gradient(), g)          # a step does not touch g
        assert np.all(got[mask == 0] == 0)                        # the padding stays exactly zero
    if dt == "f32":
        # the device state is float32(theta) bit for bit: the same amplitudes as a fresh context given float32(theta)
        from peps_amd import capi
        cfgs = np.random.default_rng(3).integers(0, DP, size=(4, L, L)).astype(np.int32)
        ctx.set_configs(cfgs)
        a = ctx.evaluate_amplitude()
        fresh = capi.Context(L, L, D, DP, CHI, dtype=capi.F32, max_walkers=4)
        fresh.state_upload(got.astype(np.float32))
        fresh.set_configs(cfgs)
        b = fresh.evaluate_amplitude()
        fresh.close()
        assert np.all(np.isfinite(a)) and np.all(a != 0) and np.array_equal(a, b)


@pytest.mark.parametrize("dt", DTYPES)
def test_clip(dt):
    ctx, rng, _ = _begin(dt, 20)
    cplx = dt == "c128"
    g = _rand(rng, cplx)
    r = opt_ref.norm([g])
    # no-op cases leave g bit-identical; the norm is reproducible
    for cv, cn in ((0.0, 0.0), (-1.0, -2.0), (0.0, 2.0 * r), (100.0, 0.0)):
        ctx.opt_set_gradient(g)
        n1 = ctx.opt_clip(cv, cn)
        n2 = ctx.opt_clip(cv, cn)
        assert n1 == n2 and abs(n1 - r) <= 1e-14 * r, (cv, cn, n1, r)
        assert np.array_equal(ctx.opt_get_gradient(), g), (cv, cn)
    amax = float(np.max(np.abs(g)))
    for cv, cn in ((0.8, 0.0), (0.0, r / 2), (0.8, r / 4), (0.8, 10 * r)):
        ctx.opt_set_gradient(g)
        nb = ctx.opt_clip(cv, cn)
        want = opt_ref.clip([g], cv, cn)[0]
        got = ctx.opt_get_gradient()
        err = float(np.max(np.abs(got - want)))
        print("%s clip (%g, %g): norm before %.15e (numpy %.15e), max |g - ref| = %.3e" % (dt, cv, cn, nb, r, err))
        assert abs(nb - r) <= 1e-14 * r
        # one division and one product per element (plus the 1e-14 of the norm in the global scale factor)
        assert err <= (4 * EPS + 2e-14) * amax
        assert not np.array_equal(got, g) and np.all(got[_mask() == 0] == 0)
        if cv > 0:
            assert float(np.max(np.abs(got))) <= cv * (1 + 4 * EPS)


@pytest.fixture(scope="module")
def tfim(fixtures_dir):
    """the reference's 2x2 transverse-field Ising state on a float64 context: exact-sum accumulation over all 16 configurations with
    the holes resident, the O* samples of the same 16 walkers in the SR store"""
    from peps_amd import capi, synthetic
    from peps_amd.capi import LEFT, RIGHT, UP, DOWN, HORIZONTAL
    s = qlten_io.load_sitps(os.path.join(fixtures_dir, "transverse_ising_tps_double_from_simple_update"))
    flat = synthetic.sitps_to_flat(s, 4)
    cfgs = np.array(vmc.generate_all_binary_configs(2, 2), dtype=np.int32)
    ctx = capi.Context(2, 2, 4, 2, 8, dtype=capi.F64, max_walkers=16)
    ctx.state_upload(flat)
    ctx.set_configs(cfgs)
    psi = ctx.evaluate_amplitude()
    ctx.set_configs(cfgs)
    ctx.generate_bmps_approach(UP)
    model = vmc.TransverseFieldIsingSquareOBC(1.0)
    eloc = np.array([model.CalDiagTermEnergy(c) for c in cfgs])
    for row in range(2):
        ctx.init_bten(LEFT, row)
        ctx.grow_full_bten(RIGHT, row, 1, True)
        p = ctx.trace(row, 0, HORIZONTAL)
        for col in range(2):
            ctx.punch_hole_store(row, col, HORIZONTAL)
            ex = ctx.replace_one_trace(row, col, HORIZONTAL, (1 - cfgs[:, row, col])[:, None])[:, 0]
            eloc += -1.0 * ex / p
            if col < 1:
                ctx.shift_bten_window(RIGHT)
        if row < 1:
            ctx.shift_bmps_window(DOWN)
    ctx.grad_reset()
    ctx.grad_accumulate(psi, eloc, exact_sum=True)
    ctx.sr_begin(16)
    ctx.sr_append(psi)
    w = psi ** 2
    yield ctx, flat, float(np.sum(w * eloc)), float(np.sum(w))
    ctx.close()


def test_gradient_from_accumulators_equals_the_host_finish(tfim):
    ctx, flat, e_sum, w_sum = tfim
    ctx.opt_begin()
    e, gnorm = ctx.opt_gradient_from_accumulators(e_sum, w_sum)
    so, seo = ctx.grad_read()
    e_ref, (g_ref,) = opt_ref.finish([so], [seo], e_sum, w_sum)
    g = ctx.opt_get_gradient()
    gmax = float(np.max(np.abs(g_ref)))
    print("E = %.14f, |E - ref| = %.3e, max |g - ref| = %.3e, max |g| = %.3e" % (e, abs(e - e_ref), float(np.max(np.abs(g - g_ref))), gmax))
    assert abs(e - (-5.19991995228)) < 1e-9              # the reference's own number for this state
    assert abs(e - e_ref) <= 1e-13
    assert float(np.max(np.abs(g - g_ref))) <= 1e-13 * gmax and gmax > 0
    assert abs(gnorm - opt_ref.norm([g_ref])) <= 1e-13 * gnorm


def test_natural_gradient_equals_the_host_vector_solve(tfim):
    """the same loop on the same HBM vectors: 1e-12 |x| is a cap, not an expected error"""
    ctx, flat, e_sum, w_sum = tfim
    ctx.opt_begin()
    ctx.opt_gradient_from_accumulators(e_sum, w_sum)
    g = ctx.opt_get_gradient()
    x, res, it, why = ctx.sr_cg_solve(g, None, 1e-3, 32, 1e-5, 0.0, 20, 0.5)
    res_d, it_d, why_d, nrm = ctx.opt_natural_gradient(1e-3, 32, 1e-5, 0.0, 20, 0.5)
    xd = ctx.opt_get_gradient()
    xn = float(np.linalg.norm(x.ravel()))
    print("iterations %d / %d, reason %d / %d, |x_dev - x_host| = %.3e, |x| = %.3e" % (it_d, it, why_d, why, float(np.linalg.norm((xd - x).ravel())), xn))
    assert (it_d, why_d) == (it, why) and it > 0
    assert float(np.linalg.norm((xd - x).ravel())) <= 1e-12 * xn
    assert abs(res_d - res) <= 1e-12 * max(res, 1e-300) + 1e-300 and abs(nrm - xn) <= 1e-12 * xn


@pytest.mark.parametrize("dt", DTYPES)
def test_refusals_leave_everything_untouched(dt):
    from peps_amd import capi
    ctx = capi.Context(L, L, D, DP, CHI, dtype={"f64": capi.F64, "f32": capi.F32, "c128": capi.C128}[dt], max_walkers=4)
    rng = np.random.default_rng(30)
    cplx = dt == "c128"
    theta, g = _rand(rng, cplx), _rand(rng, cplx)
    adam = (0.9, 0.999, 1e-8, 0.0)
    # PEPSGPU_ESTATE: no state yet, then every call before opt_begin
    with pytest.raises(RuntimeError):
        ctx.opt_begin()
    ctx.state_upload(theta)
    for call in (lambda: ctx.opt_step(2, 0.01, adam), lambda: ctx.opt_set_gradient(g), ctx.opt_get_gradient, ctx.opt_read_state,
                 lambda: ctx.opt_clip(1.0, 1.0), lambda: ctx.opt_scale_state(0.5), lambda: ctx.opt_gradient_from_accumulators(1.0, 1.0),
                 ctx.opt_natural_gradient):
        with pytest.raises(RuntimeError):
            call()
    ctx.opt_begin()
    if dt == "f32":
        theta = theta.astype(np.float32).astype(np.float64)
    with pytest.raises(RuntimeError):
        ctx.opt_natural_gradient()                        # empty sample store
    with pytest.raises(RuntimeError):
        ctx.opt_gradient_from_accumulators(1.0, 1.0)      # nothing accumulated
    ctx.grad_reset()
    for bad_w in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ctx.opt_gradient_from_accumulators(1.0, bad_w)
    ctx.opt_set_gradient(g)
    ctx.opt_step(2, 0.01, adam)                           # one good Adam step: the rule state is live for what follows
    st = opt_ref.RuleState([theta])
    want = opt_ref.adam([theta], [g], st, 0.01, *adam)
    before = ctx.opt_read_state()
    bad = [(2, float("nan"), adam), (2, float("inf"), adam), (2, -0.01, adam), (3, 0.01, adam), (-1, 0.01, adam), (2, 0.01, adam[:3]),
           (0, 0.01, adam), (1, 0.01, (1e-8,)), (2, 0.01, (1.0, 0.999, 1e-8, 0.0)), (2, 0.01, (0.9, -0.1, 1e-8, 0.0)),
           (2, 0.01, (0.9, 1.5, 1e-8, 0.0))]
    for rule, lr, params in bad:
        with pytest.raises(ValueError):
            ctx.opt_step(rule, lr, params)
    assert np.array_equal(ctx.opt_read_state(), before) and np.array_equal(ctx.opt_get_gradient(), g)
    # ... and a successful step on the same context continues the trajectory as if nothing had been refused (timestep 2, same moments)
    ctx.opt_step(2, 0.01, adam)
    want = opt_ref.adam(want, [g], st, 0.01, *adam)
    assert float(np.max(np.abs(ctx.opt_read_state() - want[0]))) <= 8 * EPS * float(np.max(np.abs(want[0])))
    ctx.opt_end()
    with pytest.raises(RuntimeError):
        ctx.opt_read_state()
    ctx.close()

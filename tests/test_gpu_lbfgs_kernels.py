"""L-BFGS on the device-resident optimizer buffers through the C ABI (pepsgpu_lbfgs_*, peps_amd/csrc/engine_lbfgs.h) against the NumPy
restatement tests/lbfgs_ref.py, on a diagonal quadratic f = 1/2 sum h |theta - t|^2 whose gradient is computed in NumPy from
pepsgpu_opt_read_state and set with pepsgpu_opt_set_gradient.  Shapes where the element-wise grid and the dots can go wrong:
2x3 with D = 3 (slot 81: less than one block, odd, every site has dimension-1 legs), 3x3 with D = 4 (slot exactly 256, one interior
site), 2x2 with D = 5 (slot 625: a partial last block, odd); float64, float32 and complex contexts each.
Element-wise results are held to 8 eps max|ref| (single roundings; the restatement is driven by the device's own state and direction,
so nothing compounds); directions and scalars to lbfgs_ref.COEF_GATE, the gate of the CPU test for the coefficient-space recursion.
Padding: every array read back is zero outside the tensor elements; the tail of a slot beyond a site's live elements does not come back
through the ABI, but the dots run over it, so a value there would show in the norms and slopes compared here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_ref as L  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
DP, CHI = 2, 8
SHAPES = {"2x3D3": (2, 3, 3), "3x3D4": (3, 3, 4), "2x2D5": (2, 2, 5)}
DTYPES = ["f64", "f32", "c128"]


def _mask(rows, cols, bond):
    m = np.zeros((rows, cols, DP, bond, bond, bond, bond))
    for r in range(rows):
        for c in range(cols):
            m[r, c, :, :(1 if c == 0 else bond), :(1 if r == rows - 1 else bond), :(1 if c == cols - 1 else bond), :(1 if r == 0 else bond)] = 1.0
    return m


_CTX = {}


def _ctx(shape, dt):
    from peps_amd import capi
    if (shape, dt) not in _CTX:
        rows, cols, bond = SHAPES[shape]
        _CTX[(shape, dt)] = capi.Context(rows, cols, bond, DP, CHI, dtype={"f64": capi.F64, "f32": capi.F32, "c128": capi.C128}[dt], max_walkers=4)
    return _CTX[(shape, dt)]


class Problem:
    """a fresh random state uploaded and adopted, the quadratic, and the restatement's state"""

    def __init__(self, shape, dt, seed, history=2):
        self.rng = np.random.default_rng(seed)
        self.ctx, self.cplx = _ctx(shape, dt), dt == "c128"
        self.mask = _mask(*SHAPES[shape])
        self.h = (0.5 + 1.5 * self.rng.random(self.mask.shape)) * self.mask
        self.t = self.rand()
        self.ctx.state_upload(self.rand())
        self.ctx.opt_begin()
        self.ctx.lbfgs_begin(history)
        self.st = L.State()

    def rand(self, scale=1.0):
        x = self.rng.standard_normal(self.mask.shape)
        if self.cplx:
            x = x + 1j * self.rng.standard_normal(self.mask.shape)
        return scale * x * self.mask

    def gradient(self, theta):
        return self.h * (theta - self.t)

    def evaluate(self):
        """theta from the device, its gradient to the device"""
        theta = self.ctx.opt_read_state()
        g = self.gradient(theta)
        self.ctx.opt_set_gradient(g)
        return theta, g


def _norm(x):
    return float(np.sqrt(L.real_inner([x], [x])))


def _check_direction(pb, g, p, label):
    """pepsgpu_lbfgs_direction against the sequential two-loop recursion of the restatement on the same history"""
    dphi0, nrm, reset = pb.ctx.lbfgs_direction(p.min_curvature, p.max_direction_norm)
    d_ref, dphi0_ref, reset_ref = L.search_direction(pb.st, [g], p)
    d = pb.ctx.lbfgs_get_direction()
    dev = _norm(d - d_ref[0]) / _norm(d_ref[0])
    print("%s: |d - ref| / |ref| = %.3e, dphi0 %.15e (ref %.15e), |d| %.15e" % (label, dev, dphi0, dphi0_ref, nrm))
    assert reset == reset_ref
    assert dev <= L.COEF_GATE
    assert abs(dphi0 - dphi0_ref) <= L.COEF_GATE * _norm(g) * _norm(d_ref[0])
    assert abs(nrm - _norm(d_ref[0])) <= L.COEF_GATE * _norm(d_ref[0])
    assert np.all(d[pb.mask == 0] == 0)
    return d, dphi0, nrm


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_updates_directions_and_ring_follow_the_restatement(shape, dt):
    """six iterations with history_size 2: five updates, so the ring evicts three times"""
    pb = Problem(shape, dt, 11)
    ctx = pb.ctx
    p = L.LBFGSParams(history_size=2)
    for it in range(6):
        theta, g = pb.evaluate()
        oc, cv = ctx.lbfgs_update(p.min_curvature, p.use_damping)
        oc_ref, cv_ref = L.update_history(pb.st, [theta], [g], p)
        assert oc == oc_ref == (L.NONE if it == 0 else L.PUSHED)
        if it:
            s, y = pb.st.history[-1][:2]
            assert abs(cv - cv_ref) <= L.COEF_GATE * _norm(s[0]) * _norm(y[0])
        d, dphi0, nrm = _check_direction(pb, g, p, "%s %s iteration %d" % (shape, dt, it))
        assert dphi0 < 0
        # the same call on the same buffers gives the same bytes
        again = ctx.lbfgs_direction(p.min_curvature, p.max_direction_norm)
        assert again == (dphi0, nrm, False) and np.array_equal(ctx.lbfgs_get_direction(), d)
        slope = ctx.lbfgs_slope()
        assert slope == ctx.lbfgs_slope() and abs(slope - dphi0) <= L.COEF_GATE * _norm(g) * nrm
        alpha = (0.3, 1.0, 0.7, 0.45, 1.0, 0.2)[it]
        ctx.lbfgs_trial(alpha)
        want = L.trial_point([theta], [d], alpha)[0]
        got = ctx.opt_read_state()
        assert float(np.max(np.abs(got - want))) <= 8 * EPS * float(np.max(np.abs(want)))
        assert np.all(got[pb.mask == 0] == 0)
        assert np.array_equal(ctx.opt_get_gradient(), g)           # a trial does not touch g
        ctx.lbfgs_commit()
        pb.st.anchor_theta, pb.st.anchor_g = [theta], [g]
    assert ctx.lbfgs_counters() == {"skip_curvature": 0, "damping": 0, "descent_reset": 0, "history": 2}
    for i in range(2):
        s, y = ctx.lbfgs_get_pair(i)
        s_ref, y_ref = pb.st.history[i][0][0], pb.st.history[i][1][0]
        assert float(np.max(np.abs(s - s_ref))) <= 8 * EPS * float(np.max(np.abs(s_ref)))
        assert float(np.max(np.abs(y - y_ref))) <= 8 * EPS * float(np.max(np.abs(y_ref)))
        assert np.all(s[pb.mask == 0] == 0) and np.all(y[pb.mask == 0] == 0)
    with pytest.raises(IndexError):
        ctx.lbfgs_get_pair(2)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_trial_zero_restores_the_base_and_the_contractor_holds_the_trial_state(shape, dt):
    from peps_amd import capi
    pb = Problem(shape, dt, 12)
    ctx = pb.ctx
    rows, cols, bond = SHAPES[shape]
    theta, g = pb.evaluate()
    ctx.lbfgs_direction()
    ctx.lbfgs_trial(0.625)
    moved = ctx.opt_read_state()
    assert not np.array_equal(moved, theta)
    # the device state is T(theta): the same amplitudes as a fresh context given theta
    cfgs = np.random.default_rng(3).integers(0, DP, size=(4, rows, cols)).astype(np.int32)
    ctx.set_configs(cfgs)
    a = ctx.evaluate_amplitude()
    fresh = capi.Context(rows, cols, bond, DP, CHI, dtype={"f64": capi.F64, "f32": capi.F32, "c128": capi.C128}[dt], max_walkers=4)
    fresh.state_upload(moved)
    fresh.set_configs(cfgs)
    b = fresh.evaluate_amplitude()
    fresh.close()
    assert np.all(np.isfinite(a)) and np.all(a != 0) and np.array_equal(a, b)
    ctx.lbfgs_trial(0.0)
    back = ctx.opt_read_state()
    assert back.tobytes() == theta.tobytes()                        # bit for bit


@pytest.mark.parametrize("dt", ["f64", "c128"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_damping_skip_descent_reset_and_norm_cap(shape, dt):
    """each branch forced by a constructed (s, y) far from its threshold: <s,y> = -1/2 against min_curvature 1e-3"""
    pb = Problem(shape, dt, 13)
    ctx = pb.ctx
    p = L.LBFGSParams(history_size=2, min_curvature=1e-3)

    def anchor_and_step(alpha):
        theta, g = pb.evaluate()
        ctx.lbfgs_direction(p.min_curvature, p.max_direction_norm)
        d = ctx.lbfgs_get_direction()
        ctx.lbfgs_trial(alpha)
        ctx.lbfgs_commit()
        pb.st.anchor_theta, pb.st.anchor_g = [theta], [g]
        theta1 = ctx.opt_read_state()
        return theta, g, d, theta1

    # skip: y = -s / (2 |s|^2) without damping
    theta, g, d, theta1 = anchor_and_step(0.5)
    s = theta1 - theta
    y = -0.5 * s / L.real_inner([s], [s])
    g1 = g + y
    ctx.opt_set_gradient(g1)
    no_damp = p.replace(use_damping=False)
    oc, cv = ctx.lbfgs_update(no_damp.min_curvature, False)
    oc_ref, cv_ref = L.update_history(pb.st, [theta1], [g1], no_damp)
    assert oc == oc_ref == L.SKIPPED and abs(cv - cv_ref) <= L.COEF_GATE * _norm(s) * _norm(g1 - g) and abs(cv + 0.5) < 1e-12
    assert ctx.lbfgs_counters() == {"skip_curvature": 1, "damping": 0, "descent_reset": 0, "history": 0}
    # damping: the same pair with damping is lifted and pushed
    oc, cv = ctx.lbfgs_update(p.min_curvature, True)
    oc_ref, cv_ref = L.update_history(pb.st, [theta1], [g1], p)
    assert oc == oc_ref == L.PUSHED_DAMPED and cv > p.min_curvature
    assert abs(cv - cv_ref) <= L.COEF_GATE * _norm(s) * _norm(pb.st.history[-1][1][0])
    s_dev, y_dev = ctx.lbfgs_get_pair(0)
    y_ref = pb.st.history[-1][1][0]
    assert float(np.max(np.abs(y_dev - y_ref))) <= 8 * EPS * float(np.max(np.abs(y_ref)))
    assert float(np.max(np.abs(s_dev - s))) <= 8 * EPS * float(np.max(np.abs(s)))
    assert ctx.lbfgs_counters() == {"skip_curvature": 1, "damping": 1, "descent_reset": 0, "history": 1}
    # the direction through the damped pair, then the norm cap at a quarter of its length
    d, dphi0, nrm = _check_direction(pb, g1, p, "%s %s damped pair" % (shape, dt))
    capped = p.replace(max_direction_norm=0.25 * nrm)
    d_c, dphi0_c, nrm_c = _check_direction(pb, g1, capped, "%s %s capped" % (shape, dt))
    assert abs(nrm_c - 0.25 * nrm) <= L.COEF_GATE * nrm
    # descent reset: a pair with y = -s pushed under a threshold of -1e9, gradient s: <g, d> >= 0
    ctx.lbfgs_reset()
    pb.st.reset()
    loose = p.replace(min_curvature=-1e9)
    theta, g, d, theta1 = anchor_and_step(0.5)
    s = theta1 - theta
    g1 = g - s
    ctx.opt_set_gradient(g1)
    oc, cv = ctx.lbfgs_update(loose.min_curvature, True)
    oc_ref, cv_ref = L.update_history(pb.st, [theta1], [g1], loose)
    assert oc == oc_ref == L.PUSHED and cv < 0
    ctx.opt_set_gradient(s)
    dphi0, nrm, reset = ctx.lbfgs_direction(loose.min_curvature, loose.max_direction_norm)
    d_ref, dphi0_ref, reset_ref = L.search_direction(pb.st, [s], loose)
    assert reset and reset_ref
    assert np.array_equal(ctx.lbfgs_get_direction(), -s)
    assert abs(dphi0 - dphi0_ref) <= L.COEF_GATE * abs(dphi0_ref) and abs(nrm - _norm(s)) <= L.COEF_GATE * nrm
    assert ctx.lbfgs_counters() == {"skip_curvature": 0, "damping": 0, "descent_reset": 1, "history": 0}
    ctx.lbfgs_trial(0.0)
    assert ctx.lbfgs_update(p.min_curvature, True) == (L.NONE, 0.0)          # the anchor went with the history


def test_refusals_leave_everything_untouched():
    from peps_amd import capi
    shape = "2x3D3"
    rows, cols, bond = SHAPES[shape]
    mask = _mask(rows, cols, bond)
    rng = np.random.default_rng(5)
    ctx = capi.Context(rows, cols, bond, DP, CHI, dtype=capi.F64, max_walkers=4)
    theta = rng.standard_normal(mask.shape) * mask
    ctx.state_upload(theta)
    with pytest.raises(RuntimeError):
        ctx.lbfgs_begin(2)                                   # before opt_begin
    ctx.opt_begin()
    g = rng.standard_normal(mask.shape) * mask
    ctx.opt_set_gradient(g)
    for call in (lambda: ctx.lbfgs_update(), lambda: ctx.lbfgs_direction(), lambda: ctx.lbfgs_trial(0.1), lambda: ctx.lbfgs_slope(),
                 lambda: ctx.lbfgs_commit(), lambda: ctx.lbfgs_reset(), lambda: ctx.lbfgs_get_direction(), lambda: ctx.lbfgs_counters()):
        with pytest.raises(RuntimeError):
            call()                                           # before lbfgs_begin
    for bad in (0, 33, -1):
        with pytest.raises(ValueError):
            ctx.lbfgs_begin(bad)
    ctx.lbfgs_begin(32)
    ctx.lbfgs_begin(2)
    for call in (lambda: ctx.lbfgs_slope(), lambda: ctx.lbfgs_trial(0.1), lambda: ctx.lbfgs_commit()):
        with pytest.raises(RuntimeError):
            call()                                           # no direction yet
    # one pair in the history, a direction pending
    ctx.lbfgs_direction()
    ctx.lbfgs_trial(0.5)
    ctx.lbfgs_commit()
    theta1 = ctx.opt_read_state()
    g1 = g + 0.5 * (theta1 - theta)
    ctx.opt_set_gradient(g1)
    assert ctx.lbfgs_update()[0] == L.PUSHED
    ctx.lbfgs_direction()
    before = (ctx.opt_read_state(), ctx.opt_get_gradient(), ctx.lbfgs_get_direction(), ctx.lbfgs_get_pair(0), ctx.lbfgs_counters())
    for alpha in (float("nan"), -0.1, float("inf")):
        with pytest.raises(ValueError):
            ctx.lbfgs_trial(alpha)
    with pytest.raises(ValueError):
        ctx.lbfgs_update(float("nan"), True)
    with pytest.raises(ValueError):
        ctx.lbfgs_direction(float("nan"), 1.0)
    with pytest.raises(IndexError):
        ctx.lbfgs_get_pair(1)
    after = (ctx.opt_read_state(), ctx.opt_get_gradient(), ctx.lbfgs_get_direction(), ctx.lbfgs_get_pair(0), ctx.lbfgs_counters())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    assert np.array_equal(before[3][0], after[3][0]) and np.array_equal(before[3][1], after[3][1]) and before[4] == after[4]
    ctx.lbfgs_trial(0.25)                                    # the pending direction is still usable
    ctx.opt_end()                                            # frees the L-BFGS buffers with the optimizer's
    with pytest.raises(RuntimeError):
        ctx.lbfgs_counters()
    ctx.close()

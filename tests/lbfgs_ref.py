"""NumPy restatement of the reference's L-BFGS (optimizer/optimizer_impl.h) on lists of equally shaped arrays, like tests/opt_ref.py:

    update_history        UpdateLBFGSHistoryFromAnchor_        :1443-1486
    direction_sequential  ComputeLBFGSSearchDirection_         :1488-1532   (the reference's own two-loop recursion on vectors)
    direction_coefficient the same recursion on the coefficients of [s_1..s_m, y_1..y_m, g] from their inner products, then one
                          linear combination: what the device runs (peps_amd/csrc/engine_lbfgs.h)
    search_direction      either form plus the descent guard    :620-641
    strong_wolfe          StrongWolfeLBFGSStep_                 :1547-1662
    optimize              the L-BFGS schedule of IterativeOptimize (:244-249, 619-675, 847-857) with the closing evaluation and the
                          stopping test of this repository's Optimizer (peps_amd/host/qlpeps_gpu.h)

Inner products are RealInnerProduct_ (:1398-1401): Re<a, b>, the plain dot over real and imaginary parts.  Element-wise results
(s, y, the damped y, the trial point) use the operation order of the kernels, so that they differ from the device by the rounding of
single operations only."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
FIXED, STRONG_WOLFE = 0, 1
NONE, PUSHED, PUSHED_DAMPED, SKIPPED = 0, 1, 2, 3


class LBFGSParams:
    """the fourteen fields and defaults of LBFGSParams (optimizer_params.h:119-152)"""
    FIELDS = ("history_size", "tolerance_grad", "tolerance_change", "max_eval", "step_mode", "wolfe_c1", "wolfe_c2", "min_step",
              "max_step", "min_curvature", "use_damping", "max_direction_norm", "allow_fallback_to_fixed_step",
              "fallback_fixed_step_scale")

    def __init__(self, history_size=10, tolerance_grad=1e-5, tolerance_change=1e-9, max_eval=20, step_mode=FIXED, wolfe_c1=1e-4,
                 wolfe_c2=0.9, min_step=1e-8, max_step=1.0, min_curvature=1e-12, use_damping=True, max_direction_norm=1e3,
                 allow_fallback_to_fixed_step=False, fallback_fixed_step_scale=0.2):
        for k in self.FIELDS:
            setattr(self, k, locals()[k])

    def as_list(self):
        """the array the shim entries take"""
        return [float(getattr(self, k)) for k in self.FIELDS]

    def replace(self, **kw):
        d = {k: getattr(self, k) for k in self.FIELDS}
        d.update(kw)
        return LBFGSParams(**d)


def reference_setting(**kw):
    """CreateStrongWolfeLBFGSParams of test_optimizer_lbfgs_exact_sum.cpp:32-52"""
    d = dict(history_size=10, tolerance_grad=1e-8, tolerance_change=1e-10, max_eval=128, step_mode=STRONG_WOLFE, wolfe_c1=1e-4,
             wolfe_c2=0.99, min_step=1e-8, max_step=1.0)
    d.update(kw)
    return LBFGSParams(**d)


# stopping criteria of the reference's exact-sum tests (:49-51)
REFERENCE_STOP = dict(energy_tolerance=1e-12, gradient_tolerance=1e-6)
# the line search's zoom is exercised by A; zoom, bracket doubling and history eviction by B; FAIL ends at iteration 0 after two trials
SETTING_A = (reference_setting(wolfe_c2=0.1, history_size=5, max_step=64.0), 4.0)
SETTING_B = (reference_setting(wolfe_c2=0.5, history_size=3, max_step=16.0), 1.0)
SETTING_FAIL = (reference_setting(wolfe_c2=0.1, max_step=1.0), 0.5)
STEPS_A = [2, 0.28125, 1.25, 1, 2, 1, 1, 4]
STEPS_B = [2, 0.25, 1, 1, 1, 1, 1, 0.5]


# Largest relative deviation |d_coefficient - d_sequential| / |d_sequential| over every direction of the TFIM and Heisenberg runs with
# the reference setting and of the runs with settings A and B (tests/test_cpu_lbfgs_ref.py measures it again), and the gate every
# comparison of a direction or of a scalar derived from one uses: ten times that.
COEF_DEVIATION_MEASURED = 7.88e-16
COEF_GATE = 10.0 * COEF_DEVIATION_MEASURED
# Amplification of evaluator noise into the first eight energies of settings A and B: seeded relative noise of 1e-10 on every
# evaluated energy and gradient element (seeds 0..4, oracle_evaluator(noise=...)) moves them by at most 1.49e-9 = AMPLIFICATION * 1e-10 |E|
# (A: 2.04, B: 2.85) and changes none of the first nine step lengths.
AMPLIFICATION = 2.85


def real_inner(a, b):
    acc = 0.0
    for x, y in zip(a, b):
        acc += float(np.sum(x.real * y.real + x.imag * y.imag)) if np.iscomplexobj(x) or np.iscomplexobj(y) else float(np.sum(x * y))
    return acc


class State:
    """history [(s, y, rho, sy, yy)], oldest first; anchor; the three counters"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.history = []
        self.anchor_theta = self.anchor_g = None
        self.skip_curvature = self.damping = self.descent_reset = 0

    def drop(self):
        """the descent reset: history and anchor go, the counters stay (see engine_lbfgs.h)"""
        self.history = []
        self.anchor_theta = self.anchor_g = None


def update_history(st, theta, g, p):
    """returns (outcome, curvature)"""
    if st.anchor_theta is None:
        return NONE, 0.0
    if p.history_size == 0:
        raise ValueError("LBFGS history_size must be > 0")
    s = [a - b for a, b in zip(theta, st.anchor_theta)]
    y = [a - b for a, b in zip(g, st.anchor_g)]
    curvature = real_inner(s, y)
    yy = real_inner(y, y)
    damped = False
    if curvature <= p.min_curvature and p.use_damping and yy > EPS:
        c = (p.min_curvature - curvature + 1e-15) / yy
        y = [b + c * a for a, b in zip(s, y)]
        curvature = real_inner(s, y)
        yy = real_inner(y, y)
        st.damping += 1
        damped = True
    if curvature <= p.min_curvature:
        st.skip_curvature += 1
        return SKIPPED, curvature
    st.history.append((s, y, 1.0 / curvature, curvature, yy))
    while len(st.history) > p.history_size:
        st.history.pop(0)
    return (PUSHED_DAMPED if damped else PUSHED), curvature


def _gamma(st, p):
    _, _, _, sy, yy = st.history[-1]
    return sy / yy if (yy > EPS and sy > p.min_curvature) else 1.0


def _cap(d, p):
    if p.max_direction_norm > 0.0:
        nrm = np.sqrt(real_inner(d, d))
        if nrm > p.max_direction_norm and nrm > 0.0:
            d = [x * (p.max_direction_norm / nrm) for x in d]
    return d


def direction_sequential(st, g, p):
    d = [-1.0 * x for x in g]
    if st.history:
        q = [np.array(x) for x in g]
        alpha = [0.0] * len(st.history)
        for i in range(len(st.history) - 1, -1, -1):
            s, y, rho = st.history[i][:3]
            alpha[i] = rho * real_inner(s, q)
            q = [a + (-alpha[i]) * b for a, b in zip(q, y)]
        gamma = _gamma(st, p)
        r = [gamma * x for x in q]
        for i in range(len(st.history)):
            s, y, rho = st.history[i][:3]
            beta = rho * real_inner(y, r)
            r = [a + (alpha[i] - beta) * b for a, b in zip(r, s)]
        d = [-1.0 * x for x in r]
    return _cap(d, p)


def direction_coefficient(st, g, p):
    m = len(st.history)
    if m == 0:
        return _cap([-(1.0 * x) for x in g], p)
    basis = [h[0] for h in st.history] + [h[1] for h in st.history]
    gram = np.array([[real_inner(a, b) for b in basis] for a in basis])
    bg = np.array([real_inner(a, g) for a in basis])

    def dot(a, c, cg):
        acc = 0.0
        for j in range(2 * m):
            acc += c[j] * gram[a, j]
        return acc + cg * bg[a]

    c, cg, alpha = [0.0] * (2 * m), 1.0, [0.0] * m
    for i in range(m - 1, -1, -1):
        alpha[i] = st.history[i][2] * dot(i, c, cg)
        c[m + i] += -alpha[i]
    gamma = _gamma(st, p)
    c = [x * gamma for x in c]
    cg *= gamma
    for i in range(m):
        beta = st.history[i][2] * dot(m + i, c, cg)
        c[i] += alpha[i] - beta
    d = []
    for k, x in enumerate(g):
        t = cg * x
        for j in range(2 * m):
            t = t + c[j] * basis[j][k]
        d.append(-t)
    return _cap(d, p)


def search_direction(st, g, p, form=direction_sequential):
    """(d, dphi0, was_reset): the direction, then the descent guard"""
    d = form(st, g, p)
    dphi0 = real_inner(g, d)
    if dphi0 >= 0.0:
        st.descent_reset += 1
        st.drop()
        d = [-(1.0 * x) for x in g]
        return d, real_inner(g, d), True
    return d, dphi0, False


def trial_point(theta_base, d, alpha):
    return [np.array(t) if alpha == 0.0 else t + alpha * x for t, x in zip(theta_base, d)]


def strong_wolfe(eval_alpha, learning_rate, p, phi0, dphi0):
    """eval_alpha(alpha) -> (phi, dphi).  Returns (alpha or None when the search fails, evaluations, zoom entries, doublings)"""
    if p.wolfe_c1 <= 0.0 or p.wolfe_c1 >= 1.0 or p.wolfe_c2 <= p.wolfe_c1 or p.wolfe_c2 >= 1.0:
        raise ValueError("LBFGS strong-Wolfe parameters must satisfy 0 < c1 < c2 < 1")
    if p.max_eval == 0:
        raise ValueError("LBFGS max_eval must be > 0 for strong-Wolfe mode")
    if p.tolerance_grad < 0.0:
        raise ValueError("LBFGS tolerance_grad must be >= 0 for strong-Wolfe mode")
    if dphi0 >= 0.0:
        return None, 0, 0, 0
    threshold = max(-p.wolfe_c2 * dphi0, p.tolerance_grad)
    n = [0]

    def ev(alpha):
        n[0] += 1
        return eval_alpha(alpha)

    def zoom(alo, phi_alo, ahi):
        while n[0] < p.max_eval:
            alpha = 0.5 * (alo + ahi)
            phi, dphi = ev(alpha)
            if phi > phi0 + p.wolfe_c1 * alpha * dphi0 or phi >= phi_alo:
                ahi = alpha
            else:
                if abs(dphi) <= threshold:
                    return alpha
                if dphi * (ahi - alo) >= 0.0:
                    ahi = alo
                alo, phi_alo = alpha, phi
            if abs(ahi - alo) <= p.tolerance_change:
                break
        return None

    alpha_prev, phi_prev = 0.0, phi0
    alpha = min(max(max(learning_rate, p.min_step), p.min_step), p.max_step)
    if alpha <= 0.0:
        alpha = p.min_step
    outer = doublings = 0
    while n[0] < p.max_eval:
        phi, dphi = ev(alpha)
        if phi > phi0 + p.wolfe_c1 * alpha * dphi0 or (outer > 0 and phi >= phi_prev):
            return zoom(alpha_prev, phi_prev, alpha), n[0], 1, doublings
        if abs(dphi) <= threshold:
            return alpha, n[0], 0, doublings
        if dphi >= 0.0:
            return zoom(alpha, phi, alpha_prev), n[0], 1, doublings
        alpha_prev, phi_prev = alpha, phi
        nxt = min(alpha * 2.0, p.max_step)
        if nxt - alpha <= p.tolerance_change:
            break
        alpha = nxt
        doublings += 1
        outer += 1
    return None, n[0], 0, doublings


class LineSearchFailed(RuntimeError):
    pass


def optimize(evaluate, theta0, p, lr, iterations, energy_tolerance=0.0, gradient_tolerance=0.0, plateau_patience=0,
             form=direction_sequential, on_direction=None):
    """evaluate(theta) -> (energy, gradient list).  Returns a dict: energies, grad_norms, steps, theta, the three counters,
    line_search_evaluations, zoom_entries, doublings, converged.  on_direction(state, g) is called before every direction is computed
    (for comparisons of the two forms).  A failed search raises LineSearchFailed with .theta = the base."""
    if p.history_size == 0:
        raise ValueError("LBFGS history_size must be > 0")
    patience = plateau_patience if plateau_patience > 0 else iterations + 1
    st = State()
    theta = [np.array(x) for x in theta0]
    out = dict(energies=[], grad_norms=[], steps=[], line_search_evaluations=0, zoom_entries=0, doublings=0, converged=False)
    previous, lowest, stale = 0.0, np.inf, 0

    def finish():
        out.update(theta=theta, skip_curvature=st.skip_curvature, damping=st.damping, descent_reset=st.descent_reset,
                   history=len(st.history))
        return out

    for it in range(iterations):
        e, g = evaluate(theta)
        e = float(np.real(e))
        gn = float(np.sqrt(real_inner(g, g)))
        out["energies"].append(e)
        out["grad_norms"].append(gn)
        if e < lowest:
            lowest, stale = e, 0
        else:
            stale += 1
        update_history(st, theta, g, p)
        if it > 0 and (gn < gradient_tolerance or abs(e - previous) < energy_tolerance or stale >= patience):
            out["converged"] = True
            return finish()
        if on_direction is not None:
            on_direction(st, g)
        d, dphi0, _ = search_direction(st, g, p, form)
        base = theta
        if p.step_mode == FIXED:
            used = max(0.0, lr)
        else:
            def eval_alpha(alpha):
                et, gt = evaluate(trial_point(base, d, alpha))
                return float(np.real(et)), real_inner(gt, d)
            alpha, n, z, dbl = strong_wolfe(eval_alpha, lr, p, e, dphi0)
            out["line_search_evaluations"] += n
            out["zoom_entries"] += z
            out["doublings"] += dbl
            if alpha is not None:
                used = alpha
            elif p.allow_fallback_to_fixed_step:
                used = max(0.0, max(p.min_step, lr * p.fallback_fixed_step_scale))
            else:
                err = LineSearchFailed("L-BFGS strong-Wolfe line search failed at iteration %d after %d trials" % (it, n))
                err.theta, err.trials, err.iteration = base, n, it
                raise err
        st.anchor_theta, st.anchor_g = base, g
        theta = trial_point(base, d, used)
        out["steps"].append(used)
        previous = e
    e, g = evaluate(theta)
    out["energies"].append(float(np.real(e)))
    out["grad_norms"].append(float(np.sqrt(real_inner(g, g))))
    return finish()


# ---- the restatement driven by the oracle's exact-sum evaluator on the reference's 2x2 fixtures ----
TFIM_E0 = -2.0 * (np.sqrt(2 - 2 * np.cos(np.pi / 4)) + np.sqrt(2 - 2 * np.cos(3 * np.pi / 4)))   # Calculate2x2OBCTransverseIsingEnergy(1, 1)
HEISENBERG_E0 = -2.0                                                                            # Calculate2x2HeisenbergEnergy(1)


def oracle_evaluator(sitps, model_name, noise=None):
    """(evaluate, theta0, nested): evaluate(theta) -> (E, gradient list) by oracle.vmc.exact_sum_energy_evaluator on the 2x2 lattice,
    SVD(1, 8, 1e-16); model "tfim" (16 binary configurations, h = 1) or "xxz" (the 6 configurations of two up spins, J = 1).  noise =
    (rng, rel): every energy and gradient element is multiplied by 1 + rel * N(0, 1)."""
    from oracle import vmc
    from oracle.bmps import BMPSTruncateParams
    rows, cols, d = len(sitps), len(sitps[0]), len(sitps[0][0])
    if model_name == "tfim":
        cfgs, model = vmc.generate_all_binary_configs(cols, rows), vmc.TransverseFieldIsingSquareOBC(1.0)
    else:
        cfgs, model = vmc.generate_all_permutation_configs([2, 2], cols, rows), vmc.SquareSpinOneHalfXXZModelOBC()
    tp = BMPSTruncateParams.SVD(1, 8, 1e-16)
    idx = [(r, c, s) for r in range(rows) for c in range(cols) for s in range(d)]

    def nested(flat):
        return [[[flat[(r * cols + c) * d + s] for s in range(d)] for c in range(cols)] for r in range(rows)]

    def evaluate(theta):
        e, grad, _ = vmc.exact_sum_energy_evaluator(nested(theta), cfgs, tp, model)
        g = [np.asarray(grad[r][c][s]) for r, c, s in idx]
        e = float(np.real(e))
        if noise is not None:
            rng, rel = noise
            e *= 1.0 + rel * rng.standard_normal()
            g = [x * (1.0 + rel * rng.standard_normal(x.shape)) for x in g]
        return e, g

    theta0 = [np.array(sitps[r][c][s], dtype=np.float64) for r, c, s in idx]
    return evaluate, theta0, nested

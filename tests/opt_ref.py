"""NumPy restatement of the optimisation step the device runs (peps_amd/csrc/engine_opt.h), on lists of per-site arrays (any
list of equally shaped ndarrays works: one padded state array in a list, or one array per (site, component)).

    finish   g = (S_EO - conj(E) S_O) / W                         exact_summation_energy_evaluator.h:286-295
    clip     element-wise, then global norm                       optimizer_impl.h:311-316, split_index_tps_impl.h:566-580
    sgd      decoupled decay, momentum, Nesterov                  optimizer_impl.h:949-990
    adagrad  acc += |g|^2, theta -= lr g inv(sqrt(acc))           optimizer_impl.h:1252-1307
    adam     bias-corrected moments, decoupled decay              optimizer_impl.h:1327-1396

inv(x) = qlten::ElementWiseInv(eps) is taken as 1 / (x + eps) in both rules.  The order of the floating-point operations is the one
of the kernels, so that the two differ by the rounding of single operations only.  The schedulers restate lr_schedulers.h:40-103."""
import numpy as np


def abs2(x):
    return x.real * x.real + x.imag * x.imag if np.iscomplexobj(x) else x * x


def norm(g):
    return float(np.sqrt(sum(float(np.sum(abs2(x))) for x in g)))


def finish(so, seo, e_loc_sum, weight_sum):
    energy = e_loc_sum / weight_sum
    return energy, [(b - np.conj(energy) * a) / weight_sum for a, b in zip(so, seo)]


def clip(g, clip_value=0.0, clip_norm=0.0):
    """ElementWiseClipTo, then ClipByGlobalNorm; a bound <= 0 is off"""
    g = [np.array(x) for x in g]
    if clip_value > 0.0:
        for x in g:
            if np.iscomplexobj(x):
                a = np.abs(x)
                big = a > clip_value
                x[big] = x[big] * (clip_value / a[big])
            else:
                big = np.abs(x) > clip_value
                x[big] = np.copysign(clip_value, x[big])
    if clip_norm > 0.0:
        r = norm(g)
        if r > 0.0 and r > clip_norm:
            g = [x * (clip_norm / r) for x in g]
    return g


class RuleState:
    """velocity, m1 (element type), m2, acc (real), Adam timestep: cleared at `begin`"""

    def __init__(self, like):
        self.velocity = [np.zeros_like(x) for x in like]
        self.m1 = [np.zeros_like(x) for x in like]
        self.m2 = [np.zeros(x.shape) for x in like]
        self.acc = None
        self.t = 0


def sgd(theta, g, st, lr, momentum=0.0, nesterov=False, weight_decay=0.0):
    out = []
    for i, (th, gi) in enumerate(zip(theta, g)):
        if weight_decay > 0.0:
            th = th * (1.0 - lr * weight_decay)
        upd = gi
        if momentum > 0.0:
            st.velocity[i] = momentum * st.velocity[i] + gi
            upd = momentum * st.velocity[i] + gi if nesterov else st.velocity[i]
        out.append(th + (-lr) * upd)
    return out


def adagrad(theta, g, st, lr, epsilon, initial_accumulator_value=0.0, mask=None):
    """mask (optional, per array): where the accumulator starts at initial_accumulator_value (the tensor elements; the padding of a
    padded array starts at zero and its gradient is zero)"""
    if st.acc is None:
        st.acc = [np.full(x.shape, float(initial_accumulator_value)) * (1.0 if mask is None else mask[i]) for i, x in enumerate(theta)]
    out = []
    for i, (th, gi) in enumerate(zip(theta, g)):
        st.acc[i] = st.acc[i] + abs2(gi)
        rate = 1.0 / (np.sqrt(st.acc[i]) + epsilon)
        out.append(th + -((rate * gi) * lr))
    return out


def adam(theta, g, st, lr, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.0):
    st.t += 1
    inv_bc1 = 1.0 / (1.0 - beta1 ** st.t)
    inv_bc2 = 1.0 / (1.0 - beta2 ** st.t)
    out = []
    for i, (th, gi) in enumerate(zip(theta, g)):
        if weight_decay > 0.0:
            th = th * (1.0 - lr * weight_decay)
        st.m2[i] = beta2 * st.m2[i] + (1.0 - beta2) * abs2(gi)
        den = 1.0 / (np.sqrt(inv_bc2 * st.m2[i]) + epsilon)
        st.m1[i] = beta1 * st.m1[i] + (1.0 - beta1) * gi
        out.append(th + -((den * (inv_bc1 * st.m1[i])) * lr))
    return out


RULES = {"sgd": 0, "adagrad": 1, "adam": 2}


def step(rule, theta, g, st, lr, params, mask=None):
    """the rule by the id and parameter list of pepsgpu_opt_step"""
    if rule == 0:
        return sgd(theta, g, st, lr, params[0], bool(params[1]), params[2])
    if rule == 1:
        return adagrad(theta, g, st, lr, params[0], params[1], mask)
    return adam(theta, g, st, lr, *params)


# lr_schedulers.h:40-103
def constant_lr(lr, iteration):
    return lr


def exponential_decay_lr(initial_lr, decay_rate, decay_steps, iteration):
    return initial_lr * decay_rate ** (iteration / float(decay_steps))


def step_lr(initial_lr, step_size, gamma, iteration):
    return initial_lr * gamma ** (iteration // step_size)


# ---- the restatement driven by the oracle's exact-sum evaluator (the trajectory the device optimizer is compared with) ----
# the five rule settings of the convergence checks: (name, rule, lr, parameters of pepsgpu_opt_step)
SETTINGS = [
    ("adam", 2, 0.02, (0.9, 0.999, 1e-8, 0.0)),
    ("adagrad", 1, 0.1, (1e-8, 0.0)),
    ("sgd_momentum", 0, 0.05, (0.9, 0.0, 0.0)),
    ("sgd_nesterov", 0, 0.05, (0.9, 1.0, 0.0)),
    ("sgd_plain", 0, 0.2, (0.0, 0.0, 0.0)),
]
TFIM_E0 = -2.0 * (np.sqrt(2 - 2 * np.cos(np.pi / 4)) + np.sqrt(2 - 2 * np.cos(3 * np.pi / 4)))   # test_optimizer_adam_exact_sum.cpp


def oracle_tfim_trajectory(sitps, rule, lr, params, iterations, clip_value=0.0, clip_norm=0.0):
    """evaluate -> clip -> step on the 2x2 transverse-field Ising state, all 16 binary configurations, SVD(1, 8, 1e-16):
    returns (energies[iterations + 1], gradient norms[iterations + 1], final state in the shape of `sitps`)"""
    from oracle import vmc
    from oracle.bmps import BMPSTruncateParams
    rows, cols, d = len(sitps), len(sitps[0]), len(sitps[0][0])
    cfgs = vmc.generate_all_binary_configs(cols, rows)
    tp = BMPSTruncateParams.SVD(1, 8, 1e-16)
    model = vmc.TransverseFieldIsingSquareOBC(1.0)
    idx = [(r, c, s) for r in range(rows) for c in range(cols) for s in range(d)]

    def nested(flat):
        return [[[flat[(r * cols + c) * d + s] for s in range(d)] for c in range(cols)] for r in range(rows)]

    theta = [np.array(sitps[r][c][s], dtype=np.float64) for r, c, s in idx]
    st = RuleState(theta)
    energies, norms = [], []
    for it in range(iterations + 1):
        e, grad, _ = vmc.exact_sum_energy_evaluator(nested(theta), cfgs, tp, model)
        g = [np.asarray(grad[r][c][s]) for r, c, s in idx]
        energies.append(float(np.real(e)))
        norms.append(norm(g))
        if it == iterations:
            break
        theta = step(rule, theta, clip(g, clip_value, clip_norm), st, lr, params)
    return np.array(energies), np.array(norms), nested(theta)

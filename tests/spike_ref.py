"""Plain-Python restatement of the reference's spike recovery and step-selector rules, written from its text (file:line below refer to
include/qlpeps/optimizer/ of the reference): the tracker, the four signals, the decision, the event log, the accepted-trajectory
bookkeeping of IterativeOptimize and the two selection rules.  Everything is double arithmetic in the reference's order of
operations, so the C++ host layer must agree to rounding of a possibly contracted multiply-add (1e-14 relative) and, where only
comparisons are involved, exactly."""
import math

SPIKE_DEFAULTS = dict(enable_auto_recover=True, redo_mc_max_retries=2, factor_err=100.0, factor_grad=1e10, factor_ngrad=10.0,
                      sr_min_iters_suspicious=1, enable_rollback=False, ema_window=50, sigma_k=10.0)      # optimizer_params.h:299-313
SIZE_MAX = 2 ** 64 - 1
K_SELECTOR_LATE_SIGMA = 1.0                                                                                # optimizer_impl.h:147


class EMA:
    """spike_detection.h:80-114"""

    def __init__(self, window=50):
        self.alpha = 2.0 / (float(window) + 1.0)
        self.reset()

    def reset(self):
        self.mean, self.var, self.initialized = 0.0, 0.0, False

    def update(self, x):
        if not self.initialized:
            self.mean, self.var, self.initialized = x, 0.0, True
            return
        delta = x - self.mean
        self.mean += self.alpha * delta
        self.var = (1.0 - self.alpha) * (self.var + self.alpha * delta * delta)

    @property
    def std(self):
        return math.sqrt(self.var)


def ema_series(series, window):
    t, out = EMA(window), []
    for x in series:
        t.update(x)
        out.append((t.mean, t.var))
    return out


class Guard:
    """the detection state of Optimizer: four trackers, has_prev_state_, the event log and its counters"""

    def __init__(self, **cfg):
        self.cfg = dict(SPIKE_DEFAULTS)
        self.cfg.update(cfg)
        w = self.cfg["ema_window"]
        self.energy, self.error, self.grad, self.ngrad = EMA(w), EMA(w), EMA(w), EMA(w)
        self.has_base = False
        self.events = []
        self.resamples = self.rollbacks = self.forced = 0

    def s1s2(self, error, grad_norm):                       # optimizer_impl.h:1871-1887
        c = self.cfg
        if self.error.initialized and self.error.mean > 0.0 and error > c["factor_err"] * self.error.mean:
            return "S1_ERRORBAR"
        if self.grad.initialized and self.grad.mean > 0.0 and grad_norm > c["factor_grad"] * self.grad.mean:
            return "S2_GRAD_NORM"
        return "NONE"

    def s3(self, ngrad_norm, sr_iters):                     # :1889-1905
        c = self.cfg
        if self.ngrad.initialized and self.ngrad.mean > 0.0 and ngrad_norm > c["factor_ngrad"] * self.ngrad.mean:
            return "S3_NGRAD_ANOMALY"
        if sr_iters <= c["sr_min_iters_suspicious"]:
            return "S3_NGRAD_ANOMALY"
        return "NONE"

    def s4(self, energy):                                   # :1907-1919
        if not self.energy.initialized:
            return "NONE"
        delta = energy - self.energy.mean
        if delta > 0.0 and self.energy.std > 0.0 and delta > self.cfg["sigma_k"] * self.energy.std:
            return "S4_ENERGY_SPIKE"
        return "NONE"

    def decide(self, signal, attempts, step):               # :1921-1944
        if signal == "NONE":
            return "ACCEPT"
        if signal == "S4_ENERGY_SPIKE":
            return "ROLLBACK"
        if attempts < self.cfg["redo_mc_max_retries"]:
            return "RESAMPLE"
        if self.cfg["enable_rollback"] and self.has_base and step > 0:
            return "ROLLBACK"
        return "ACCEPT_WARN"

    def log(self, step, attempt, signal, action, value, threshold):      # :1955-1973
        if action == "RESAMPLE":
            self.resamples += 1
        elif action == "ROLLBACK":
            self.rollbacks += 1
        elif action == "ACCEPT_WARN":
            self.forced += 1
        self.events.append(dict(step=step, attempt=attempt, signal=signal, action=action, value=value, threshold=threshold))


def replay(records, algo, **cfg):
    """IterativeOptimize's acceptance loop (:233-297, 683-774, 838-841) over scripted evaluations (energy, error, grad_norm, ngrad_norm,
    cg_iters): one record per evaluator call.  Returns (guard, actions per record, iteration per record, accepted record indices, the
    tracker values (mean, var) x 4 after every record)."""
    g = Guard(**cfg)
    c = g.cfg
    is_sr, is_minsr = algo == "sr", algo == "minsr"
    it, attempts = 0, 0
    actions, iters, accepted, ema = [], [], [], []
    for k, (energy, error, gnorm, ngnorm, cg) in enumerate(records):
        iters.append(it)
        verdict, warned = None, False

        def act(action):
            nonlocal attempts, verdict, warned
            if action == "RESAMPLE":
                attempts += 1
                verdict = action
            elif action == "ROLLBACK":
                g.has_base = False                          # (restoring consumes the saved state)
                attempts = 0
                verdict = action
            elif action == "ACCEPT_WARN":
                warned = True

        if c["enable_auto_recover"] and it > 0:             # B
            sig = g.s1s2(error, gnorm)
            if sig != "NONE":
                a = g.decide(sig, attempts, it)
                s1 = sig == "S1_ERRORBAR"
                g.log(it, attempts, sig, a, error if s1 else gnorm, c["factor_err"] * g.error.mean if s1 else c["factor_grad"] * g.grad.mean)
                act(a)
        if verdict is None and (is_sr or is_minsr) and c["enable_auto_recover"] and it > 0:      # D
            sig = g.s3(ngnorm, SIZE_MAX if is_minsr else int(cg))
            if sig != "NONE":
                a = g.decide(sig, attempts, it)
                g.log(it, attempts, sig, a, ngnorm, c["factor_ngrad"] * g.ngrad.mean)
                act(a)
        if verdict is None and c["enable_rollback"] and it > 0:                                   # D2
            if g.s4(energy) != "NONE":
                g.log(it, attempts, "S4_ENERGY_SPIKE", "ROLLBACK", energy, g.energy.mean + c["sigma_k"] * g.energy.std)
                act("ROLLBACK")
        if verdict is None:                                 # E, F
            g.energy.update(energy)
            g.error.update(error)
            g.grad.update(gnorm)
            if is_sr or is_minsr:
                g.ngrad.update(ngnorm)
            if c["enable_rollback"]:
                g.has_base = True
            accepted.append(k)
            verdict = "ACCEPT_WARN" if warned else "ACCEPT"
            it += 1
            attempts = 0
        actions.append(verdict)
        ema.append([(t.mean, t.var) for t in (g.energy, g.error, g.grad, g.ngrad)])
    return g, actions, iters, accepted, ema


def trigger_csv(events):
    """:1841-1856: header, then step,attempt,signal,action,value,threshold with the two doubles as %.6e"""
    out = "step,attempt,signal,action,value,threshold\n"
    for e in events:
        out += "%d,%d,%s,%s,%.6e,%.6e\n" % (e["step"], e["attempt"], e["signal"], e["action"], e["value"], e["threshold"])
    return out


def candidates(kind, base_lr, max_line_search_steps=3):     # :358-373
    if kind == "initial":
        return [base_lr * float(i) for i in range(1, max_line_search_steps + 1)]
    return [base_lr, base_lr * 0.5]


def select_initial(results):                                # :491-498: the first of equal energies
    sel, best = results[0][0], results[0][1]
    for eta, energy, _ in results:
        if energy < best:
            best, sel = energy, eta
    return sel


def select_periodic(results, it, max_iterations, ratio):    # :499-517
    (eta, e_eta, err_eta), (half, e_half, err_half) = results
    if float(it) < ratio * float(max_iterations):
        return half if e_half < e_eta else eta
    return half if (e_eta - e_half) > K_SELECTOR_LATE_SIGMA * max(err_eta, err_half) else eta


def next_base_lr(kind, base_lr, selected):                  # :534-538
    return selected if kind == "initial" else min(base_lr, selected)


def acceptance_flags(rates):                                # mc_energy_grad_evaluator.h:401-420, a walker in the role of a rank
    if not len(rates):
        return []
    mx = max(rates)
    return [w for w, r in enumerate(rates) if r < 0.5 * mx]

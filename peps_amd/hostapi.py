"""ctypes binding of libpepshost.so: the C++ host layer (peps_amd/host/qlpeps_gpu.h) that mirrors the
reference's updater / solver / evaluator surface on top of the pepsgpu C ABI."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpepshost.so")

SYMBOLS = ["pepshost_last_error", "pepshost_mc_sweeps", "pepshost_energy_and_holes", "pepshost_exact_sum_partial", "pepshost_exact_sum_measure_partial",
           "pepshost_mc_energy_grad_partial", "pepshost_exact_sum_finish", "pepshost_load_sitps", "pepshost_dump_sitps",
           "pepshost_dump_configuration", "pepshost_load_configuration", "pepshost_fermion_energy",
           "pepshost_fermion_exact_sum_partial", "pepshost_fermion_mc_sweeps", "pepshost_measure",
           "pepshost_set_truncate_params", "pepshost_set_device", "pepshost_get_device",
           "pepshost_energy_and_holes_c128", "pepshost_exact_sum_partial_c128", "pepshost_exact_sum_finish_c128",
           "pepshost_mc_energy_grad_partial_c128", "pepshost_mc_sweeps_c128", "pepshost_load_sitps_c128", "pepshost_dump_sitps_c128",
           "pepshost_mc_engine_warmup", "pepshost_mc_engine_warmup_dist", "pepshost_suwa_todo_chain", "pepshost_load_configuration2", "pepshost_configuration_from_text",
           "pepshost_fermion_measure_energy", "pepshost_fermion_energy_prm", "pepshost_fermion_measure_energy_prm", "pepshost_measure_c128", "pepshost_exact_sum_measure_partial_c128", "pepshost_fermion_energy_c128",
           "pepshost_fermion_exact_sum_partial_c128", "pepshost_fermion_mc_sweeps_c128", "pepshost_fermion_measure_energy_c128",
           "pepshost_fermion_mc_sweeps_updater", "pepshost_tnn3_table",
           "pepshost_optimize_exact_sum", "pepshost_optimize_exact_sum_c128", "pepshost_lr_schedule",
           "pepshost_sr_step_samples", "pepshost_sr_step_samples_c128",
           "pepshost_minsr_step_samples", "pepshost_minsr_step_samples_c128",
           "pepshost_fermion_optimize_exact_sum", "pepshost_fermion_optimize_exact_sum_c128",
           "pepshost_fermion_sr_step_samples", "pepshost_fermion_sr_step_samples_c128", "pepshost_fermion_exact_sum_partial_prm",
           "pepshost_lbfgs_exact_sum", "pepshost_lbfgs_exact_sum_c128", "pepshost_fermion_lbfgs_exact_sum", "pepshost_fermion_lbfgs_exact_sum_c128",
           "pepshost_fermion_observables", "pepshost_fermion_exact_sum_measure_partial", "pepshost_fermion_measure",
           "pepshost_fermion_measure_updater", "pepshost_hubbard_sector_table", "pepshost_hubbard_hop_table",
           "pepshost_fermion_observables_sc", "pepshost_fermion_exact_sum_measure_partial_sc", "pepshost_fermion_measure_sc",
           "pepshost_sc_pair_corr_mapping",
           "pepshost_vmc_optimize", "pepshost_vmc_optimize_c128", "pepshost_fermion_vmc_optimize", "pepshost_mc_evaluate_resident",
           "pepshost_binned_energy_stat",
           "pepshost_ema_track", "pepshost_spike_replay", "pepshost_acceptance_rate_check", "pepshost_step_select", "pepshost_step_candidates",
           "pepshost_validate_guards", "pepshost_guarded_optimize_exact_sum", "pepshost_guarded_vmc_optimize"]

_lib = None
_C128 = 3                                   # PEPSGPU_C128 (include/pepsgpu.h)

# updater ids of the shim: MCUpdateSquareNNExchangeOBC, MCUpdateSquareNNFullSpaceUpdateOBC, MCUpdateSquareTNN3SiteExchange
UPDATER_ID = {"exchange": 0, "fullspace": 1, "tnn3": 2}
# ... of the fermionic entries: MCUpdateSquareNNExchangeOBC, MCUpdateSquareTNN3SiteExchange, MCUpdateSquareNNHubbardU1U1OBC
FERMION_UPDATER_ID = {"exchange": 0, "tnn3": 2, "hubbard_u1u1": 3}


def _updater_id(updater):
    # (any other name has always meant the full-space updater in these calls)
    return UPDATER_ID.get(updater, 1)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libpepshost.so not built: run __graft_entry__.build()")
        from . import capi
        capi.lib()                         # make sure libpepsgpu.so is resolvable first
        _lib = C.CDLL(LIB_PATH)
        _lib.pepshost_last_error.restype = C.c_char_p
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _ck(rc):
    if rc != 0:
        msg = lib().pepshost_last_error().decode()
        raise {1: ValueError, 3: RuntimeError, 4: IndexError}.get(rc, RuntimeError)("pepshost error %d: %s" % (rc, msg))


MODEL_ID = {"xxz": 0, "tfim": 1, "j1j2": 2, "triangle": 3, "trij1j2": 4}   # params: xxz (jz, jxy, pinning00); tfim (h,); j1j2 (jz, jxy, jz2, jxy2, pinning00);
# triangle (SpinOneHalfTriHeisenbergSqrPEPS: none; energy_and_holes / exact_sum_partial / measure); trij1j2 (SpinOneHalfTriJ1J2HeisenbergSqrPEPS: (j2,);
# energy_and_holes / exact_sum_partial / measure)


def _dims(flat):
    rows, cols, d, D = flat.shape[0], flat.shape[1], flat.shape[2], flat.shape[3]
    return rows, cols, d, D


def set_device(device=None):
    """GPU of every contractor the calls below build: one rank per GPU, so the default is LOCAL_RANK (else 0)."""
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    l = lib()
    l.pepshost_set_device.argtypes = [C.c_int]
    _ck(l.pepshost_set_device(int(device)))


def get_device():
    return lib().pepshost_get_device()


def set_truncate_params(d_min=-1, trunc_err=0.0, scheme=0, convergence_tol=0.0, iter_max=0):
    """BMPSTruncateParams used by every following call (D_max = the call's chi): SVD / Variational2Site / Variational1Site
    (bmps.h:47-98).  set_truncate_params() restores SVD(chi, chi, 0)."""
    l = lib()
    l.pepshost_set_truncate_params.argtypes = [C.c_int, C.c_double, C.c_int, C.c_double, C.c_int]
    _ck(l.pepshost_set_truncate_params(d_min, trunc_err, scheme, convergence_tol, iter_max))


def mc_sweeps(flat, configs, seeds, chi, updater="exchange", n_sweeps=1, dtype=1):
    flat = np.ascontiguousarray(flat, dtype=np.float64)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(configs, dtype=np.int32).copy()
    n = cfg.shape[0]
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    amps = np.zeros(n)
    rates = np.zeros(n)
    _ck(lib().pepshost_mc_sweeps(rows, cols, D, d, chi, dtype, _p(flat, C.c_double), n, _p(cfg, C.c_int32),
                                 _p(sd, C.c_uint64), _updater_id(updater), n_sweeps,
                                 _p(amps, C.c_double), _p(rates, C.c_double)))
    return cfg, amps, rates


def mc_engine_warmup(flat, configs, seeds, chi, warmup_sweeps=0, rescue=True, amp_min=0.0, amp_max=0.0, dtype=1, max_over_ranks=None,
                     exchange_valid_config=None):
    """MonteCarloEngine: configuration validity / rescue, warm-up, NormalizeStateOrder1 (monte_carlo_engine.h).
    Returns (scaled state, configs, amplitudes, overall scale factor, walkers rescued).
    Several ranks: max_over_ranks(x) -> max over the ranks (the MPI_Allreduce of NormalizeStateOrder1) and
    exchange_valid_config(n_invalid, have_valid, cfg) -> (total invalid | -1, cfg of the first valid rank) (the Allgather + BCast of
    EnsureConfigurationValidity); peps_amd.dist has both (allreduce_max, exchange_valid_configuration).  Both are collectives: every
    rank must pass them."""
    st = np.array(flat, dtype=np.float64, order="C")
    rows, cols, d, D = _dims(st)
    cfg = np.array(configs, dtype=np.int32, order="C")
    n = cfg.shape[0]
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    amps, out = np.zeros(n), np.zeros(3)
    if max_over_ranks is None and exchange_valid_config is None:
        _ck(lib().pepshost_mc_engine_warmup(rows, cols, D, d, chi, dtype, _p(st, C.c_double), n, _p(cfg, C.c_int32), _p(sd, C.c_uint64),
                                            warmup_sweeps, int(rescue), C.c_double(amp_min), C.c_double(amp_max), _p(amps, C.c_double),
                                            _p(out, C.c_double)))
        return st, cfg, amps, float(out[0]), int(out[1])
    MAXF = C.CFUNCTYPE(C.c_double, C.c_double)
    EXF = C.CFUNCTYPE(C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32))
    sites = rows * cols

    def _ex(n_invalid, have_valid, ptr):
        mine = np.ctypeslib.as_array(ptr, shape=(sites,))
        tot, got = exchange_valid_config(int(n_invalid), bool(have_valid), mine.copy())
        mine[:] = np.asarray(got, dtype=np.int32).ravel()
        return int(tot)

    mx = MAXF(lambda x: float(max_over_ranks(float(x)))) if max_over_ranks is not None else C.cast(None, MAXF)
    ex = EXF(_ex) if exchange_valid_config is not None else C.cast(None, EXF)
    _ck(lib().pepshost_mc_engine_warmup_dist(rows, cols, D, d, chi, dtype, _p(st, C.c_double), n, _p(cfg, C.c_int32), _p(sd, C.c_uint64),
                                             warmup_sweeps, int(rescue), C.c_double(amp_min), C.c_double(amp_max), _p(amps, C.c_double),
                                             _p(out, C.c_double), mx, ex))
    return st, cfg, amps, float(out[0]), int(out[1])


def energy_and_holes(flat, configs, chi, model="xxz", params=(1.0, 1.0, 0.0), holes=True, dtype=1):
    flat = np.ascontiguousarray(flat, dtype=np.float64)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(configs, dtype=np.int32)
    n = cfg.shape[0]
    p = np.array(list(params) + [0.0] * 8, dtype=np.float64)
    amps, en = np.zeros(n), np.zeros(n)
    h = np.zeros((n, rows, cols, D, D, D, D)) if holes else None
    psi = np.zeros((rows + cols, n))
    npsi = C.c_int(0)
    _ck(lib().pepshost_energy_and_holes(rows, cols, D, d, chi, dtype, _p(flat, C.c_double), n, _p(cfg, C.c_int32),
                                        MODEL_ID[model], _p(p, C.c_double), _p(amps, C.c_double),
                                        _p(en, C.c_double), _p(h, C.c_double), _p(psi, C.c_double), C.byref(npsi)))
    return amps, en, h, psi[:npsi.value]


def exact_sum_partial(flat, all_configs, chi, model="xxz", params=(1.0, 1.0, 0.0), rank=0, size=1, batch=64, dtype=1):
    flat = np.ascontiguousarray(flat, dtype=np.float64)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(all_configs, dtype=np.int32)
    p = np.array(list(params) + [0.0] * 8, dtype=np.float64)
    packed = np.zeros(2 * flat.size + 4)
    _ck(lib().pepshost_exact_sum_partial(rows, cols, D, d, chi, dtype, _p(flat, C.c_double), _p(cfg, C.c_int32),
                                         cfg.shape[0], MODEL_ID[model], _p(p, C.c_double), rank, size, batch,
                                         _p(packed, C.c_double)))
    return packed


def exact_sum_measure_partial(flat, all_configs, chi, model="xxz", params=(1.0, 1.0, 0.0), rank=0, size=1, batch=64, dtype=1):
    """Rank-local part of ExactSumMeasurerMPI (exact_summation_measurer.h:103-257) through the C++ measurement solver:
    (dict key -> sum_S |psi(S)|^2 O_loc(S), sum_S |psi(S)|^2) over configurations rank, rank + size, ...  Sum both over
    the ranks and divide.  all_configs = None: every binary configuration (GenerateAllBinaryConfigs, :53-72).
    A complex `flat` runs the QLTEN_Complex instantiation (float64 arithmetic; `dtype` is ignored): complex sums."""
    cplx = np.iscomplexobj(flat)
    flat = np.ascontiguousarray(flat, dtype=np.complex128 if cplx else np.float64)
    rows, cols, d, D = _dims(flat)
    cfg = None if all_configs is None else np.ascontiguousarray(all_configs, dtype=np.int32)
    p = np.zeros(8, dtype=np.float64)
    p[:len(params)] = params
    cap = 4 * (rows * cols) ** 2 + 65536
    vals = np.zeros(cap, dtype=np.float64)
    keys = C.create_string_buffer(4096)
    nvals = C.c_long(0)
    l = lib()
    l.pepshost_exact_sum_measure_partial.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int, C.c_int,
                                                     C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int,
                                                     C.POINTER(C.c_double), C.c_long, C.POINTER(C.c_long)]
    l.pepshost_exact_sum_measure_partial_c128.argtypes = [C.c_int] * 5 + l.pepshost_exact_sum_measure_partial.argtypes[6:]
    if cplx:
        _ck(l.pepshost_exact_sum_measure_partial_c128(rows, cols, D, d, chi, _cp(flat),
                                                      None if cfg is None else _p(cfg, C.c_int32), -1 if cfg is None else cfg.shape[0],
                                                      MODEL_ID[model], _p(p, C.c_double), rank, size, batch, keys, 4096,
                                                      _p(vals, C.c_double), cap, C.byref(nvals)))
    else:
        _ck(l.pepshost_exact_sum_measure_partial(rows, cols, D, d, chi, dtype, _p(flat, C.c_double),
                                                 None if cfg is None else _p(cfg, C.c_int32), -1 if cfg is None else cfg.shape[0],
                                                 MODEL_ID[model], _p(p, C.c_double), rank, size, batch, keys, 4096,
                                                 _p(vals, C.c_double), cap, C.byref(nvals)))
    out, off, z = {}, 1, 2 if cplx else 1
    for item in filter(None, keys.value.decode().split(";")):    # a rank without configurations reports no keys
        key, ln = item.split(":")
        seg = vals[off:off + z * int(ln)].copy()
        out[key] = seg.view(np.complex128) if cplx else seg
        off += z * int(ln)
    return out, float(vals[0])


RULE_ID = {"sgd": 0, "adagrad": 1, "adam": 2}   # rule_params: sgd (momentum, nesterov, weight_decay); adagrad (epsilon, initial_accumulator_value);
# adam (beta1, beta2, epsilon, weight_decay)
LR_SCHEDULE_ID = {"constant": 0, "exponential": 1, "step": 2}   # args: (lr,); (initial_lr, decay_rate, decay_steps); (initial_lr, step_size, gamma)


def optimize_exact_sum(flat, all_configs, chi, model, params, rule, lr, rule_params, iterations, clip_value=0.0, clip_norm=0.0, dtype=1,
                       batch=64, return_grad_norms=False):
    """Optimizer::IterativeOptimize of the C++ host layer with the exact-summation evaluator, the whole loop inside one C++ call: the
    state is uploaded once, every iteration evaluates, finishes the gradient, clips and steps on the device.  Returns
    (energies[iterations + 1], final flat state [, gradient norms[iterations + 1]]).  A complex `flat` runs the QLTEN_Complex
    instantiation (`dtype` is ignored)."""
    cplx = np.iscomplexobj(flat)
    flat = np.ascontiguousarray(flat, dtype=np.complex128 if cplx else np.float64)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(all_configs, dtype=np.int32)
    p = np.array(list(params) + [0.0] * 8, dtype=np.float64)
    rp = np.ascontiguousarray([float(x) for x in rule_params], dtype=np.float64)
    rid = RULE_ID[rule] if isinstance(rule, str) else int(rule)
    energies = np.zeros(iterations + 1, dtype=flat.dtype)
    norms = np.zeros(iterations + 1)
    state = np.zeros_like(flat)
    l = lib()
    tail = [C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_double, C.POINTER(C.c_double), C.c_int, C.c_int,
            C.c_double, C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    l.pepshost_optimize_exact_sum.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_double)] + tail
    l.pepshost_optimize_exact_sum_c128.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_double)] + tail
    rest = (_p(cfg, C.c_int32), cfg.shape[0], MODEL_ID[model], _p(p, C.c_double), rid, float(lr), _p(rp, C.c_double), rp.size, int(iterations),
            float(clip_value), float(clip_norm), int(min(batch, cfg.shape[0])))
    if cplx:
        _ck(l.pepshost_optimize_exact_sum_c128(rows, cols, D, d, chi, _cp(flat), *rest, _cp(energies), _p(norms, C.c_double), _cp(state)))
    else:
        _ck(l.pepshost_optimize_exact_sum(rows, cols, D, d, chi, dtype, _p(flat, C.c_double), *rest, _p(energies, C.c_double),
                                          _p(norms, C.c_double), _p(state, C.c_double)))
    return (energies, state, norms) if return_grad_norms else (energies, state)


LBFGS_FIELDS = ("history_size", "tolerance_grad", "tolerance_change", "max_eval", "step_mode", "wolfe_c1", "wolfe_c2", "min_step", "max_step",
                "min_curvature", "use_damping", "max_direction_norm", "allow_fallback_to_fixed_step", "fallback_fixed_step_scale")
LBFGS_DEFAULTS = (10, 1e-5, 1e-9, 20, 0, 1e-4, 0.9, 1e-8, 1.0, 1e-12, True, 1e3, False, 0.2)   # LBFGSParams, optimizer_params.h:135-143
LBFGS_STEP_MODE = {"fixed": 0, "strong_wolfe": 1}


class LineSearchError(RuntimeError):
    """a strong-Wolfe search failed without the fallback; .state = the state the optimizer was left with (the base of that search)"""


def _lbfgs_array(lbfgs):
    """LBFGSParams as the array of the shim: a dict of field names (missing ones take the reference's defaults), a sequence of the
    fourteen values, or any object with those attributes"""
    if lbfgs is None:
        lbfgs = {}
    if isinstance(lbfgs, dict):
        unknown = set(lbfgs) - set(LBFGS_FIELDS)
        if unknown:
            raise ValueError("unknown LBFGSParams fields: %s" % sorted(unknown))
        vals = [lbfgs.get(k, dflt) for k, dflt in zip(LBFGS_FIELDS, LBFGS_DEFAULTS)]
    elif hasattr(lbfgs, LBFGS_FIELDS[0]):
        vals = [getattr(lbfgs, k) for k in LBFGS_FIELDS]
    else:
        vals = list(lbfgs)
        if len(vals) != len(LBFGS_FIELDS):
            raise ValueError("LBFGSParams has %d fields" % len(LBFGS_FIELDS))
    vals = [LBFGS_STEP_MODE[v] if isinstance(v, str) else v for v in vals]
    return np.array([float(v) for v in vals], dtype=np.float64)


def _lbfgs_result(rc, energies, norms, steps, state, info):
    if rc != 0:
        try:
            _ck(rc)
        except RuntimeError as err:
            if "line search failed" in str(err):
                e = LineSearchError(str(err))
                e.state = state
                raise e from None
            raise
    ne, ns = int(info[0]), int(info[1])
    return {"energies": energies[:ne].copy(), "grad_norms": norms[:ne].copy(), "steps": steps[:ns].copy(), "state": state,
            "skip_curvature": int(info[2]), "damping": int(info[3]), "descent_reset": int(info[4]),
            "line_search_evaluations": int(info[5]), "converged": bool(info[6])}


def lbfgs_optimize_exact_sum(flat, cfgs, chi, model, params, lr, lbfgs, iterations, energy_tolerance=0.0, gradient_tolerance=0.0,
                             plateau_patience=0, dtype=1, batch=64):
    """Optimizer::IterativeOptimize of the C++ host layer with LBFGSParams and the exact-summation evaluator, the whole loop inside one
    C++ call: history, anchor, direction and every trial point of the line search stay on the device.  `lbfgs`: see _lbfgs_array.  A
    tolerance of 0 / a patience of 0 switches that stopping criterion off.  Returns a dict: energies (one per iteration and the closing
    evaluation; line-search evaluations are not in it), grad_norms, steps (the step length of every iteration), state (final flat
    state), skip_curvature, damping, descent_reset, line_search_evaluations, converged.  A failed search without the fallback raises
    LineSearchError.  A complex `flat` runs the QLTEN_Complex instantiation (`dtype` is ignored)."""
    cplx = np.iscomplexobj(flat)
    flat = np.ascontiguousarray(flat, dtype=np.complex128 if cplx else np.float64)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(cfgs, dtype=np.int32)
    p = np.array(list(params) + [0.0] * 8, dtype=np.float64)
    lb = _lbfgs_array(lbfgs)
    energies = np.zeros(iterations + 1, dtype=flat.dtype)
    norms, steps, info = np.zeros(iterations + 1), np.zeros(max(iterations, 1)), np.zeros(8)
    state = np.zeros_like(flat)
    l = lib()
    dpt = C.POINTER(C.c_double)
    tail = [C.POINTER(C.c_int32), C.c_int, C.c_int, dpt, C.c_double, dpt, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, dpt, dpt, dpt, dpt, dpt]
    l.pepshost_lbfgs_exact_sum.argtypes = [C.c_int] * 6 + [dpt] + tail
    l.pepshost_lbfgs_exact_sum_c128.argtypes = [C.c_int] * 5 + [dpt] + tail
    rest = (_p(cfg, C.c_int32), cfg.shape[0], MODEL_ID[model], _p(p, C.c_double), float(lr), _p(lb, C.c_double), int(iterations),
            float(energy_tolerance), float(gradient_tolerance), int(plateau_patience), int(min(batch, cfg.shape[0])), _cp(energies),
            _p(norms, C.c_double), _p(steps, C.c_double), _cp(state), _p(info, C.c_double))
    if cplx:
        rc = l.pepshost_lbfgs_exact_sum_c128(rows, cols, D, d, chi, _cp(flat), *rest)
    else:
        rc = l.pepshost_lbfgs_exact_sum(rows, cols, D, d, chi, dtype, _p(flat, C.c_double), *rest)
    return _lbfgs_result(rc, energies, norms, steps, state, info)


def sr_step_samples(flat, configs, chi, model, params, lr, diag_shift=0.001, cg_max_iter=100, cg_relative_tolerance=1e-4,
                    normalize_update=False, dtype=1):
    """One stochastic-reconfiguration iteration of the C++ Optimizer on a given sample set (weight 1 per sample): gradient from the
    resident accumulators, natural gradient solved on the device, theta -= lr x (lr / |x| with normalize_update).  Returns (state after
    the step, dict with the energies before / after, CG iterations, |x| and the CG residual norm).  Models: "xxz", "tfim"."""
    cplx = np.iscomplexobj(flat)
    flat = np.ascontiguousarray(flat, dtype=np.complex128 if cplx else np.float64)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(configs, dtype=np.int32)
    p = np.array(list(params) + [0.0] * 8, dtype=np.float64)
    state, info = np.zeros_like(flat), np.zeros(5)
    l = lib()
    tail = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_double), C.c_double, C.c_double, C.c_int, C.c_double,
            C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    l.pepshost_sr_step_samples.argtypes = [C.c_int] * 6 + tail
    l.pepshost_sr_step_samples_c128.argtypes = [C.c_int] * 5 + tail
    rest = (cfg.shape[0], _p(cfg, C.c_int32), MODEL_ID[model], _p(p, C.c_double), float(lr), float(diag_shift), int(cg_max_iter),
            float(cg_relative_tolerance), int(bool(normalize_update)), _cp(state), _p(info, C.c_double))
    if cplx:
        _ck(l.pepshost_sr_step_samples_c128(rows, cols, D, d, chi, _cp(flat), *rest))
    else:
        _ck(l.pepshost_sr_step_samples(rows, cols, D, d, chi, dtype, _cp(flat), *rest))
    return state, {"energy_before": info[0], "energy_after": info[1], "cg_iterations": int(info[2]), "direction_norm": info[3],
                   "cg_residual_norm": info[4]}


def minsr_step_samples(flat, configs, chi, model, params, lr, r_pinv=1e-12, a_pinv=0.0, soft_cutoff=True, dtype=1, exact_sum=False):
    """One MinSR iteration of the C++ Optimizer (MinSRParams) on a given sample set (weight 1 per sample): gradient from the resident
    accumulators, the MinSR direction x from the resident O* store and the samples' local energies on the device, theta -= lr x.
    Returns (state after the step, dict with the energies before / after, |x|, the largest eigenvalue of T, the cutoff, the number of
    eigenvalues kept and the Jacobi sweeps).  Models: "xxz", "tfim".  exact_sum=True evaluates by exact summation over `configs`
    instead: that evaluator keeps no sample set and the update refuses (ValueError)."""
    cplx = np.iscomplexobj(flat)
    flat = np.ascontiguousarray(flat, dtype=np.complex128 if cplx else np.float64)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(configs, dtype=np.int32)
    p = np.array(list(params) + [0.0] * 8, dtype=np.float64)
    state, info = np.zeros_like(flat), np.zeros(7)
    l = lib()
    tail = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double,
            C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    l.pepshost_minsr_step_samples.argtypes = [C.c_int] * 6 + tail
    l.pepshost_minsr_step_samples_c128.argtypes = [C.c_int] * 5 + tail
    rest = (cfg.shape[0], _p(cfg, C.c_int32), MODEL_ID[model], _p(p, C.c_double), float(lr), float(r_pinv), float(a_pinv),
            int(bool(soft_cutoff)), int(bool(exact_sum)), _cp(state), _p(info, C.c_double))
    if cplx:
        _ck(l.pepshost_minsr_step_samples_c128(rows, cols, D, d, chi, _cp(flat), *rest))
    else:
        _ck(l.pepshost_minsr_step_samples(rows, cols, D, d, chi, dtype, _cp(flat), *rest))
    return state, {"energy_before": info[0], "energy_after": info[1], "direction_norm": info[2], "lambda_max": info[3], "cutoff": info[4],
                   "n_kept": int(info[5]), "sweeps": int(info[6])}


def lr_schedule(kind, args, iteration):
    """LearningRateScheduler::GetLearningRate of the host layer: kind "constant" (lr,), "exponential" (initial_lr, decay_rate,
    decay_steps), "step" (initial_lr, step_size, gamma)"""
    a = np.ascontiguousarray([float(x) for x in args], dtype=np.float64)
    out = C.c_double(0.0)
    l = lib()
    l.pepshost_lr_schedule.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int, C.c_long, C.POINTER(C.c_double)]
    _ck(l.pepshost_lr_schedule(LR_SCHEDULE_ID[kind] if isinstance(kind, str) else int(kind), _p(a, C.c_double), a.size, int(iteration),
                               C.byref(out)))
    return out.value


def exact_sum_finish(packed, shape):
    rows, cols, d, D = shape[:4]
    packed = np.ascontiguousarray(packed, dtype=np.float64)
    e = C.c_double(0)
    grad = np.zeros((rows, cols, d, D, D, D, D))
    _ck(lib().pepshost_exact_sum_finish(rows, cols, D, d, _p(packed, C.c_double), C.byref(e), _p(grad, C.c_double)))
    return e.value, grad


def load_sitps(directory, D):
    rows, cols, d = C.c_int(0), C.c_int(0), C.c_int(0)
    _ck(lib().pepshost_load_sitps(directory.encode(), D, C.byref(rows), C.byref(cols), C.byref(d), None, 0))
    flat = np.zeros((rows.value, cols.value, d.value, D, D, D, D))
    _ck(lib().pepshost_load_sitps(directory.encode(), D, C.byref(rows), C.byref(cols), C.byref(d),
                                  _p(flat, C.c_double), flat.size))
    return flat


def mc_energy_grad_partial(flat, configs, seeds, chi, updater="exchange", model="xxz", params=(1.0, 1.0, 0.0),
                           warmup_sweeps=1, n_samples=1, dtype=1):
    """Rank-local MCEnergyGradEvaluator loop; returns (packed accumulators, final configs, accept rates)."""
    flat = np.ascontiguousarray(flat, dtype=np.float64)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(configs, dtype=np.int32).copy()
    n = cfg.shape[0]
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    p = np.array(list(params) + [0.0] * 8, dtype=np.float64)
    packed = np.zeros(2 * flat.size + 4)
    acc = np.zeros(n)
    _ck(lib().pepshost_mc_energy_grad_partial(rows, cols, D, d, chi, dtype, _p(flat, C.c_double), n, _p(cfg, C.c_int32),
                                              _p(sd, C.c_uint64), _updater_id(updater),
                                              MODEL_ID[model], _p(p, C.c_double), warmup_sweeps, n_samples,
                                              _p(packed, C.c_double), _p(acc, C.c_double)))
    return packed, cfg, acc


def measure(flat, configs, chi, model="xxz", params=(1.0, 1.0, 0.0), seeds=None, updater="exchange", warmup_sweeps=0,
            n_samples=0, sweeps_between_samples=1, dump_dir="", dtype=1):
    """Registry observables of the C++ measurement solver (SquareNNNModelMeasurementSolver::EvaluateObservables,
    square_nnn_model_measurement_solver.h) on fixed configurations (n_samples = 0: dict key -> [walker][len]) or a whole
    MCPEPSMeasurer run (n_samples > 0: dict key -> (mean[len], stderr[len]) across the walkers; configs updated in place;
    dump_dir: stats/*.csv + samples/psi.csv as the reference writes them).  Also returns the psi summary of the last
    sample: (psi_mean[walker], psi_rel_err[walker]).  A complex `flat` runs the QLTEN_Complex instantiation: complex values and means,
    real standard errors."""
    cplx = np.iscomplexobj(flat)
    flat = np.ascontiguousarray(flat, dtype=np.complex128 if cplx else np.float64)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(configs, dtype=np.int32)
    n = cfg.shape[0]
    sd = np.ascontiguousarray(np.zeros(n) if seeds is None else seeds, dtype=np.uint64)
    p = np.zeros(8, dtype=np.float64)
    p[:len(params)] = params
    cap = 8 * n * (rows * cols) ** 2 + 65536
    vals = np.zeros(cap, dtype=np.float64)
    keys = C.create_string_buffer(4096)
    nvals = C.c_long(0)
    l = lib()
    l.pepshost_measure.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_uint64),
                                   C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                   C.c_int, C.POINTER(C.c_double), C.c_long, C.POINTER(C.c_long)]
    l.pepshost_measure_c128.argtypes = [C.c_int] * 5 + l.pepshost_measure.argtypes[6:]
    if cplx:
        _ck(l.pepshost_measure_c128(rows, cols, D, d, chi, _cp(flat), n, _p(cfg, C.c_int32), _p(sd, C.c_uint64),
                                    UPDATER_ID[updater], MODEL_ID[model], _p(p, C.c_double), warmup_sweeps,
                                    n_samples, sweeps_between_samples, dump_dir.encode(), keys, 4096, _p(vals, C.c_double), cap,
                                    C.byref(nvals)))
        vals = vals[:nvals.value].view(np.complex128)          # every number is a (re, im) pair
    else:
        _ck(l.pepshost_measure(rows, cols, D, d, chi, dtype, _p(flat, C.c_double), n, _p(cfg, C.c_int32), _p(sd, C.c_uint64),
                               UPDATER_ID[updater], MODEL_ID[model], _p(p, C.c_double), warmup_sweeps,
                               n_samples, sweeps_between_samples, dump_dir.encode(), keys, 4096, _p(vals, C.c_double), cap,
                               C.byref(nvals)))
    out, off = {}, 0
    for item in keys.value.decode().strip(";").split(";"):
        key, ln = item.split(":")
        ln = int(ln)
        if n_samples > 0:
            out[key] = (vals[off:off + ln].copy(), np.real(vals[off + ln:off + 2 * ln]).copy())
            off += 2 * ln
        else:
            out[key] = vals[off:off + n * ln].reshape(n, ln).copy()
            off += n * ln
    psi = (vals[off:off + n].copy(), np.real(vals[off + n:off + 2 * n]).copy())
    if n_samples > 0:
        configs[...] = cfg
    return out, psi


def dump_sitps(directory, flat):
    """SplitIndexTPS::Dump (split_index_tps_impl.h:300-330) of a padded OBC state."""
    flat = np.ascontiguousarray(flat, dtype=np.float64)
    rows, cols, d, D = _dims(flat)
    os.makedirs(directory, exist_ok=True)
    _ck(lib().pepshost_dump_sitps(directory.encode(), rows, cols, D, d, _p(flat, C.c_double)))


def dump_configuration(directory, label, config):
    cfg = np.ascontiguousarray(config, dtype=np.int32)
    _ck(lib().pepshost_dump_configuration(directory.encode(), label, cfg.shape[0], cfg.shape[1], _p(cfg, C.c_int32)))


def load_configuration(directory, label, rows, cols):
    out = np.zeros((rows, cols), dtype=np.int32)
    _ck(lib().pepshost_load_configuration(directory.encode(), label, rows, cols, _p(out, C.c_int32)))
    return out


def try_load_configuration(directory, label, rows, cols):
    """Configuration::Load (configuration.h:356-393): the configuration, or None where the reference returns false (missing file, `.shape`
    sidecar of another size, payload that does not parse) -- no exception for those."""
    out = np.zeros((rows, cols), dtype=np.int32)
    ok = C.c_int(0)
    _ck(lib().pepshost_load_configuration2(directory.encode(), label, rows, cols, _p(out, C.c_int32), C.byref(ok)))
    return out if ok.value else None


def configuration_from_text(text, rows, cols):
    """Configuration::StreamRead (configuration.h:446-455); RuntimeError when the text holds too few numbers"""
    out = np.zeros((rows, cols), dtype=np.int32)
    _ck(lib().pepshost_configuration_from_text(text.encode(), rows, cols, _p(out, C.c_int32)))
    return out


def fermion_energy(state, configs, chi, t, V=0.0, dtype=1, model="spinless", J=0.0, mu=0.0, t2=0.0, U=0.0):
    """C++ host layer on a fermionic state (peps_amd.fermion.FermionState): amplitudes (row-major mode order),
    E_loc of the spinless t-V model (model="spinless"), of the t-J-V model (model="tj") or of the Hubbard model (model="hubbard":
    t, U, mu), psi along every route.
    A complex state (SplitIndexTPS<QLTEN_Complex, fZ2QN>) runs the complex instantiation in float64 (`dtype` ignored)."""
    if model not in ("spinless", "tj", "hubbard"):
        raise ValueError("fermion_energy: model must be 'spinless', 'tj' or 'hubbard'")
    cplx = state.is_complex
    et = np.complex128 if cplx else np.float64
    flat = np.ascontiguousarray(state.extended_flat(), dtype=et)
    rows, cols, D = flat.shape[0], flat.shape[1], flat.shape[3]
    cfg = np.ascontiguousarray(configs, dtype=np.int32)
    n = cfg.shape[0]
    nf = np.ascontiguousarray(state.nf, dtype=np.int32)
    amps, en = np.zeros(n, et), np.zeros(n, et)
    psi = np.zeros((rows + cols, n), et)
    npsi = C.c_int(0)
    prm = np.array([t, V, t2, 0.0] if model == "spinless" else [t, J, V, mu], dtype=np.float64)
    if model == "hubbard" or t2 != 0.0 and model != "spinless":      # the Hubbard and the t-t'-J model: the entry with a parameter count
        prm = np.array([t, U, mu] if model == "hubbard" else [t, J, V, mu, t2], dtype=np.float64)
        _ck(lib().pepshost_fermion_energy_prm(rows, cols, D, state.d, _p(nf, C.c_int32), chi, _C128 if cplx else dtype,
                                              _cp(flat), n, _p(cfg, C.c_int32), FERMION_MODEL_ID[model], prm.size,
                                              _p(prm, C.c_double), _cp(amps),
                                              _cp(en), _cp(psi),
                                              C.byref(npsi)))
    elif cplx:
        _ck(lib().pepshost_fermion_energy_c128(rows, cols, D, state.d, _p(nf, C.c_int32), chi, _cp(flat), n,
                                               _p(cfg, C.c_int32), 0 if model == "spinless" else 1, _p(prm, C.c_double),
                                               _cp(amps), _cp(en), _cp(psi), C.byref(npsi)))
    else:
        _ck(lib().pepshost_fermion_energy(rows, cols, D, state.d, _p(nf, C.c_int32), chi, dtype, _p(flat, C.c_double), n,
                                          _p(cfg, C.c_int32), 0 if model == "spinless" else 1, _p(prm, C.c_double),
                                          _p(amps, C.c_double), _p(en, C.c_double), _p(psi, C.c_double), C.byref(npsi)))
    return amps, en, psi[:npsi.value]


def fermion_mc_sweeps(state, configs, seeds, chi, n_sweeps=1, dtype=1, updater="exchange"):
    """n_sweeps sweeps of a fermionic state; updater "exchange" (MCUpdateSquareNNExchangeOBC), "tnn3"
    (MCUpdateSquareTNN3SiteExchange, real element types) or "hubbard_u1u1" (MCUpdateSquareNNHubbardU1U1OBC, every element type)"""
    if updater not in FERMION_UPDATER_ID:
        raise ValueError("fermion_mc_sweeps: updater must be 'exchange', 'tnn3' or 'hubbard_u1u1'")
    cplx = state.is_complex
    et = np.complex128 if cplx else np.float64
    flat = np.ascontiguousarray(state.extended_flat(), dtype=et)
    rows, cols, D = flat.shape[0], flat.shape[1], flat.shape[3]
    cfg = np.ascontiguousarray(configs, dtype=np.int32).copy()
    n = cfg.shape[0]
    nf = np.ascontiguousarray(state.nf, dtype=np.int32)
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    amps, rates = np.zeros(n, et), np.zeros(n)
    if updater != "exchange":
        if cplx and updater == "tnn3":
            raise ValueError("fermion_mc_sweeps: the three-site updater takes real fermionic states")
        _ck(lib().pepshost_fermion_mc_sweeps_updater(rows, cols, D, state.d, _p(nf, C.c_int32), chi, _C128 if cplx else dtype, _cp(flat), n,
                                                     _p(cfg, C.c_int32), _p(sd, C.c_uint64), FERMION_UPDATER_ID[updater], n_sweeps,
                                                     _cp(amps), _p(rates, C.c_double)))
    elif cplx:
        _ck(lib().pepshost_fermion_mc_sweeps_c128(rows, cols, D, state.d, _p(nf, C.c_int32), chi, _cp(flat), n,
                                                  _p(cfg, C.c_int32), _p(sd, C.c_uint64), n_sweeps, _cp(amps), _p(rates, C.c_double)))
    else:
        _ck(lib().pepshost_fermion_mc_sweeps(rows, cols, D, state.d, _p(nf, C.c_int32), chi, dtype, _p(flat, C.c_double), n,
                                             _p(cfg, C.c_int32), _p(sd, C.c_uint64), n_sweeps, _p(amps, C.c_double),
                                             _p(rates, C.c_double)))
    return cfg, amps, rates


def fermion_measure_energy(state, configs, seeds, chi, warmup_sweeps, n_samples, sweeps_between=1, model="tj", t=1.0, J=0.0, V=0.0, mu=0.0,
                           t2=0.0, dtype=1):
    """MCPEPSMeasurer's energy samples on a fermionic state with ONE std::mt19937 stream per walker over warm-up, rebuild and samples
    (pepshost_fermion_measure_energy): (energies [sample][walker], final configurations, accept rates)."""
    cplx = state.is_complex
    et = np.complex128 if cplx else np.float64
    flat = np.ascontiguousarray(state.extended_flat(), dtype=et)
    rows, cols, D = flat.shape[0], flat.shape[1], flat.shape[3]
    cfg = np.ascontiguousarray(configs, dtype=np.int32).copy()
    n = cfg.shape[0]
    nf = np.ascontiguousarray(state.nf, dtype=np.int32)
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    prm = np.array([t, J, V, mu] if model == "tj" else [t, V, t2, 0.0], dtype=np.float64)
    en, rates = np.zeros((n_samples, n), et), np.zeros(n)
    if model == "tj" and t2 != 0.0:                   # the t-t'-J model: the entry with a parameter count carries t2
        prm = np.array([t, J, V, mu, t2], dtype=np.float64)
        _ck(lib().pepshost_fermion_measure_energy_prm(rows, cols, D, state.d, _p(nf, C.c_int32), chi, _C128 if cplx else dtype,
                                                      _cp(flat), n, _p(cfg, C.c_int32), _p(sd, C.c_uint64),
                                                      warmup_sweeps, n_samples, sweeps_between, 1, prm.size, _p(prm, C.c_double),
                                                      _cp(en), _p(rates, C.c_double)))
    elif cplx:
        _ck(lib().pepshost_fermion_measure_energy_c128(rows, cols, D, state.d, _p(nf, C.c_int32), chi, _cp(flat), n,
                                                       _p(cfg, C.c_int32), _p(sd, C.c_uint64), warmup_sweeps, n_samples, sweeps_between,
                                                       1 if model == "tj" else 0, _p(prm, C.c_double), _cp(en), _p(rates, C.c_double)))
    else:
        _ck(lib().pepshost_fermion_measure_energy(rows, cols, D, state.d, _p(nf, C.c_int32), chi, dtype, _p(flat, C.c_double), n,
                                                  _p(cfg, C.c_int32), _p(sd, C.c_uint64), warmup_sweeps, n_samples, sweeps_between,
                                                  1 if model == "tj" else 0, _p(prm, C.c_double), _p(en, C.c_double), _p(rates, C.c_double)))
    return en, cfg, rates


def fermion_exact_sum(state, all_configs, chi, t, V=0.0, batch=64, dtype=1, model="spinless", J=0.0, mu=0.0, t2=0.0, U=0.0):
    """ExactSumEnergyEvaluator on a fermionic state: (energy, gradient [rows][cols][d][D^4] with respect to the
    stored site-tensor components, zero on parity-forbidden entries).  The spinless t-V model, or -- with model="tj" or a
    diagonal hop t2 -- the models of fermion_energy through the entry that takes a parameter list."""
    from . import fermion
    if model != "spinless" or t2 != 0.0:
        cplx = state.is_complex
        flat = np.ascontiguousarray(state.extended_flat(), dtype=np.complex128 if cplx else np.float64)
        rows, cols, D = flat.shape[0], flat.shape[1], flat.shape[3]
        cfg = np.ascontiguousarray(all_configs, dtype=np.int32)
        nf = np.ascontiguousarray(state.nf, dtype=np.int32)
        prm = np.array([t, V, t2, 0.0] if model == "spinless" else [t, U, mu] if model == "hubbard" else [t, J, V, mu, t2], dtype=np.float64)
        packed = np.zeros(4 * flat.size + 5 if cplx else 2 * flat.size + 4)
        _ck(lib().pepshost_fermion_exact_sum_partial_prm(rows, cols, D, state.d, _p(nf, C.c_int32), chi, _C128 if cplx else dtype, _cp(flat),
                                                         _p(cfg, C.c_int32), cfg.shape[0], FERMION_MODEL_ID[model], _p(prm, C.c_double),
                                                         prm.size, 0, 1, batch, _p(packed, C.c_double)))
        if cplx:
            e = np.zeros(2)
            grad = np.zeros(flat.shape, dtype=np.complex128)
            _ck(lib().pepshost_exact_sum_finish_c128(rows, cols, D, 4 * state.d, _p(packed, C.c_double), _p(e, C.c_double), _cp(grad)))
            return complex(e[0], e[1]), fermion.fold_gradient(state, grad)
        e, grad_ext = exact_sum_finish(packed, (rows, cols, 4 * state.d, D))
        return e, fermion.fold_gradient(state, grad_ext)
    if state.is_complex:                    # QLTEN_Complex: packed = 4 m + 5 doubles, finished by pepshost_exact_sum_finish_c128 on 4 d components
        flat = np.ascontiguousarray(state.extended_flat(), dtype=np.complex128)
        rows, cols, D = flat.shape[0], flat.shape[1], flat.shape[3]
        cfg = np.ascontiguousarray(all_configs, dtype=np.int32)
        nf = np.ascontiguousarray(state.nf, dtype=np.int32)
        packed = np.zeros(4 * flat.size + 5)
        _ck(lib().pepshost_fermion_exact_sum_partial_c128(rows, cols, D, state.d, _p(nf, C.c_int32), chi, _cp(flat),
                                                          _p(cfg, C.c_int32), cfg.shape[0], C.c_double(t), C.c_double(V), 0, 1, batch,
                                                          _p(packed, C.c_double)))
        e = np.zeros(2)
        grad = np.zeros(flat.shape, dtype=np.complex128)
        _ck(lib().pepshost_exact_sum_finish_c128(rows, cols, D, 4 * state.d, _p(packed, C.c_double), _p(e, C.c_double), _cp(grad)))
        return complex(e[0], e[1]), fermion.fold_gradient(state, grad)
    flat = np.ascontiguousarray(state.extended_flat(), dtype=np.float64)
    rows, cols, D = flat.shape[0], flat.shape[1], flat.shape[3]
    cfg = np.ascontiguousarray(all_configs, dtype=np.int32)
    nf = np.ascontiguousarray(state.nf, dtype=np.int32)
    packed = np.zeros(2 * flat.size + 4)
    _ck(lib().pepshost_fermion_exact_sum_partial(rows, cols, D, state.d, _p(nf, C.c_int32), chi, dtype, _p(flat, C.c_double),
                                                 _p(cfg, C.c_int32), cfg.shape[0], C.c_double(t), C.c_double(V), 0, 1, batch,
                                                 _p(packed, C.c_double)))
    e, grad_ext = exact_sum_finish(packed, (rows, cols, 4 * state.d, D))
    return e, fermion.fold_gradient(state, grad_ext)


# params: spinless (t, V, t2); tj (t, J, V, mu[, t2]); hubbard (t, U, mu) -- as fermion_energy passes them
FERMION_MODEL_ID = {"spinless": 0, "tj": 1, "hubbard": 3}
# the measurement entries also know SquaretJNNModel, the nearest-neighbour form of the registry: tjnn (t, J, mu)
FERMION_MEASURE_MODEL_ID = {"spinless": 0, "tj": 1, "tjnn": 2, "hubbard": 3}


def _fermion_measure_head(state, chi, model, params, dtype):
    """(is complex, leading arguments rows .. flat of the fermionic measurement shims, the arrays that must stay alive)"""
    cplx = state.is_complex
    flat = np.ascontiguousarray(state.extended_flat(), dtype=np.complex128 if cplx else np.float64)
    rows, cols, D = flat.shape[0], flat.shape[1], flat.shape[3]
    nf = np.ascontiguousarray(state.nf, dtype=np.int32)
    prm = np.array([float(x) for x in params], dtype=np.float64)
    head = (rows, cols, D, state.d, _p(nf, C.c_int32), chi, _C128 if cplx else dtype, _cp(flat))
    return cplx, head, (FERMION_MEASURE_MODEL_ID[model], prm.size, _p(prm, C.c_double)), (flat, nf, prm)


def _keyed(keys, vals, cplx):
    """[(key, len)] and the value array (complex: every number a (re, im) pair) of an output in the format of pepshost_measure"""
    items = [(k, int(ln)) for k, ln in (item.split(":") for item in filter(None, keys.value.decode().split(";")))]
    return items, (vals.view(np.complex128) if cplx else vals)


def _ref_bonds(ref_bonds):
    """the selected reference bonds of SC_singlet_pair_corr as the trailing arguments (count, [n][2] int32 or NULL) of the *_sc shims"""
    rb = np.ascontiguousarray(np.asarray(ref_bonds, dtype=np.int32).reshape(-1, 2))
    return rb.shape[0], (_p(rb, C.c_int32) if rb.shape[0] else None), rb


def sc_pair_corr_mapping(rows, cols, ref_bonds=()):
    """GenerateSCPairCorrIndexMapping of the host layer's SingletPairCorrelationMixin: [n_pairs][6] = (ref_y, ref_x, 0, tgt_y, tgt_x, 0)
    per value of SC_singlet_pair_corr; ref_bonds = selected reference bonds (y, x) of the left site, none: all.  Needs no device."""
    nb, pb, keep = _ref_bonds(ref_bonds)
    count = C.c_long(0)
    _ck(lib().pepshost_sc_pair_corr_mapping(rows, cols, nb, pb, None, C.c_long(0), C.byref(count)))
    out = np.zeros((count.value, 6), dtype=np.int32)
    _ck(lib().pepshost_sc_pair_corr_mapping(rows, cols, nb, pb, _p(out, C.c_int32), C.c_long(count.value), C.byref(count)))
    return out


def _sc_pairs(rows, cols, sc_pair_corr, ref_bonds):
    return int(sc_pair_corr_mapping(rows, cols, ref_bonds).shape[0]) if sc_pair_corr else 0


def fermion_observables(state, configs, chi, model="tj", params=(1.0, 0.3, 0.0, 0.0), dtype=1, sc_pair_corr=False, ref_bonds=()):
    """Registry of the C++ measurement solver of a fermionic model (SquareNNNModelMeasurementSolver on SquareSpinlessFermion /
    SquaretJVModel / SquaretJNNModel) on a batch of configurations: dict key -> [walker][len] with energy, charge, bond_energy_h / _v
    (/ _dr / _ur) and, for the t-J models, spin_z and the bond-singlet pairing order SC_bond_singlet_h / _v; and the psi summary
    (psi_mean [walker], psi_rel_err [walker]).  params: spinless (t, V, t2), tj (t, J, V, mu, t2), tjnn (t, J, mu), hubbard (t, U, mu:
    SquareHubbardModel, with spin_z and double_occupancy).  sc_pair_corr (t-J models): also SC_singlet_pair_corr, the pair-pair
    correlation of the selected horizontal reference bonds ref_bonds = [(y, x)] (none: all) with every horizontal bond of the rows
    below, in the order of sc_pair_corr_mapping."""
    cplx, head, tail, keep = _fermion_measure_head(state, chi, model, params, dtype)
    cfg = np.ascontiguousarray(configs, dtype=np.int32)
    n, sites = cfg.shape[0], cfg.shape[1] * cfg.shape[2]
    cap = 2 * (16 * n * sites + n * _sc_pairs(cfg.shape[1], cfg.shape[2], sc_pair_corr, ref_bonds) + 4096)
    vals, keys, nvals = np.zeros(cap, dtype=np.float64), C.create_string_buffer(4096), C.c_long(0)
    if sc_pair_corr:
        nb, pb, keep_rb = _ref_bonds(ref_bonds)
        _ck(lib().pepshost_fermion_observables_sc(*head, n, _p(cfg, C.c_int32), *tail, keys, 4096, _p(vals, C.c_double),
                                                  C.c_long(cap), C.byref(nvals), 1, nb, pb))
    else:
        _ck(lib().pepshost_fermion_observables(*head, n, _p(cfg, C.c_int32), *tail, keys, 4096, _p(vals, C.c_double),
                                               C.c_long(cap), C.byref(nvals)))
    items, v = _keyed(keys, vals[:nvals.value], cplx)
    out, off = {}, 0
    for key, ln in items:
        out[key] = v[off:off + n * ln].reshape(n, ln).copy()
        off += n * ln
    return out, (v[off:off + n].copy(), np.real(v[off + n:off + 2 * n]).copy())


def fermion_exact_sum_measure(state, all_configs, chi, model="tj", params=(1.0, 0.3, 0.0, 0.0), rank=0, size=1, batch=64, dtype=1,
                              sc_pair_corr=False, ref_bonds=()):
    """Rank-local part of ExactSumMeasurerMPI on a fermionic state through the C++ measurement solver: (dict key ->
    sum_S |psi(S)|^2 O_loc(S), sum_S |psi(S)|^2) over the configurations rank, rank + size, ...; sum both over the ranks and divide.
    Every configuration must have a non-zero amplitude (hand over the parity-allowed ones)."""
    cplx, head, tail, keep = _fermion_measure_head(state, chi, model, params, dtype)
    cfg = np.ascontiguousarray(all_configs, dtype=np.int32)
    cap = 2 * (16 * cfg.shape[1] * cfg.shape[2] + _sc_pairs(cfg.shape[1], cfg.shape[2], sc_pair_corr, ref_bonds) + 4096)
    vals, keys, nvals = np.zeros(cap, dtype=np.float64), C.create_string_buffer(4096), C.c_long(0)
    if sc_pair_corr:
        nb, pb, keep_rb = _ref_bonds(ref_bonds)
        _ck(lib().pepshost_fermion_exact_sum_measure_partial_sc(*head, _p(cfg, C.c_int32), cfg.shape[0], *tail, rank, size, batch,
                                                                keys, 4096, _p(vals, C.c_double), C.c_long(cap), C.byref(nvals), 1, nb, pb))
    else:
        _ck(lib().pepshost_fermion_exact_sum_measure_partial(*head, _p(cfg, C.c_int32), cfg.shape[0], *tail, rank, size, batch,
                                                             keys, 4096, _p(vals, C.c_double), C.c_long(cap), C.byref(nvals)))
    items, _ = _keyed(keys, vals, False)
    out, off, z = {}, 1, 2 if cplx else 1
    for key, ln in items:
        seg = vals[off:off + z * ln].copy()
        out[key] = seg.view(np.complex128) if cplx else seg
        off += z * ln
    return out, float(vals[0])


def fermion_measure(state, configs, seeds, chi, warmup_sweeps, n_samples, sweeps_between=1, model="tj", params=(1.0, 0.3, 0.0, 0.0), dtype=1,
                    updater="exchange", sc_pair_corr=False, ref_bonds=()):
    """MCPEPSMeasurer with the exchange updater (or updater="hubbard_u1u1") on a fermionic state: dict key -> (mean [len], stderr [len])
    across the walkers, the psi summary of the last sample, the energy samples [sample][walker], the final configurations and the accept
    rates.  Warm-up, samples and ONE std::mt19937 stream per walker as fermion_measure_energy: with the exchange updater the energy
    samples are the numbers that call returns."""
    if updater not in ("exchange", "hubbard_u1u1"):
        raise ValueError("fermion_measure: updater must be 'exchange' or 'hubbard_u1u1'")
    if sc_pair_corr and updater != "exchange":
        raise ValueError("fermion_measure: SC_singlet_pair_corr is measured with the exchange updater (t-J models)")
    cplx, head, tail, keep = _fermion_measure_head(state, chi, model, params, dtype)
    cfg = np.ascontiguousarray(configs, dtype=np.int32).copy()
    n, sites = cfg.shape[0], cfg.shape[1] * cfg.shape[2]
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    cap = 2 * (32 * sites + 2 * _sc_pairs(cfg.shape[1], cfg.shape[2], sc_pair_corr, ref_bonds) + 2 * n + 4096)
    vals, keys, nvals = np.zeros(cap, dtype=np.float64), C.create_string_buffer(4096), C.c_long(0)
    en, rates = np.zeros((n_samples, n), np.complex128 if cplx else np.float64), np.zeros(n)
    if sc_pair_corr:
        nb, pb, keep_rb = _ref_bonds(ref_bonds)
        _ck(lib().pepshost_fermion_measure_sc(*head, n, _p(cfg, C.c_int32), _p(sd, C.c_uint64), warmup_sweeps, n_samples,
                                              sweeps_between, *tail, keys, 4096, _p(vals, C.c_double), C.c_long(cap), C.byref(nvals), _cp(en),
                                              _p(rates, C.c_double), 1, nb, pb))
    elif updater == "exchange":
        _ck(lib().pepshost_fermion_measure(*head, n, _p(cfg, C.c_int32), _p(sd, C.c_uint64), warmup_sweeps, n_samples,
                                           sweeps_between, *tail, keys, 4096, _p(vals, C.c_double), C.c_long(cap), C.byref(nvals), _cp(en),
                                           _p(rates, C.c_double)))
    else:
        _ck(lib().pepshost_fermion_measure_updater(*head, n, _p(cfg, C.c_int32), _p(sd, C.c_uint64), FERMION_UPDATER_ID[updater], warmup_sweeps,
                                                   n_samples, sweeps_between, *tail, keys, 4096, _p(vals, C.c_double), C.c_long(cap),
                                                   C.byref(nvals), _cp(en), _p(rates, C.c_double)))
    items, v = _keyed(keys, vals[:nvals.value], cplx)
    out, off = {}, 0
    for key, ln in items:
        out[key] = (v[off:off + ln].copy(), np.real(v[off + ln:off + 2 * ln]).copy())
        off += 2 * ln
    return out, (v[off:off + n].copy(), np.real(v[off + n:off + 2 * n]).copy()), en, cfg, rates


def _fermion_head(state, dtype):
    """(element type, decorated flat state, leading arguments of the fermionic optimizer shims up to chi)"""
    cplx = state.is_complex
    et = np.complex128 if cplx else np.float64
    flat = np.ascontiguousarray(state.extended_flat(), dtype=et)
    rows, cols, D = flat.shape[0], flat.shape[1], flat.shape[3]
    nf = np.ascontiguousarray(state.nf, dtype=np.int32)
    par = np.zeros((rows, cols, 4, D), dtype=np.uint8)
    for r in range(rows):
        for c in range(cols):
            for leg in range(4):
                p = np.asarray(state.par[r][c][leg])
                par[r, c, leg, :len(p)] = p
    return cplx, flat, nf, par, (rows, cols, D, state.d, _p(nf, C.c_int32), par.ctypes.data_as(C.POINTER(C.c_uint8)))


def _fermion_prm(model, params):
    prm = [float(x) for x in params]
    if model == "spinless":
        prm = (prm + [0.0] * 4)[:4]                         # [t, V, t2, -]
    elif model == "hubbard":
        prm = (prm + [0.0] * 3)[:3]                         # [t, U, mu]
    else:
        prm = prm + [0.0] * max(0, 4 - len(prm))            # [t, J, V, mu, (t2)]
    return np.array(prm, dtype=np.float64)


def fermion_optimize_exact_sum(state, all_configs, chi, model, params, rule, lr, rule_params, iterations, clip_value=0.0, clip_norm=0.0,
                               dtype=1, batch=64, return_grad_norms=False):
    """optimize_exact_sum on a fermionic state (peps_amd.fermion.FermionState): the decorated components are uploaded once, every
    iteration evaluates, folds and projects the gradient, clips and steps on the device.  model "spinless" (t, V, t2), "tj"
    (t, J, V, mu[, t2]) or "hubbard" (t, U, mu).  Returns (energies[iterations + 1], final stored tensors [rows][cols][d][D^4] [, norms of the gradient over
    the stored parameters]); FermionState.from_stored(state, stored) is the state after the run."""
    cplx, flat, nf, par, head = _fermion_head(state, dtype)
    cfg = np.ascontiguousarray(all_configs, dtype=np.int32)
    prm = _fermion_prm(model, params)
    rp = np.ascontiguousarray([float(x) for x in rule_params], dtype=np.float64)
    rid = RULE_ID[rule] if isinstance(rule, str) else int(rule)
    energies = np.zeros(iterations + 1, dtype=flat.dtype)
    norms = np.zeros(iterations + 1)
    stored = np.zeros((flat.shape[0], flat.shape[1], state.d) + flat.shape[3:], dtype=flat.dtype)
    l = lib()
    dpt, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    tail = [dpt, i32, C.c_int, C.c_int, dpt, C.c_int, C.c_int, C.c_double, dpt, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, dpt, dpt, dpt]
    lead = [C.c_int] * 4 + [i32, C.POINTER(C.c_uint8), C.c_int]
    l.pepshost_fermion_optimize_exact_sum.argtypes = lead + [C.c_int] + tail
    l.pepshost_fermion_optimize_exact_sum_c128.argtypes = lead + tail
    rest = (_cp(flat), _p(cfg, C.c_int32), cfg.shape[0], FERMION_MODEL_ID[model], _p(prm, C.c_double), prm.size, rid, float(lr),
            _p(rp, C.c_double), rp.size, int(iterations), float(clip_value), float(clip_norm), int(min(batch, cfg.shape[0])),
            _cp(energies), _p(norms, C.c_double), _cp(stored))
    if cplx:
        _ck(l.pepshost_fermion_optimize_exact_sum_c128(*head, chi, *rest))
    else:
        _ck(l.pepshost_fermion_optimize_exact_sum(*head, chi, dtype, *rest))
    return (energies, stored, norms) if return_grad_norms else (energies, stored)


def fermion_lbfgs_optimize_exact_sum(state, cfgs, chi, model, params, lr, lbfgs, iterations, energy_tolerance=0.0, gradient_tolerance=0.0,
                                     plateau_patience=0, dtype=1, batch=64):
    """lbfgs_optimize_exact_sum on a fermionic state (peps_amd.fermion.FermionState); model and params as fermion_optimize_exact_sum.
    "state" of the result holds the stored tensors [rows][cols][d][D^4]; the gradient norms and every threshold of LBFGSParams are over
    the stored parameters."""
    cplx, flat, nf, par, head = _fermion_head(state, dtype)
    cfg = np.ascontiguousarray(cfgs, dtype=np.int32)
    prm = _fermion_prm(model, params)
    lb = _lbfgs_array(lbfgs)
    energies = np.zeros(iterations + 1, dtype=flat.dtype)
    norms, steps, info = np.zeros(iterations + 1), np.zeros(max(iterations, 1)), np.zeros(8)
    stored = np.zeros((flat.shape[0], flat.shape[1], state.d) + flat.shape[3:], dtype=flat.dtype)
    l = lib()
    dpt, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    tail = [dpt, i32, C.c_int, C.c_int, dpt, C.c_int, C.c_double, dpt, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, dpt, dpt, dpt, dpt, dpt]
    lead = [C.c_int] * 4 + [i32, C.POINTER(C.c_uint8), C.c_int]
    l.pepshost_fermion_lbfgs_exact_sum.argtypes = lead + [C.c_int] + tail
    l.pepshost_fermion_lbfgs_exact_sum_c128.argtypes = lead + tail
    rest = (_cp(flat), _p(cfg, C.c_int32), cfg.shape[0], FERMION_MODEL_ID[model], _p(prm, C.c_double), prm.size, float(lr),
            _p(lb, C.c_double), int(iterations), float(energy_tolerance), float(gradient_tolerance), int(plateau_patience),
            int(min(batch, cfg.shape[0])), _cp(energies), _p(norms, C.c_double), _p(steps, C.c_double), _cp(stored), _p(info, C.c_double))
    if cplx:
        rc = l.pepshost_fermion_lbfgs_exact_sum_c128(*head, chi, *rest)
    else:
        rc = l.pepshost_fermion_lbfgs_exact_sum(*head, chi, dtype, *rest)
    return _lbfgs_result(rc, energies, norms, steps, stored, info)


def fermion_sr_step_samples(state, configs, chi, model, params, lr, diag_shift=0.001, cg_max_iter=100, cg_relative_tolerance=1e-4,
                            normalize_update=False, dtype=1):
    """sr_step_samples on a fermionic state: the natural gradient is solved in the stored parameters on the device.  Returns (stored
    tensors after the step [rows][cols][d][D^4], dict as sr_step_samples; the norms are over the stored parameters)."""
    cplx, flat, nf, par, head = _fermion_head(state, dtype)
    cfg = np.ascontiguousarray(configs, dtype=np.int32)
    prm = _fermion_prm(model, params)
    stored = np.zeros((flat.shape[0], flat.shape[1], state.d) + flat.shape[3:], dtype=flat.dtype)
    info = np.zeros(5)
    l = lib()
    dpt, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    tail = [dpt, C.c_int, i32, C.c_int, dpt, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, dpt, dpt]
    lead = [C.c_int] * 4 + [i32, C.POINTER(C.c_uint8), C.c_int]
    l.pepshost_fermion_sr_step_samples.argtypes = lead + [C.c_int] + tail
    l.pepshost_fermion_sr_step_samples_c128.argtypes = lead + tail
    rest = (_cp(flat), cfg.shape[0], _p(cfg, C.c_int32), FERMION_MODEL_ID[model], _p(prm, C.c_double), prm.size, float(lr), float(diag_shift),
            int(cg_max_iter), float(cg_relative_tolerance), int(bool(normalize_update)), _cp(stored), _p(info, C.c_double))
    if cplx:
        _ck(l.pepshost_fermion_sr_step_samples_c128(*head, chi, *rest))
    else:
        _ck(l.pepshost_fermion_sr_step_samples(*head, chi, dtype, *rest))
    return stored, {"energy_before": info[0], "energy_after": info[1], "cg_iterations": int(info[2]), "direction_norm": info[3],
                    "cg_residual_norm": info[4]}


# ---- Monte-Carlo VMC on the resident state: MCEnergyGradEvaluator and VMCPEPSOptimizer of the host layer ----
VMC_ALGO_ID = {"sgd": 0, "adagrad": 1, "adam": 2, "sr": 3, "minsr": 4, "lbfgs": 5}   # rule_params: sgd / adagrad / adam as RULE_ID;
# sr (diag_shift, cg_max_iter, cg_relative_tolerance, normalize_update); minsr (r_pinv, a_pinv, soft_cutoff); lbfgs: a dict of LBFGS_FIELDS


def binned_energy_stat(samples):
    """MeanAndBinnedErrorSqrtNUniformBin of the host layer on samples[sample][walker] (a walker plays the role of an MPI rank): per
    walker bins of max(1, floor(sqrt(S))) samples, trailing samples dropped, bin means gathered walker-major; returns (mean of the bin
    means, their standard error; inf for one bin in total).  Needs no device."""
    cplx = np.iscomplexobj(samples)
    a = np.ascontiguousarray(samples, dtype=np.complex128 if cplx else np.float64)
    if a.ndim != 2:
        raise ValueError("samples must be [sample][walker]")
    mean, err = np.zeros(2), C.c_double(0.0)
    l = lib()
    l.pepshost_binned_energy_stat.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    _ck(l.pepshost_binned_energy_stat(_cp(a), a.shape[0], a.shape[1], int(cplx), _p(mean, C.c_double), C.byref(err)))
    return (complex(mean[0], mean[1]) if cplx else float(mean[0])), err.value


def _vmc_rule(algo, rule_params):
    aid = VMC_ALGO_ID[algo] if isinstance(algo, str) else int(algo)
    rp = _lbfgs_array(rule_params) if aid == 5 else np.ascontiguousarray([float(x) for x in rule_params], dtype=np.float64)
    return aid, rp


def _vmc_result(energies, errors, norms, accept, state, lowest, probe, info, cfg):
    ne = int(info[0])
    return {"energies": energies[:ne], "energy_errors": errors[:ne], "grad_norms": norms[:ne], "accept_rates": accept[:ne], "state": state,
            "lowest_state": lowest, "min_energy": float(info[1]), "max_abs_psi": float(info[2]), "current_energy": float(info[3]),
            "configs": cfg, "probe_state": probe,
            "timings": {"evaluation_s": float(info[4]), "optimize_s": float(info[5]), "total_s": float(info[6])}}


def _vmc_paths(tps_dump_base_name, energy_dir, config_dump_path):
    return tuple((x or "").encode() for x in (tps_dump_base_name, energy_dir, config_dump_path))


def vmc_optimize(flat, configs, seeds, chi, model, params, updater, algo, lr, rule_params, iterations, warmup_sweeps=0, samples_per_walker=1,
                 sweeps_between_samples=1, clip_value=0.0, clip_norm=0.0, dtype=1, finalize=True, probe_iteration=-1, tps_dump_base_name="",
                 energy_dir="", config_dump_path=""):
    """VMCPEPSOptimizer::Execute of the C++ host layer in one call: the state is uploaded once; WarmUp (sweeps, one normalisation on the
    device), then Optimizer::IterativeOptimize with MCEnergyGradEvaluator on persistent chains (one mt19937 per walker, `seeds`), the
    closing refresh + normalisation and DumpData.  Returns a dict: energies / energy_errors / grad_norms [iterations + 1], accept_rates
    [iterations + 1][walker], state (final), lowest_state (the parameters of the lowest energy, snapshotted in HBM), min_energy,
    max_abs_psi (over the walkers at return), configs (final).  A complex `flat` runs the QLTEN_Complex instantiation.  finalize=False
    stops before the closing normalisation; probe_iteration >= 0 reads the state inside an OptimizationCallback at that iteration.
    energy_dir="" writes no energy_trajectory.csv (the reference writes ./energy)."""
    cplx = np.iscomplexobj(flat)
    flat = np.ascontiguousarray(flat, dtype=np.complex128 if cplx else np.float64)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(configs, dtype=np.int32).reshape(-1, rows, cols).copy()
    n = cfg.shape[0]
    sd = np.ascontiguousarray(seeds, dtype=np.uint64).ravel()
    p = np.array(list(params) + [0.0] * 8, dtype=np.float64)
    aid, rp = _vmc_rule(algo, rule_params)
    mc = np.array([warmup_sweeps, samples_per_walker, sweeps_between_samples], dtype=np.float64)
    opt = np.array([aid, lr, iterations, clip_value, clip_norm, int(bool(finalize)), probe_iteration], dtype=np.float64)
    ne = int(iterations) + 1
    energies = np.zeros(ne, dtype=flat.dtype)
    errors, norms, accept, info = np.zeros(ne), np.zeros(ne), np.zeros((ne, max(n, 1))), np.zeros(8)
    state, lowest = np.zeros_like(flat), np.zeros_like(flat)
    probe = np.zeros_like(flat) if probe_iteration >= 0 else None
    l = lib()
    dpt, i32, cs = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_char_p
    tail = [dpt, C.c_int, i32, C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int, dpt, dpt, dpt, dpt, C.c_int, cs, cs, cs] + [dpt] * 8
    l.pepshost_vmc_optimize.argtypes = [C.c_int] * 6 + tail
    l.pepshost_vmc_optimize_c128.argtypes = [C.c_int] * 5 + tail
    rest = (_cp(flat), n, _p(cfg, C.c_int32), _p(sd, C.c_uint64), sd.size, UPDATER_ID[updater], MODEL_ID[model], _p(p, C.c_double),
            _p(mc, C.c_double), _p(opt, C.c_double), _p(rp, C.c_double), rp.size, *_vmc_paths(tps_dump_base_name, energy_dir, config_dump_path),
            _cp(energies), _p(errors, C.c_double), _p(norms, C.c_double), _p(accept, C.c_double), _cp(state), _cp(lowest),
            _cp(probe) if probe is not None else None, _p(info, C.c_double))
    if cplx:
        _ck(l.pepshost_vmc_optimize_c128(rows, cols, D, d, chi, *rest))
    else:
        _ck(l.pepshost_vmc_optimize(rows, cols, D, d, chi, dtype, *rest))
    return _vmc_result(energies, errors, norms, accept, state, lowest, probe, info, cfg)


def fermion_vmc_optimize(state, configs, seeds, chi, model, params, updater, algo, lr, rule_params, iterations, warmup_sweeps=0,
                         samples_per_walker=1, sweeps_between_samples=1, clip_value=0.0, clip_norm=0.0, dtype=1, finalize=True,
                         probe_iteration=-1, tps_dump_base_name="", energy_dir="", config_dump_path=""):
    """vmc_optimize on a fermionic state (peps_amd.fermion.FermionState): model "spinless" / "tj" / "hubbard" with params as
    fermion_optimize_exact_sum, updater "exchange", "tnn3" or (Hubbard only) "hubbard_u1u1".  The states of the result are the stored
    tensors [rows][cols][d][D^4]."""
    cplx, flat, nf, par, head = _fermion_head(state, dtype)
    rows, cols = flat.shape[0], flat.shape[1]
    cfg = np.ascontiguousarray(configs, dtype=np.int32).reshape(-1, rows, cols).copy()
    n = cfg.shape[0]
    sd = np.ascontiguousarray(seeds, dtype=np.uint64).ravel()
    prm = _fermion_prm(model, params)
    aid, rp = _vmc_rule(algo, rule_params)
    mc = np.array([warmup_sweeps, samples_per_walker, sweeps_between_samples], dtype=np.float64)
    opt = np.array([aid, lr, iterations, clip_value, clip_norm, int(bool(finalize)), probe_iteration], dtype=np.float64)
    ne = int(iterations) + 1
    energies = np.zeros(ne, dtype=flat.dtype)
    errors, norms, accept, info = np.zeros(ne), np.zeros(ne), np.zeros((ne, max(n, 1))), np.zeros(8)
    shape = (rows, cols, state.d) + flat.shape[3:]
    stored, lowest = np.zeros(shape, dtype=flat.dtype), np.zeros(shape, dtype=flat.dtype)
    probe = np.zeros(shape, dtype=flat.dtype) if probe_iteration >= 0 else None
    l = lib()
    dpt, i32, cs = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_char_p
    l.pepshost_fermion_vmc_optimize.argtypes = ([C.c_int] * 4 + [i32, C.POINTER(C.c_uint8), C.c_int, C.c_int, dpt, C.c_int, i32, C.POINTER(C.c_uint64),
                                                 C.c_int, C.c_int, C.c_int, dpt, C.c_int, dpt, dpt, dpt, C.c_int, cs, cs, cs] + [dpt] * 8)
    _ck(l.pepshost_fermion_vmc_optimize(*head, chi, _C128 if cplx else dtype, _cp(flat), n, _p(cfg, C.c_int32), _p(sd, C.c_uint64), sd.size,
                                        FERMION_UPDATER_ID[updater], FERMION_MODEL_ID[model], _p(prm, C.c_double), prm.size, _p(mc, C.c_double),
                                        _p(opt, C.c_double), _p(rp, C.c_double), rp.size,
                                        *_vmc_paths(tps_dump_base_name, energy_dir, config_dump_path), _cp(energies), _p(errors, C.c_double),
                                        _p(norms, C.c_double), _p(accept, C.c_double), _cp(stored), _cp(lowest),
                                        _cp(probe) if probe is not None else None, _p(info, C.c_double)))
    return _vmc_result(energies, errors, norms, accept, stored, lowest, probe, info, cfg)


def mc_evaluate_resident(state, configs, seeds, chi, model, params, updater="exchange", warmup_sweeps=0, n_samples=1, n_evaluates=1,
                         normalize=False, collect_sr=False, dtype=1, step=None):
    """MCEnergyGradEvaluator::Evaluate alone on the resident state, `n_evaluates` times on one engine with no step between them (the
    chains persist).  `state`: a flat bosonic array (real or complex) or a peps_amd.fermion.FermionState.  Warm-up: the plain sweeps, or
    MonteCarloEngine::WarmUp (with its normalisation on the device) when normalize.  Returns a dict with, per evaluation: energy_samples
    [k][sample][walker], S_O / S_EO [k][...] (pepsgpu_grad_read), e_loc_sum, weight_sum, energy_error, sr_count, accept_rates [k][walker];
    configs (final).  step = dict(algo, lr, rule_params[, clip_value, clip_norm]): after the last evaluation the optimizer step is composed
    by hand on the contractor (finish, clip, natural gradient / MinSR direction, step); "state" is then theta read back, "step_energy" and
    "step_grad_norm" what the finish returned."""
    fermion = hasattr(state, "extended_flat")
    if fermion:
        cplx, flat, nf, par, head = _fermion_head(state, dtype)
        rows, cols, D, d = flat.shape[0], flat.shape[1], flat.shape[3], state.d
        prm = _fermion_prm(model, params)
        uid, mid = FERMION_UPDATER_ID[updater], FERMION_MODEL_ID[model]
        nfp, parp = _p(nf, C.c_int32), par.ctypes.data_as(C.POINTER(C.c_uint8))
    else:
        cplx = np.iscomplexobj(state)
        flat = np.ascontiguousarray(state, dtype=np.complex128 if cplx else np.float64)
        rows, cols, d, D = _dims(flat)
        prm = np.array(list(params) + [0.0] * 8, dtype=np.float64)
        uid, mid = UPDATER_ID[updater], MODEL_ID[model]
        nfp, parp = None, None
    cfg = np.ascontiguousarray(configs, dtype=np.int32).reshape(-1, rows, cols).copy()
    n = cfg.shape[0]
    sd = np.ascontiguousarray(seeds, dtype=np.uint64).ravel()
    if sd.size != n:
        raise ValueError("one seed per walker")
    et = flat.dtype
    es = np.zeros((n_evaluates, n_samples, n), dtype=et)
    so, seo = np.zeros((n_evaluates,) + flat.shape, dtype=et), np.zeros((n_evaluates,) + flat.shape, dtype=et)
    sc, acc = np.zeros((n_evaluates, 5)), np.zeros((n_evaluates, n))
    opt = rp = theta = None
    sinfo = np.zeros(2)
    if step is not None:
        aid, rp = _vmc_rule(step["algo"], step["rule_params"])
        opt = np.array([aid, step["lr"], 0, step.get("clip_value", 0.0), step.get("clip_norm", 0.0)], dtype=np.float64)
        theta = np.zeros((rows, cols, d) + flat.shape[3:], dtype=et)
    l = lib()
    dpt, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    l.pepshost_mc_evaluate_resident.argtypes = ([C.c_int] * 4 + [i32, C.POINTER(C.c_uint8), C.c_int, C.c_int, dpt, C.c_int, i32, C.POINTER(C.c_uint64),
                                                 C.c_int, C.c_int, dpt] + [C.c_int] * 6 + [dpt, dpt, C.c_int] + [dpt] * 7)
    _ck(l.pepshost_mc_evaluate_resident(rows, cols, D, d, nfp, parp, chi, _C128 if cplx else dtype, _cp(flat), n, _p(cfg, C.c_int32),
                                        _p(sd, C.c_uint64), uid, mid, _p(prm, C.c_double), prm.size, int(warmup_sweeps), int(bool(normalize)),
                                        int(n_samples), int(n_evaluates), int(bool(collect_sr)), _p(opt, C.c_double), _p(rp, C.c_double),
                                        rp.size if rp is not None else 0, _cp(es), _cp(so), _cp(seo), _p(sc, C.c_double), _p(acc, C.c_double),
                                        _cp(theta) if theta is not None else None, _p(sinfo, C.c_double)))
    e_sum = sc[:, 0] + 1j * sc[:, 1] if cplx else sc[:, 0].copy()
    out = {"energy_samples": es, "S_O": so, "S_EO": seo, "e_loc_sum": e_sum, "weight_sum": sc[:, 2].copy(), "energy_error": sc[:, 3].copy(),
           "sr_count": sc[:, 4].astype(int), "accept_rates": acc, "configs": cfg}
    if step is not None:
        out.update(state=theta, step_energy=float(sinfo[0]), step_grad_norm=float(sinfo[1]))
    return out


# ---- spike recovery, step selectors and checkpoints (qlpeps_gpu.h: SpikeGuard, OptimizerParams; pepshost.cpp: GuardSpec) ----
SPIKE_SIGNALS = ("NONE", "S1_ERRORBAR", "S2_GRAD_NORM", "S3_NGRAD_ANOMALY", "S4_ENERGY_SPIKE")      # SignalName
SPIKE_ACTIONS = ("ACCEPT", "RESAMPLE", "ROLLBACK", "ACCEPT_WARN")                                    # ActionName
# SpikeRecoveryParams, optimizer_params.h:299-313 (the reference's defaults)
SPIKE_DEFAULTS = dict(enable_auto_recover=True, redo_mc_max_retries=2, factor_err=100.0, factor_grad=1e10, factor_ngrad=10.0,
                      sr_min_iters_suspicious=1, enable_rollback=False, ema_window=50, sigma_k=10.0, log_trigger_csv_path="")
# InitialStepSelectorParams / PeriodicStepSelectorParams, :164-184
SELECTOR_DEFAULTS = dict(initial=dict(enabled=False, max_line_search_steps=3, enable_in_deterministic=False),
                         periodic=dict(enabled=False, every_n_steps=10, phase_switch_ratio=0.3, enable_in_deterministic=False))


def _guard_array(spike, selectors, checkpoint, scheduler=None, energy_tolerance=0.0, gradient_tolerance=0.0, plateau_patience=0,
                 probe_iteration=-1, events_cap=0):
    """the 24 doubles of the shim's GuardSpec and the two paths.  spike=None: recovery off (what the two-argument OptimizerParams
    constructor of this tree gives); a dict: the reference's defaults with the given fields replaced."""
    sp = dict(SPIKE_DEFAULTS)
    if spike is None:
        sp["enable_auto_recover"] = False
    else:
        unknown = set(spike) - set(sp)
        if unknown:
            raise ValueError("unknown spike fields %s" % sorted(unknown))
        sp.update(spike)
    sel = {k: dict(v) for k, v in SELECTOR_DEFAULTS.items()}
    for k, v in (selectors or {}).items():
        if k not in sel or set(v) - set(sel[k]):
            raise ValueError("selectors = dict(initial=dict(...), periodic=dict(...)) with the fields of %s" % (SELECTOR_DEFAULTS,))
        sel[k].update(v)
        if "enabled" not in v:                              # naming a selector enables it
            sel[k]["enabled"] = True
    ck = dict(every_n_steps=0, base_path="")
    ck.update(checkpoint or {})
    ini, per = sel["initial"], sel["periodic"]
    g = np.array([sp["enable_auto_recover"], sp["redo_mc_max_retries"], sp["factor_err"], sp["factor_grad"], sp["factor_ngrad"],
                  sp["sr_min_iters_suspicious"], sp["enable_rollback"], sp["ema_window"], sp["sigma_k"],
                  ini["enabled"], ini["max_line_search_steps"], ini["enable_in_deterministic"],
                  per["enabled"], per["every_n_steps"], per["phase_switch_ratio"], per["enable_in_deterministic"],
                  ck["every_n_steps"], 1.0 if scheduler else 0.0, energy_tolerance, gradient_tolerance, plateau_patience, probe_iteration,
                  events_cap, 0.0], dtype=np.float64)
    return g, sp["log_trigger_csv_path"].encode(), ck["base_path"].encode()


def _schedule_arrays(schedule):
    if not schedule:
        return None, None, 0
    eo, es = schedule.get("error_override"), schedule.get("energy_shift")
    n = len(eo) if eo is not None else len(es)
    eo = np.full(n, np.nan) if eo is None else np.ascontiguousarray(eo, dtype=np.float64)
    es = np.zeros(n) if es is None else np.ascontiguousarray(es, dtype=np.float64)
    if eo.size != n or es.size != n:
        raise ValueError("error_override and energy_shift have one entry per evaluator call")
    return eo, es, n


def _events(ev, n):
    return [dict(step=int(e[0]), attempt=int(e[1]), signal=SPIKE_SIGNALS[int(e[2])], action=SPIKE_ACTIONS[int(e[3])], value=float(e[4]),
                 threshold=float(e[5])) for e in ev[:n]]


def ema_track(series, window, reset_at=-1):
    """EMATracker(window) of the host layer fed with `series`: (mean, var) after every Update.  reset_at >= 0 calls Reset() before that
    observation.  Needs no device."""
    a = np.ascontiguousarray(series, dtype=np.float64).ravel()
    mean, var = np.zeros(a.size), np.zeros(a.size)
    l = lib()
    dpt = C.POINTER(C.c_double)
    l.pepshost_ema_track.argtypes = [dpt, C.c_int, C.c_long, C.c_int, dpt, dpt]
    _ck(l.pepshost_ema_track(_p(a, C.c_double), a.size, int(window), int(reset_at), _p(mean, C.c_double), _p(var, C.c_double)))
    return mean, var


def spike_replay(records, algo, spike_params=None):
    """The optimizer's own detect / decide / EMA code (SpikeGuard) on a scripted list of evaluations (energy, error, grad_norm,
    ngrad_norm, cg_iters), in the order IterativeOptimize would make them: a rejected evaluation is followed by the next record at the
    same iteration.  algo "sr" judges S3 with the CG iterations, "minsr" on the norm only, any other rule has no S3.  Returns a dict:
    actions / iterations per record, ema [record][energy, error, grad, ngrad][mean, var], events, total_resamples / total_rollbacks /
    total_forced_accepts, csv (the trigger CSV as text).  Needs no device."""
    rec = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 5)
    n = rec.shape[0]
    aid = VMC_ALGO_ID[algo] if isinstance(algo, str) else int(algo)
    g, _, _ = _guard_array(dict(spike_params or {}), None, None)
    actions, iters = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    ema, cap = np.zeros((n, 4, 2)), 3 * n + 8
    ev, counts = np.zeros((cap, 6)), np.zeros(4)
    csv = C.create_string_buffer(256 * (cap + 1))
    l = lib()
    dpt, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    l.pepshost_spike_replay.argtypes = [dpt, C.c_int, C.c_int, dpt, i32, i32, dpt, dpt, C.c_int, dpt, C.c_char_p, C.c_long]
    _ck(l.pepshost_spike_replay(_p(rec, C.c_double), n, aid, _p(g, C.c_double), _p(actions, C.c_int32), _p(iters, C.c_int32),
                                _p(ema, C.c_double), _p(ev, C.c_double), cap, _p(counts, C.c_double), csv, len(csv)))
    return {"actions": [SPIKE_ACTIONS[a] for a in actions], "iterations": iters, "ema": ema, "events": _events(ev, int(counts[0])),
            "total_resamples": int(counts[1]), "total_rollbacks": int(counts[2]), "total_forced_accepts": int(counts[3]),
            "csv": csv.value.decode()}


def acceptance_rate_check(rates):
    """AcceptanceRateCheck of the evaluator (a walker plays the rank): the indices of the walkers whose rate is below half the maximum."""
    a = np.ascontiguousarray(rates, dtype=np.float64).ravel()
    flags = np.zeros(max(a.size, 1), dtype=np.int32)
    l = lib()
    l.pepshost_acceptance_rate_check.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32)]
    _ck(l.pepshost_acceptance_rate_check(_p(a, C.c_double), a.size, _p(flags, C.c_int32)))
    return [int(w) for w in np.nonzero(flags[:a.size])[0]]


def step_select(kind, results, iter, max_iter, base_lr, ratio=0.3):
    """The selection rule of the "initial" / "periodic" step selector on trial results [(eta, energy, error), ...]; returns (selected
    eta, the selector's base learning rate afterwards).  Needs no device."""
    r = np.ascontiguousarray(results, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(2)
    l = lib()
    dpt = C.POINTER(C.c_double)
    l.pepshost_step_select.argtypes = [C.c_int, dpt, C.c_int, C.c_long, C.c_long, C.c_double, C.c_double, dpt]
    _ck(l.pepshost_step_select({"initial": 0, "periodic": 1}[kind], _p(r, C.c_double), r.shape[0], int(iter), int(max_iter), float(base_lr),
                               float(ratio), _p(out, C.c_double)))
    return float(out[0]), float(out[1])


def step_candidates(kind, base_lr, max_line_search_steps=3):
    """the learning rates a selector tries from base_lr: "initial" base_lr * 1 .. max_line_search_steps, "periodic" (base_lr, base_lr / 2)"""
    out, n = np.zeros(max(int(max_line_search_steps), 2)), C.c_int(0)
    l = lib()
    l.pepshost_step_candidates.argtypes = [C.c_int, C.c_double, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
    _ck(l.pepshost_step_candidates({"initial": 0, "periodic": 1}[kind], float(base_lr), int(max_line_search_steps), _p(out, C.c_double),
                                   out.size, C.byref(n)))
    return out[:n.value].copy()


def validate_guards(algo, lr, rule_params, spike=None, selectors=None, scheduler=None, n_walkers=None, n_seeds=None, samples_per_walker=1):
    """OptimizerParams::ValidateGuards (n_walkers None) or VMCPEPSOptimizerParams::Validate for these settings: raises ValueError with the
    optimizer's message, before and without any device call."""
    aid, rp = _vmc_rule(algo, rule_params)
    g, _, _ = _guard_array(spike, selectors, None, scheduler=scheduler)
    l = lib()
    dpt = C.POINTER(C.c_double)
    l.pepshost_validate_guards.argtypes = [C.c_int, dpt, C.c_int, C.c_double, dpt, C.c_int, C.c_int, C.c_int]
    nw = -1 if n_walkers is None else int(n_walkers)
    _ck(l.pepshost_validate_guards(aid, _p(rp, C.c_double), rp.size, float(lr), _p(g, C.c_double), nw,
                                   nw if n_seeds is None else int(n_seeds), int(samples_per_walker)))


def _guarded_result(energies, errors, norms, eta, ev, state, lowest, probe, info):
    ne, nev = int(info[0]), int(info[1])
    out = {"energies": energies[:ne], "energy_errors": errors[:ne], "grad_norms": norms[:ne], "selected_eta": eta[:int(info[13])],
           "events": _events(ev, min(nev, ev.shape[0])), "n_events": nev, "total_resamples": int(info[2]), "total_rollbacks": int(info[3]),
           "total_forced_accepts": int(info[4]), "evaluator_calls": int(info[5]), "energy_only_calls": int(info[6]),
           "total_iterations": int(info[7]), "converged": bool(info[8]), "min_energy": float(info[9]), "sr_iterations": int(info[10]),
           "sr_natural_grad_norm": float(info[11]), "sr_residual_norm": float(info[12]), "state": state,
           "lowest_state": lowest if info[14] else None, "probe_state": probe}
    return out


class GuardedRunError(RuntimeError):
    """the guarded loop threw (a non-finite selector trial, an exhausted schedule): .state = theta as the optimizer was left with,
    .evaluator_calls = evaluator calls made"""


def _guarded_exact_sum(head, fermion, cplx, dtype, flat, stored_shape, cfgs, chi, mid, prm, algo, lr, rule_params, iterations, clip_value,
                       clip_norm, batch, spike, selectors, checkpoint, schedule, scheduler, energy_tolerance, gradient_tolerance,
                       plateau_patience, probe_iteration):
    cfg = np.ascontiguousarray(cfgs, dtype=np.int32)
    aid, rp = _vmc_rule(algo, rule_params)
    eo, es, ns = _schedule_arrays(schedule)
    cap = 4 * (int(iterations) + ns) + 16
    g, csv, ckp = _guard_array(spike, selectors, checkpoint, scheduler, energy_tolerance, gradient_tolerance, plateau_patience, probe_iteration, cap)
    opt = np.array([aid, lr, iterations, clip_value, clip_norm], dtype=np.float64)
    ne = int(iterations) + 1
    et = flat.dtype
    energies = np.zeros(ne, dtype=et)
    errors, norms, eta, ev, info = np.zeros(ne), np.zeros(ne), np.zeros(ne), np.zeros((cap, 6)), np.zeros(16)
    state, lowest = np.zeros(stored_shape, dtype=et), np.zeros(stored_shape, dtype=et)
    probe = np.zeros(stored_shape, dtype=et) if probe_iteration >= 0 else None
    l = lib()
    dpt, i32, cs = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_char_p
    l.pepshost_guarded_optimize_exact_sum.argtypes = ([C.c_int] * 4 + [i32, C.POINTER(C.c_uint8), C.c_int, C.c_int, dpt, i32, C.c_int, C.c_int, dpt,
                                                       C.c_int, dpt, dpt, C.c_int, C.c_int, dpt, cs, cs, dpt, dpt, C.c_int] + [dpt] * 9)
    rc = l.pepshost_guarded_optimize_exact_sum(*head, chi, _C128 if cplx else dtype, _cp(flat), _p(cfg, C.c_int32), cfg.shape[0], mid,
                                               _p(prm, C.c_double), prm.size, _p(opt, C.c_double), _p(rp, C.c_double), rp.size,
                                               int(min(batch, cfg.shape[0])), _p(g, C.c_double), csv, ckp, _p(eo, C.c_double),
                                               _p(es, C.c_double), ns, _cp(energies), _p(errors, C.c_double), _p(norms, C.c_double),
                                               _p(eta, C.c_double), _p(ev, C.c_double), _cp(state), _cp(lowest),
                                               _cp(probe) if probe is not None else None, _p(info, C.c_double))
    if rc not in (0, 1):                                    # (1: a refusal before the loop, nothing to report)
        err = GuardedRunError("pepshost error %d: %s" % (rc, l.pepshost_last_error().decode()))
        err.state, err.evaluator_calls = state, int(info[5])
        raise err
    _ck(rc)
    return _guarded_result(energies, errors, norms, eta, ev, state, lowest, probe, info)


def guarded_optimize_exact_sum(flat, all_configs, chi, model, params, algo, lr, rule_params, iterations, spike=None, selectors=None,
                               checkpoint=None, schedule=None, clip_value=0.0, clip_norm=0.0, dtype=1, batch=64, scheduler=None,
                               energy_tolerance=0.0, gradient_tolerance=0.0, plateau_patience=0, probe_iteration=-1):
    """Optimizer::IterativeOptimize with spike recovery, step selectors and checkpoints on a fixed set of configurations, the whole loop in
    one C++ call.  algo "sgd" / "adagrad" / "adam" / "lbfgs" evaluate by exact summation over all_configs (optimize_exact_sum); "sr" /
    "minsr" take all_configs as a sample set of weight 1 (sr_step_samples, minsr_step_samples).  A complex `flat` runs the QLTEN_Complex
    instantiation.
      spike      None: recovery off; dict(...): SpikeRecoveryParams, the reference's defaults with these fields replaced
      selectors  dict(initial=dict(...), periodic=dict(...)): naming one enables it
      checkpoint dict(every_n_steps, base_path)
      schedule   dict(error_override=[...], energy_shift=[...]), one entry per evaluator call: the error bar is replaced where the entry
                 is not NaN, energy_shift * weight_sum is added to e_loc_sum (energy and gradient move); a call beyond the schedule raises
      scheduler  True: a ConstantLR scheduler at lr (what a step selector refuses)
    Returns a dict: energies / energy_errors / grad_norms of the accepted evaluations, selected_eta per iteration (0 where no selector
    ran), events (dicts step, attempt, signal, action, value, threshold) and the three counters, evaluator_calls, state (final),
    lowest_state, min_energy, probe_state (theta at on_iteration of probe_iteration), SR diagnostics.  A throw from the loop raises
    GuardedRunError carrying the state."""
    cplx = np.iscomplexobj(flat)
    flat = np.ascontiguousarray(flat, dtype=np.complex128 if cplx else np.float64)
    rows, cols, d, D = _dims(flat)
    prm = np.array(list(params) + [0.0] * 8, dtype=np.float64)
    return _guarded_exact_sum((rows, cols, D, d, None, None), False, cplx, dtype, flat, flat.shape, all_configs, chi, MODEL_ID[model], prm, algo,
                              lr, rule_params, iterations, clip_value, clip_norm, batch, spike, selectors, checkpoint, schedule, scheduler,
                              energy_tolerance, gradient_tolerance, plateau_patience, probe_iteration)


def fermion_guarded_optimize_exact_sum(state, all_configs, chi, model, params, algo, lr, rule_params, iterations, spike=None, selectors=None,
                                       checkpoint=None, schedule=None, clip_value=0.0, clip_norm=0.0, dtype=1, batch=64, scheduler=None,
                                       energy_tolerance=0.0, gradient_tolerance=0.0, plateau_patience=0, probe_iteration=-1):
    """guarded_optimize_exact_sum on a fermionic state (peps_amd.fermion.FermionState); model and params as fermion_optimize_exact_sum;
    the states of the result are the stored tensors [rows][cols][d][D^4]."""
    cplx, flat, nf, par, head = _fermion_head(state, dtype)
    shape = (flat.shape[0], flat.shape[1], state.d) + flat.shape[3:]
    return _guarded_exact_sum(head, True, cplx, dtype, flat, shape, all_configs, chi, FERMION_MODEL_ID[model], _fermion_prm(model, params), algo,
                              lr, rule_params, iterations, clip_value, clip_norm, batch, spike, selectors, checkpoint, schedule, scheduler,
                              energy_tolerance, gradient_tolerance, plateau_patience, probe_iteration)


def guarded_vmc_optimize(flat, configs, seeds, chi, model, params, updater, algo, lr, rule_params, iterations, warmup_sweeps=0,
                         samples_per_walker=1, sweeps_between_samples=1, spike=None, selectors=None, checkpoint=None, schedule=None,
                         clip_value=0.0, clip_norm=0.0, dtype=1, scheduler=None):
    """VMCPEPSOptimizer::WarmUpAndOptimize with spike recovery, step selectors and checkpoints (no closing normalisation, no dumps);
    spike / selectors / checkpoint / schedule / scheduler as guarded_optimize_exact_sum.  The schedule wraps the executor's own
    evaluator; the selector trials use its energy-only variant.  Every refusal of VMCPEPSOptimizerParams::Validate is raised before
    any device call.  Returns the dict of guarded_optimize_exact_sum plus accept_rates [accepted evaluation][walker] and configs; the
    trajectories, lowest_state and min_energy are the executor's own (accepted evaluations only)."""
    cplx = np.iscomplexobj(flat)
    flat = np.ascontiguousarray(flat, dtype=np.complex128 if cplx else np.float64)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(configs, dtype=np.int32).reshape(-1, rows, cols).copy()
    n = cfg.shape[0]
    sd = np.ascontiguousarray(seeds, dtype=np.uint64).ravel()
    p = np.array(list(params) + [0.0] * 8, dtype=np.float64)
    aid, rp = _vmc_rule(algo, rule_params)
    eo, es, ns = _schedule_arrays(schedule)
    cap = 4 * (int(iterations) + ns) + 16
    g, csv, ckp = _guard_array(spike, selectors, checkpoint, scheduler, events_cap=cap)
    mc = np.array([warmup_sweeps, samples_per_walker, sweeps_between_samples], dtype=np.float64)
    opt = np.array([aid, lr, iterations, clip_value, clip_norm, 0, -1], dtype=np.float64)
    ne = int(iterations) + 1
    energies = np.zeros(ne, dtype=flat.dtype)
    errors, norms, eta, ev, info = np.zeros(ne), np.zeros(ne), np.zeros(ne), np.zeros((cap, 6)), np.zeros(16)
    accept = np.zeros((ne, max(n, 1)))
    state, lowest = np.zeros_like(flat), np.zeros_like(flat)
    l = lib()
    dpt, i32, cs = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_char_p
    l.pepshost_guarded_vmc_optimize.argtypes = ([C.c_int] * 4 + [i32, C.POINTER(C.c_uint8), C.c_int, C.c_int, dpt, C.c_int, i32, C.POINTER(C.c_uint64),
                                                 C.c_int, C.c_int, C.c_int, dpt, C.c_int, dpt, dpt, dpt, C.c_int, dpt, cs, cs, dpt, dpt, C.c_int]
                                                + [dpt] * 9)
    _ck(l.pepshost_guarded_vmc_optimize(rows, cols, D, d, None, None, chi, _C128 if cplx else dtype, _cp(flat), n, _p(cfg, C.c_int32),
                                        _p(sd, C.c_uint64), sd.size, UPDATER_ID[updater], MODEL_ID[model], _p(p, C.c_double), 8,
                                        _p(mc, C.c_double), _p(opt, C.c_double), _p(rp, C.c_double), rp.size, _p(g, C.c_double), csv, ckp,
                                        _p(eo, C.c_double), _p(es, C.c_double), ns, _cp(energies), _p(errors, C.c_double),
                                        _p(norms, C.c_double), _p(eta, C.c_double), _p(ev, C.c_double), _p(accept, C.c_double), _cp(state),
                                        _cp(lowest), _p(info, C.c_double)))
    out = _guarded_result(energies, errors, norms, eta, ev, state, lowest, None, info)
    out.update(accept_rates=accept[:int(info[0])], configs=cfg)
    return out


# ---- TenElemT = QLTEN_Complex (std::complex<double>): the same host classes instantiated for the complex element type ----
def _cflat(flat):
    return np.ascontiguousarray(flat, dtype=np.complex128)


def _cp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def load_sitps_complex(directory, D):
    rows, cols, d = C.c_int(0), C.c_int(0), C.c_int(0)
    _ck(lib().pepshost_load_sitps_c128(directory.encode(), D, C.byref(rows), C.byref(cols), C.byref(d), None, 0))
    flat = np.zeros((rows.value, cols.value, d.value, D, D, D, D), dtype=np.complex128)
    _ck(lib().pepshost_load_sitps_c128(directory.encode(), D, C.byref(rows), C.byref(cols), C.byref(d), _cp(flat), C.c_size_t(2 * flat.size)))
    return flat


def dump_sitps_complex(directory, flat):
    flat = _cflat(flat)
    rows, cols, d, D = _dims(flat)
    os.makedirs(directory, exist_ok=True)
    _ck(lib().pepshost_dump_sitps_c128(directory.encode(), rows, cols, D, d, _cp(flat)))


def energy_and_holes_complex(flat, configs, chi, model="xxz", params=(1.0, 1.0, 0.0), holes=True):
    """CalEnergyAndHoles of the C++ host layer on a COMPLEX state (BMPSContractorT<QLTEN_Complex>, PEPSGPU_C128 context):
    (amplitudes, energies, holes = Dag(hole) [n][rows][cols][D^4] or None, psi_list [n_psi][n]), all complex128."""
    flat = _cflat(flat)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(configs, dtype=np.int32)
    n = cfg.shape[0]
    p = np.array(list(params) + [0.0] * 8, dtype=np.float64)
    amps = np.zeros(n, dtype=np.complex128)
    en = np.zeros(n, dtype=np.complex128)
    hl = np.zeros((n, rows, cols, D, D, D, D), dtype=np.complex128) if holes else None
    psi = np.zeros((rows + cols, n), dtype=np.complex128)
    npsi = C.c_int(0)
    _ck(lib().pepshost_energy_and_holes_c128(rows, cols, D, d, chi, _cp(flat), n, _p(cfg, C.c_int32), MODEL_ID[model], _p(p, C.c_double),
                                             _cp(amps), _cp(en), _cp(hl) if holes else None, _cp(psi), C.byref(npsi)))
    return amps, en, hl, psi[:npsi.value]


def exact_sum_complex(flat, all_configs, chi, model="xxz", params=(1.0, 1.0, 0.0), size=1, batch=64):
    """ExactSumEnergyEvaluator on a complex state, the `size` rank-partials summed here: (energy complex, gradient complex128
    in the upload layout).  Holes resident in HBM, O* accumulation with the conjugations of
    exact_summation_energy_evaluator.h:228-240 on the device (pepsgpu_grad_accumulate for PEPSGPU_C128)."""
    flat = _cflat(flat)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(all_configs, dtype=np.int32)
    p = np.array(list(params) + [0.0] * 8, dtype=np.float64)
    m = flat.size
    tot = np.zeros(4 * m + 5)
    for rank in range(size):
        packed = np.zeros(4 * m + 5)
        _ck(lib().pepshost_exact_sum_partial_c128(rows, cols, D, d, chi, _cp(flat), _p(cfg, C.c_int32), cfg.shape[0], MODEL_ID[model],
                                                  _p(p, C.c_double), rank, size, batch, _p(packed, C.c_double)))
        tot += packed
    e = np.zeros(2)
    grad = np.zeros(flat.shape, dtype=np.complex128)
    _ck(lib().pepshost_exact_sum_finish_c128(rows, cols, D, d, _p(tot, C.c_double), _p(e, C.c_double), _cp(grad)))
    return complex(e[0], e[1]), grad


def mc_sweeps_complex(flat, configs, seeds, chi, updater="exchange", n_sweeps=1):
    flat = _cflat(flat)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(configs, dtype=np.int32).copy()
    n = cfg.shape[0]
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    amps = np.zeros(n, dtype=np.complex128)
    rates = np.zeros(n)
    _ck(lib().pepshost_mc_sweeps_c128(rows, cols, D, d, chi, _cp(flat), n, _p(cfg, C.c_int32), _p(sd, C.c_uint64),
                                      _updater_id(updater), n_sweeps, _cp(amps), _p(rates, C.c_double)))
    return cfg, amps, rates


def mc_energy_grad_complex(flat, configs, seeds, chi, updater="exchange", model="xxz", params=(1.0, 1.0, 0.0), warmup_sweeps=1, n_samples=1):
    """MCEnergyGradEvaluator loop on a complex state: (energy, gradient, final configs, accept rates)"""
    flat = _cflat(flat)
    rows, cols, d, D = _dims(flat)
    cfg = np.ascontiguousarray(configs, dtype=np.int32).copy()
    n = cfg.shape[0]
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    p = np.array(list(params) + [0.0] * 8, dtype=np.float64)
    packed = np.zeros(4 * flat.size + 5)
    acc = np.zeros(n)
    _ck(lib().pepshost_mc_energy_grad_partial_c128(rows, cols, D, d, chi, _cp(flat), n, _p(cfg, C.c_int32), _p(sd, C.c_uint64),
                                                   _updater_id(updater), MODEL_ID[model], _p(p, C.c_double), warmup_sweeps,
                                                   n_samples, _p(packed, C.c_double), _p(acc, C.c_double)))
    e = np.zeros(2)
    grad = np.zeros(flat.shape, dtype=np.complex128)
    _ck(lib().pepshost_exact_sum_finish_c128(rows, cols, D, d, _p(packed, C.c_double), _p(e, C.c_double), _cp(grad)))
    return complex(e[0], e[1]), grad, cfg, acc


def suwa_todo_chain(init_state, weights, seed, n_steps):
    """The chain of n_steps SuwaTodoStateUpdate calls (suwa_todo_update.h:53-112) with std::mt19937(seed), on the host alone (no GPU):
    states[t] for t = 1..n_steps."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    out = np.zeros(int(n_steps), dtype=np.int32)
    _ck(lib().pepshost_suwa_todo_chain(int(init_state), _p(w, C.c_double), int(w.size), C.c_uint64(int(seed)), C.c_long(int(n_steps)),
                                       _p(out, C.c_int32)))
    return out


def tnn3_table(d, nf=None, order=0):
    """The triple table of the three-site exchange (pepsgpu_sweep_slice_tnn3), built by the host layer without a device.
    nf None: bosonic, d states per site -> [d^3][20]; else fermionic (parities nf[d]) over the 4 d extended states of mode
    order `order` (0 row-major, 1 column-major) -> [(4 d)^3][20]."""
    l = lib()
    l.pepshost_tnn3_table.argtypes = [C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32)]
    dp = d if nf is None else 4 * d
    out = np.zeros((dp ** 3, 20), dtype=np.int32)
    nfa = None if nf is None else np.ascontiguousarray(nf, dtype=np.int32)
    _ck(l.pepshost_tnn3_table(d, None if nfa is None else _p(nfa, C.c_int32), order, _p(out, C.c_int32)))
    return out


def hubbard_tables():
    """The tables of the Hubbard model as the host layer builds them, without a device: (sector table [16][10] of
    MCUpdateSquareNNHubbardU1U1OBC, hop table [16][2][2] of SquareHubbardModel) -- peps_amd.fermion.hubbard_sector_table() and
    hubbard_hop_table() state the same rules."""
    sec, hop = np.zeros((16, 10), dtype=np.int32), np.zeros((16, 2, 2), dtype=np.int32)
    _ck(lib().pepshost_hubbard_sector_table(_p(sec, C.c_int32)))
    _ck(lib().pepshost_hubbard_hop_table(_p(hop, C.c_int32)))
    return sec, hop

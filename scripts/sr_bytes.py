"""Every output of the stochastic-reconfiguration layer (peps_amd/csrc/engine_sr.h and its callers in engine_opt.h) on a small
store, written to an .npz, and a byte comparison of two such files: the check that a rewrite of that layer computes what the
parent commit computed.  The library is the one capi.py loads (PEPSGPU_LIB selects another build).

    python scripts/sr_bytes.py run OUT.npz                 (needs a GPU)
    python scripts/sr_bytes.py compare A.npz B.npz          (prints every key that differs; exit status 1 if one does)

The store is the one of tests/test_gpu_sr.py: 4x4, D = 3, chi = 9, two batches of 24 walkers (16 for C128), once per dtype."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

L, D, CHI = 4, 3, 9


def _store(capi, synthetic, name):
    """the resident store of one dtype and the host-side O* samples (for the oracle's S and the trace bound)"""
    from peps_amd.capi import LEFT, RIGHT, UP, DOWN, HORIZONTAL
    cplx = name == "C128"
    nb = 16 if cplx else 24
    flat = synthetic.sitps_to_flat(synthetic.make_sitps(L, D), D)
    if cplx:
        flat = flat.astype(np.complex128)
        flat = flat * np.exp(2j * np.pi * np.random.default_rng(12).random(flat.shape)) * (np.abs(flat) > 0)
    ctx = capi.Context(L, L, D, 2, CHI, dtype=getattr(capi, name), max_walkers=nb)
    ctx.state_upload(flat)
    ctx.sr_begin(2 * nb)
    samples = []
    for batch in range(2):
        cfgs = synthetic.make_configs(L, nb, "heisenberg", seed0=300 + (40 if cplx else 50) * batch)
        ctx.set_configs(cfgs)
        psi = ctx.evaluate_amplitude()
        ctx.set_configs(cfgs)
        ctx.generate_bmps_approach(UP)
        ostar = np.zeros((nb, L, L, 2, D, D, D, D), dtype=np.complex128 if cplx else np.float64)
        for row in range(L):
            ctx.init_bten(LEFT, row)
            ctx.grow_full_bten(RIGHT, row, 1, True)
            for col in range(L):
                h = ctx.punch_hole(row, col, HORIZONTAL)
                ctx.punch_hole_store(row, col, HORIZONTAL)
                for w in range(nb):
                    ostar[w, row, col, cfgs[w, row, col]] = np.conj(h[w]) / np.conj(psi[w])
                if col < L - 1:
                    ctx.shift_bten_window(RIGHT)
            if row < L - 1:
                ctx.shift_bmps_window(DOWN)
        ctx.sr_append(psi)
        samples += list(ostar)
    return ctx, samples, (np.abs(flat.reshape(L, L, 2, D, D, D, D)) > 0).astype(np.float64)


def _one_dtype(name, out):
    import torch
    from oracle import sr as osr
    from peps_amd import capi, sr, synthetic
    ctx, samples, mask = _store(capi, synthetic, name)
    cplx = name == "C128"
    n = len(samples)
    shp = mask.shape
    rng = np.random.default_rng(7)

    def draw(size=shp):
        return rng.standard_normal(size) + (1j * rng.standard_normal(size) if cplx else 0.0)

    def put(key, *vals):
        for k, v in enumerate(vals):
            out["%s/%s/%d" % (name, key, k)] = np.asarray(v)

    total = ctx.sr_sum()
    put("sr_sum", total)
    mean = total / n
    for k in range(2):
        v = draw()
        put("sr_matvec%d" % k, ctx.sr_matvec(v, np.vdot(mean.ravel(), v.ravel()) if cplx else float(np.sum(mean * v)), 1.0 / n))
    # right-hand side in the range of S plus a little outside it, scaled so that p * (A p) = O(1) (the validity test of the complex
    # solver is absolute)
    host_mean = np.mean(samples, axis=0)
    full = osr.SRSMatrix(samples, host_mean, 1, 1e-3)
    b = (full * (mask * draw()).ravel()).reshape(shp) + 0.01 * draw() * mask
    b = b / np.sqrt(abs(np.vdot(b.ravel(), full * b.ravel())))
    x = None
    for shift, interval in ((1e-3, 20), (1e-2, 3)):
        x, res, it, why = ctx.sr_cg_solve(b, None, shift, 200, 1e-8, 0.0, interval, 0.5)
        put("cg_shift%g_recompute%d" % (shift, interval), x, res, it, why)
        put("cg_shift%g_warm_start" % shift, *ctx.sr_cg_solve(b, x, shift, 200, 1e-6, 0.0, interval, 0.5))
    put("cg_max_iter3", *ctx.sr_cg_solve(b, None, 1e-3, 3, 1e-14, 0.0, 20, 0.5))
    put("cg_max_iter0", *ctx.sr_cg_solve(b, x, 1e-3, 0, 1e-14, 0.0, 20, 0.5))
    put("cg_zero_rhs", *ctx.sr_cg_solve(np.zeros_like(b), None, 1e-3, 50, 1e-8, 0.0, 20, 0.5))
    below = -2.0 * float(sum(np.vdot(s.ravel(), s.ravel()).real for s in samples)) / n      # below -lambda_max(S): -2 trace bound
    put("cg_indefinite", *ctx.sr_cg_solve(b, None, below, 50, 1e-8, 0.0, 20, 0.5))
    put("sr_gram_local", ctx.sr_gram())
    batch = sr.DeviceSampleBatch(ctx)
    remote = batch.export("cuda:0")
    put("sr_gram_remote", batch.gram_with(remote))
    del remote
    put("sr_weighted_sum", ctx.sr_weighted_sum(draw(n)))
    e_loc = draw(n)
    ctx.opt_begin()
    for kw in ({"r_pinv": 1e-5, "a_pinv": 0.0, "soft_cutoff": True}, {"r_pinv": 1e-6, "a_pinv": 1e-9, "soft_cutoff": False}):
        nrm, info = ctx.minsr_direction(e_loc, e_loc.mean() if cplx else float(e_loc.mean()), **kw)
        put("minsr_direction_soft%d" % kw["soft_cutoff"], ctx.opt_get_gradient(), nrm, info["lambda_max"], info["cutoff"], info["n_kept"],
            info["sweeps"])
    ctx.opt_set_gradient(b)
    res, it, why, nrm = ctx.opt_natural_gradient(1e-3, 200, 1e-8, 0.0, 20, 0.5)
    put("opt_natural_gradient", ctx.opt_get_gradient(), res, it, why, nrm)
    ctx.close()
    torch.cuda.synchronize()


def _fermion(out):
    """opt_natural_gradient with a fermionic decoration set: the set-up of tests/test_gpu_opt_fermion.py::test_sr_solves_in_the_stored_parameters"""
    import test_gpu_opt_fermion as tf
    st = tf._load(os.path.join(ROOT, "tests", "golden", "ref_fixtures"), "spinless_fermion_tps_t2_0.000000_double_from_simple_update")
    ctx, es, ws = tf._accumulated_context(st, tf._half_filling(), 8, "spinless", (1.0, 0.0, 0.0), exact_sum=False, sr=True)
    ctx.fermion_decoration_set(st)
    ctx.opt_begin()
    e0, g_norm = ctx.opt_gradient_from_accumulators(es, ws)
    res, it, why, x_norm = ctx.opt_natural_gradient(1e-3, 200, 1e-10, 0.0, 20, 0.5)
    for k, v in enumerate((ctx.opt_get_gradient(), e0, g_norm, res, it, why, x_norm)):
        out["F64/opt_natural_gradient_fermion/%d" % k] = np.asarray(v)
    ctx.close()


def run(path):
    out = {}
    for name in ("F32", "F64", "C128"):
        _one_dtype(name, out)
    _fermion(out)
    np.savez(path, **out)
    print("%d arrays -> %s" % (len(out), path))


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    differ = []
    for key in sorted(set(a.files) | set(b.files)):
        if key not in a.files or key not in b.files:
            differ.append((key, "missing in %s" % (path_a if key not in a.files else path_b)))
            continue
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.dtype != y.dtype or x.shape != y.shape:
            differ.append((key, "%s %s against %s %s" % (x.dtype, x.shape, y.dtype, y.shape)))
        elif not np.array_equal(x.reshape(-1).view(np.uint8), y.reshape(-1).view(np.uint8)):
            differ.append((key, "max |a - b| = %.3e" % float(np.max(np.abs(x.astype(np.complex128) - y.astype(np.complex128))))))
    for key, what in differ:
        print("DIFFERS %s: %s" % (key, what))
    print("%d keys, %d differ" % (len(set(a.files) | set(b.files)), len(differ)))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)

#!/usr/bin/env python
"""MinSR on the device against its host orchestration, two measurements (no gate: a record only):

  eigh   ctx.diag_eigh (two-sided parallel Jacobi in HBM, peps_amd/csrc/eigh_jacobi.h; the call includes the upload of the matrix and
         the read-back of w and Z) against numpy.linalg.eigh on the host's threads, for centred Gram matrices at n = 256, 1024, 4096
  minsr  ctx.minsr_direction (Gram, centering, eigensolve, cutoff, back-substitution on the device) against
         peps_amd.sr.minsr_direction(DeviceSampleBatch(ctx)) (Gram read back, NumPy centering, host eigh, weights uploaded) on the same
         resident O* store at the C3 shape (10 x 10, D = 6, chi = 24, float32 context), 1024 samples (256 if the store does not fit)

Protocol of scripts/bench_opt_step.py: each variant runs in child processes of its own, the two alternating (device, host, device,
...), three children per variant; a child warms up, then times its repetitions with a host clock around calls that end in a stream
synchronise.  Reported: the median over all repetitions of all children of a variant with min / max / quartiles, and every value.

    python scripts/bench_minsr.py [--children 3] [--out profiles/minsr_bench.json] [--sizes 256,1024,4096]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

C3 = dict(L=10, D=6, chi=24, walkers=256)
EIGH_REPS = {256: (2, 10), 1024: (1, 4), 4096: (0, 1)}       # n -> (warm-up, timed repetitions) per child
MINSR_REPS = (1, 3)
TAG = "BENCH_MINSR "


def centred_gram(n):
    import numpy as np
    x = np.random.default_rng(n).standard_normal((n, 2 * n))
    g = x @ x.T
    m = g.sum(axis=1) / n
    t = (g - m[:, None] - m[None, :] + m.sum() / n) / n
    return (t + t.T) / 2


def child_eigh(variant, n):
    import numpy as np
    a = centred_gram(n)
    warmup, reps = EIGH_REPS.get(n, (1, 3))
    times, extra = [], {}
    if variant == "device":
        from peps_amd import capi
        ctx = capi.Context(2, 2, 2, 2, 4, dtype=capi.F64, max_walkers=1)
        ctx.diag_eigh(centred_gram(64))          # loads the code object; the timed sizes get their own warm-up where they can afford it
        for k in range(warmup + reps):
            ctx.sync()
            t0 = time.perf_counter()
            w, z, sweeps = ctx.diag_eigh(a)      # ends in a stream synchronise and the copies back
            t1 = time.perf_counter()
            if k >= warmup:
                times.append(t1 - t0)
        extra["sweeps"] = sweeps
        ctx.close()
    else:
        for k in range(warmup + reps):
            t0 = time.perf_counter()
            w, z = np.linalg.eigh(a)
            t1 = time.perf_counter()
            if k >= warmup:
                times.append(t1 - t0)
    extra["residual_over_n_eps_normF"] = float(np.linalg.norm(a @ z - z * w) / (n * 2.0 ** -52 * np.linalg.norm(a)))
    print(TAG + json.dumps(dict(extra, variant=variant, n=n, seconds=times)))


def child_minsr(variant):
    import numpy as np
    from peps_amd import capi, sr, synthetic
    from peps_amd.capi import LEFT, RIGHT, UP, DOWN, HORIZONTAL
    L, D, chi, nb = C3["L"], C3["D"], C3["chi"], C3["walkers"]
    ctx = capi.Context(L, L, D, 2, chi, dtype=capi.F32, max_walkers=nb)
    ctx.state_upload(synthetic.sitps_to_flat(synthetic.make_sitps(L, D), D))
    ns = 1024
    try:
        ctx.sr_begin(ns)
    except RuntimeError:                         # the store does not fit
        ns = 256
        ctx.sr_begin(ns)
    for batch in range(ns // nb):
        cfgs = synthetic.make_configs(L, nb, "heisenberg", seed0=500 + 1000 * batch)
        ctx.set_configs(cfgs)
        psi = ctx.evaluate_amplitude()
        ctx.set_configs(cfgs)
        ctx.generate_bmps_approach(UP)
        for row in range(L):
            ctx.init_bten(LEFT, row)
            ctx.grow_full_bten(RIGHT, row, 1, True)
            for col in range(L):
                ctx.punch_hole_store(row, col, HORIZONTAL)
                if col < L - 1:
                    ctx.shift_bten_window(RIGHT)
            if row < L - 1:
                ctx.shift_bmps_window(DOWN)
        ctx.sr_append(psi)
    ctx.opt_begin()
    e_loc = np.random.default_rng(3).standard_normal(ns)
    e_mean = float(e_loc.mean())
    kw = dict(r_pinv=1e-5, a_pinv=0.0, soft_cutoff=True)       # (above the f32 rounding of the Gram entries)
    warmup, reps = MINSR_REPS
    times, extra = [], {}
    batch = sr.DeviceSampleBatch(ctx)
    for k in range(warmup + reps):
        ctx.sync()
        t0 = time.perf_counter()
        if variant == "device":
            nrm, info = ctx.minsr_direction(e_loc, e_mean, **kw)      # ends in a stream synchronise (the norm's read-back)
        else:
            d, nrm = sr.minsr_direction(batch, e_loc, e_mean, **kw)   # ends with host arrays
        t1 = time.perf_counter()
        if k >= warmup:
            times.append(t1 - t0)
    extra["direction_norm"] = float(nrm)
    if variant == "device":
        extra.update(sweeps=info["sweeps"], n_kept=info["n_kept"])
    ctx.close()
    print(TAG + json.dumps(dict(extra, variant=variant, samples=ns, seconds=times)))


def summary(v):
    import numpy as np
    a = np.sort(np.asarray(v))
    return {"median_ms": 1e3 * float(np.median(a)), "min_ms": 1e3 * float(a[0]), "max_ms": 1e3 * float(a[-1]),
            "q25_ms": 1e3 * float(np.percentile(a, 25)), "q75_ms": 1e3 * float(np.percentile(a, 75)), "n": int(a.size),
            "all_ms": [1e3 * float(x) for x in v]}


def run_children(children, extra, timeout):
    got = {"device": [], "host": []}
    notes = {"device": [], "host": []}
    for k in range(children):
        for variant in ("device", "host"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant] + extra, capture_output=True, text=True,
                               timeout=timeout)
            if r.returncode != 0:          # a child that failed ends the measurement: nothing more is started on the device
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit("child %s %s #%d failed with status %d" % (variant, extra, k, r.returncode))
            rec = json.loads([x for x in r.stdout.splitlines() if x.startswith(TAG)][-1][len(TAG):])
            got[variant] += rec.pop("seconds")
            notes[variant].append(rec)
            print("child %d %s %s done" % (k, variant, extra), flush=True)
    return got, notes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("device", "host"))
    ap.add_argument("--part", choices=("eigh", "minsr"), default="eigh")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--children", type=int, default=3)
    ap.add_argument("--sizes", default="256,1024,4096")
    ap.add_argument("--skip-minsr", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minsr_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child_eigh(a.child, a.n) if a.part == "eigh" else child_minsr(a.child)
    out = {"metric": "MinSR on the device against its host orchestration: the eigensolver alone, and the whole direction on a resident store",
           "protocol": {"children_per_variant": a.children, "order": "device, host alternating",
                        "clock": "time.perf_counter around calls that end in a stream synchronise (device) or in host arrays (host)",
                        "host_threads": os.environ.get("OMP_NUM_THREADS", "unset"),
                        "eigh_warmup_reps_per_child": {str(k): v for k, v in EIGH_REPS.items()}, "minsr_warmup_reps_per_child": MINSR_REPS},
           "eigh": {}, "minsr": None}
    for n in [int(x) for x in a.sizes.split(",") if x]:
        got, notes = run_children(a.children, ["--part", "eigh", "--n", str(n)], 900)
        rec = {"device": summary(got["device"]), "host": summary(got["host"]), "device_children": notes["device"], "host_children": notes["host"]}
        rec["device_over_host_median"] = rec["device"]["median_ms"] / rec["host"]["median_ms"]
        out["eigh"][str(n)] = rec
        print("eigh n = %d: device median %.1f ms [%.1f, %.1f] (%s sweeps), numpy median %.1f ms [%.1f, %.1f]" % (
            n, rec["device"]["median_ms"], rec["device"]["min_ms"], rec["device"]["max_ms"], notes["device"][0].get("sweeps"),
            rec["host"]["median_ms"], rec["host"]["min_ms"], rec["host"]["max_ms"]), flush=True)
    if not a.skip_minsr:
        got, notes = run_children(a.children, ["--part", "minsr"], 900)
        rec = {"shape": dict(C3, dtype="f32", samples=notes["device"][0]["samples"]), "device": summary(got["device"]), "host": summary(got["host"]),
               "device_children": notes["device"], "host_children": notes["host"]}
        rec["host_over_device_median"] = rec["host"]["median_ms"] / rec["device"]["median_ms"]
        out["minsr"] = rec
        print("minsr C3, %d samples: device median %.1f ms [%.1f, %.1f], python path median %.1f ms [%.1f, %.1f]" % (
            rec["shape"]["samples"], rec["device"]["median_ms"], rec["device"]["min_ms"], rec["device"]["max_ms"], rec["host"]["median_ms"],
            rec["host"]["min_ms"], rec["host"]["max_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
        f.write("\n")


if __name__ == "__main__":
    main()

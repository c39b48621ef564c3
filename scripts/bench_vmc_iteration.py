#!/usr/bin/env python
"""One VMC iteration at the C3 shape (10x10, D = 6, d = 2, chi = 24, float32 context, synthetic state, XXZ model, exchange updater),
split into sampling, the optimizer's tail and the rest of the executor.  Variants:

  device_adam  hostapi.vmc_optimize (VMCPEPSOptimizer::Execute): resident state, persistent chains, Adam step in HBM
  device_sr    the same with the stochastic-reconfiguration step (O* store and CG solve in HBM)
  host_adam    what a caller had to do without the executor: per iteration hostapi.mc_energy_grad_partial (a fresh contractor from the
               host state -- the upload is part of that call --, chains restarted from the seeds, packed sums back to the host) + the
               Adam update in NumPy on the padded arrays.  There is no host path for SR: the loop does not return the O* samples.

Each variant runs in child processes of its own, alternating (device_adam, device_sr, host_adam, device_adam, ...), `--children` of
each.  A child runs one untimed iteration first (allocations, code objects), then `--iterations` timed ones.  The device variants report
the executor's own host clocks (VMCPEPSOptimizer::GetTimings: seconds in the evaluator, in IterativeOptimize, in all); per iteration:
sampling = evaluator / evaluations, tail = (IterativeOptimize - evaluator) / iterations, rest = all - IterativeOptimize (warm-up
normalisation, closing refresh + normalisation; no dumps).  The host variant times the call and the NumPy update with perf_counter.
No gate: a measurement only.

    python scripts/bench_vmc_iteration.py [--children 3] [--iterations 3] [--walkers 256] [--samples 2] [--out profiles/vmc_iteration_bench.json]
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

L, D, CHI = 10, 6, 24
XXZ = (1.0, 1.0, 0.0)
ADAM = (0.9, 0.999, 1e-8, 0.0)
SR = (1e-3, 100, 1e-4, 0)
LR = 0.01
F32 = 0
VARIANTS = ("device_adam", "device_sr", "host_adam")


def child(mode, iterations, walkers, samples):
    import numpy as np
    from peps_amd import hostapi, synthetic
    flat = synthetic.sitps_to_flat(synthetic.make_sitps(L, D), D)
    cfgs = synthetic.make_configs(L, walkers, "heisenberg")
    seeds = np.arange(walkers, dtype=np.uint64) + 1
    out = {"mode": mode}
    if mode.startswith("device"):
        algo, rp = ("adam", ADAM) if mode == "device_adam" else ("sr", SR)
        kw = dict(warmup_sweeps=0, samples_per_walker=samples, dtype=F32)
        hostapi.vmc_optimize(flat, cfgs, seeds, CHI, "xxz", XXZ, "exchange", algo, LR, rp, 1, **kw)          # untimed
        r = hostapi.vmc_optimize(flat, cfgs, seeds, CHI, "xxz", XXZ, "exchange", algo, LR, rp, iterations, **kw)
        t = r["timings"]
        out.update(sampling_s=t["evaluation_s"] / (iterations + 1), tail_s=(t["optimize_s"] - t["evaluation_s"]) / iterations,
                   rest_s=t["total_s"] - t["optimize_s"], total_s=t["total_s"], evaluations=iterations + 1,
                   energies=[float(np.real(e)) for e in r["energies"]])
    else:
        theta = flat.copy()
        m1, m2 = np.zeros_like(theta), np.zeros_like(theta)
        samp, tail, energies = [], [], []
        for k in range(iterations + 1):
            t0 = time.perf_counter()
            packed, cfgs, _ = hostapi.mc_energy_grad_partial(theta, cfgs, seeds, CHI, "exchange", "xxz", XXZ, 0, samples, F32)
            t1 = time.perf_counter()
            m = theta.size
            so, seo = packed[:m].reshape(theta.shape), packed[m:2 * m].reshape(theta.shape)
            w, es = packed[2 * m], packed[2 * m + 1]
            e = es / w
            g = (seo - e * so) / w
            t = k + 1
            m1 = ADAM[0] * m1 + (1 - ADAM[0]) * g
            m2 = ADAM[1] * m2 + (1 - ADAM[1]) * g * g
            theta = theta - LR * (m1 / (1 - ADAM[0] ** t)) / (np.sqrt(m2 / (1 - ADAM[1] ** t)) + ADAM[2])
            t2 = time.perf_counter()
            energies.append(float(e))
            if k > 0:                                                   # the first iteration is the untimed one
                samp.append(t1 - t0)
                tail.append(t2 - t1)
        out.update(sampling_s=sum(samp) / len(samp), tail_s=sum(tail) / len(tail), rest_s=0.0, total_s=sum(samp) + sum(tail),
                   evaluations=iterations, energies=energies)
    print("BENCH_VMC_ITERATION " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=VARIANTS)
    ap.add_argument("--children", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--walkers", type=int, default=256)
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vmc_iteration_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.iterations, a.walkers, a.samples)
    import numpy as np
    runs = {v: [] for v in VARIANTS}
    for k in range(a.children):
        for mode in VARIANTS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--iterations", str(a.iterations), "--walkers",
                                str(a.walkers), "--samples", str(a.samples)], capture_output=True, text=True, timeout=400)
            if r.returncode != 0:          # a child that failed ends the measurement: nothing more is started on the device
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit("child %s #%d failed with status %d" % (mode, k, r.returncode))
            line = [x for x in r.stdout.splitlines() if x.startswith("BENCH_VMC_ITERATION ")][-1]
            runs[mode].append(json.loads(line[len("BENCH_VMC_ITERATION "):]))
            print("%s #%d: sampling %.1f ms  tail %.2f ms  rest %.1f ms per iteration" % (
                mode, k, 1e3 * runs[mode][-1]["sampling_s"], 1e3 * runs[mode][-1]["tail_s"], 1e3 * runs[mode][-1]["rest_s"]), flush=True)
    out = {"metric": "one VMC iteration at the C3 shape, split into sampling, optimizer tail and the rest of the executor",
           "shape": {"rows": L, "cols": L, "D": D, "d": 2, "chi": CHI, "dtype": "f32", "walkers": a.walkers, "samples_per_walker": a.samples,
                     "model": "xxz", "updater": "exchange"},
           "protocol": {"children_per_variant": a.children, "timed_iterations_per_child": a.iterations, "untimed_iterations_per_child": 1,
                        "order": "device_adam, device_sr, host_adam alternating", "clock": "steady_clock inside the executor / perf_counter"},
           "gate": "none: measured only"}
    for mode in VARIANTS:
        out[mode] = {key + "_ms": {"median": 1e3 * float(np.median([x[key + "_s"] for x in runs[mode]])),
                                   "all": [1e3 * x[key + "_s"] for x in runs[mode]]} for key in ("sampling", "tail", "rest")}
        out[mode]["iteration_ms_median"] = out[mode]["sampling_ms"]["median"] + out[mode]["tail_ms"]["median"]
        out[mode]["energies_first_child"] = runs[mode][0]["energies"]
    out["host_over_device_adam_iteration"] = out["host_adam"]["iteration_ms_median"] / out["device_adam"]["iteration_ms_median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in VARIANTS + ("host_over_device_adam_iteration",)}))


if __name__ == "__main__":
    main()

"""A/B of the parent build against this tree for the span-only truncation of the low-rank sites (JrSelect::span): the C4 headline
of bench.py on one GPU, every run a fresh child process under its own time limit, the parent's library selected with
PEPSGPU_LIB.  The switch PEPSGPU_TRUNC_SPAN is never the yardstick.

    python scripts/trunc_span_ab.py --ref <parent's libpepsgpu.so> [--phases speed,profile,share,physics,full] [--out FILE]

phases (each adds its record to FILE, default profiles/trunc_span_ab.json; a phase stops at the first child that fails):
    speed    three alternating pairs of `python bench.py --steps 10 --warmup 2`: value and the kernel categories per step
    profile  per build `rocprofv3 --kernel-trace --stats -- python bench.py --steps 2 --warmup 1` and a second process with
             `--pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES` (no tracing domain beside it): duration and counters per
             full-grid launch of jacobi_rows_tiny4_kernel<8> and <4>;  --wait adds a third with SQ_WAIT_ANY SQ_WAIT_INST_ANY
    share    one PEPSGPU_DEBUG_VERBOSE step of 4 096 walkers on the tree: walker-sites on the span path and fallen back
    physics  2 048 seeded walkers per build, f32 against the float64 engine of the same build: |a32 / a64 - 1| median, p99, max;
             the tree with PEPSGPU_TRUNC_SPAN=0 against the parent as bytes; absorptions_redone of a two-step headline run
    full     one `python bench.py --full` per build: the full_rank and real_rank legs
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_LIB = os.path.join(ROOT, "peps_amd", "lib", "libpepsgpu.so")
CATS = ("jacobi", "jacobi_edge", "contract", "contract_chain", "cholesky")
KERNEL = "jacobi_rows_tiny4_kernel"

_WORKER = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
from peps_amd import capi, synthetic
mode, nw = sys.argv[1], int(sys.argv[2])
L, D, chi, _ = synthetic.CONFIGS["C4"]
sitps = synthetic.make_sitps(L, D, noise=0.1)
# amplitudes of order one, as bench.py scales them (the float64 engine is the same code in both builds)
c0 = capi.Context(L, L, D, 2, chi, dtype=capi.F64, max_walkers=1)
c0.state_upload(synthetic.sitps_to_flat(sitps, D, np.float64))
c0.set_configs(synthetic.checkerboard(L)[None])
sitps = synthetic.rescale_sitps(sitps, float(c0.evaluate_amplitude()[0]))
c0.close()
def amps(dtype, steps=1):
    ctx = capi.Context(L, L, D, 2, chi, dtype=dtype, max_walkers=nw)
    ctx.state_upload(synthetic.sitps_to_flat(sitps, D, np.float64))
    a = None
    for s in range(steps):
        ctx.set_configs(synthetic.make_configs(L, nw, "heisenberg", seed0=100 + s))
        a = ctx.evaluate_amplitude()
    st = ctx.stats()
    ctx.close()
    return np.asarray(a, dtype=np.float64), st
if mode == "physics":
    a32, _ = amps(capi.F32)
    a64, _ = amps(capi.F64)
    rel = np.abs(a32 / a64 - 1)
    np.save(sys.argv[3], a32)
    print(json.dumps({"n": nw, "median": float(np.median(rel)), "p99": float(np.percentile(rel, 99)), "max": float(np.max(rel))}))
elif mode == "redone":
    _, st = amps(capi.F32, steps=2)
    print(json.dumps({"walkers": nw, "steps": 2, "absorptions": int(st["absorptions"]), "absorptions_redone": int(st["absorptions_redone"])}))
elif mode == "share":
    amps(capi.F32)
    print(json.dumps({"walkers": nw}))
'''


def child(cmd, env, limit, cwd=ROOT):
    e = dict(os.environ)
    e.pop("PEPSGPU_TRUNC_SPAN", None)
    e.pop("PEPSGPU_LIB", None)
    e.update(env)
    # the time limit is the child's own (`timeout` also ends what the child started); any failure ends the whole script
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd, env=e, capture_output=True, text=True, timeout=limit + 60)
    if r.returncode != 0:
        raise RuntimeError("child failed (%d): %s\n%s" % (r.returncode, " ".join(cmd), r.stderr[-3000:]))
    return r


def last_json(text):
    for ln in reversed(text.strip().splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    raise RuntimeError("no JSON line in the child's output")


def lib_env(build, ref):
    return {"PEPSGPU_LIB": ref} if build == "parent" else {}


def phase_speed(ref, limit):
    runs = []
    for i in (1, 2, 3):
        for build in ("parent", "tree"):
            line = last_json(child([sys.executable, "bench.py", "--steps", "10", "--warmup", "2"], lib_env(build, ref), limit).stdout)
            km = line.get("kernel_ms", {})
            rec = {"run": "bench_%s_%d" % (build, i), "build": build, "command": "python bench.py --steps 10 --warmup 2",
                   "value": line["value"], "ms_per_step": line.get("ms_per_step")}
            for c in CATS:
                rec[c + "_ms_per_step"] = km[c] / 10 if c in km else None      # (kernel_ms is the sum over the timed steps)
            runs.append(rec)
            print(json.dumps(rec), flush=True)
    p = [r["value"] for r in runs if r["build"] == "parent"]
    t = [r["value"] for r in runs if r["build"] == "tree"]
    spread = (max(p) - min(p)) / min(p)
    gap = min(t) / max(p) - 1
    verdict = {"parent_spread": spread, "gap_best_parent_to_worst_tree": gap, "gap_of_means": (sum(t) / 3) / (sum(p) / 3) - 1,
               "every_tree_above_every_parent": min(t) > max(p), "gap_exceeds_three_spreads": gap > 3 * spread}
    verdict["gain"] = verdict["every_tree_above_every_parent"] and verdict["gap_exceeds_three_spreads"]
    print(json.dumps(verdict), flush=True)
    return {"runs": runs, "verdict": verdict}


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else None


def _inst(name):
    m = re.search(KERNEL + r"<(\d+)>", name) or re.search(KERNEL + r"ILi(\d+)E", name)
    return "tiny4<%s>" % m.group(1) if m else None


def _full_grid(rows, key):
    """the launches of the largest grid of each instantiation: the full-grid launches of the headline"""
    out = {}
    for inst in sorted({r[0] for r in rows}):
        mine = [r for r in rows if r[0] == inst]
        g = max(r[1] for r in mine)
        vals = [r[2] for r in mine if r[1] == g]
        out[inst] = {"grid": g, "launches": len(vals), key + "_median": _median(vals), key + "_mean": sum(vals) / len(vals)}
    return out


def phase_profile(ref, limit, wait):
    bench = [sys.executable, "bench.py", "--steps", "2", "--warmup", "1"]
    res = {"command": "rocprofv3 ... -- python bench.py --steps 2 --warmup 1; one process with --kernel-trace --stats, a second with "
                      "--pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES and no tracing domain"}
    passes = [("trace", ["--kernel-trace", "--stats"]), ("pmc", ["--pmc", "SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_WAVE_CYCLES"])]
    if wait:
        passes.append(("pmc_wait", ["--pmc", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_WAVE_CYCLES"]))
    for build in ("parent", "tree"):
        res[build] = {}
        for tag, opts in passes:
            d = tempfile.mkdtemp(prefix="trunc_span_")
            try:
                child(["rocprofv3"] + opts + ["--output-format", "csv", "-d", d, "-o", tag, "--"] + bench, lib_env(build, ref), limit)
                if tag == "trace":
                    rows, total = [], 0.0
                    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                        for r in csv.DictReader(open(f)):
                            dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                            total += dur
                            inst = _inst(r["Kernel_Name"])
                            if inst:
                                rows.append((inst, int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0), dur))
                    res[build]["trace"] = {"all_kernels_ms": total / 1e3, "launches_of_the_kernel": len(rows),
                                           "kernel_ms": sum(r[2] for r in rows) / 1e3, "full_grid": _full_grid(rows, "us")}
                else:
                    per = {}
                    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                        for r in csv.DictReader(open(f)):
                            inst = _inst(r["Kernel_Name"])
                            if inst:
                                per.setdefault(r["Counter_Name"], []).append(
                                    (inst, int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0), float(r["Counter_Value"] or 0)))
                    res[build][tag] = {c: _full_grid(rows, "value") for c, rows in per.items()}
            finally:
                shutil.rmtree(d, ignore_errors=True)
            print(build, tag, json.dumps(res[build][tag]), flush=True)
    return res


def _worker(args, env, limit):
    with tempfile.NamedTemporaryFile("w", suffix=".py", delete=False) as f:
        f.write(_WORKER % {"root": ROOT})
    try:
        return child([sys.executable, f.name] + args, env, limit)
    finally:
        os.unlink(f.name)


def phase_share(limit):
    r = _worker(["share", "4096"], {"PEPSGPU_DEBUG_SWEEPS": "1", "PEPSGPU_DEBUG_VERBOSE": "1"}, limit)
    sites = span = back = live = 0
    by_shape = {}
    for ln in r.stderr.splitlines():
        m = re.search(r"jacobi m=(\d+) len=(\d+) .* span=(\d+) span_fell_back=(\d+)", ln)
        if not m:
            continue
        sites += 1
        span += int(m.group(3))
        back += int(m.group(4))
        s = by_shape.setdefault("m=%s len=%s" % (m.group(1), m.group(2)), [0, 0, 0])
        s[0] += 1; s[1] += int(m.group(3)); s[2] += int(m.group(4))
    rec = {"walkers": 4096, "jacobi_launches": sites, "walker_sites": sites * 4096, "span": span, "fell_back": back,
           "span_share": span / max(sites * 4096, 1), "fell_back_share": back / max(sites * 4096, 1),
           "by_shape_launches_span_fell_back": by_shape}
    print(json.dumps(rec), flush=True)
    return rec


def phase_physics(ref, limit):
    import numpy as np
    res = {"what": "2 048 walkers (seed 100), C4 headline state, f32 against the float64 engine of the same build"}
    d = tempfile.mkdtemp(prefix="trunc_span_")
    try:
        for name, env in (("parent", lib_env("parent", ref)), ("tree", {}), ("tree_switch_0", {"PEPSGPU_TRUNC_SPAN": "0"})):
            res[name] = last_json(_worker(["physics", "2048", os.path.join(d, name + ".npy")], env, limit).stdout)
            print(name, json.dumps(res[name]), flush=True)
        a = {n: np.load(os.path.join(d, n + ".npy")) for n in ("parent", "tree", "tree_switch_0")}
        res["tree_switch_0_equals_parent_as_bytes"] = a["parent"].tobytes() == a["tree_switch_0"].tobytes()
        res["tree_vs_parent_max_rel"] = float(np.max(np.abs(a["tree"] / a["parent"] - 1)))
        res["gate_max_below_1e-5"] = res["tree"]["max"] < 1e-5
        res["tree_median_within_twice_parent"] = res["tree"]["median"] <= 2 * res["parent"]["median"]
        for name, env in (("parent", lib_env("parent", ref)), ("tree", {})):
            res[name]["headline_two_steps"] = last_json(_worker(["redone", "49152"], env, limit).stdout)
            print(name, json.dumps(res[name]["headline_two_steps"]), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}), flush=True)
    return res


def phase_full(ref, limit):
    res = {"command": "python bench.py --full"}
    for build in ("parent", "tree"):
        line = last_json(child([sys.executable, "bench.py", "--full"], lib_env(build, ref), limit).stdout)
        res[build] = {"value": line["value"], "full_rank": (line.get("full_rank") or {}).get("value"),
                      "real_rank": (line.get("real_rank") or {}).get("value")}
        print(build, json.dumps(res[build]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="libpepsgpu.so of the parent commit")
    ap.add_argument("--phases", default="speed,profile,share,physics")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trunc_span_ab.json"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child process")
    ap.add_argument("--wait", action="store_true", help="profile: a third pass with SQ_WAIT_ANY SQ_WAIT_INST_ANY")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref)
    assert os.path.exists(ref) and os.path.exists(TREE_LIB) and not os.path.samefile(ref, TREE_LIB)
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out["what"] = ("A/B of the parent build against this tree on the C4 headline (12x12, D = 8, chi = 32, f32, 49 152 walkers), one MI355X, "
                   "fresh processes, alternating parent and tree (PEPSGPU_LIB selects the parent's library); PEPSGPU_TRUNC_SPAN is never the yardstick")
    for ph in a.phases.split(","):
        if ph == "speed":
            out["speed"] = phase_speed(ref, a.timeout)
        elif ph == "profile":
            out["profile"] = phase_profile(ref, a.timeout, a.wait)
        elif ph == "share":
            out["share"] = phase_share(a.timeout)
        elif ph == "physics":
            out["same_physics"] = phase_physics(ref, a.timeout)
        elif ph == "full":
            out["full"] = phase_full(ref, max(a.timeout, 900))
        else:
            raise SystemExit("unknown phase " + ph)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

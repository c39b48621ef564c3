"""A/B of the parent build against this tree for the batched per-walker loads at the entry of the tensor-GEMM kernels
(tg_entry_load in peps_amd/csrc/tgemm.h): the C4 headline of bench.py on one GPU, every run a fresh child process under its own
time limit, the parent's library selected with PEPSGPU_LIB.  Modelled on scripts/trunc_span_ab.py.

    python scripts/entry_extents_ab.py --ref <parent's libpepsgpu.so> [--phases trace3,speed,profile,same,full] [--out FILE]

phases (each adds its record to FILE, default profiles/entry_extents_ab.json; a phase stops at the first child that fails):
    trace3   the stop condition of the work: three `rocprofv3 --kernel-trace` runs of the parent and one of the tree, the median of
             the full-grid launches of every tensor-GEMM instantiation; the fall of M and Y against the parent's spread of medians
    speed    three alternating pairs of `python bench.py --steps 10 --warmup 2`: value, ms_per_step, kernel_ms of every run
    profile  per build `rocprofv3 --kernel-trace --stats -- python bench.py --steps 2 --warmup 1` and a second process with
             `--pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_INSTS_SALU SQ_INSTS_SMEM` (no tracing domain beside it)
    same     bench.py --steps 2 --warmup 1 --dump-outputs on both builds, headline and `--state real --walkers 2048`:
             amplitudes.npy equal as bytes
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
# the instantiations of the headline: the chained absorption, Y = Tt V^T (staged B) and M = R Tt (transposed epilogue)
HEADLINE = {"chain": "tgemm_chain_kernel<true, false, false, 6144, 6, false, false>",
            "Y": "tgemm_direct_kernel<true, false, false, 1>", "M": "tgemm_direct_kernel<true, false, false, 2>",
            "chain3": "tgemm_chain3_kernel<true, false, false, 4096, 4>"}


def child(cmd, env, limit, cwd=ROOT):
    e = dict(os.environ)
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


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if v else None


def _inst(name):
    m = re.search(r"(tgemm_(?:direct|chain3|chain)_kernel<[^>]*>)", name)
    return m.group(1) if m else None


def _full_grid(rows, key):
    """the launches of the largest grid of each instantiation: the full-grid launches of the headline"""
    out = {}
    for inst in sorted({r[0] for r in rows}):
        mine = [r for r in rows if r[0] == inst]
        g = max(r[1] for r in mine)
        vals = [r[2] for r in mine if r[1] == g]
        out[inst] = {"grid": g, "launches": len(vals), key + "_median": _median(vals), key + "_mean": sum(vals) / len(vals)}
    return out


def _grid(r):
    g = 1
    for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"):
        g *= int(r.get(k, 1) or 1)
    return g if "Grid_Size_X" in r else int(r.get("Grid_Size", 0) or 0)


BENCH2 = [sys.executable, "bench.py", "--steps", "2", "--warmup", "1"]


def _trace(build, ref, limit):
    d = tempfile.mkdtemp(prefix="entry_extents_")
    try:
        child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "trace", "--"] + BENCH2, lib_env(build, ref), limit)
        rows, total = [], 0.0
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                total += dur
                inst = _inst(r["Kernel_Name"])
                if inst:
                    rows.append((inst, _grid(r), dur))
        return {"all_kernels_ms": total / 1e3, "tgemm_ms": sum(r[2] for r in rows) / 1e3, "full_grid": _full_grid(rows, "us")}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _pmc(build, ref, limit):
    d = tempfile.mkdtemp(prefix="entry_extents_")
    try:
        child(["rocprofv3", "--pmc", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_INSTS_SALU", "SQ_INSTS_SMEM", "--output-format", "csv", "-d", d,
               "-o", "pmc", "--"] + BENCH2, lib_env(build, ref), limit)
        per = {}
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                inst = _inst(r["Kernel_Name"])
                if inst in HEADLINE.values():
                    per.setdefault(r["Counter_Name"], []).append((inst, _grid(r), float(r["Counter_Value"] or 0)))
        res = {c: _full_grid(rows, "value") for c, rows in per.items()}
        share = {}
        for inst in res.get("SQ_WAVE_CYCLES", {}):
            w = res["SQ_WAVE_CYCLES"][inst]["value_median"]
            a = res.get("SQ_WAIT_ANY", {}).get(inst, {}).get("value_median")
            if w and a is not None:
                share[inst] = a / w
        res["wait_share_of_wave_cycles"] = share
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def phase_trace3(ref, limit):
    res = {"command": "rocprofv3 --kernel-trace --stats -- python bench.py --steps 2 --warmup 1; parent three times, tree once",
           "parent": [], "tree": []}
    for build in ("parent", "tree", "parent", "parent"):
        t = _trace(build, ref, limit)
        res[build].append(t)
        print(build, json.dumps({k: t["full_grid"].get(v, {}).get("us_median") for k, v in HEADLINE.items()}), flush=True)
    verdict = {}
    for k, inst in HEADLINE.items():
        p = [t["full_grid"][inst]["us_median"] for t in res["parent"] if inst in t["full_grid"]]
        tr = [t["full_grid"][inst]["us_median"] for t in res["tree"] if inst in t["full_grid"]]
        if p and tr:
            verdict[k] = {"parent_medians_us": p, "tree_medians_us": tr, "parent_spread_us": max(p) - min(p),
                          "fall_us": _median(p) - tr[0], "falls_by_more_than_the_spread": min(p) - tr[0] > max(p) - min(p)}
    res["verdict"] = verdict
    print(json.dumps(verdict), flush=True)
    return res


def phase_speed(ref, limit):
    runs = []
    for i in (1, 2, 3):
        for build in ("parent", "tree"):
            line = last_json(child([sys.executable, "bench.py", "--steps", "10", "--warmup", "2"], lib_env(build, ref), limit).stdout)
            rec = {"run": "bench_%s_%d" % (build, i), "build": build, "command": "python bench.py --steps 10 --warmup 2",
                   "value": line["value"], "ms_per_step": line.get("ms_per_step"), "kernel_ms": line.get("kernel_ms", {})}
            runs.append(rec)
            print(json.dumps(rec), flush=True)
    p = [r["value"] for r in runs if r["build"] == "parent"]
    t = [r["value"] for r in runs if r["build"] == "tree"]
    spread = (max(p) - min(p)) / min(p)
    gap = min(t) / max(p) - 1
    verdict = {"parent_spread": spread, "gap_best_parent_to_worst_tree": gap, "gap_of_means": (sum(t) / 3) / (sum(p) / 3) - 1,
               "every_tree_above_every_parent": min(t) > max(p), "gap_exceeds_three_spreads": gap > 3 * spread}
    verdict["gain"] = verdict["every_tree_above_every_parent"] and verdict["gap_exceeds_three_spreads"]
    cats = {}
    for c in ("contract", "contract_chain"):
        pc = [r["kernel_ms"][c] / 10 for r in runs if r["build"] == "parent" and c in r["kernel_ms"]]
        tc = [r["kernel_ms"][c] / 10 for r in runs if r["build"] == "tree" and c in r["kernel_ms"]]
        if pc and tc:
            cats[c] = {"parent_ms_per_step": pc, "tree_ms_per_step": tc, "change_of_means": (sum(tc) / len(tc)) / (sum(pc) / len(pc)) - 1}
    verdict["categories"] = cats
    print(json.dumps(verdict), flush=True)
    return {"runs": runs, "verdict": verdict}


def phase_profile(ref, limit):
    res = {"command": "rocprofv3 ... -- python bench.py --steps 2 --warmup 1; one process with --kernel-trace --stats, a second with "
                      "--pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_INSTS_SALU SQ_INSTS_SMEM and no tracing domain"}
    for build in ("parent", "tree"):
        t = _trace(build, ref, limit)
        t["full_grid"] = {k: v for k, v in t["full_grid"].items() if k in HEADLINE.values()}
        res[build] = {"trace": t}
        print(build, "trace", json.dumps(t), flush=True)
        res[build]["pmc"] = _pmc(build, ref, limit)
        print(build, "pmc", json.dumps(res[build]["pmc"]), flush=True)
    return res


def phase_same(ref, limit):
    res = {}
    d = tempfile.mkdtemp(prefix="entry_extents_")
    try:
        for leg, extra in (("headline", []), ("real_2048", ["--state", "real", "--walkers", "2048"])):
            blobs = {}
            for build in ("parent", "tree"):
                o = os.path.join(d, leg + "_" + build)
                child(BENCH2 + ["--dump-outputs", o] + extra, lib_env(build, ref), limit)
                blobs[build] = open(os.path.join(o, "amplitudes.npy"), "rb").read()
            res[leg] = {"command": " ".join(["python"] + BENCH2[1:] + ["--dump-outputs", "DIR"] + extra), "bytes": len(blobs["tree"]),
                        "amplitudes_equal_as_bytes": blobs["parent"] == blobs["tree"]}
            print(leg, json.dumps(res[leg]), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
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
    ap.add_argument("--phases", default="speed,profile,same")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entry_extents_ab.json"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child process")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref)
    assert os.path.exists(ref) and os.path.exists(TREE_LIB) and not os.path.samefile(ref, TREE_LIB)
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out["what"] = ("A/B of the parent build against this tree on the C4 headline (12x12, D = 8, chi = 32, f32, 49 152 walkers), one MI355X, "
                   "fresh processes, alternating parent and tree (PEPSGPU_LIB selects the parent's library)")
    for ph in a.phases.split(","):
        fn = {"trace3": phase_trace3, "speed": phase_speed, "profile": phase_profile, "same": phase_same}.get(ph)
        if fn:
            out[ph] = fn(ref, a.timeout)
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

"""A/B of the parent build against this tree for the leg-8 specialisation of the chained contraction pair (tgemm_chain_d8_kernel in
peps_amd/csrc/tgemm_d8.h, routed by tgemm_chain_launch): the C4 headline of bench.py on one GPU, every run a fresh child process
under its own time limit, the parent's library selected with PEPSGPU_LIB.  Modelled on scripts/wave_slots_ab.py.

    python scripts/chain_d8_ab.py --ref <parent's libpepsgpu.so> [--phases speed,trace3,pmc,same,full] [--out FILE]

phases (each adds its record to FILE, default profiles/chain_d8_ab.json; a phase stops at the first child that fails):
    speed    three alternating pairs of `python bench.py --steps 10 --warmup 2`.  A gain: every tree run above every parent run, and
             the gap from the best parent run to the worst tree run above the parent's own spread
    trace3   three `rocprofv3 --kernel-trace --stats` runs of the parent and one of the tree: the median of the full-grid launches of
             the chained pair (kept when the tree's median lies below the parent's range) and, as controls, of M, Y and the factor
    pmc      per build one `rocprofv3 --pmc` run with no tracing domain beside the counters: instructions and cycles per wave of the
             full-grid chained launches
    same     bench.py --steps 2 --warmup 1 --dump-outputs on both builds, headline and `--state real --walkers 2048`:
             amplitudes.npy equal as bytes
    full     one `python bench.py --full` per build: the full_rank and real_rank legs
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_slots_audit as audit_mod  # noqa: E402

TREE_LIB = os.path.join(ROOT, "peps_amd", "lib", "libpepsgpu.so")
GENERIC = "tgemm_chain_kernel<true, false, false, 6144, 6, false, false>"
# the kernel of the change, parent and tree name
ITEMS = {"chain": {"parent": GENERIC, "tree": "tgemm_chain_d8_kernel"}}
# what the change must leave alone
OTHERS = {"M": {"parent": "tgemm_direct_kernel<true, false, false, 2>", "tree": "tgemm_direct_kernel<true, false, false, 2>"},
          "Y": {"parent": "tgemm_direct_kernel<true, false, false, 1>", "tree": "tgemm_direct_kernel<true, false, false, 1>"},
          "factor": {"parent": "gram_chol_wave_split_kernel", "tree": "gram_chol_wave_split_kernel"},
          "chain_generic_left": {"parent": GENERIC, "tree": GENERIC}}
COUNTERS = ["SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_SMEM", "SQ_WAVES", "SQ_WAVE_CYCLES", "SQ_ACTIVE_INST_VALU", "SQ_VALU_MFMA_BUSY_CYCLES"]
BENCH2 = [sys.executable, "bench.py", "--steps", "2", "--warmup", "1"]


def child(cmd, env, limit, cwd=ROOT):
    e = dict(os.environ)
    e.pop("PEPSGPU_LIB", None)
    e.update(env)
    # the time limit is the child's own (`timeout` also ends what the child started); any failure ends the whole script
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd, env=e, capture_output=True, text=True, timeout=limit + 60)
    if r.returncode != 0:
        raise RuntimeError("child failed (%d): %s\n%s\n[...]\n%s" % (r.returncode, " ".join(cmd), r.stderr[:3000], r.stderr[-3000:]))
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


def _full_grid(tr, build):
    """the launches of the largest grid of each named kernel: the full-grid launches of the headline"""
    out = {"all_kernels_ms": sum(v["us_total"] for v in tr.values()) / 1e3}
    for name, k in list(ITEMS.items()) + list(OTHERS.items()):
        mine = {g: v for (kern, g), v in tr.items() if kern == k[build]}
        if mine:
            g = max(mine)
            out[name] = {"kernel": k[build], "grid": g, "block": mine[g]["block"], "launches": mine[g]["launches"],
                         "us_median": mine[g]["us_median"], "us_mean": mine[g]["us_mean"],
                         "ms_all_grids": sum(v["us_total"] for v in mine.values()) / 1e3}
    return out


def phase_trace3(ref, limit, _a):
    res = {"command": "rocprofv3 --kernel-trace --stats -- python bench.py --steps 2 --warmup 1; parent three times, tree once",
           "parent": [], "tree": []}
    for build in ("parent", "tree", "parent", "parent"):
        d = tempfile.mkdtemp(prefix="chain_d8_")
        try:
            child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "trace", "--"] + BENCH2,
                  lib_env(build, ref), limit)
            t = _full_grid(audit_mod.read_trace(d), build)
        finally:
            shutil.rmtree(d, ignore_errors=True)
        res[build].append(t)
        print(build, json.dumps(t), flush=True)
    verdict = {}
    for name in list(ITEMS) + list(OTHERS):
        p = [t[name]["us_median"] for t in res["parent"] if name in t]
        tr = [t[name]["us_median"] for t in res["tree"] if name in t]
        if p and tr:
            verdict[name] = {"parent_medians_us": p, "tree_median_us": tr[0], "parent_range_us": [min(p), max(p)],
                             "fall_us": _median(p) - tr[0], "outside_the_parents_range": tr[0] < min(p) or tr[0] > max(p),
                             "faster": tr[0] < min(p)}
    res["verdict"] = verdict
    print(json.dumps(verdict), flush=True)
    return res


def phase_pmc(ref, limit, _a):
    """counters of the full-grid chained launches, per wave (SQ_WAVES of the same launches)"""
    res = {"command": "rocprofv3 --pmc %s -- python bench.py --steps 2 --warmup 1 (no tracing domain)" % " ".join(COUNTERS)}
    for build in ("parent", "tree"):
        d = tempfile.mkdtemp(prefix="chain_d8_")
        try:
            child(["rocprofv3", "--pmc"] + COUNTERS + ["--output-format", "csv", "-d", d, "-o", "pmc", "--"] + BENCH2, lib_env(build, ref), limit)
            pm = audit_mod.read_pmc(d)
        finally:
            shutil.rmtree(d, ignore_errors=True)
        mine = {g: v for (kern, g), v in pm.items() if kern == ITEMS["chain"][build]}
        if not mine:
            raise RuntimeError("no chained launches among the counters of the %s build" % build)
        g = max(mine)
        c = {k: v[0] for k, v in mine[g].items()}
        n = {k: v[1] for k, v in mine[g].items()}
        waves = c.get("SQ_WAVES", 0.0)
        rec = {"kernel": ITEMS["chain"][build], "grid": g, "dispatches": max(n.values()), "sums": c}
        if waves:
            rec["per_wave"] = {k: v / waves for k, v in c.items() if k != "SQ_WAVES"}
        if c.get("SQ_WAVE_CYCLES"):
            rec["valu_busy_share"] = c.get("SQ_ACTIVE_INST_VALU", 0.0) / c["SQ_WAVE_CYCLES"]
        res[build] = rec
        print(build, json.dumps(rec), flush=True)
    if "per_wave" in res["parent"] and "per_wave" in res["tree"]:
        res["tree_over_parent_per_wave"] = {k: res["tree"]["per_wave"][k] / v for k, v in res["parent"]["per_wave"].items()
                                            if v and k in res["tree"]["per_wave"]}
        print(json.dumps(res["tree_over_parent_per_wave"]), flush=True)
    return res


def phase_speed(ref, limit, _a):
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
               "every_tree_above_every_parent": min(t) > max(p), "gap_exceeds_parent_spread": gap > spread}
    verdict["gain"] = verdict["every_tree_above_every_parent"] and verdict["gap_exceeds_parent_spread"]
    cats = {}
    for c in ("cholesky", "contract", "contract_chain"):
        pc = [r["kernel_ms"][c] / 10 for r in runs if r["build"] == "parent" and c in r["kernel_ms"]]
        tc = [r["kernel_ms"][c] / 10 for r in runs if r["build"] == "tree" and c in r["kernel_ms"]]
        if pc and tc:
            cats[c] = {"parent_ms_per_step": pc, "tree_ms_per_step": tc, "change_of_means": (sum(tc) / len(tc)) / (sum(pc) / len(pc)) - 1}
    verdict["categories"] = cats
    print(json.dumps(verdict), flush=True)
    return {"runs": runs, "verdict": verdict}


def phase_same(ref, limit, _a):
    res = {}
    d = tempfile.mkdtemp(prefix="chain_d8_")
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


def phase_full(ref, limit, _a):
    res = {"command": "python bench.py --full"}
    for build in ("parent", "tree"):
        line = last_json(child([sys.executable, "bench.py", "--full"], lib_env(build, ref), max(limit, 900)).stdout)
        res[build] = {"value": line["value"], "full_rank": (line.get("full_rank") or {}).get("value"),
                      "real_rank": (line.get("real_rank") or {}).get("value")}
        print(build, json.dumps(res[build]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="libpepsgpu.so of the parent commit")
    ap.add_argument("--phases", default="speed,trace3,pmc,same")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_d8_ab.json"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child process")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref)
    assert os.path.exists(ref) and os.path.exists(TREE_LIB) and not os.path.samefile(ref, TREE_LIB)
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out["what"] = ("A/B of the parent build against this tree on the C4 headline (12x12, D = 8, chi = 32, f32, 49 152 walkers), one MI355X, "
                   "fresh processes, alternating parent and tree (PEPSGPU_LIB selects the parent's library)")
    fns = {"trace3": phase_trace3, "speed": phase_speed, "pmc": phase_pmc, "same": phase_same, "full": phase_full}
    for ph in a.phases.split(","):
        if ph not in fns:
            raise SystemExit("unknown phase " + ph)
        out[ph] = fns[ph](ref, a.timeout, a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

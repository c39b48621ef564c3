"""CPU suite: `python bench.py --gpus N` starts N ranks itself (child torch.distributed.run) and rank 0 prints ONE JSON line
with n_gpus = N.  --dry-run skips the device work (there is no GPU here): launcher, rendezvous (gloo through the
PEPS_BENCH_BACKEND hook), barrier, max-over-ranks reduction and the JSON contract are what is covered."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env=None):
    env = dict(os.environ, PEPS_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_gpus_2_launches_two_ranks():
    out = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--dry-run"])
    assert out["n_gpus"] == 2 and out["ranks_reported_by_backend"] == 2
    assert out["dry_run"] is True and out["value"] is None          # a dry run never carries a number
    assert out["scaling"] == "weak" and out["metric"] == "configuration-amplitudes/sec"


def test_bench_gpus_1_dry_run_is_single_process():
    out = _run(["--gpus", "1", "--dry-run"])
    assert out["n_gpus"] == 1 and out["ranks_reported_by_backend"] == 1


def _bench_module():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_result_line_stays_compact_and_complete():
    """the stdout line keeps every headline field and the headline of each leg, in a few KB (the full record of round 6 was
    25 KB: a reader that keeps only the end of the output lost the line), and drops nothing the full record does not hold"""
    bench = _bench_module()
    full = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_driver_run.json")))
    line = bench.result_line(full)
    text = json.dumps(line)
    assert len(text) < 6000
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "higher_is_better"):
        assert line[k] == full[k]
    assert line["real_rank"]["value"] == full["real_rank"]["value"]
    assert line["full_rank"]["ms_per_step"] == full["full_rank"]["ms_per_step"]
    assert line["other_modes"]["complex128"]["amp_per_s"] == full["other_modes"]["complex128"]["amp_per_s"]
    err = bench.result_line({"metric": "m", "value": 1.0, "real_rank": {"error": "x" * 5000}})
    assert err["real_rank"] == {"error": "x" * 300}


def test_dump_outputs_writes_float64_and_samples_large_batches(tmp_path, monkeypatch):
    import numpy as np
    bench = _bench_module()
    a = np.arange(1000, dtype=np.float64) * 0.5
    info = bench.dump_outputs(str(tmp_path / "small"), {"amplitudes": a})
    got = np.load(tmp_path / "small" / "amplitudes.npy")
    assert info["sampled"] is False and got.dtype == np.float64 and np.array_equal(got, a)
    # above the cap: a seeded sample, the same indices on every run, stored beside the values
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4000)
    for d in ("s1", "s2"):
        info = bench.dump_outputs(str(tmp_path / d), {"amplitudes": a})
        assert info["sampled"] is True
    i1, i2 = (np.load(tmp_path / d / "amplitudes_index.npy") for d in ("s1", "s2"))
    v1 = np.load(tmp_path / "s1" / "amplitudes.npy")
    assert np.array_equal(i1, i2) and v1.nbytes + i1.nbytes <= 4000
    assert np.array_equal(v1, a[i1.astype(np.int64)])

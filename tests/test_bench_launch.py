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


def test_config_pool_makes_the_batches_of_the_serial_generators(monkeypatch):
    """the inputs of the timed steps made in chunks by worker processes are, array for array, what the generators of
    peps_amd.synthetic make in one piece per batch (a batch that is not a whole number of chunks included)"""
    import numpy as np
    from peps_amd import synthetic
    bench = _bench_module()
    monkeypatch.setattr(bench.ConfigPool, "CHUNK", 96)
    L, nw, total = 12, 250, 3
    for rank, world in ((0, 1), (1, 2)):
        seeds = bench.batch_seeds(nw, total, rank, world)
        assert seeds == [7 + (s * world + rank) * nw for s in range(total)]
        for real, workers in ((False, 3), (True, 3), (False, 1)):
            got = bench.ConfigPool(real, L, nw, seeds, workers).batches()
            want = [synthetic.make_configs_near_neel(L, nw, seed0=s) if real else synthetic.make_configs(L, nw, "heisenberg", seed0=s)
                    for s in seeds]
            assert len(got) == total
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


def test_plain_run_leaves_the_extras_to_full():
    """--full is off by default; a plain run's parser still accepts every switch of a --full run"""
    bench = _bench_module()
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"]
        assert bench.parse().full is False
        sys.argv = sys.argv + ["--full", "--no-real-rank"]
        args = bench.parse()
        assert args.full is True and args.no_real_rank is True
    finally:
        sys.argv = argv


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

"""Checkpoints of the device-resident Optimizer (SaveCheckpoint_ / WriteTrajectoryCsv_, optimizer_impl.h:1980-2049 of the reference)
through hostapi.guarded_optimize_exact_sum: every_n_steps = 2 over 5 iterations on the 2x2 transverse-field Ising state."""
import os

import numpy as np
import pytest

from oracle import qlten_io, vmc
from peps_amd import synthetic

pytestmark = pytest.mark.gpu

F64 = 1
TFIM = ("tfim", (1.0,))
ADAM = (0.9, 0.999, 1e-8, 0.0)


@pytest.fixture(scope="module")
def tfim(fixtures_dir):
    s = qlten_io.load_sitps(os.path.join(fixtures_dir, "transverse_ising_tps_double_from_simple_update"))
    return synthetic.sitps_to_flat(s, 4), np.array(vmc.generate_all_binary_configs(2, 2), dtype=np.int32)


def _csv(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "iteration,energy,energy_error" and lines[-1] == ""
    rows = [x.split(",") for x in lines[1:-1]]
    return [int(r[0]) for r in rows], np.array([float(r[1]) for r in rows]), np.array([float(r[2]) for r in rows])


def test_checkpoints_every_two_steps(tfim, tmp_path):
    from peps_amd import hostapi
    flat, cfgs = tfim
    base = str(tmp_path / "ckpt")
    err = np.linspace(0.01, 0.02, 6)
    got = hostapi.guarded_optimize_exact_sum(flat, cfgs, 8, *TFIM, "adam", 0.02, ADAM, 5, dtype=F64, batch=16,
                                             checkpoint=dict(every_n_steps=2, base_path=base), schedule=dict(error_override=err))
    assert sorted(os.listdir(base)) == ["energy_trajectory.csv", "step_2", "step_4"]
    for step in (2, 4):
        d = os.path.join(base, "step_%d" % step)
        # the state after the step of iteration `step`: that of an unguarded run of step + 1 iterations
        _, want = hostapi.optimize_exact_sum(flat, cfgs, 8, *TFIM, "adam", 0.02, ADAM, step + 1, dtype=F64, batch=16)
        assert hostapi.load_sitps(d, 4).tobytes() == want.tobytes()
        meta = dict(line.split(" ") for line in open(os.path.join(d, "checkpoint_meta.txt")).read().strip().split("\n"))
        assert list(meta) == ["step", "energy", "error"] and int(meta["step"]) == step
        assert float(meta["energy"]) == got["energies"][step] and float(meta["error"]) == err[step]      # 17 digits round-trip
        it, e, er = _csv(os.path.join(d, "trajectory_snapshot.csv"))
        assert it == list(range(step + 1))
        assert e.tobytes() == got["energies"][:step + 1].tobytes() and er.tobytes() == err[:step + 1].tobytes()
    it, e, er = _csv(os.path.join(base, "energy_trajectory.csv"))      # rewritten at every checkpoint: the last one stands
    assert it == list(range(5)) and e.tobytes() == got["energies"][:5].tobytes() and er.tobytes() == err[:5].tobytes()
    # checkpoints change nothing else
    plain, state = hostapi.optimize_exact_sum(flat, cfgs, 8, *TFIM, "adam", 0.02, ADAM, 5, dtype=F64, batch=16)
    assert got["energies"].tobytes() == plain.tobytes() and got["state"].tobytes() == state.tobytes()


def test_nothing_is_written_when_disabled(tfim, tmp_path):
    from peps_amd import hostapi
    flat, cfgs = tfim
    base = str(tmp_path / "off")
    hostapi.guarded_optimize_exact_sum(flat, cfgs, 8, *TFIM, "adam", 0.02, ADAM, 3, dtype=F64, batch=16,
                                       checkpoint=dict(every_n_steps=0, base_path=base))
    hostapi.guarded_optimize_exact_sum(flat, cfgs, 8, *TFIM, "adam", 0.02, ADAM, 3, dtype=F64, batch=16, checkpoint=dict(every_n_steps=1))
    hostapi.guarded_optimize_exact_sum(flat, cfgs, 8, *TFIM, "adam", 0.02, ADAM, 3, dtype=F64, batch=16)
    assert not os.path.exists(base) and os.listdir(str(tmp_path)) == []


def test_fermionic_checkpoint_holds_the_stored_tensors(fixtures_dir, tmp_path):
    import itertools
    from peps_amd import fermion, hostapi
    st = fermion.FermionState.load(os.path.join(fixtures_dir, "spinless_fermion_tps_t2_0.000000_double_from_simple_update"))
    cfgs = np.array([np.array(p).reshape(2, 2) for p in sorted(set(itertools.permutations([0, 0, 1, 1])))], dtype=np.int32)
    base = str(tmp_path / "fermion")
    model = ("spinless", (1.0, 0.0, 0.0))
    hostapi.fermion_guarded_optimize_exact_sum(st, cfgs, 16, *model, "sgd", 0.1, (0.0, 0.0, 0.0), 2, dtype=F64, batch=6,
                                               checkpoint=dict(every_n_steps=1, base_path=base))
    _, stored = hostapi.fermion_optimize_exact_sum(st, cfgs, 16, *model, "sgd", 0.1, (0.0, 0.0, 0.0), 2, dtype=F64, batch=6)
    assert os.listdir(base).count("step_1") == 1 and "step_2" not in os.listdir(base)
    assert hostapi.load_sitps(os.path.join(base, "step_1"), st.D).tobytes() == stored.tobytes()

"""The MinSR step of the C++ Optimizer (MinSRParams, Optimizer::MinSRUpdate in peps_amd/host/qlpeps_gpu.h) through
hostapi.minsr_step_samples, on the reference's 2 x 2 transverse-field Ising state (float64, chi = 8, the 16 configurations as a sample
set with weight 1).

The energy after the step.  With weight 1 per configuration the "energy" is the plain mean of the 16 local energies, not a variational
energy, and the MinSR step need not lower it.  On the oracle (oracle/sr.py::minsr_direction on O* samples and local energies from
oracle/vmc.py, r_pinv = 1e-12, a_pinv = 0, soft cutoff) it goes from -5.239677446524458 to -5.234431690212235 at lr = 0.1, to
-5.235879109128816 at lr = 0.05 and to -5.237877516004191 at lr = 0.02: up at every one of the three rates, so there is no rate at which
"energy_after < energy_before" could be asked of the device.  The test asks for more instead: energy_after equals the oracle's value at
lr = 0.1 (and is therefore finite, and on the same side of energy_before as the oracle's)."""
import os

import numpy as np
import pytest

from oracle import qlten_io, vmc
from peps_amd import synthetic

pytestmark = pytest.mark.gpu

F64 = 1
LR = 0.1
ORACLE_E_BEFORE = -5.239677446524458
ORACLE_E_AFTER = -5.234431690212235        # lr = 0.1
KW = dict(r_pinv=1e-12, a_pinv=0.0, soft_cutoff=True)


@pytest.fixture(scope="module")
def tfim(fixtures_dir):
    s = qlten_io.load_sitps(os.path.join(fixtures_dir, "transverse_ising_tps_double_from_simple_update"))
    return s, synthetic.sitps_to_flat(s, 4), np.array(vmc.generate_all_binary_configs(2, 2), dtype=np.int32)


@pytest.fixture(scope="module")
def host_step(tfim):
    from peps_amd import hostapi
    s, flat, cfgs = tfim
    return hostapi.minsr_step_samples(flat, cfgs, 8, "tfim", (1.0,), LR, dtype=F64, **KW)


def test_minsr_step_of_the_optimizer_equals_the_c_abi(tfim, host_step):
    """holes, grad_accumulate, sr_append, opt_begin, minsr_direction put together from the C ABI: both sides run the same kernels on the
    same inputs, so theta_1 agrees to 1e-12 lr max|g|."""
    from peps_amd import capi, hostapi
    from peps_amd.capi import LEFT, RIGHT, UP, DOWN, HORIZONTAL
    s, flat, cfgs = tfim
    amps, en, _, _ = hostapi.energy_and_holes(flat, cfgs, 8, "tfim", (1.0,), False, F64)
    ctx = capi.Context(2, 2, 4, 2, 8, dtype=capi.F64, max_walkers=16)
    ctx.state_upload(flat)
    ctx.set_configs(cfgs)
    ctx.generate_bmps_approach(UP)
    for row in range(2):
        ctx.init_bten(LEFT, row)
        ctx.grow_full_bten(RIGHT, row, 1, True)
        for col in range(2):
            ctx.punch_hole_store(row, col, HORIZONTAL)
            if col < 1:
                ctx.shift_bten_window(RIGHT)
        if row < 1:
            ctx.shift_bmps_window(DOWN)
    ctx.grad_reset()
    ctx.grad_accumulate(amps, en, exact_sum=False)
    ctx.sr_begin(16)
    ctx.sr_append(amps)
    ctx.opt_begin()
    e0, _ = ctx.opt_gradient_from_accumulators(float(np.sum(en)), 16.0)
    nrm, cinfo = ctx.minsr_direction(en, e0, **KW)
    g = ctx.opt_get_gradient()
    ctx.close()
    state, info = host_step
    want = flat - LR * g
    err = float(np.max(np.abs(state - want)))
    print("MinSR step: |x| %.12e / %.12e, max |theta - ref| = %.3e (bound %.3e), E %.12f -> %.12f, info %s"
          % (info["direction_norm"], nrm, err, 1e-12 * LR * float(np.max(np.abs(g))), info["energy_before"], info["energy_after"], info))
    assert err <= 1e-12 * LR * float(np.max(np.abs(g)))
    assert abs(info["energy_before"] - e0) < 1e-12
    assert abs(info["direction_norm"] - nrm) <= 1e-12 * nrm
    assert (info["lambda_max"], info["cutoff"], info["n_kept"], info["sweeps"]) == (cinfo["lambda_max"], cinfo["cutoff"], cinfo["n_kept"],
                                                                                    cinfo["sweeps"])
    assert info["n_kept"] == 15 and 1 <= info["sweeps"] <= 30          # 16 centred samples: one zero eigenvalue
    assert np.all(state[flat == 0] == 0)
    # the energies against the oracle's (module docstring): the suite's float64 energy parity is 1e-10; the step adds the direction's
    # parity (1e-7 relative, tests/test_gpu_minsr.py) times lr |x| = 0.04 times the slope of the energy, of order one
    assert np.isfinite(info["energy_after"])
    assert abs(info["energy_before"] - ORACLE_E_BEFORE) < 1e-9
    assert abs(info["energy_after"] - ORACLE_E_AFTER) < 1e-7


def test_complex_twin_follows_the_real_step(tfim, host_step):
    from peps_amd import hostapi
    s, flat, cfgs = tfim
    state, info = host_step
    sc, ic = hostapi.minsr_step_samples(flat.astype(np.complex128), cfgs, 8, "tfim", (1.0,), LR, **KW)
    print("complex twin: max |Re theta - theta_real| = %.3e, max |Im theta| = %.3e, dE_after %.3e"
          % (float(np.max(np.abs(sc.real - state))), float(np.max(np.abs(sc.imag))), abs(ic["energy_after"] - info["energy_after"])))
    assert sc.dtype == np.complex128
    assert np.max(np.abs(sc.real - state)) < 1e-10 and np.max(np.abs(sc.imag)) < 1e-10
    assert abs(ic["energy_before"] - info["energy_before"]) < 1e-10 and abs(ic["energy_after"] - info["energy_after"]) < 1e-10
    assert abs(ic["direction_norm"] - info["direction_norm"]) < 1e-10


def test_an_evaluator_without_samples_is_refused(tfim):
    """MinSRParams with the exact-summation evaluator: no sample set, so Optimizer::MinSRUpdate throws std::invalid_argument"""
    from peps_amd import hostapi
    s, flat, cfgs = tfim
    with pytest.raises(ValueError):
        hostapi.minsr_step_samples(flat, cfgs, 8, "tfim", (1.0,), LR, dtype=F64, exact_sum=True, **KW)

"""The condition under which test_gpu_env_config.py may hold the HIP kernels to the project's tolerances (TOL_RK4 = 1e-10, TOL_RK45 = 1e-8,
x 50 with the thermal field): the case must be well conditioned.  Checked here on the CPU, on the same (configuration, input batch) pairs:
when the largest component of every start row moves by one ulp, the oracle's own answer moves by less than tolerance / 100 in both steps,
and no RK45 solve changes its number of accepted points or attempts (a fork of the accept / reject sequence would make any difference in
rounding visible at the size of a step).  An input that fails this is to be replaced, not met with a wider tolerance."""
import numpy as np
import pytest

import env_config_cases as ecc


@pytest.fixture(scope="module")
def stg(oracle_mod):
    import spin_torque_gym_amd as s
    return s


@pytest.mark.parametrize("name", [c[0] for c in ecc.matrix_cases()])
def test_oracle_moves_less_than_a_hundredth_of_the_tolerance_per_ulp(stg, name):
    from helpers import OracleBackend
    name, n, seed, f64, over, kw = ecc.case(name)
    m0, tgt, acts = ecc.inputs(n, seed, f64=f64)
    base, c0, att0 = ecc.run_steps(stg, n, m0, tgt, acts, B=OracleBackend, over=over, **kw)
    moved, c1, att1 = ecc.run_steps(stg, n, m0, tgt, acts, B=OracleBackend, over=over, ulp=True, **kw)
    tol = ecc.tol_for(kw["solver"], kw["include_thermal_fluctuations"])
    worst = 0.0
    for k, (a, b) in enumerate(zip(base, moved)):
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["term"], b["term"]), (name, k)
        worst = max(worst, float(np.abs(a["m"] - b["m"]).max()))
    print(f"{name}: oracle |dm| per ulp of m0 = {worst:.3e} (tolerance / 100 = {tol / 100:.1e}), work {c0}")
    assert not np.array_equal(base[0]["m"], moved[0]["m"]) or (base[0]["status"] == 1).all()      # (the ulp did reach the solver)
    assert worst < tol / 100, (name, worst)
    assert c0 == c1 and np.array_equal(att0, att1), (name, c0, c1)       # accepted points (oracle work units) and attempts: no fork

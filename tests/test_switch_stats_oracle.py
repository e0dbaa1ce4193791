"""What the counts of stg_switch_stats should be, asked of the CPU oracle (no GPU): tests/switch_stats_ref.py oracle_path runs the header's
stream rule on helpers.OracleBackend -- one backend of R problems per condition at env_id0 = g * trial_stride + trial0, phase after phase
at env_step + p -- and tests/test_gpu_switch_stats_config.py holds the fused kernel to its counts integer for integer.  That comparison
is only sound if no trial of the oracle sits near a decision: here, from the oracle alone, every projection of every case is shown to lie
further than `margin` from threshold 0 and from every inner edge of the 7 bins.  margin = 100 x the tolerance tests/test_gpu_brown_config.py
holds stg_solve to the oracle at (1e-10): 1e-8.  A condition, not a measurement: the GPU test asserts it again before it compares.

Cases: the conditions of switch_stats_ref.conditions(), R = 192, P = 1 and P = 3 (equilibrate 30 ps, pulse, relax 20 ps); rk4 / euler +
brown, rk4 + ou (correlation_time 7e-13), rk4 + white at the defaults and at the three (max_step, gamma, temperature) settings of
tests/test_wave_config_host.py; RK45 + white at a current below the solver's gate (switch_stats_ref.RK45_J_SCALE says why).

Measured here, smallest distance of any projection to a decision over the 8 cases of a form (bound 1e-8): rk4 + brown 4.2e-5, euler +
brown 4.8e-5, rk4 + ou 4.0e-3, rk4 + white 4.0e-3, rk45 + white 3.2e-2."""
import numpy as np
import pytest

import brown_ref as br
import switch_stats_ref as ssr

CASES = [(s, n, k, P) for s, n in ssr.ORACLE_FORMS for k in (None, 0, 1, 2) for P in (1, 3)]
_SMALLEST = {}


@pytest.fixture(scope="module")
def stg(oracle_mod):
    import spin_torque_gym_amd as s
    return s


def test_settings_and_margin_are_the_projects():
    import test_brown_oracle
    import test_gpu_brown_config
    import wave_config_cases as wcc
    assert ssr.SETTINGS == test_brown_oracle.SETTINGS and ssr.CORR_TIME == wcc.CORR_TIME != 1e-12
    assert ssr.margin() == 100 * test_gpu_brown_config.TOL == 1e-8
    from spin_torque_gym_amd import _lib
    assert ssr.WAVES == _lib.SWITCH_STATS_WAVES


@pytest.mark.parametrize("solver,noise,k,P", CASES)
def test_oracle_cases_are_conditioned(stg, solver, noise, k, P):
    case = ssr.oracle_case(stg, solver, noise, k, P)
    n_sw, n_failed, hist = case["counts"]
    print(f"{solver} {noise} setting {k} P = {P}: switched {n_sw.tolist()}, smallest distance to a decision {case['distance']:.2e} (margin {ssr.margin():.0e})")
    _SMALLEST[(solver, noise)] = min(_SMALLEST.get((solver, noise), np.inf), case["distance"])
    ssr.check_conditioned(case, solver, noise, k, P)
    # the settings reach the chain: another setting, other projections
    if k is not None:
        assert not np.array_equal(case["proj"], ssr.oracle_case(stg, solver, noise, None, P)["proj"])


@pytest.mark.parametrize("k", (None, 0, 1))
def test_max_step_decides_in_a_phase_of_every_setting_that_allows_it(k):
    """dt = min(max_step, T / 100): a phase of the three-phase chain has n > 100 sub-steps of max_step each (the defaults, settings 0 and
    1), next to phases with n = 100; setting 2 (max_step = 1e-10) has none, for the reason at switch_stats_ref.LONG_RELAX"""
    max_step = 1e-12 if k is None else ssr.SETTINGS[k][0]
    _, T = ssr.phases(k, 3)
    n, dt = br.substeps(T.reshape(-1), max_step)
    print(f"setting {k}: sub-steps {sorted(set(n.tolist()))}")
    assert (n > 100).any() and (n == 100).any()
    assert (dt[n > 100] >= max_step).all() and (dt[n > 100] < max_step * 1.01).all()
    if k == 1:
        assert 333 in n.tolist() and (br.substeps(ssr.phases(k, 1)[1][0], max_step)[0] > 100).any()       # the pulses themselves: P = 1 too
    n2, _ = br.substeps(ssr.phases(2, 3)[1].reshape(-1), ssr.SETTINGS[2][0])
    assert (n2 == 100).all()


@pytest.mark.parametrize("P", (1, 3))
def test_rk45_case_is_unsaturated_and_conditioned(stg, P):
    case = ssr.oracle_case(stg, "rk45", "white", None, P)
    pr = case["proj"].reshape(ssr.G, ssr.ORACLE_R)
    print(f"rk45 white P = {P}: proj per condition {pr.min(axis=1).tolist()} ... spread {(pr.max(axis=1) - pr.min(axis=1)).tolist()}, distance {case['distance']:.2e}")
    _SMALLEST[("rk45", "white")] = min(_SMALLEST.get(("rk45", "white"), np.inf), case["distance"])
    ssr.check_conditioned(case, "rk45", "white", None, P)
    assert (np.abs(case["J"]) < 1e-12).all() and ((pr.max(axis=1) - pr.min(axis=1)) > 1e-8).all()       # below the gate; the field tells the trials apart
    # ... and the file's own J saturates every trial (why another input is needed)
    m0, J, T, tgt = ssr.conditions()
    m, _ = ssr.oracle_path(stg, "rk45", "white", m0, J[None], T[None], 8, env_step=ssr.ORACLE_ENV_STEP)
    assert (ssr.proj(m, np.repeat(tgt, 8, axis=0)) > 1.0 - 1e-12).all()


def test_oracle_path_is_the_headers_stream_rule(stg, oracle_mod):
    """trial r of condition g is the oracle's solve on the stream of env id g * trial_stride + trial0 + r at env_step + p -- spelled out
    with oracle.simple_solve, ids beyond 2^33 included; a skipped phase passes m through, a failed one ends the trial"""
    from helpers import oracle_config, oracle_params
    m0, Jp, Tp, tgt = ssr.conditions()
    J = np.stack([np.zeros(ssr.G), Jp, np.zeros(ssr.G)])
    T = np.stack([np.array([3e-11, 0.0, 3e-11]), Tp, np.array([2e-11, 2e-11, -1e-11])])
    R, trial0, stride, step = 5, 2 ** 33 + 5, 2 ** 34, 6
    m, failed = ssr.oracle_path(stg, "rk4", "brown", m0, J, T, R, env_step=step, trial0=trial0, trial_stride=stride)
    cfg = oracle_config(ssr.env_config("rk4", "brown"))
    po = oracle_params(ssr.flat_tables(stg))[0]
    for g in range(ssr.G):
        for r in range(R):
            x, bad = m0[g], False
            for p in range(3):
                if T[p, g] == 0.0 or bad:
                    continue
                o = oracle_mod.simple_solve(x, T[p, g], po, cfg, J[p, g], env_id=g * stride + trial0 + r, env_step=step + p)
                x, bad = o["m_final"], not o["success"]
            assert np.array_equal(m[:, g * R + r], x) and failed[g * R + r] == bad, (g, r)
    assert failed.reshape(ssr.G, R).all(axis=1).tolist() == [False, False, True]
    small, _ = ssr.oracle_path(stg, "rk4", "brown", m0, J, T, R, env_step=step, trial0=5, trial_stride=stride)
    assert np.abs(small - m).max() > 1e-3                                          # the high bits of the id are part of the key


def test_zz_smallest_distances():
    """prints what the tests above measured (the module docstring and profiles/NOTEBOOK.md hold the figures of a run)"""
    for (solver, noise), d in sorted(_SMALLEST.items()):
        print(f"{solver} + {noise}: smallest distance of a projection to a decision = {d:.2e}")

"""The waveform restatements off their defaults, host side (no GPU): what tests/test_gpu_wave_config.py holds the kernels against is
itself pinned here.

  * tests/waveform_ref.py with gamma, max_step, temperature and the thermal field against the fixed-step rows the reference computed
    (tests/golden/G24_wave_config.npz), thermal off and on, at TOL_RK4;
  * its two noise models on rectangular pulses in zero field against oracle.simple_solve at several max_step / gamma / temperature
    values -- the Ornstein-Uhlenbeck branch, which the reference solvers do not have, is anchored this way;
  * tests/wave_step_ref.py under the non-default episode configuration against the env steps of G24, and its SOT and VCMA resistance
    forms against oracle.resistance;
  * the builder of the knots cases (tests/test_gpu_knots_config.py) against the shaped case, bit for bit;
  * what G24 holds."""
import numpy as np
import pytest

from conftest import sot_default_params, stt_default_params, vcma_default_params
from env_config_cases import FIXED_MAX_STEPS, RK45_SETTINGS, TOL_RK4
import wave_config_cases as wcc
import wave_step_ref
import waveform_ref


def test_g24_covers_what_it_should(golden):
    g = golden("G24_wave_config")
    solver, thermal = g["sv_solver"], g["sv_thermal"]
    rk = solver == 2
    for s in RK45_SETTINGS:
        sel = rk & ~thermal & (g["sv_rtol"] == s["rtol"]) & (g["sv_atol"] == s["atol"]) & (g["sv_max_step"] == s["max_step"]) & (g["sv_gamma"] == s["gamma"])
        assert (sel & (g["sv_kj"] > 0) & (g["sv_kh"] > 0)).any() and (sel & (g["sv_kj"] == 0) & (g["sv_kh"] > 0)).any(), s
    for method in (0, 1):
        for ms in FIXED_MAX_STEPS:
            assert ((solver == method) & ~thermal & (g["sv_max_step"] == ms)).sum() == 2
        assert set(g["sv_temperature"][(solver == method) & thermal]) == {77.0, 250.0, 450.0}
    assert (rk & thermal).sum() >= 2 and len({(r, a) for r, a in zip(g["sv_rtol"][rk & thermal], g["sv_atol"][rk & thermal])}) == 2
    assert (g["sv_env_id"][thermal] > 0).all() and (g["sv_env_step"][thermal] > 0).all()
    assert (g["sv_attempts"][rk] > g["sv_n_points"][rk]).any() and g["sv_success"].all()
    assert int(g["sv_n_points"][~rk].max()) <= 1000
    k = int(g["sv_traj_case"])
    assert rk[k] and len(g["sv_traj_t"]) == g["sv_n_points"][k] + 1 == len(g["sv_traj_energy"]) == len(g["sv_traj_torques"])
    # env level: every episode field off its default, three-step episodes, both limits hit, a float64 action float32 cannot carry
    assert (g["ev_max_duration"], g["ev_success_threshold"], g["ev_energy_penalty_weight"], g["ev_max_steps"], g["ev_temperature"]) == \
        (2e-9, 0.6, 0.25, 3, 250.0) and len(g["ev_targets"]) == 5
    assert (g["ev_max_current"][~g["ev_thermal"]] == 1.5e6).all() and g["ev_thermal"].any()
    assert (np.abs(g["ev_action"][:, 0]) > g["ev_max_current"]).any() and (g["ev_action"][:, 1] > 2e-9).any()
    f64 = g["ev_act_f64"]
    assert f64.any() and (g["ev_action"][f64].astype(np.float32).astype(np.float64) != g["ev_action"][f64]).any(axis=1).all()
    assert (np.abs(g["ev_alignment"] - 0.6) > 1e-6).all() and g["ev_terminated"].any() and g["ev_truncated"].any()
    assert max(np.bincount(g["ev_episode"])) == 3 and set(g["ev_solver"]) == {0, 1} and set(g["ev_max_step"]) == set(FIXED_MAX_STEPS)


def test_restatement_reproduces_the_golden_fixed_step_rows(golden, oracle_mod):
    g = golden("G24_wave_config")
    worst = {False: 0.0, True: 0.0}
    for k in np.nonzero(g["sv_solver"] < 2)[0]:
        cur, fld = wcc.g24_solve_knots(g, k)
        p = stt_default_params(volume=float(g["sv_volume"][k]))
        thermal = None
        if g["sv_thermal"][k]:
            thermal = waveform_ref.thermal_field(oracle_mod, p, "stt_mram", float(g["sv_gamma"][k]), float(g["sv_temperature"][k]),
                                                 int(g["sv_seed"][k]), [int(g["sv_env_id"][k])], int(g["sv_env_step"][k]))
        r = waveform_ref.solve(g["sv_m0"][k][None], [float(g["sv_T"][k])], p, wcc.g24_solver(g, k), current=cur, field=fld,
                               max_step=float(g["sv_max_step"][k]), temperature=float(g["sv_temperature"][k]), gamma=float(g["sv_gamma"][k]),
                               thermal=thermal)
        err = float(np.abs(r["m_final"][0] - g["sv_m_final"][k]).max())
        worst[bool(g["sv_thermal"][k])] = max(worst[bool(g["sv_thermal"][k])], err)
        assert bool(r["success"][0]) and int(r["n_steps"][0]) == int(g["sv_n_points"][k]), k
        assert err <= TOL_RK4, (k, err)
    print(f"worst |m_ref - m_golden|: thermal off {worst[False]:.2e}, thermal on {worst[True]:.2e}")


def test_restatement_reproduces_the_golden_env_steps(golden, oracle_mod):
    g = golden("G24_wave_config")
    worst = 0.0
    for k in range(len(g["ev_T"])):
        cur, fld = wcc.g24_env_tables(g, k)
        p = stt_default_params(volume=float(g["ev_volume"][k]))
        st = dict(m=g["ev_m_before"][k][None], target=g["ev_target"][k][None], total_energy=[g["ev_etot_before"][k]], step_count=[g["ev_step_before"][k]])
        thermal = None
        if g["ev_thermal"][k]:
            thermal = dict(oracle=oracle_mod, seed=int(g["ev_seed"]), env_id0=int(g["ev_env_id"]), rng_step=[int(g["ev_step_before"][k])])
        r = wave_step_ref.step(st, wcc.g24_env_action(g, k), p, ("rk4", "euler")[int(g["ev_solver"][k])], current=cur, field=fld,
                               cfg=wcc.g24_env_cfg(g, k), thermal=thermal)
        assert r["J"][0] == g["ev_J"][k] and r["T"][0] == g["ev_T"][k] and r["status"][0] == wave_step_ref.STATUS_OK, k
        got = dict(m=r["m"][0], obs=r["obs"][0], reward=r["reward"][0], terminated=r["terminated"][0], truncated=r["truncated"][0], energy=r["energy"][0])
        worst = max(worst, wcc.check_step_against_g24(g, k, got, TOL_RK4, "restatement"))
    print(f"worst |m_ref - m_golden| over {len(g['ev_T'])} env steps = {worst:.2e}")


@pytest.mark.parametrize("noise", ("white", "ou"))
@pytest.mark.parametrize("method", ("rk4", "euler"))
def test_thermal_restatement_is_the_oracles_rectangular_solve(oracle_mod, method, noise):
    """rectangular pulses in zero field: the restatement's thermal branches against oracle.simple_solve on the same stream"""
    p = stt_default_params(volume=wcc.VOL_THERMAL)
    rng = np.random.default_rng(6)
    n = 6
    m0 = wcc.unit_rows(rng, n)
    T, J = rng.uniform(2e-11, 2e-10, n), rng.uniform(-2e6, 2e6, n) * wcc.J_THERMAL
    for ms, gamma, temp in ((2.5e-12, 1.9e5, 77.0), (3e-13, 2.5e5, 450.0), (1e-10, 2.21e5, 250.0)):
        c = oracle_mod.make_config(solver=method, thermal=True, temperature=temp, gamma=gamma, max_step=ms, seed=5, noise_model=int(noise == "ou"),
                                   noise_corr_time=wcc.CORR_TIME)
        th = waveform_ref.thermal_field(oracle_mod, p, "stt_mram", gamma, temp, 5, np.arange(n) + 3, 2, noise, wcc.CORR_TIME)
        r = waveform_ref.solve(m0, T, p, method, J=J, max_step=ms, temperature=temp, gamma=gamma, thermal=th)
        off = waveform_ref.solve(m0, T, p, method, J=J, max_step=ms, temperature=temp, gamma=gamma)
        o = [oracle_mod.simple_solve(m0[i], T[i], oracle_mod.make_params(p), c, J[i], env_id=3 + i, env_step=2) for i in range(n)]
        err = float(np.abs(r["m_final"] - np.array([x["m_final"] for x in o])).max())
        shift = float(np.abs(r["m_final"] - off["m_final"]).max())
        print(f"{method} {noise} max_step={ms:g} gamma={gamma:g} {temp:g} K: |m_ref - m_oracle| = {err:.1e}; the field moves m by {shift:.1e}")
        assert r["success"].all() and all(x["success"] for x in o) and r["n_steps"].tolist() == [x["n_steps"] for x in o]
        assert err <= 1e-13 and shift > 1e-7
    # thermal on at temperature 0: the input gate rejects every problem
    r = waveform_ref.solve(m0, T, p, method, J=J, temperature=0.0, thermal=dict(th, strength=0.0))
    assert not r["success"].any() and (r["n_steps"] == 0).all() and np.array_equal(r["m_final"], m0)


def test_resistance_forms_are_the_oracles(oracle_mod):
    rng = np.random.default_rng(7)
    m = wcc.unit_rows(rng, 40) * rng.uniform(0.9, 1.1, (40, 1))            # (not all of unit length: the STT form normalises, the others do not)
    for dtype, p in (("stt_mram", stt_default_params()), ("sot_mram", sot_default_params(polarization=0.7)),
                     ("sot_mram", sot_default_params(heavy_metal_thickness=3e-9, heavy_metal_resistivity=1e-7, thickness=2e-9)),
                     ("vcma_mram", vcma_default_params(polarization=0.6)),
                     ("vcma_mram", vcma_default_params(resistance_parallel=0.4, resistance_antiparallel=0.5))):     # under the 1 Ohm floor
        want = np.array([oracle_mod.resistance(row, oracle_mod.make_params(p, dtype)) for row in m])
        got = wave_step_ref.resistance(m, p, dtype)
        assert np.all(np.abs(got - want) <= 4e-16 * np.abs(want)), (dtype, np.abs(got - want).max())
    three = [wave_step_ref.resistance(m, p, t) for t, p in zip(wcc.DEV_TYPES, wcc.class_table(False))]
    assert not np.allclose(three[0], three[1]) and not np.allclose(three[0], three[2])


@pytest.mark.parametrize("method,noise", wcc.SHAPED_DIRECT)
def test_knots_builder_reproduces_the_shaped_case_bit_for_bit(oracle_mod, method, noise):
    """wave_config_cases.with_knots / run_knots_ref against shaped_ref: a knots problem whose knot times are the shape's, whose
    amplitudes are the shape's values in every env and at every step, and whose limit does not clip them is the shaped problem, and the
    restatement must give it the same rows, bit for bit.  (float64 actions that hold the float32 (J, T) widened, which parse to the same
    values: a float32 action cannot carry the value -0.15.)"""
    s, want = wcc.shaped_ref(method, noise, oracle_mod)
    assert s["acts"].dtype == np.float32
    amp = np.broadcast_to(s["shape"].values, s["acts"].shape[:2] + (len(s["shape"].values),))
    acts = np.concatenate([s["acts"].astype(np.float64), amp], axis=2)
    p = wcc.with_knots(s, s["shape"].times, 1.0, acts)
    for k in range(wcc.K_SHAPED):
        assert np.array_equal(p["cur"][k][0], s["cur"][k][0]) and np.array_equal(p["cur"][k][1], s["cur"][k][1]), k
    got = wcc.run_knots_ref(p, method, noise, oracle_mod)
    for k, (a, b) in enumerate(zip(got, want)):
        assert sorted(a) == sorted(b)
        for key in a:
            assert a[key].dtype == b[key].dtype and np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), (method, noise, k, key)
    # and the committed knots case is built by the same two functions from the same shaped problem
    q, _ = wcc.knots_ref(method, noise, oracle_mod)
    base = wcc.shaped_problem(method, noise, False, wcc.KNOTS_SEED)
    assert np.array_equal(q["acts"][:, :, :2], base["acts"]) and repr(q["cfg"]) == repr(base["cfg"]) and repr(q["plist"]) == repr(base["plist"])
    for key in base["state"]:
        assert np.array_equal(q["state"][key], base["state"][key]), key
    assert np.array_equal(q["fk"][0], base["fk"][0]) and np.array_equal(q["fk"][1], base["fk"][1]) and np.array_equal(q["cls"], base["cls"])


def test_old_arguments_give_old_results():
    """the new keywords at their defaults are the old functions"""
    p = stt_default_params(volume=wcc.VOL)
    rng = np.random.default_rng(8)
    m0, T = wcc.unit_rows(rng, 5), rng.uniform(2e-11, 1e-10, 5)
    cur, fld = wcc.tables(rng, 5, 4, T, 1), wcc.tables(rng, 5, 3, T, 3)
    a = waveform_ref.solve(m0, T, p, "rk4", current=cur, field=fld)
    b = waveform_ref.solve(m0, T, p, "rk4", current=cur, field=fld, gamma=2.21e5, thermal=None)
    assert np.array_equal(a["m_final"], b["m_final"])
    c = waveform_ref.solve(m0, T, p, "rk4", current=cur, field=fld, gamma=1.9e5)
    assert np.abs(a["m_final"] - c["m_final"]).max() > 1e-6


def test_tables_draws_what_the_step_wave_tests_draw():
    """wave_config_cases.tables is a copy of test_gpu_step_wave._tables: the same generator state gives the same knots"""
    import test_gpu_step_wave
    for width, K in ((1, 4), (3, 17)):
        T = np.random.default_rng(1).uniform(2e-11, 2e-10, 50)
        a = wcc.tables(np.random.default_rng(9), 50, K, T, width)
        b = test_gpu_step_wave._tables(np.random.default_rng(9), 50, K, T, width)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

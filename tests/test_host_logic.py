"""Host-side logic on CPU: the same SpinTorqueEnv / SpinTorqueVecEnv code the GPU runs, with the oracle injected as
the backend (test seam), against the golden vectors.  Also the device parameter surface."""
import numpy as np
import pytest
import torch

from conftest import sot_default_params, stt_default_params, vcma_default_params
from helpers import OracleBackend
from test_oracle_golden import EPISODE_CFG, _episode_params


@pytest.fixture(scope="module")
def stg(oracle_mod):
    import spin_torque_gym_amd as s
    return s


def test_facade_episodes_vs_golden_g6(stg, golden):
    g = golden("G6_env_episode")
    for k, tag in enumerate(g["episode_tags"]):
        tag = str(tag)
        dev, d = _episode_params(tag)
        env = stg.SpinTorqueEnv(device_type=dev, device_params=d, include_thermal_fluctuations=False,
                                backend=OracleBackend, **EPISODE_CFG.get(tag, {}))
        obs0, info0 = env.reset(seed=0, options={"initial_state": g[f"ep{k}_m0"], "target_state": g[f"ep{k}_target"]})
        assert np.allclose(obs0, g[f"ep{k}_obs"][0], rtol=2e-7, atol=1e-12), tag
        assert set(info0) == {"step_count", "total_energy", "current_alignment", "is_success", "target_reached",
                              "magnetization_magnitude", "device_type", "episode_history"}
        for j, a in enumerate(g[f"ep{k}_actions"]):
            obs, r, te, tr, info = env.step(np.array(a, dtype=np.float32))
            assert obs.dtype == np.float32 and obs.shape == (12,)
            assert np.allclose(obs, g[f"ep{k}_obs"][j + 1], rtol=2e-7, atol=1e-12), (tag, j)
            rr = g[f"ep{k}_reward"][j]
            assert abs(r - rr) <= 1e-11 * max(1.0, abs(rr)), (tag, j, r, rr)
            assert te == bool(g[f"ep{k}_terminated"][j]) and tr == bool(g[f"ep{k}_truncated"][j])
            assert info["simulation_success"] == bool(g[f"ep{k}_success"][j])
            assert abs(info["energy_consumed"] - g[f"ep{k}_energy"][j]) <= 1e-13 * max(abs(g[f"ep{k}_energy"][j]), 1e-300)
            for key in ("final_magnetization", "pulse_duration", "current_density", "alignment_improvement",
                        "reward_components", "total_reward", "episode_history"):
                assert key in info
        assert len(env.episode_history) == len(g[f"ep{k}_actions"])
        an = env.analyze_episode()
        assert an["episode_length"] == len(g[f"ep{k}_actions"])
        env.close()


def test_reset_seed_parity_g9(stg, golden):
    g = golden("G9_reset_seeds")
    env = stg.SpinTorqueEnv(include_thermal_fluctuations=False, backend=OracleBackend)
    for s in range(64):
        obs, _ = env.reset(seed=s)
        assert np.abs(env.current_magnetization - g["state"][s, :3]).max() <= 1e-15
        assert np.array_equal(env.target_magnetization, g["state"][s, 3:])
        assert np.allclose(obs, g["obs"][s], rtol=2e-7, atol=0)
    env.reset(seed=1234)
    for row in g["continued_from_1234"]:
        env.reset()
        assert np.abs(env.current_magnetization - row[:3]).max() <= 1e-15


def test_error_paths_match_reference(stg):
    env = stg.SpinTorqueEnv(include_thermal_fluctuations=False, backend=OracleBackend)
    with pytest.raises(RuntimeError, match="reset"):
        env.step(np.zeros(2, dtype=np.float32))
    env.reset(seed=0)
    # wrong shape -> replaced by [0, 1e-12] (monitoring.py:300-302): a legal, tiny relaxation step
    obs, r, te, tr, info = env.step(np.zeros(3, dtype=np.float32))
    assert "error" not in info and info["current_density"] == 0.0 and info["pulse_duration"] == 1e-12
    # discrete action mode ends in the catch-all
    env2 = stg.SpinTorqueEnv(include_thermal_fluctuations=False, action_mode="discrete", backend=OracleBackend)
    env2.reset(seed=0)
    obs, r, te, tr, info = env2.step(3)
    assert r == -1.0 and te is False and tr is True and "error" in info
    with pytest.raises(ValueError):
        stg.SpinTorqueEnv(action_mode="bogus", backend=OracleBackend)
    # non-STT type without explicit params: the env-side defaults lack 'easy_axis' 
    with pytest.raises(RuntimeError, match="easy_axis"):
        stg.SpinTorqueEnv(device_type="sot_mram", backend=OracleBackend)
    with pytest.raises(ValueError):
        stg.DeviceFactory().create_device("nope", {})


def test_device_surface_vs_golden_g7(stg, golden):
    g = golden("G7_resistance")
    fac = stg.DeviceFactory()
    assert fac.get_available_devices() == ["stt_mram", "sot_mram", "vcma_mram"]
    for dev, dflt in (("stt_mram", stt_default_params), ("sot_mram", sot_default_params), ("vcma_mram", vcma_default_params)):
        d = fac.get_default_parameters(dev)
        ref = dflt()
        assert set(d) == set(ref)
        for key in ref:
            assert np.array_equal(np.asarray(d[key]), np.asarray(ref[key])), key
        device = fac.create_device(dev, d)
        got = np.array([device.compute_resistance(m.copy()) for m in g["m"]])
        assert np.allclose(got, g[f"R_{dev}"], rtol=1e-15, atol=0)
        got = np.array([device.compute_resistance(m * 1.7) for m in g["m"]])
        assert np.allclose(got, g[f"R_{dev}_scaled"], rtol=1e-15, atol=0)
    # reference pins (tests/unit/test_devices.py:84,89)
    stt = fac.create_default_device("stt_mram")
    assert abs(stt.compute_resistance(np.array([0, 0, 1.0])) - 1e3) < 10
    assert abs(stt.compute_resistance(np.array([0, 0, -1.0])) - 2e3) < 20
    # VCMA anisotropy pins (tests/unit/test_devices.py:268-278)
    v = fac.create_default_device("vcma_mram")
    assert v.effective_anisotropy(0.0) == v.base_anisotropy
    assert v.effective_anisotropy(100.0) == v.effective_anisotropy(v.breakdown_voltage)
    with pytest.raises(RuntimeError, match="Missing required parameter"):
        fac.create_device("stt_mram", {"volume": 1e-24})
    with pytest.raises(RuntimeError, match="Damping"):
        fac.create_device("stt_mram", stt_default_params(damping=2.0))


def test_params_validity_predicate(stg):
    assert stg.params_valid_as_stt(stt_default_params())
    assert not stg.params_valid_as_stt(sot_default_params())                  # no 'polarization'
    assert stg.params_valid_as_stt(sot_default_params(polarization=0.7))
    assert not stg.params_valid_as_stt(stt_default_params(volume=1e-31))
    assert not stg.params_valid_as_stt(stt_default_params(uniaxial_anisotropy=10.0))
    assert not stg.params_valid_as_stt(stt_default_params(easy_axis=np.zeros(3)))
    p = stg.flatten_params(stg.DeviceFactory().create_device("sot_mram", sot_default_params()))
    assert p.params_valid == 0 and p.dev_type == 1 and p.r_series > 0


def test_vec_env_layout_and_state_dict(stg):
    n = 6
    env = stg.SpinTorqueVecEnv(n, diagnostics=True, device_params=stt_default_params(volume=8.75e-11), include_thermal_fluctuations=False,
                               backend=OracleBackend, seed=3)
    with pytest.raises(RuntimeError):
        env.step(torch.zeros((n, 2)))
    obs, _ = env.reset(seed=1)
    assert tuple(obs.shape) == (n, 12)
    st = env.get_state()
    assert torch.all(torch.abs(torch.linalg.norm(st["m"], dim=0) - 1) < 1e-14)
    a = torch.tensor([[2e6, 3e-10]] * n, dtype=torch.float32)
    obs, r, te, tr, info = env.step(a)
    assert tuple(obs.shape) == (n, 12) and r.dtype == torch.float32 and te.dtype == torch.bool
    sd = env.state_dict()
    o1, r1, *_ = env.step(a)
    env2 = stg.SpinTorqueVecEnv(n, diagnostics=True, device_params=stt_default_params(volume=8.75e-11), include_thermal_fluctuations=False,
                                backend=OracleBackend, seed=3)
    env2.load_state_dict(sd)
    o2, r2, *_ = env2.step(a)
    assert torch.equal(o1, o2) and torch.equal(r1, r2)
    with pytest.raises(ValueError, match="zero"):
        env.reset(options={"initial_state": np.zeros((n, 3))})
    # masked reset only touches the selected envs
    before = env.get_state()["m"].clone()
    mask = torch.tensor([1, 0, 0, 1, 0, 0], dtype=torch.uint8)
    env.reset(options={"mask": mask})
    after = env.get_state()
    assert torch.equal(after["m"][:, 1], before[:, 1]) and not torch.equal(after["m"][:, 0], before[:, 0])
    assert int(after["step_count"][0]) == 0 and int(after["step_count"][1]) == 2


def test_solver_facades_vs_golden(stg, golden):
    """The reference-shaped solver classes (physics.py) over the oracle backend: result dict keys, shapes and values."""
    from spin_torque_gym_amd.physics import LLGSSolver, RobustLLGSSolver, SimpleLLGSSolver, ThermalFluctuations
    g1, g4 = golden("G1_simple_rk4_relax"), golden("G4_llgs_rk45_relax")
    params = stt_default_params()
    rs = RobustLLGSSolver(method="rk4", rtol=1e-3, atol=1e-6, timeout=2.0, max_retries=2, fallback_method="euler",
                          backend=OracleBackend)
    r = rs.solve(g1["m0"][0], (0, 1e-9), params, lambda t: 0.0 if t > 1e-9 else 0.0, lambda t: np.zeros(3), False, 300.0)
    assert r["success"] and r["m"].shape == g1["traj0_m"].shape
    assert np.abs(r["m"] - g1["traj0_m"]).max() <= 1e-12 and np.abs(r["t"] - g1["traj0_t"]).max() <= 1e-24
    # failure -> fallback result with the initial state (robust_solver.py:278-299)
    bad = rs.solve(g1["m0"][0], (0, 1e-9), params, lambda t: 1e6, None, False, 300.0)
    assert bad["success"] is False and bad.get("is_fallback") and np.allclose(bad["m"][-1], g1["m0"][0])
    assert rs.get_statistics()["total_solves"] == 2
    with pytest.raises(NotImplementedError):
        rs.solve(g1["m0"][0], (0, 1e-9), params, lambda t: 1e6 * t, None, False, 300.0)
    with pytest.warns(UserWarning):
        assert SimpleLLGSSolver(method="bogus", backend=OracleBackend).method == "euler"
    ls = LLGSSolver(backend=OracleBackend)
    c = g4["cases"][0]
    r = ls.solve(c[:3], (0, c[3]), params, lambda t: 0.0, lambda t: np.zeros(3), thermal_noise=False)
    assert set(r) == {"t", "m", "energy", "torques", "success"} and r["success"]
    assert len(r["t"]) == len(g4["t_0"]) and np.abs(r["m"] - g4["m_0"]).max() <= 1e-9
    assert np.abs(r["energy"] - g4["energy_0"]).max() <= 1e-9 * np.abs(g4["energy_0"]).max()
    assert np.array_equal(r["torques"], np.zeros(len(r["t"]))) and np.array_equal(g4["torques_0"], r["torques"])   # J = 0
    g5 = golden("G5_llgs_rk45_stt")
    c5 = g5["cases"][4]                                            # volume 9.7e-6, J = 5e5: |tau_stt| + |tau_fl| per point (A8)
    r5 = ls.solve(c5[:3], (0, c5[3]), stt_default_params(volume=9.7e-6), lambda t: c5[4], None, thermal_noise=False)
    assert len(r5["t"]) == len(g5["t_4"]) and np.abs(r5["torques"] - g5["torques_4"]).max() <= 1e-9 * np.abs(g5["torques_4"]).max()
    # find_stable_states (llgs_solver.py:264-305) against the recorded run (G18): same global-np.random draws
    g18 = golden("G18_stable_states")
    np.random.seed(int(g18["default_seed"]))
    st = ls.find_stable_states(params, n_trials=len(g18["default_m_init"]))
    assert st.shape == g18["default_stable_states"].shape and np.abs(st - g18["default_stable_states"]).max() <= 1e-8
    st2 = ls.find_stable_states(params, n_trials=len(g18["default_m_init"]), seed=int(g18["default_seed"]))
    assert np.array_equal(st, st2)
    # batched form
    rb = rs.solve_batch(g1["m0"][:4], np.zeros(4), np.full(4, 1e-10), params)
    assert rb["m_final"].shape == (4, 3) and rb["success"].all() and (rb["n_points"] == 100).all()
    # ThermalFluctuations formulas (G8) and seeded white noise
    g8 = golden("G8_thermal")
    for alpha, ms, vol, T, s_llgs, _ in g8["grid"][:20]:
        assert np.isclose(ThermalFluctuations(temperature=T).compute_noise_strength(alpha, ms, vol), s_llgs, rtol=1e-15)
    tf = ThermalFluctuations(temperature=300.0, seed=7)
    white = np.array([tf.generate_thermal_field(0.01, 800e3, params["volume"], 1e-12, correlated=False) for _ in range(4000)])
    assert np.allclose(white.std(axis=0), g8["tf_white_std"], rtol=1e-12)      # same seeded generator as the reference
    assert ThermalFluctuations(0.0).compute_noise_strength(0.01, 8e5, 1e-24) == 0.0
    # the correlated (Ornstein-Uhlenbeck) sequences of the reference class, same seeds (G14)
    g14 = golden("G14_thermal_ou")
    for i, (seed, tau, dt, _) in enumerate(g14["cases"]):
        tf = ThermalFluctuations(temperature=300.0, correlation_time=tau, seed=int(seed))
        seq = np.array([tf.generate_thermal_field(0.01, 800e3, 1e-24, dt, correlated=True) for _ in range(64)])
        assert np.array_equal(seq, g14[f"field_{i}"])
    # Neel-Brown closed forms (G15): stability analysis, retention, seeded switching times, temperature sweep
    g15 = golden("G15_thermal_scalars")
    base = stg.DeviceFactory().get_default_parameters("stt_mram")
    small = dict(base); small["volume"] = float(g15["volumes"][1])
    for tag, T, dp in (("a", 300.0, base), ("b", 350.0, small), ("c", 77.0, small)):
        tf = ThermalFluctuations(temperature=T, seed=5)
        st = tf.analyze_thermal_stability(dp, time_scale=10.0)
        got = np.array([st["thermal_stability_factor"], st["energy_barrier_J"], st["energy_barrier_kT"], st["switching_probability"],
                        st["retention_time_years"], float(st["is_thermally_stable"]), st["temperature_K"]])
        assert np.allclose(got, g15[f"stab_{tag}"], rtol=1e-13, atol=0, equal_nan=True)
        e_b = dp["uniaxial_anisotropy"] * dp["volume"]
        assert np.allclose([tf.compute_retention_time(e_b), tf.compute_retention_time(e_b, failure_rate=1e-6, attempt_frequency=2e9)],
                           g15[f"retention_{tag}"], rtol=1e-13)
        assert np.allclose([tf.sample_switching_time(e_b) for _ in range(8)], g15[f"times_{tag}"], rtol=1e-13)   # same PCG64 draws
        sw = tf.generate_temperature_sweep((50.0, 400.0), dp, n_points=9)
        for k, v in sw.items():
            assert np.allclose(v, g15[f"sweep_{tag}_{k}"], rtol=1e-13, atol=0), (tag, k)
        assert tf.temperature == float(g15[f"temp_after_{tag}"][0])
    assert ThermalFluctuations(0.0).compute_retention_time(1e-19) == float("inf")


def test_array_env_facade_vs_golden_g13(stg, golden):
    """SpinTorqueArrayEnv facade (host code) over the oracle backend: reset draws (PCG64), step outputs, info keys."""
    from helpers import OracleArrayBackend
    from test_oracle_golden import G13_EPISODES, array_device_params
    g = golden("G13_array_env")
    seeds = dict(zip([str(t) for t in g["episode_tags"]], range(len(g["episode_tags"]))))
    for k, tag in enumerate(g["episode_tags"]):
        tag = str(tag)
        ckw, coup, dev, over = G13_EPISODES[tag]
        kw = dict(array_size=(ckw["rows"], ckw["cols"]), action_mode=ckw["action_mode"], device_type=dev,
                  device_params=array_device_params(dev, over) if (over or dev != "stt_mram") else None,
                  observation_mode=ckw.get("obs_mode", "array"), include_coupling=ckw.get("include_coupling", True))
        for key in ("max_steps", "max_current", "max_duration", "success_threshold", "energy_penalty_weight", "temperature"):
            if key in ckw:
                kw[key] = ckw[key]
        if coup:
            kw.update(coupling_type=coup[0], coupling_strength=coup[1])
        env = stg.SpinTorqueArrayEnv(backend=OracleArrayBackend, **kw)
        obs, info = env.reset(seed=seeds[tag])
        assert np.abs(env.current_pattern - g[f"ep{k}_pattern"][0]).max() <= 1e-15, tag         # same PCG64 draws
        assert np.allclose(obs.reshape(-1), g[f"ep{k}_obs"][0], rtol=2e-7, atol=1e-12), tag
        if coup:
            assert np.allclose(env.coupling_matrix, g[f"ep{k}_coupling"], rtol=1e-15, atol=0), tag
        for j, a in enumerate(g[f"ep{k}_actions"]):
            obs, r, te, tr, info = env.step(a)
            assert obs.shape == ((ckw["rows"], ckw["cols"], 6) if kw["observation_mode"] == "array" else (ckw["rows"] * ckw["cols"] * 6 + 4,))
            assert np.allclose(obs.reshape(-1), g[f"ep{k}_obs"][j + 1], rtol=2e-7, atol=1e-12), (tag, j)
            assert abs(r - g[f"ep{k}_reward"][j]) <= 1e-11 * max(1.0, abs(g[f"ep{k}_reward"][j])), (tag, j)
            assert te == bool(g[f"ep{k}_terminated"][j]) and tr == bool(g[f"ep{k}_truncated"][j])
            assert abs(info["pattern_similarity"] - g[f"ep{k}_similarity"][j]) <= 1e-12
            for key in ("energy_consumed", "affected_devices", "current_density", "pulse_duration", "pattern_improvement"):
                assert key in info
        env.close()
    with pytest.raises(ValueError):
        stg.SpinTorqueArrayEnv(action_mode="bogus", backend=OracleArrayBackend)
    env = stg.SpinTorqueArrayEnv(backend=OracleArrayBackend)
    env.reset(seed=0)
    with pytest.raises(ValueError, match="NaN"):
        env.step(np.array([np.nan, 1e6, 1e-9], dtype=np.float32))


def _check_dict_episode_g17(stg, golden, backend, m_tol):
    """observation_mode='dict' of the array env against the recorded reference episode (golden G17)."""
    g = golden("G17_array_dict")
    env = stg.SpinTorqueArrayEnv(array_size=(2, 3), action_mode="individual", observation_mode="dict", max_steps=5,
                                 coupling_type="dipolar", coupling_strength=0.2, backend=backend)
    keys = ("current_pattern", "target_pattern", "pattern_similarity", "steps_remaining", "total_energy")
    assert set(getattr(env.observation_space, "spaces", env.observation_space).keys()) == set(keys)

    def check(obs, j):
        assert set(obs.keys()) == set(keys)
        for k, dt in zip(keys, g["dtypes"]):
            assert obs[k].dtype == np.dtype(str(dt)) and obs[k].shape == g[k][j].shape, (k, j)
        assert np.abs(obs["current_pattern"] - g["current_pattern"][j]).max() <= m_tol, j
        assert np.array_equal(obs["target_pattern"], g["target_pattern"][j])
        assert abs(float(obs["pattern_similarity"][0]) - float(g["pattern_similarity"][j][0])) <= max(m_tol, 1e-7)
        assert int(obs["steps_remaining"][0]) == int(g["steps_remaining"][j][0])
        e = float(g["total_energy"][j][0])
        assert abs(float(obs["total_energy"][0]) - e) <= 2e-7 * abs(e), j

    obs, _ = env.reset(seed=17)
    check(obs, 0)
    for j, a in enumerate(g["actions"]):
        obs, r, te, tr, _ = env.step(a)
        check(obs, j + 1)
        assert abs(r - g["reward"][j]) <= 1e-9 * max(1.0, abs(g["reward"][j]))
        assert te == bool(g["terminated"][j]) and tr == bool(g["truncated"][j])
    env.close()


def test_array_env_dict_observation_vs_golden_g17(stg, golden):
    from helpers import OracleArrayBackend
    _check_dict_episode_g17(stg, golden, OracleArrayBackend, 1e-7)


def test_device_class_analysis_helpers_vs_golden_g16(stg, golden):
    """Analysis helpers of the SOT / VCMA device classes (host closed forms): power, switching thresholds, energy
    barriers, switching-time and leakage estimates against the reference classes' outputs (golden G16)."""
    g = golden("G16_device_helpers")
    fac = stg.DeviceFactory()
    ms_ = g["m"]
    sot = fac.create_device("sot_mram", fac.get_default_parameters("sot_mram"))
    th = sot.get_switching_threshold()
    assert np.allclose([th["critical_current_density"], th["critical_field"], th["damping_like_efficiency"], th["field_like_efficiency"]],
                       g["sot_threshold"], rtol=1e-14)
    js = g["sot_J"]
    assert np.allclose([sot.compute_power_consumption(j, 1e-9, ms_[0]) for j in js], g["sot_power"], rtol=1e-14)
    with np.errstate(over="ignore"):
        got = np.array([[sot.estimate_switching_time(j, T) for j in js] for T in (300.0, 400.0)])
    assert np.allclose(got, g["sot_time"], rtol=1e-13, equal_nan=True)
    assert np.allclose([sot.compute_energy_barrier(m) for m in ms_], g["sot_barrier"], rtol=1e-14)
    vc = fac.create_device("vcma_mram", fac.get_default_parameters("vcma_mram"))
    th = vc.get_switching_threshold()
    assert np.allclose([th["critical_voltage"], th["thermal_switching_voltage"], th["breakdown_voltage"], th["vcma_coefficient"]],
                       g["vcma_threshold"], rtol=1e-14)
    vs = g["vcma_V"]
    assert np.allclose([vc.compute_power_consumption(v, 1e-9) for v in vs], g["vcma_power"], rtol=1e-14)
    with np.errstate(over="ignore"):
        prob = np.array([[vc.compute_switching_probability(v, 1e-9, T) for v in vs] for T in (300.0, 0.0)])
        times = np.array([vc.estimate_switching_time(v, 300.0) for v in vs])
    assert np.allclose(prob, g["vcma_prob"], rtol=1e-13, atol=0) and np.allclose(times, g["vcma_time"], rtol=1e-13, equal_nan=True)
    assert np.allclose([vc.compute_energy_barrier(ms_[0], v) for v in vs], g["vcma_barrier"], rtol=1e-14)
    assert np.allclose([vc.compute_leakage_current(v) for v in vs], g["vcma_leak"], rtol=1e-14)
    assert np.isclose(vc.capacitance, g["vcma_cap"][0], rtol=1e-15)
    vc.update_temperature(350.0)
    th = vc.get_switching_threshold()
    assert np.allclose([th["critical_voltage"], th["thermal_switching_voltage"]], g["vcma_threshold_350"], rtol=1e-14)


def test_factory_validate_parameters(stg):
    fac = stg.DeviceFactory()
    out = fac.validate_parameters("STT_MRAM", {"damping": 0.02})
    assert out["damping"] == 0.02 and out["volume"] == fac.get_default_parameters("stt_mram")["volume"]
    with pytest.raises(ValueError, match="Damping"):
        fac.validate_parameters("stt_mram", {"damping": 1.5})
    with pytest.raises(ValueError, match="Volume"):
        fac.validate_parameters("stt_mram", {"volume": 0.0})
    assert fac.validate_parameters("sot_mram", {"damping": 7.0})["damping"] == 7.0       # the reference's SOT validator is empty


def test_unseeded_envs_get_distinct_thermal_stream_keys(stg):
    """an unseeded SpinTorqueEnv must not key its thermal stream with a constant -- parallel workers would
    replay the same noise step for step (the reference draws from the unseeded global np.random)."""
    envs = [stg.SpinTorqueEnv(backend=OracleBackend) for _ in range(3)]
    seeds = {e._vec.cfg.seed for e in envs}
    assert len(seeds) == 3, seeds
    same = [stg.SpinTorqueEnv(seed=5, backend=OracleBackend)._vec.cfg.seed for _ in range(2)]
    assert same[0] == same[1] == 5


def test_checkpoint_resumes_noise_streams_in_a_fresh_unseeded_env(stg):
    """state_dict carries cfg.seed (Philox key of the thermal field and the device-side auto-resets) and
    env_id0, so a new env built with seed=None continues bit for bit."""
    n = 48
    kw = dict(device_params=stt_default_params(volume=1e-27), include_thermal_fluctuations=True, autoreset=True, max_steps=2,
              backend=OracleBackend)
    rng = np.random.default_rng(0)
    acts = [np.stack([rng.uniform(-2e6, 2e6, n), rng.uniform(1e-10, 2e-10, n)], axis=1).astype(np.float32) for _ in range(3)]
    e1 = stg.SpinTorqueVecEnv(n, diagnostics=True, seed=None, env_id0=640, **kw)
    e1.reset(seed=3)
    e1.step(torch.from_numpy(acts[0]))
    sd = e1.state_dict()
    assert sd["cfg_seed"] == e1.cfg.seed and sd["env_id0"] == 640
    want = [tuple(t.clone() for t in e1.step(torch.from_numpy(a))[:4]) for a in acts[1:]]
    e2 = stg.SpinTorqueVecEnv(n, diagnostics=True, seed=None, **kw)                 # another key, another env_id0
    assert e2.cfg.seed != e1.cfg.seed
    e2.load_state_dict(sd)
    assert e2.cfg.seed == e1.cfg.seed and e2.env_id0 == 640
    got = [tuple(t.clone() for t in e2.step(torch.from_numpy(a))[:4]) for a in acts[1:]]
    for a, b in zip(want, got):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(e1.get_state()["m"], e2.get_state()["m"])
    assert e1.reset()[0].equal(e2.reset()[0])                     # host PCG64 state travelled too


def test_performance_stats_timer_table(stg):
    """get_performance_stats (spin_torque_env.py:711-718): profiler table in the reference's get_stats shape
    (utils/performance.py:456-474), fed by host timers and the device counters."""
    env = stg.SpinTorqueEnv(include_thermal_fluctuations=False, backend=OracleBackend)
    env.reset(seed=0)
    for _ in range(3):
        env.step(np.array([0.0, 1e-10], dtype=np.float32))
    st = env.get_performance_stats()
    assert set(st) == {"profiler", "optimizer", "solver", "health"}
    p = st["profiler"]
    for op, cnt in (("env_step", 3), ("env_reset", 1), ("step", 3), ("reset", 1)):
        assert p[f"{op}_count"] == cnt and p[f"{op}_min_time"] <= p[f"{op}_avg_time"] <= p[f"{op}_max_time"]
        assert abs(p[f"{op}_total_time"] - cnt * p[f"{op}_avg_time"]) < 1e-9
    assert p["env_steps"] == 3 and p["solver_work_units"] == 300 and p["noop_steps"] == 0
    assert st["solver"]["solve_count"] == 3 and st["solver"]["avg_solve_time"] > 0
    assert st["health"]["performance_metrics"]["total_steps"] == 3


def test_vector_env_spaces(stg):
    """gymnasium.vector.VectorEnv surface: num_envs, single_* and batched spaces."""
    env = stg.SpinTorqueVecEnv(5, diagnostics=True, include_thermal_fluctuations=False, backend=OracleBackend)
    assert env.num_envs == 5 and env.single_action_space.shape == (2,) and env.single_observation_space.shape == (12,)
    assert env.action_space.shape == (5, 2) and env.observation_space.shape == (5, 12)
    a = env.action_space.sample()
    assert a.shape == (5, 2) and a.dtype == np.float32 and np.all(np.abs(a[:, 0]) <= 2e6) and np.all((a[:, 1] >= 0) & (a[:, 1] <= 5e-9))
    obs, _ = env.reset(seed=0)
    obs, r, te, tr, info = env.step(torch.from_numpy(a))
    assert tuple(obs.shape) == (5, 12) and tuple(r.shape) == (5,) and te.dtype == torch.bool


def test_autoreset_returns_terminal_observation_without_diagnostics(stg):
    """the product default is diagnostics=False; with autoreset=True a finished env's obs row is the NEW
    episode's first observation, so the terminal one must still come back (info['final_obs']) -- a learner that bootstraps at
    truncation needs it.  Host logic over the oracle seam; the HIP path is checked by
    tests/test_gpu_parity.py::test_diagnostics_off_is_the_same_step_with_fewer_outputs."""
    n = 6
    kw = dict(device_params=stt_default_params(volume=8.75e-11), include_thermal_fluctuations=False, seed=3, autoreset=True,
              max_steps=2, backend=OracleBackend)
    a = torch.tensor([[1e5, 2e-10]] * n, dtype=torch.float32)
    res = {}
    for diag in (False, True):
        env = stg.SpinTorqueVecEnv(n, diagnostics=diag, **kw)
        env.reset(seed=1)
        _, _, _, tr1, info1 = env.step(a)
        assert "final_obs" in info1 and not bool(tr1.any())
        obs, _, te, tr, info = env.step(a)                       # max_steps = 2: truncated now, reset in the same step
        assert bool(tr.all()) and ("reward_f64" in info) is diag
        fo = info["final_obs"]
        assert tuple(fo.shape) == (n, 12)
        assert bool((fo[:, 8] == 0.0).all()) and bool((obs[:, 8] == 1.0).all())    # steps remaining: terminal 0, new episode all
        assert bool((fo[:, 10] != 0).all()) and bool((obs[:, 10] == 0).all())      # last action: the pulse vs zeros after reset
        res[diag] = (fo.clone(), obs.clone())
        om, _, _, trm, im = env.step_many(a.unsqueeze(0).repeat(2, 1, 1))
        assert tuple(im["final_obs"].shape) == (2, n, 12) and bool(trm.any()) and bool((im["final_obs"][trm][:, 8] == 0).all())
        env.close()
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1])


_GYM_DROP_IN = r"""
import os, sys
root = sys.argv[1]
for p in (root, os.path.join(root, "spin-torque-rl-gym_amd"), os.path.join(root, "tests"), os.path.join(root, "tests", "golden")):
    sys.path.insert(0, p)
import numpy as np
import gym_stub
gym_stub.install()                                   # a `gymnasium` is importable from here on
import gymnasium
import spin_torque_gym_amd as stg                    # registers on import, like the reference package
reg = sys.modules["gymnasium.envs.registration"].registry
assert reg["SpinTorque-v0"] == dict(entry_point="spin_torque_gym_amd.envs:SpinTorqueEnv", max_episode_steps=100,
                                    kwargs={"device_type": "stt_mram"}), reg["SpinTorque-v0"]
assert reg["SpinTorqueArray-v0"] == dict(entry_point="spin_torque_gym_amd.array_env:SpinTorqueArrayEnv", max_episode_steps=200,
                                         kwargs={"array_size": (4, 4), "device_type": "stt_mram"}), reg["SpinTorqueArray-v0"]
assert stg.register_envs() is True and len([k for k in reg if k.startswith("SpinTorque")]) == 2      # idempotent
ours = {k: dict(reg[k]) for k in ("SpinTorque-v0", "SpinTorqueArray-v0")}
from helpers import OracleBackend, OracleArrayBackend
# gym.make('SpinTorque-v0', **kwargs) builds the facade class, a gymnasium.Env, with the registered kwargs
env = gymnasium.make("SpinTorque-v0", include_thermal_fluctuations=False, backend=OracleBackend)
assert type(env) is stg.SpinTorqueEnv and isinstance(env, gymnasium.Env) and env.device_type == "stt_mram"
assert env.spec["max_episode_steps"] == 100 and env.max_steps == 100
obs, info = env.reset(seed=3)
assert obs.shape == (12,) and obs.dtype == np.float32 and info["step_count"] == 0
out = env.step(np.array([0.0, 1e-10], dtype=np.float32))
assert len(out) == 5 and out[0].shape == (12,) and isinstance(out[1], float) and out[4]["step_count"] == 1
assert env.action_space.shape == (2,) and env.observation_space.shape == (12,)
env.close()
arr = gymnasium.make("SpinTorqueArray-v0", backend=OracleArrayBackend)
assert type(arr) is stg.SpinTorqueArrayEnv and isinstance(arr, gymnasium.Env) and arr.array_size == (4, 4) and arr.max_steps == 200
o, info = arr.reset(seed=1)
o2, r, te, tr, info = arr.step(np.array([3, 0.0, 1e-10], dtype=np.float32))
assert np.asarray(o2).shape == np.asarray(o).shape and isinstance(r, float)
arr.close()
# the unmodified reference's own final registrations, recorded by tests/golden/make_golden.py (G19)
import json
g = np.load(os.path.join(root, "tests", "golden", "G19_registrations.npz"), allow_pickle=False)
refreg = {str(k): dict(entry_point=str(e), max_episode_steps=int(s), kwargs=json.loads(str(kw)))
          for k, e, s, kw in zip(g["ids"], g["entry_point"], g["max_episode_steps"], g["kwargs_json"])}
for k, mine in ours.items():
    ref = refreg[k]
    assert ref["max_episode_steps"] == mine["max_episode_steps"], (k, ref, mine)
    assert ref["kwargs"] == json.loads(json.dumps(mine["kwargs"], sort_keys=True)), (k, ref, mine)
    assert ref["entry_point"].split(":")[1] == mine["entry_point"].split(":")[1]
print("reference registrations checked")
print("ok")
"""


def test_gym_make_drop_in_registrations(oracle_mod):
    """with a `gymnasium` importable (tests/golden/gym_stub.py; the real package is not in this image),
    `import spin_torque_gym_amd` registers 'SpinTorque-v0' and 'SpinTorqueArray-v0' with the reference's final
    max_episode_steps / kwargs (spin_torque_gym/__init__.py:14-24 overridden by envs/__init__.py:14-26: 100 / 200), the entry
    points resolve to the facade classes, and `gymnasium.make(id, **kwargs)` builds working envs (stepped here on the oracle
    backend).  The unmodified reference's own registry, recorded as G19, is compared as well.  Runs in a fresh
    interpreter so that the stand-in `gymnasium` does not leak into the other tests' modules."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-B", "-c", _GYM_DROP_IN, root], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


def test_render_human_four_panels_of_both_facades(stg):
    """VERDICT r3 item 8 / spin_torque_env.py:571-655, array_env.py:608-676: render('human') draws the reference's picture -- macrospin
    env: 3-D arrows of m and the target in the unit sphere + energy / alignment (with the success threshold) / applied-current
    histories from `episode_history`; array env: m_z maps of the current and target patterns + similarity / energy histories -- on ONE
    persistent figure that is redrawn in place and closed by close().  Host-side; non-interactive Agg backend; the oracle seam."""
    import matplotlib
    matplotlib.use("Agg", force=True)
    import matplotlib.pyplot as plt
    from helpers import OracleArrayBackend
    before = set(plt.get_fignums())
    env = stg.SpinTorqueEnv(device_params=stt_default_params(volume=8.75e-11), include_thermal_fluctuations=False, render_mode="human",
                            backend=OracleBackend)
    assert env.renderer is not None and env.renderer.ok                    # created at construction, as in the reference
    env.reset(seed=1)
    assert env.render() is None                                             # no history yet: only the 3-D panel has content
    fig = env.renderer.fig
    assert len(fig.axes) == 4 and fig.axes[0].name == "3d" and fig.axes[0].get_title() == "Magnetization State"
    assert [ax.get_title() for ax in fig.axes[1:]] == ["", "", ""]
    for a in ([5e5, 2e-10], [-1e6, 1e-10], [0.0, 3e-10]):
        env.step(np.array(a, dtype=np.float32))
    assert env.render("human") is None and env.renderer.fig is fig          # the same figure, redrawn
    assert [ax.get_title() for ax in fig.axes] == ["Magnetization State", "Energy Consumption", "Target Alignment", "Applied Current"]
    energy_ax, align_ax, cur_ax = fig.axes[1:]
    assert np.allclose(energy_ax.lines[0].get_ydata(), [h["energy"] for h in env.episode_history])
    assert np.allclose(align_ax.lines[0].get_ydata(), [h["alignment"] for h in env.episode_history])
    assert np.allclose(align_ax.lines[1].get_ydata(), env.success_threshold)            # the dashed threshold line
    assert np.allclose(cur_ax.lines[0].get_ydata(), [5e5, -1e6, 0.0]) and list(cur_ax.lines[0].get_xdata()) == [1, 2, 3]
    from spin_torque_gym_amd.render import frame_of
    img = frame_of(fig)
    assert img.dtype == np.uint8 and img.shape[2] == 3 and img.std() > 0
    rgb = env.render("rgb_array")                                           # the 2-D projection stays what it was
    assert rgb.ndim == 3 and rgb.shape[2] == 3
    env.close()
    assert env.renderer is None and set(plt.get_fignums()) == before        # close() closes the figure
    # a facade built without a render mode creates the figure at the first render('human')
    env = stg.SpinTorqueEnv(include_thermal_fluctuations=False, backend=OracleBackend)
    assert env.renderer is None
    with pytest.raises(RuntimeError, match="reset"):
        env.render("human")
    env.reset(seed=2)
    env.render("human")
    assert env.renderer is not None and len(env.renderer.fig.axes) == 4
    env.close()
    # the array env: two m_z maps (each with a colour bar) + similarity and energy histories
    arr = stg.SpinTorqueArrayEnv(array_size=(2, 3), include_thermal_fluctuations=False, render_mode="human", backend=OracleArrayBackend)
    arr.reset(seed=0)
    arr.render()
    for k in range(2):
        arr.step(np.array([k, 1e6, 2e-10], dtype=np.float32))
        arr.render()                                                        # redrawn every step: the colour bars must not pile up
    f = arr.renderer.fig
    titles = [ax.get_title() for ax in f.axes]
    assert titles[:4] == ["Current Pattern (Mz)", "Target Pattern (Mz)", "Pattern Similarity Progress", "Energy Consumption per Step"]
    assert len(f.axes) == 6                                                 # four panels + two colour bars
    assert np.allclose(f.axes[0].images[0].get_array(), arr.current_pattern[:, :, 2])
    assert np.allclose(f.axes[2].lines[0].get_ydata(), [h["similarity"] for h in arr.episode_history])
    rgb = arr.render("rgb_array")
    assert rgb.ndim == 3 and rgb.shape[2] == 3
    with pytest.raises(ValueError, match="Unsupported render mode"):
        arr.render("bogus")
    arr.close()
    assert set(plt.get_fignums()) == before

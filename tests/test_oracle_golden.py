"""Pins the CPU oracle (oracle/stg_oracle.c) against the golden vectors recorded from the imported
Python reference (tests/golden/make_golden.py).  CPU only.

Tolerances: the oracle follows the NumPy operation order without FMA, so RK4 results agree to a few
ulp per sub-step (asserted <= 1e-12 absolute on unit vectors); SciPy's RK45 goes through BLAS dot
products and libm pow whose last-bit behaviour the C code cannot replicate, asserted <= 1e-9
(accept/reject sequences are additionally required to be identical: same point counts).
"""
import numpy as np
import pytest

from conftest import sot_default_params, stt_default_params, vcma_default_params


def test_g1_simple_rk4_relax(golden, oracle_mod):
    o = oracle_mod
    g = golden("G1_simple_rk4_relax")
    p = o.make_params(stt_default_params())
    c = o.make_config("rk4")
    worst = 0.0
    for k in range(len(g["T"])):
        r = o.simple_solve(g["m0"][g["m0_index"][k]], g["T"][k], p, c, 0.0)
        assert r["success"] == bool(g["success"][k])
        assert r["n_steps"] == g["n_steps"][k]
        worst = max(worst, np.abs(r["m_final"] - g["m_final"][k]).max())
    assert worst <= 1e-12, worst
    # full trajectories
    for tag, idx, T in (("traj0", 0, 1e-9), ("traj1", 29, float(np.float32(3.3e-10)))):
        r = o.simple_solve(g["m0"][idx], T, p, c, 0.0, want_traj=True)
        assert r["m"].shape == g[tag + "_m"].shape
        assert np.abs(r["m"] - g[tag + "_m"]).max() <= 1e-12


def test_g2_simple_rk4_stt(golden, oracle_mod):
    o = oracle_mod
    g = golden("G2_simple_rk4_stt")
    c = o.make_config("rk4")
    worst = 0.0
    switched = 0
    for k in range(len(g["T"])):
        p = o.make_params(stt_default_params(volume=float(g["volume"][k])))
        m0 = g["m0"][g["m0_index"][k]]
        r = o.simple_solve(m0, g["T"][k], p, c, g["J"][k])
        assert r["success"] == bool(g["success"][k])
        assert r["n_steps"] == g["n_steps"][k]          # H5: truncation of T/dt
        worst = max(worst, np.abs(r["m_final"] - g["m_final"][k]).max())
        switched += int(m0[2] > 0.9 and g["m_final"][k][2] < -0.9)
    assert worst <= 1e-11, worst
    assert switched > 0                                  # the fixture does contain +z -> -z switching
    p = o.make_params(stt_default_params(volume=float(g["traj_volume"])))
    r = o.simple_solve(g["m0"][int(g["traj_m0_index"])], float(g["traj_T"]), p, c, float(g["traj_J"]), want_traj=True)
    assert np.abs(r["m"] - g["traj_m"]).max() <= 1e-11


def test_g3_simple_degenerate(golden, oracle_mod):
    """Overflow semantics: success flag, first all-zero row, last row -- exactly."""
    o = oracle_mod
    g = golden("G3_simple_degenerate")
    p = o.make_params(stt_default_params())
    c = o.make_config("rk4")
    n_fail = 0
    for k in range(len(g["J"])):
        r = o.simple_solve(g["m0"][g["m0_index"][k]], g["T"][k], p, c, g["J"][k])
        assert r["success"] == bool(g["success"][k]), k
        assert r["first_zero_row"] == g["first_zero_row"][k], k
        if r["success"]:
            assert np.abs(r["m_final"] - g["robust_m_last"][k]).max() <= 1e-12
        else:
            n_fail += 1
    assert n_fail > 50


@pytest.mark.parametrize("name,vols", [("G4_llgs_rk45_relax", {0: None}), ("G5_llgs_rk45_stt", {0: 9.7e-6, 1: 2e-6})])
def test_g4_g5_llgs_rk45(golden, oracle_mod, name, vols):
    o = oracle_mod
    g = golden(name)
    c = o.make_config("rk45")
    for k, case in enumerate(g["cases"]):
        m0, T, J, tag, succ = case[:3], case[3], case[4], int(case[5]), bool(case[6])
        d = stt_default_params() if vols[tag] is None else stt_default_params(volume=vols[tag])
        p = o.make_params(d)
        r = o.llgs_solve(m0, T, p, c, J)
        assert r["success"] == succ
        assert r["n_points"] == len(g[f"t_{k}"]), (k, r["n_points"], len(g[f"t_{k}"]))
        assert np.abs(r["t"] - g[f"t_{k}"]).max() <= 1e-9 * T
        assert np.abs(r["m"] - g[f"m_{k}"]).max() <= 1e-9
        e = g[f"energy_{k}"]
        assert np.abs(r["energy"] - e).max() <= 1e-9 * np.abs(e).max()
        tq = g[f"torques_{k}"]
        assert np.abs(r["torques"] - tq).max() <= 1e-9 * max(np.abs(tq).max(), 1e-300)


def _episode_params(tag):
    if tag in ("default_relax", "default_noop", "temperature_zero_noop"):
        return "stt_mram", stt_default_params()
    if tag in ("stt_switch", "stt_bad_actions", "stt_custom_cfg"):
        return "stt_mram", stt_default_params(volume=8.75e-11)
    if tag == "sot_default_noop":
        return "sot_mram", sot_default_params()
    if tag == "sot_polarized":
        return "sot_mram", sot_default_params(polarization=0.7, volume=8.75e-11)
    if tag == "vcma_polarized_tilted":
        return "vcma_mram", vcma_default_params(polarization=0.6, volume=5e-11, easy_axis=np.array([0.1, 0.0, 1.0]),
                                                reference_magnetization=np.array([0.0, 0.2, 1.0]))
    raise KeyError(tag)


EPISODE_CFG = {
    "stt_bad_actions": dict(max_steps=5),
    "stt_custom_cfg": dict(max_current=1e6, max_duration=1e-9, success_threshold=0.5, energy_penalty_weight=0.3,
                           temperature=350.0, max_steps=20),
    "temperature_zero_noop": dict(temperature=0.0),
}


def test_g6_env_episode(golden, oracle_mod):
    o = oracle_mod
    g = golden("G6_env_episode")
    for k, tag in enumerate(g["episode_tags"]):
        tag = str(tag)
        dev, d = _episode_params(tag)
        p = o.make_params(d, dev)
        c = o.make_config("rk4", thermal=False, **EPISODE_CFG.get(tag, {}))
        s = o.EnvState()
        m0 = g[f"ep{k}_m0"]
        m0 = m0 / np.linalg.norm(m0)
        tgt = g[f"ep{k}_target"]
        tgt = tgt / np.linalg.norm(tgt)
        s.m[:] = list(m0)
        s.target[:] = list(tgt)
        for j, a in enumerate(g[f"ep{k}_actions"]):
            out = o.env_step(s, a, p, c)
            ref_obs = g[f"ep{k}_obs"][j + 1]
            assert np.allclose(np.array(out.obs[:]), ref_obs, rtol=2e-7, atol=1e-12), (tag, j, np.array(out.obs[:]), ref_obs)
            ref_r = g[f"ep{k}_reward"][j]
            assert abs(out.reward - ref_r) <= 1e-11 * max(1.0, abs(ref_r)), (tag, j, out.reward, ref_r)
            assert bool(out.terminated) == bool(g[f"ep{k}_terminated"][j]), (tag, j)
            assert bool(out.truncated) == bool(g[f"ep{k}_truncated"][j]), (tag, j)
            assert (out.status != 1) == bool(g[f"ep{k}_success"][j]), (tag, j)
            ref_e = g[f"ep{k}_energy"][j]
            assert abs(out.energy - ref_e) <= 1e-13 * max(abs(ref_e), 1e-300), (tag, j)
            assert np.abs(np.array(s.m[:]) - g[f"ep{k}_m"][j + 1]).max() <= 1e-11, (tag, j)


def test_g7_resistance(golden, oracle_mod):
    o = oracle_mod
    g = golden("G7_resistance")
    for dev, dflt in (("stt_mram", stt_default_params), ("sot_mram", sot_default_params), ("vcma_mram", vcma_default_params)):
        p = o.make_params(dflt(), dev)
        got = np.array([o.resistance(m, p) for m in g["m"]])
        assert np.allclose(got, g[f"R_{dev}"], rtol=1e-14, atol=0)
        p = o.make_params(dflt(reference_magnetization=np.array([0.0, 0.2, 1.0]), resistance_parallel=1234.5,
                               resistance_antiparallel=3210.0), dev)
        got = np.array([o.resistance(m, p) for m in g["m"]])
        assert np.allclose(got, g[f"R_{dev}_tilted"], rtol=1e-14, atol=0)
        p = o.make_params(dflt(), dev)
        got = np.array([o.resistance(m * 1.7, p) for m in g["m"]])
        assert np.allclose(got, g[f"R_{dev}_scaled"], rtol=1e-14, atol=0)
    # the two numeric pins the reference's own tests hold (tests/unit/test_devices.py:84,89)
    p = o.make_params(stt_default_params())
    assert abs(o.resistance(np.array([0, 0, 1.0]), p) - 1e3) < 10
    assert abs(o.resistance(np.array([0, 0, -1.0]), p) - 2e3) < 20


def test_g8_thermal_strength_and_moments(golden, oracle_mod):
    o = oracle_mod
    g = golden("G8_thermal")
    for alpha, ms, vol, T, s_llgs, s_simple in g["grid"]:
        p = o.make_params(stt_default_params(damping=alpha, saturation_magnetization=ms, volume=vol))
        assert np.isclose(o.thermal_strength(p, 2.21e5, T, 1), s_llgs, rtol=1e-15)
        assert np.isclose(o.thermal_strength(p, 2.21e5, T, 0), s_simple, rtol=1e-15)
    # the oracle's Philox/Box-Muller normals obey the moment bounds the reference's own thermal test uses
    # (tests/test_comprehensive_suite.py:447-476: |mean| < 0.1 sigma, |std - sigma| < 0.2 sigma over 1000 draws)
    z = np.array([o.thermal_normals(1234, e, 0, c) for e in range(50) for c in range(80)])
    assert np.all(np.abs(z.mean(axis=0)) < 0.1)
    assert np.all(np.abs(z.std(axis=0) - 1.0) < 0.2)
    # tighter: 4000 draws -> standard error 0.016 / 0.011
    assert np.all(np.abs(z.mean(axis=0)) < 0.06) and np.all(np.abs(z.std(axis=0) - 1.0) < 0.04)
    # and the reference's own empirical field std (4000 draws) is consistent with sigma = strength
    p = o.make_params(stt_default_params())
    s = o.thermal_strength(p, 2.21e5, 300.0, 0)
    assert np.all(np.abs(g["simple_field_std"] / s - 1.0) < 0.05)
    assert np.isclose(o.thermal_strength(p, 2.21e5, 300.0, 1), float(g["default_strength_llgs"]), rtol=1e-15)


def test_philox_known_answer(oracle_mod):
    """Philox4x32-10 known-answer vectors from the Random123 distribution (kat_vectors)."""
    import ctypes as C
    L = oracle_mod.lib()
    L.stgo_philox4x32_10.argtypes = [C.POINTER(C.c_uint32)] * 3
    L.stgo_philox4x32_10.restype = None

    def ph(ctr, key):
        c = (C.c_uint32 * 4)(*ctr)
        k = (C.c_uint32 * 2)(*key)
        out = (C.c_uint32 * 4)()
        L.stgo_philox4x32_10(c, k, out)
        return [int(x) for x in out]
    assert ph([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert ph([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert ph([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def _diffusion_stats(samples, det):
    d = samples - det
    return d.mean(axis=0), np.sqrt((d ** 2).sum(axis=1).mean())


def check_thermal_diffusion(g, solve_many, n_rk4, n_rk45, label):
    """Shared by the CPU (oracle) and GPU (HIP) tests: statistical parity of the Langevin diffusion with the reference.
    solve_many(solver, m0, T, volume, n) -> (final m [n,3], accepted points [n])."""
    for solver, n in (("rk4", n_rk4), ("rk45", n_rk45)):
        ref, det = g[f"{solver}_samples"], g[f"{solver}_deterministic"]
        ours, npts = solve_many(solver, g[f"{solver}_m0"], float(g[f"{solver}_T"]), float(g[f"{solver}_volume"]), n)
        mean_ref, rms_ref = _diffusion_stats(ref, det)
        mean_our, rms_our = _diffusion_stats(ours, det)
        se = rms_ref / np.sqrt(len(ref))                      # standard error of the reference's sample mean
        assert np.all(np.abs(mean_our - mean_ref) < 5 * se), (label, solver, mean_our, mean_ref, se)
        # the reference's rms estimate from 4000 (rk4) / 1000 (rk45) samples has a relative standard error of 1.05 % / 2.0 %
        # (|d|^2 has a coefficient of variation of 1.33 / 1.27; measured on the fixture), so 5 % / 8 % is 4-4.75 sigma of the
        # REFERENCE's own estimate; our sample sizes keep our side's error below half of that
        tol = 0.05 if solver == "rk4" else 0.08
        assert len(ref) >= (4000 if solver == "rk4" else 1000)
        assert abs(rms_our / rms_ref - 1.0) < tol, (label, solver, rms_our, rms_ref)
        assert np.all(np.abs(np.linalg.norm(ours, axis=1) - 1) < 1e-12)
        if solver == "rk45":                                  # the noise also drives the step-size controller
            assert abs(np.mean(npts) / np.mean(g["rk45_npts"] - 1) - 1.0) < 0.02, (np.mean(npts), np.mean(g["rk45_npts"]))
        print(f"{label} {solver}: rms ours {rms_our:.3e} ref {rms_ref:.3e}")


def test_g10_thermal_on_vs_reference(golden, oracle_mod):
    """Thermal field ON against the reference.  Well-conditioned regimes: the thermal-on result equals the reference's
    (whose own thermal-on and thermal-off results agree to ~1e-10); V = 1e-30: diffusion statistics match."""
    o = oracle_mod
    g = golden("G10_thermal_diffusion")
    m0 = g["rk4_m0"]
    for vol, J, T, *rest in g["wellcond"]:
        off_ref, on_ref, ok = np.array(rest[:3]), np.array(rest[3:6]), bool(rest[6])
        assert np.abs(off_ref - on_ref).max() < 1e-7          # the reference itself: noise is (nearly) invisible here
        p = o.make_params(stt_default_params(volume=vol))
        r = o.simple_solve(m0, T, p, o.make_config("rk4", thermal=True, seed=5), J, env_id=3)
        assert r["success"] == ok and np.abs(r["m_final"] - on_ref).max() < 1e-7

    def solve_many(solver, m0, T, vol, n):
        p = o.make_params(stt_default_params(volume=vol))
        c = o.make_config(solver, thermal=True, seed=99)
        out, npts = [], []
        for e in range(n):
            if solver == "rk4":
                r = o.simple_solve(m0, T, p, c, 0.0, env_id=e)
                npts.append(r["n_steps"])
            else:
                r = o.llgs_solve(m0, T, p, c, 0.0, env_id=e, cap=1)
                npts.append(r["n_points"] - 1)
            out.append(r["m_final"])
        return np.array(out), np.array(npts)
    check_thermal_diffusion(g, solve_many, 12000, 6000, "oracle")


def test_g11_simple_euler(golden, oracle_mod):
    o = oracle_mod
    g = golden("G11_simple_euler")
    c = o.make_config("euler")
    worst = 0.0
    for k in range(len(g["T"])):
        p = o.make_params(stt_default_params(volume=float(g["volume"][k])))
        r = o.simple_solve(g["m0"][g["m0_index"][k]], g["T"][k], p, c, g["J"][k])
        assert r["success"] == bool(g["success"][k]) and r["n_steps"] == g["n_steps"][k]
        worst = max(worst, np.abs(r["m_final"] - g["m_final"][k]).max())
    assert worst <= 1e-12, worst


G12_SOT = {"default": {}, "custom": dict(spin_hall_angle=0.3, heavy_metal_thickness=4e-9, interface_transparency=0.6,
                                         field_like_efficiency=0.15, damping_like_efficiency=0.25, thickness=1.2e-9),
           "dir110": dict(current_direction=np.array([1.0, 1.0, 0.0]))}
G12_VCMA = {"default": {}, "custom": dict(vcma_coefficient=60e-6, dielectric_thickness=1.4e-9, breakdown_voltage=1.5,
                                          uniaxial_anisotropy=0.9e6)}


def test_g12_device_class_formulas(golden, oracle_mod):
    """SOTMRAMDevice.compute_spin_torque / VCMAMRAMDevice._compute_effective_anisotropy: the oracle's restatement and the
    host mirror classes against the reference device classes (the pin of the opt-in device-physics torque model)."""
    import spin_torque_gym_amd as stg
    o = oracle_mod
    g = golden("G12_device_terms")
    fac = stg.DeviceFactory()
    for tag, over in G12_SOT.items():
        d = sot_default_params(**over)
        p = o.make_params(d, "sot_mram")
        dev = fac.create_device("sot_mram", {k: v for k, v in d.items() if k != "current_direction"})
        for m, J, dl, fl in zip(g["m"], g["J"], g[f"sot_{tag}_tau_dl"], g[f"sot_{tag}_tau_fl"]):
            a, b = o.sot_torque(m, J, p)
            assert np.allclose(a, dl, rtol=1e-14, atol=0) and np.allclose(b, fl, rtol=1e-14, atol=0), tag
            a2, b2 = dev.compute_spin_torque(J, m, over.get("current_direction"))
            assert np.allclose(a2, dl, rtol=1e-14, atol=0) and np.allclose(b2, fl, rtol=1e-14, atol=0), tag
        # the reference's own unit test: the damping-like torque is perpendicular to m (tests/unit/test_devices.py:176-190)
        a, _ = o.sot_torque(np.array([0.0, 1.0, 0.0]), 1e6, p)
        assert abs(np.dot(a, [0.0, 1.0, 0.0])) < 1e-10
    for tag, over in G12_VCMA.items():
        d = vcma_default_params(**over)
        p = o.make_params(d, "vcma_mram")
        dev = fac.create_device("vcma_mram", d)
        for v, k in zip(g["volts"], g[f"vcma_{tag}_keff"]):
            assert o.vcma_keff(v, p) == k and dev.effective_anisotropy(v) == k, (tag, v)
        # tests/unit/test_devices.py:266-278
        assert o.vcma_keff(0.0, p) == d["uniaxial_anisotropy"] and o.vcma_keff(10.0, p) == o.vcma_keff(p.vcma_vbd, p)


def test_device_torque_model_reduces_to_reference_for_stt(oracle_mod):
    """torque_model = 1 leaves STT classes untouched: bit-identical to the reference RHS."""
    o = oracle_mod
    p = o.make_params(stt_default_params(volume=8.75e-11))
    m0 = np.array([0.3, 0.2, 0.93]) / np.linalg.norm([0.3, 0.2, 0.93])
    a = o.simple_solve(m0, 3.3e-10, p, o.make_config("rk4"), 1.5e6)
    b = o.simple_solve(m0, 3.3e-10, p, o.make_config("rk4", torque_model=1), 1.5e6)
    assert np.array_equal(a["m_final"], b["m_final"])
    # and SOT / VCMA classes do change the dynamics
    for dev, d in (("sot_mram", sot_default_params(polarization=0.7, volume=8.75e-11)),
                   ("vcma_mram", vcma_default_params(polarization=0.6, volume=5e-11, vcma_coefficient=3e-13))):
        p = o.make_params(d, dev)
        a = o.simple_solve(m0, 3.3e-10, p, o.make_config("rk4"), 1.5e6)
        b = o.simple_solve(m0, 3.3e-10, p, o.make_config("rk4", torque_model=1), 1.5e6)
        assert a["success"] and b["success"] and np.abs(a["m_final"] - b["m_final"]).max() > 1e-6, dev


G13_EPISODES = {
    "individual_dipolar": (dict(rows=4, cols=4, action_mode="individual"), ("dipolar", 0.1), "stt_mram", {}),
    "row_exchange": (dict(rows=4, cols=4, action_mode="row"), ("exchange", 0.3), "stt_mram", {}),
    "column_stray": (dict(rows=3, cols=5, action_mode="column", obs_mode="vector", max_steps=4), ("stray_field", 0.1), "stt_mram", {}),
    "global": (dict(rows=4, cols=4, action_mode="global"), ("dipolar", 0.1), "stt_mram", {}),
    "nocoupling_custom": (dict(rows=2, cols=3, action_mode="individual", include_coupling=False, max_current=1e6,
                               max_duration=1e-9, success_threshold=0.2, energy_penalty_weight=0.3, obs_mode="vector",
                               temperature=350.0), None, "stt_mram", {}),
    "sot_devices": (dict(rows=3, cols=3, action_mode="row"), ("dipolar", 0.1), "sot_mram", dict(aspect_ratio=2.0)),
    "vcma_devices": (dict(rows=2, cols=2, action_mode="individual"), ("dipolar", 0.1), "vcma_mram",
                     dict(aspect_ratio=0.5, reference_magnetization=np.array([0.0, 0.2, 1.0]))),
}


def array_device_params(dev, over):
    base = {"stt_mram": stt_default_params, "sot_mram": sot_default_params, "vcma_mram": vcma_default_params}[dev]
    return base(**over)


def test_g13_array_env(golden, oracle_mod):
    """SpinTorqueArray-v0: the oracle's restatement against recorded reference episodes."""
    o = oracle_mod
    g = golden("G13_array_env")
    for k, tag in enumerate(g["episode_tags"]):
        ckw, coup, dev, over = G13_EPISODES[str(tag)]
        c = o.make_array_config(**ckw)
        p = o.make_params(array_device_params(dev, over), dev)
        n = c.rows * c.cols
        cm = o.array_coupling(c.rows, c.cols, *coup) if coup else np.zeros((n, n))
        if coup:
            assert np.array_equal(cm, g[f"ep{k}_coupling"]), tag
        st = o.ArrayEnvState(g[f"ep{k}_pattern"][0], g[f"ep{k}_target"])
        assert np.allclose(o.array_observation(st, c), g[f"ep{k}_obs"][0], rtol=2e-7, atol=1e-12), tag
        for j, a in enumerate(g[f"ep{k}_actions"]):
            obs, r, te, tr, en = o.array_step(st, a, p, c, cm)
            assert np.abs(st.pattern.reshape(-1) - g[f"ep{k}_pattern"][j + 1].reshape(-1)).max() <= 1e-12, (tag, j)
            assert np.allclose(obs, g[f"ep{k}_obs"][j + 1], rtol=2e-7, atol=1e-12), (tag, j)
            rr = g[f"ep{k}_reward"][j]
            assert abs(r - rr) <= 1e-11 * max(1.0, abs(rr)), (tag, j, r, rr)
            assert te == bool(g[f"ep{k}_terminated"][j]) and tr == bool(g[f"ep{k}_truncated"][j]), (tag, j)
            assert abs(en - g[f"ep{k}_energy"][j]) <= 1e-12 * max(abs(g[f"ep{k}_energy"][j]), 1e-300), (tag, j)
    # device.compute_effective_field for the three classes, oracle and host mirror
    import spin_torque_gym_amd as stg
    fac = stg.DeviceFactory()
    for dev, over in (("stt_mram", {}), ("sot_mram", dict(aspect_ratio=2.0)),
                      ("vcma_mram", dict(aspect_ratio=0.5, reference_magnetization=np.array([0.0, 0.2, 1.0])))):
        d = array_device_params(dev, over)
        p = o.make_params(d, dev)
        device = fac.create_device(dev, d)
        for m, h in zip(g["field_m"], g[f"field_{dev}"]):
            assert np.allclose(o.device_field(m, p), h, rtol=1e-14, atol=1e-9), dev
            assert np.allclose(device.compute_effective_field(m.copy(), np.zeros(3)), h, rtol=1e-14, atol=1e-9), dev


_SOT_G13, _VCMA_G13 = dict(aspect_ratio=2.0), dict(aspect_ratio=0.5, reference_magnetization=np.array([0.0, 0.2, 1.0]))
# tag -> (array config, (coupling type, strength) or None, device type, parameter overrides): make_golden.py G20, restated as data
G20_EPISODES = {
    "1x1_individual": (dict(rows=1, cols=1, action_mode="individual", max_steps=5), ("dipolar", 0.1), "stt_mram", {}),
    "1x7_column": (dict(rows=1, cols=7, action_mode="column", obs_mode="vector"), ("exchange", 0.3), "stt_mram", {}),
    "1x7_row": (dict(rows=1, cols=7, action_mode="row", success_threshold=0.004), ("stray_field", 0.1), "stt_mram", {}),
    "7x1_row": (dict(rows=7, cols=1, action_mode="row", obs_mode="vector", max_steps=6, temperature=350.0), ("dipolar", 0.2), "stt_mram", {}),
    "7x1_column": (dict(rows=7, cols=1, action_mode="column", include_coupling=False, max_current=1e6, max_duration=1e-9,
                        energy_penalty_weight=0.3), None, "stt_mram", {}),
    "5x3_row": (dict(rows=5, cols=3, action_mode="row", max_current=5e3, obs_mode="vector"), ("dipolar", 0.1), "sot_mram", _SOT_G13),
    "3x5_row": (dict(rows=3, cols=5, action_mode="row", max_current=5e3, max_steps=4), ("exchange", 0.3), "vcma_mram", _VCMA_G13),
    "5x5_global": (dict(rows=5, cols=5, action_mode="global", obs_mode="vector", success_threshold=-0.002), ("stray_field", 0.1), "stt_mram", {}),
    "8x8_row": (dict(rows=8, cols=8, action_mode="row"), ("dipolar", 0.1), "stt_mram", {}),
    "8x8_column": (dict(rows=8, cols=8, action_mode="column", obs_mode="vector", max_steps=3), ("exchange", 0.3), "stt_mram", {}),
    "8x8_global": (dict(rows=8, cols=8, action_mode="global", max_current=5e3), ("stray_field", 0.1), "sot_mram", _SOT_G13),
    "2x32_column": (dict(rows=2, cols=32, action_mode="column", max_current=5e3, obs_mode="vector"), ("dipolar", 0.1), "vcma_mram", _VCMA_G13),
    "nan_2x3_individual": (dict(rows=2, cols=3, action_mode="individual", obs_mode="vector"), ("dipolar", 0.2), "stt_mram", {}),
    "nan_3x3_global": (dict(rows=3, cols=3, action_mode="global"), ("dipolar", 0.1), "stt_mram", {}),
}


def g20_check_step(g, k, j, pattern, obs, r, te, tr, en, tag, pat_tol=1e-12, obs_tol=(2e-7, 1e-12), r_tol=1e-11, e_tol=1e-12):
    """One step of episode k against the recording; NaN where, and only where, the reference has NaN."""
    gp = g[f"ep{k}_pattern"][j + 1].reshape(-1)
    pattern = np.asarray(pattern, dtype=np.float64).reshape(-1)
    assert np.array_equal(np.isnan(pattern), np.isnan(gp)), (tag, j)
    ok = ~np.isnan(gp)
    assert not ok.any() or np.abs(pattern[ok] - gp[ok]).max() <= pat_tol, (tag, j)
    assert np.allclose(np.asarray(obs).reshape(-1), g[f"ep{k}_obs"][j + 1], rtol=obs_tol[0], atol=obs_tol[1], equal_nan=True), (tag, j)
    rr, ee = float(g[f"ep{k}_reward"][j]), float(g[f"ep{k}_energy"][j])
    assert np.isnan(r) == np.isnan(rr) and (np.isnan(rr) or abs(r - rr) <= r_tol * max(1.0, abs(rr))), (tag, j, r, rr)
    assert bool(te) == bool(g[f"ep{k}_terminated"][j]) and bool(tr) == bool(g[f"ep{k}_truncated"][j]), (tag, j)
    assert np.isnan(en) == np.isnan(ee) and (np.isnan(ee) or abs(en - ee) <= e_tol * max(abs(ee), 1e-300)), (tag, j, en, ee)


def test_g20_array_edges(golden, oracle_mod):
    """The array env at the shapes G13 leaves out and with edge actions (index out of range / fractional, J = 0, |J| = 1e-13,
    J and T beyond their limits), and NaN / infinite J and T: np.clip keeps NaN, so J = NaN drives nothing and T = NaN
    writes NaN into the addressed cell.  Tolerances of test_g13_array_env; NaN positions must coincide."""
    o = oracle_mod
    g = golden("G20_array_edges")
    assert [str(t) for t in g["episode_tags"]] == list(G20_EPISODES)
    import spin_torque_gym_amd as stg
    kinds = dict(terminated=0, truncated=0, nan=0)
    for k, tag in enumerate(g["episode_tags"]):
        tag = str(tag)
        ckw, coup, dev, over = G20_EPISODES[tag]
        c = o.make_array_config(**ckw)
        p = o.make_params(array_device_params(dev, over), dev)
        n = c.rows * c.cols
        cm = o.array_coupling(c.rows, c.cols, *coup) if coup else np.zeros((n, n))
        if coup:     # the oracle's table, the host's table and (up to 25 cells) the reference's
            assert np.allclose(cm, stg.array_env.compute_coupling_matrix(c.rows, c.cols, *coup), rtol=1e-15, atol=0), tag
            if f"ep{k}_coupling" in g.files:
                assert np.array_equal(cm, g[f"ep{k}_coupling"]), tag
        assert np.array_equal(g[f"ep{k}_target"], stg.array_env.checkerboard_pattern(c.rows, c.cols)), tag
        st = o.ArrayEnvState(g[f"ep{k}_pattern"][0], g[f"ep{k}_target"])
        assert np.allclose(o.array_observation(st, c), g[f"ep{k}_obs"][0], rtol=2e-7, atol=1e-12), tag
        for j, a in enumerate(g[f"ep{k}_actions"]):
            obs, r, te, tr, en = o.array_step(st, a, p, c, cm)
            g20_check_step(g, k, j, st.pattern, obs, r, te, tr, en, tag)
            kinds["terminated"] += int(te); kinds["truncated"] += int(tr); kinds["nan"] += int(np.isnan(r))
    assert all(v > 0 for v in kinds.values()), kinds


def test_g14_ornstein_uhlenbeck_field(golden, oracle_mod):
    """ThermalFluctuations' correlated field (thermal_model.py:113-137): the oracle's update, fed the white samples the
    reference's seeded generator produced, reproduces the reference's field sequence; and a solve with noise_model = 1
    is a solve whose thermal field is that recurrence over the kernels' own normal stream (held per sub-step)."""
    g = golden("G14_thermal_ou")
    for i, (seed, tau, dt, strength) in enumerate(g["cases"]):
        rng = np.random.default_rng(int(seed))
        x = np.zeros(3)
        for k, ref in enumerate(g[f"field_{i}"]):
            x = oracle_mod.ou_update(x, rng.normal(0, 1, 3), dt, tau)
            assert np.allclose(strength * x, ref, rtol=1e-13, atol=0), (i, k)
    # oracle solve with the OU field == hand-rolled RK4 over the same recurrence (Simple RHS from the oracle itself)
    from conftest import stt_default_params
    p = oracle_mod.make_params(stt_default_params(volume=1e-27))
    T, J, tau = 3e-11, 0.0, 2e-12
    c = oracle_mod.make_config(solver="rk4", thermal=True, seed=21, noise_model=1, noise_corr_time=tau)
    m0 = np.array([0.3, 0.2, 0.93]); m0 /= np.linalg.norm(m0)
    out = oracle_mod.simple_solve(m0, T, p, c, J, env_id=5, env_step=2)
    n = out["n_steps"]
    dt = T / n
    hs = oracle_mod.thermal_strength(p, 2.21e5, 300.0, 0)   # SimpleLLGSSolver's constant
    m, x = m0.copy(), np.zeros(3)
    for i in range(n):
        x = oracle_mod.ou_update(x, oracle_mod.thermal_normals(21, 5, 2, i), dt, tau)   # call i = sub-step i's normals
        h = hs * x
        t = i * dt
        f = lambda y, ts: dt * oracle_mod.simple_dmdt(y, p, 2.21e5, J if ts <= T else 0.0, h)
        k1 = f(m, t); k2 = f(m + k1 / 2, t + dt / 2); k3 = f(m + k2 / 2, t + dt / 2); k4 = f(m + k3, t + dt)
        m = m + (((k1 + 2 * k2) + 2 * k3) + k4) / 6
        m = m / np.linalg.norm(m)
    assert np.abs(out["m_final"] - m).max() <= 1e-13
    # and it is a different field from the white one
    cw = oracle_mod.make_config(solver="rk4", thermal=True, seed=21)
    assert np.abs(oracle_mod.simple_solve(m0, T, p, cw, J, env_id=5, env_step=2)["m_final"] - m).max() > 1e-9


G18_PARAMS = {"default": {}, "tilted": dict(easy_axis=np.array([0.3, 0.0, 1.0]))}


def test_g18_stable_states_relaxations(golden, oracle_mod):
    """find_stable_states' ingredients (physics/llgs_solver.py:264-305): the seeded global-np.random initial states, the
    10 ns J = 0 relaxations and the first-come de-duplicated list, recorded from the reference."""
    o = oracle_mod
    g = golden("G18_stable_states")
    c = o.make_config("rk45")
    for tag in (str(t) for t in g["tags"]):
        p = o.make_params(stt_default_params(**G18_PARAMS[tag]))
        np.random.seed(int(g[f"{tag}_seed"]))
        m_init = np.array([np.random.normal(0, 1, 3) for _ in range(len(g[f"{tag}_m_init"]))])
        m_init /= np.linalg.norm(m_init, axis=1, keepdims=True)
        assert np.array_equal(m_init, g[f"{tag}_m_init"])           # the legacy MT19937 stream is the reference's
        states = []
        for m0, ref in zip(m_init, g[f"{tag}_m_final"]):
            r = o.llgs_solve(m0, 10e-9, p, c, 0.0, cap=1)
            assert r["success"] and 10000 < r["n_points"] < 12000
            assert np.abs(r["m_final"] - ref).max() <= 1e-8, (tag, np.abs(r["m_final"] - ref).max())
            if all(np.linalg.norm(r["m_final"] - s) >= 1e-6 for s in states):
                states.append(r["m_final"])
        ref_states = g[f"{tag}_stable_states"]
        assert len(states) == len(ref_states) == 2 and np.abs(np.array(states) - ref_states).max() <= 1e-8


# ------------------------------------------------------------------------------------------------
# G21: the configuration away from its defaults (solver constants, episode fields, target lists, float64 actions)
# ------------------------------------------------------------------------------------------------
G21_CFG5 = dict(success_threshold=0.6, energy_penalty_weight=0.25, max_current=1.5e6, max_duration=2e-9, temperature=250.0)
G21_EPISODE_CFG = {
    "five_targets": dict(G21_CFG5, max_steps=4),
    "one_target": dict(G21_CFG5, max_steps=3),
    "eight_targets": dict(G21_CFG5, max_steps=3),
    "float64_five_targets": dict(G21_CFG5, max_steps=6),
    "float64_beyond_safety": dict(G21_CFG5, max_current=3e8, max_steps=5),
}


def g21_llgs_settings(g):
    """-> [(rtol, atol, max_step, gamma)] in the order of the golden's setting index"""
    rows = g["llgs_cases"]
    return [tuple(rows[rows[:, 0] == s][0, 1:5]) for s in sorted(set(rows[:, 0].astype(int)))]


def test_g21_llgs_solver_constants(golden, oracle_mod):
    """LLGSSolver(rtol, atol, max_step, gamma) at four non-default settings: accepted points, times and states (as G4 / G5)."""
    o = oracle_mod
    g = golden("G21_env_config")
    p = o.make_params(stt_default_params(volume=float(g["llgs_volume"])))
    settings = g21_llgs_settings(g)
    assert len(settings) == 4 and len(g["llgs_cases"]) == 12
    per_setting = {}
    for row in g["llgs_cases"]:
        s, (rtol, atol, max_step, gamma), m0, J, T, succ = int(row[0]), row[1:5], row[5:8], row[8], row[9], bool(row[10])
        k = per_setting.setdefault(s, 0)
        per_setting[s] += 1
        c = o.make_config("rk45", rtol=rtol, atol=atol, max_step=max_step, gamma=gamma)
        r = o.llgs_solve(m0, T, p, c, J)
        rt, rm = g[f"llgs_t_{s}_{k}"], g[f"llgs_m_{s}_{k}"]
        assert T <= 3e-10 and r["success"] == succ
        assert r["n_points"] == len(rt), (s, k, r["n_points"], len(rt))
        assert np.abs(r["t"] - rt).max() <= 1e-9 * T
        assert np.abs(r["m"] - rm).max() <= 1e-9, (s, k, np.abs(r["m"] - rm).max())
        # each setting is its own computation: the default constants give another point count or another end point
        d = o.llgs_solve(m0, T, p, o.make_config("rk45"), J)
        assert d["n_points"] != len(rt) or np.abs(d["m_final"] - rm[-1]).max() > 1e-9, (s, k)


def test_g21_simple_solver_max_step(golden, oracle_mod):
    """SimpleLLGSSolver(max_step) for rk4 and euler: step count (the truncation of T / dt, H5), success and the last row (as G2)."""
    o = oracle_mod
    g = golden("G21_env_config")
    p = o.make_params(stt_default_params(volume=float(g["simple_volume"])))
    assert set(g["simple_max_step"]) == {2.5e-12, 3e-13, 1e-10} and len(g["simple_T"]) == 24
    assert 1e-12 in g["simple_T"] and any(T == float(np.float32(T)) and T != 1e-12 for T in g["simple_T"])
    worst = 0.0
    for k in range(len(g["simple_T"])):
        c = o.make_config("euler" if g["simple_euler"][k] else "rk4", max_step=float(g["simple_max_step"][k]))
        r = o.simple_solve(g["simple_m0"][g["simple_m0_index"][k]], g["simple_T"][k], p, c, g["simple_J"][k])
        assert r["success"] == bool(g["simple_success"][k]), k
        assert r["n_steps"] == g["simple_n_steps"][k], (k, r["n_steps"], g["simple_n_steps"][k])
        worst = max(worst, np.abs(r["m_final"] - g["simple_m_last"][k]).max())
    assert worst <= 1e-11, worst
    assert len(set(g["simple_n_steps"])) >= 4           # max_step does set the sub-step count


def g21_episode(g, k, o):
    """Oracle state, parameters and configuration at the start of G21 episode k, and whether its actions are float64."""
    tag = str(g["episode_tags"][k])
    p = o.make_params(stt_default_params(volume=float(g[f"ep{k}_volume"])))
    c = o.make_config("rk4", thermal=False, **G21_EPISODE_CFG[tag])
    s = o.EnvState()
    m0, tgt = g[f"ep{k}_m0"], g[f"ep{k}_target"]
    s.m[:] = list(m0 / np.linalg.norm(m0))
    s.target[:] = list(tgt / np.linalg.norm(tgt))
    return tag, p, c, s, g[f"ep{k}_actions"].dtype == np.float64


def test_g21_env_episodes_and_float64_actions(golden, oracle_mod):
    """SpinTorqueEnv episodes with 5 / 1 / 8 target_states and non-default threshold, weight, limits and temperature; two of them stepped
    with float64 action arrays (the oracle's float64 entry).  Tolerances of G6."""
    o = oracle_mod
    g = golden("G21_env_config")
    tags = [str(t) for t in g["episode_tags"]]
    assert tags == list(G21_EPISODE_CFG)
    assert [len(g[f"ep{k}_target_states"]) for k in range(3)] == [5, 1, 8]
    for k, tag in enumerate(tags):
        ts = g[f"ep{k}_target_states"]
        assert np.abs(np.linalg.norm(ts, axis=1) - 1).max() <= 1e-15           # the constructor normalises the list
        tag, p, c, s, f64 = g21_episode(g, k, o)
        assert f64 == tag.startswith("float64")
        acts = g[f"ep{k}_actions"]
        if f64:             # the recorded actions are not float32 values, and some lie beyond every limit
            finite = acts[np.isfinite(acts)]
            assert np.any(finite.astype(np.float32).astype(np.float64) != finite)
            assert np.nanmax(np.abs(acts[:, 0])) > c.max_current and np.nanmax(acts[:, 1]) > c.max_duration
        for j, a in enumerate(acts):
            out = o.env_step_f64(s, a, p, c) if f64 else o.env_step(s, a, p, c)
            ref_obs = g[f"ep{k}_obs"][j + 1]
            assert np.allclose(np.array(out.obs[:]), ref_obs, rtol=2e-7, atol=1e-12), (tag, j, np.array(out.obs[:]), ref_obs)
            ref_r = g[f"ep{k}_reward"][j]
            assert abs(out.reward - ref_r) <= 1e-11 * max(1.0, abs(ref_r)), (tag, j, out.reward, ref_r)
            assert bool(out.terminated) == bool(g[f"ep{k}_terminated"][j]), (tag, j)
            assert bool(out.truncated) == bool(g[f"ep{k}_truncated"][j]), (tag, j)
            assert (out.status != 1) == bool(g[f"ep{k}_success"][j]), (tag, j)
            ref_e = g[f"ep{k}_energy"][j]
            assert abs(out.energy - ref_e) <= 1e-13 * max(abs(ref_e), 1e-300), (tag, j)
            assert np.abs(np.array(s.m[:]) - g[f"ep{k}_m"][j + 1]).max() <= 1e-11, (tag, j)
            if f64:         # what the float64 clamps made of the action is what the observation reports (obs 10, 11)
                J, T = o.parse_action_f64(a, c)
                assert np.float32(J / c.max_current) == ref_obs[10] and np.float32(T / c.max_duration) == ref_obs[11], (tag, j, J, T)
    # beyond the safety wrapper: 2.5e8 A/m^2 came back as 1e8 under max_current = 3e8, 3 us as max_duration
    k = tags.index("float64_beyond_safety")
    assert g[f"ep{k}_obs"][1][10] == np.float32(1e8 / 3e8) and g[f"ep{k}_obs"][3][11] == np.float32(1.0)

"""NumPy restatement of ONE env step with piecewise-linear current and field waveforms (stg_step_wave; RK4 and Euler -- RK45 with the
C oracle's waveform solve handed in, see step --, the thermal field of
tests/waveform_ref.py, STT / SOT / VCMA device classes under the reference torque model), vectorised over envs: the action parse, the solve (tests/waveform_ref.py), the energy of the pulse, the state
update, observation, reward and flags.  Written from the definitions in include/spintorque_hip.h and the env-step arithmetic of the
reference env (spin_torque_env.py:310-407, 474-520); tests/test_wave_step_host.py pins it against the C oracle's rectangular step (no
tables) and against the steps the reference env itself computed under shaped pulses (tests/golden/G23_wave_step.npz).

Everything is elementwise float64 NumPy (IEEE, no fused multiply-add)."""
import numpy as np

import waveform_ref

STATUS_OK, STATUS_NOOP, STATUS_RESET, STATUS_INACTIVE = 0, 1, 2, 3

DEFAULT_CFG = dict(max_current=2e6, max_duration=5e-9, success_threshold=0.9, energy_penalty_weight=0.1, max_steps=100, temperature=300.0,
                   max_step=1e-12, skip_done=False, gamma=2.21e5, target_states=None)


def parse_actions(a, max_current, max_duration):
    """a [N,2] float32 or float64 -> (J [N], T [N]) float64: the safety clamp in the action's own dtype (NaN kept), NaN / Inf in either
    component -> (0, 1e-12), then the fp64 clips."""
    a = np.array(a)
    dt = a.dtype.type
    with np.errstate(invalid="ignore"):
        a0 = np.where(np.isnan(a[:, 0]), a[:, 0], np.clip(a[:, 0], dt(-1e8), dt(1e8)))
        a1 = np.where(np.isnan(a[:, 1]), a[:, 1], np.clip(a[:, 1], dt(1e-12), dt(1e-6)))
    bad = np.isnan(a0) | np.isnan(a1) | np.isinf(a0) | np.isinf(a1)
    a0 = np.where(bad, dt(0), a0).astype(np.float64)
    a1 = np.where(bad, dt(1e-12), a1).astype(np.float64)
    return np.clip(a0, -max_current, max_current), np.clip(a1, 1e-12, max_duration)


def tables_valid(tk, vk):
    """[N]: the table is finite with strictly increasing times"""
    tk, vk = np.asarray(tk, float), np.asarray(vk, float)
    with np.errstate(invalid="ignore"):
        inc = (np.diff(tk, axis=1) > 0).all(axis=1)
    return np.isfinite(tk).all(axis=1) & np.isfinite(vk.reshape(len(tk), -1)).all(axis=1) & inc


def pulse_sq_integral(tk, vk, T):
    """I = the integral of j(t)^2 over [0, T] per env for current tables tk [N,K], vk [N,K]: the closed form of include/spintorque_hip.h
    (stg_step_wave), piece by piece in knot order."""
    tk, vk, T = np.asarray(tk, float), np.asarray(vk, float), np.asarray(T, float)
    K = tk.shape[1]
    t0, v0 = tk[:, 0], vk[:, 0]
    I = np.where(t0 > 0.0, np.minimum(t0, T) * (v0 * v0), 0.0)
    for k in range(K - 1):
        t1, v1 = tk[:, k + 1], vk[:, k + 1]
        lo, hi = np.maximum(t0, 0.0), np.minimum(t1, T)
        sl = (v1 - v0) / (t1 - t0)
        ja = np.where(lo == t0, v0, v0 + (lo - t0) * sl)
        jb = np.where(hi == t1, v1, v0 + (hi - t0) * sl)
        piece = ((hi - lo) * ((ja * ja + ja * jb) + jb * jb)) / 3.0
        I = np.where(hi > lo, I + piece, I)
        t0, v0 = t1, v1
    return np.where(T > t0, I + (T - np.maximum(t0, 0.0)) * (v0 * v0), I)


def resistance(m, p, device_type="stt_mram"):
    """compute_resistance of the device classes per row of m [N,3]: STTMRAMDevice (stt_mram.py:78-97), SOTMRAMDevice (sot_mram.py:196-228:
    the junction plus a tenth of the heavy-metal line, floor 1 Ohm) and VCMAMRAMDevice (vcma_mram.py:236-257: floor 1 Ohm).  The SOT and
    VCMA forms take m as it is; tests/test_wave_config_host.py pins all three against oracle.resistance."""
    r_p, r_ap = p["resistance_parallel"], p["resistance_antiparallel"]
    ref = np.asarray(p.get("reference_magnetization", [0, 0, 1]), dtype=float)
    ref = ref / np.sqrt((ref[0] * ref[0] + ref[1] * ref[1]) + ref[2] * ref[2])
    if device_type != "stt_mram":
        cos = (m[:, 0] * ref[0] + m[:, 1] * ref[1]) + m[:, 2] * ref[2]
        r = r_p + (r_ap - r_p) * (1.0 - cos) / 2
        if device_type == "sot_mram":
            thickness = p.get("thickness", 1e-9)
            area = p.get("area", p.get("volume", 1e-24) / thickness)
            r = r + (p.get("heavy_metal_resistivity", 2e-7) / p.get("heavy_metal_thickness", 5e-9)) / (area * 1e-12) * 0.1
        return np.maximum(r, 1.0)
    mn = m / np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])[:, None]
    tmr = (r_ap - r_p) / r_p
    cos = (mn[:, 0] * ref[0] + mn[:, 1] * ref[1]) + mn[:, 2] * ref[2]
    return np.maximum(r_p * (1.0 + tmr * (1.0 - cos) * 0.5), r_p * 0.5)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def observation(m, target, r, p, cfg, step_count, total_energy, J, T):
    with np.errstate(over="ignore"):
        cols = [m[:, 0], m[:, 1], m[:, 2], target[:, 0], target[:, 1], target[:, 2], r / p["resistance_parallel"],
                np.full(len(m), cfg["temperature"] / 300.0), (cfg["max_steps"] - step_count) / cfg["max_steps"], total_energy * 1e12,
                J / cfg["max_current"], T / cfg["max_duration"]]
        return np.nan_to_num(np.stack(cols, axis=1).astype(np.float32), nan=0.0, posinf=1e6, neginf=-1e6)


def step(state, actions, params, method="rk4", current=None, field=None, cfg=None, cls=None, done=None, dev_types=None, thermal=None, solve=None):
    """One env step of N envs (autoreset off).
    state: dict(m [N,3], target [N,3], total_energy [N], step_count [N]); actions [N,2] float32 / float64;
    params: one device-parameter dict, or a list of them with cls [N] (class index per env);
    current = (tj [N,K], jk [N,K]) or None (the rectangular parsed J); field = (th [N,K], hk [N,K,3]) or None (zero field);
    done [N] bool with cfg['skip_done']: those envs are not stepped (STATUS_INACTIVE).
    cfg: DEFAULT_CFG's keys; gamma and max_step go to the solve; target_states (a list of rows, normalised here as the env does) only
    says which targets an env may hold: every row of state['target'] must be one of them.
    dev_types: the device type of each class ('stt_mram' | 'sot_mram' | 'vcma_mram'; None: all STT); it selects the resistance form.
    thermal = None or dict(oracle, seed, env_id0, rng_step [N], noise 'white' | 'ou', corr_time): the thermal field at cfg's temperature
    on the stream (seed, env_id0 + i, rng_step[i]), strength per class from oracle.thermal_strength (waveform_ref.thermal_field).
    method 'rk45' takes its integrator from the caller: solve(m0 [n,3], T [n], p, J [n] or None, current, field, env [n]) for the envs
    `env` of one class -> dict(success [n], n_steps [n] (accepted points excluding t0), m_final [n,3]); tests/wave_rk45_cases.py:
    rk45_solver builds it on oracle.llgs_solve_wave, thermal stream included (`thermal` stays None).  The tail -- energy from
    pulse_sq_integral, reward, flags, observation -- is the one below for every method.
    Returns dict(m, total_energy, step_count, obs [N,12] float32, reward [N] float64, terminated, truncated, energy, status, J, T, n_sub)."""
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    m0 = np.array(state["m"], dtype=float)
    target = np.array(state["target"], dtype=float)
    etot = np.array(state["total_energy"], dtype=float)
    steps = np.array(state["step_count"], dtype=np.int64)
    N = len(m0)
    plist = [params] if isinstance(params, dict) else list(params)
    dev_types = ["stt_mram"] * len(plist) if dev_types is None else list(dev_types)
    if cfg["target_states"] is not None:
        allowed = np.array(cfg["target_states"], dtype=float)
        allowed = allowed / np.linalg.norm(allowed, axis=1, keepdims=True)
        assert (np.abs(target[:, None, :] - allowed[None]).max(axis=2).min(axis=1) <= 5e-16).all(), "a target that is not in cfg['target_states']"
    cls = np.zeros(N, dtype=np.int64) if cls is None else np.asarray(cls, dtype=np.int64)
    J, T = parse_actions(actions, cfg["max_current"], cfg["max_duration"])
    ok_tab = np.ones(N, dtype=bool)
    if current is not None:
        ok_tab &= tables_valid(*current)
    if field is not None:
        ok_tab &= tables_valid(*field)
    stepped = np.ones(N, dtype=bool) if not (cfg["skip_done"] and done is not None) else ~np.asarray(done, dtype=bool)
    success, m_new, n_sub, r_before = np.zeros(N, dtype=bool), m0.copy(), np.zeros(N, dtype=np.int64), np.zeros(N)
    for c, p in enumerate(plist):
        sel = np.nonzero((cls == c))[0]
        if not len(sel):
            continue
        r_before[sel] = resistance(m0[sel], p, dev_types[c])
        run = sel[ok_tab[sel] & stepped[sel]]
        if not len(run):
            continue
        cur = None if current is None else (np.asarray(current[0])[run], np.asarray(current[1])[run])
        fld = None if field is None else (np.asarray(field[0])[run], np.asarray(field[1])[run])
        if method == "rk45":
            assert solve is not None and thermal is None, "method 'rk45' integrates with the caller's solve (tests/wave_rk45_cases.py: rk45_solver)"
            res = solve(m0[run], T[run], p, J[run] if current is None else None, cur, fld, run)
        else:
            res = waveform_ref.solve(m0[run], T[run], p, method, current=cur, J=J[run] if current is None else None, field=fld,
                                     max_step=cfg["max_step"], temperature=cfg["temperature"], gamma=cfg["gamma"],
                                     thermal=None if thermal is None else waveform_ref.thermal_field(
                                         thermal["oracle"], p, dev_types[c], cfg["gamma"], cfg["temperature"], thermal["seed"],
                                         thermal.get("env_id0", 0) + run, np.asarray(thermal["rng_step"])[run], thermal.get("noise", "white"),
                                         thermal.get("corr_time", 1e-12)))
        success[run], n_sub[run] = res["success"], res["n_steps"]
        mf = res["m_final"]
        mf = mf / np.sqrt((mf[:, 0] * mf[:, 0] + mf[:, 1] * mf[:, 1]) + mf[:, 2] * mf[:, 2])[:, None]      # spin_torque_env.py:461-464
        m_new[run] = np.where(res["success"][:, None], mf, m0[run])
    area = np.array([p.get("area", 1e-14) for p in plist])[cls]
    if current is None:
        v = J * r_before * area
        energy = np.where(np.abs(J) > 1e-12, (v * v) / r_before * T, 0.0)                                   # spin_torque_env.py:474-480
    else:
        ra = r_before * area
        with np.errstate(invalid="ignore"):
            energy = (ra * ra) / r_before * pulse_sq_integral(current[0], current[1], T)
    energy = np.where(ok_tab & stepped, energy, 0.0)
    prev_align = _dot(m0, target)
    etot = np.where(stepped, etot + energy, etot)
    steps = np.where(stepped, steps + 1, steps)
    align = _dot(m_new, target)
    is_success = align >= cfg["success_threshold"]
    reward = 10.0 * np.where(is_success, 10.0, 0.0)
    reward = reward + (-cfg["energy_penalty_weight"]) * (-energy / 1e-12)
    reward = reward + (align - prev_align)
    reward = np.where(np.isnan(reward) | np.isinf(reward), -1.0, reward)
    reward = np.minimum(np.maximum(reward, -1e6), 1e6)
    reward = np.where(stepped, reward, 0.0)
    truncated = steps >= cfg["max_steps"]
    status = np.where(stepped, np.where(success, STATUS_OK, STATUS_NOOP), STATUS_INACTIVE).astype(np.uint8)
    obs = np.zeros((N, 12), dtype=np.float32)
    for c, p in enumerate(plist):
        sel = np.nonzero(cls == c)[0]
        if len(sel):
            obs[sel] = observation(m_new[sel], target[sel], resistance(m_new[sel], p, dev_types[c]), p, cfg, steps[sel], etot[sel], J[sel], T[sel])
    return dict(m=m_new, total_energy=etot, step_count=steps, obs=obs, reward=reward, terminated=is_success, truncated=truncated,
                energy=energy, status=status, J=J, T=T, n_sub=np.where(stepped, n_sub, 0), alignment=align)


# ------------------------------------------------------------------------------------------------
# tests/golden/G23_wave_step.npz: steps of the reference env under shaped pulses and fields (shared by the host and the GPU tests)
# ------------------------------------------------------------------------------------------------
F32_ULP = float(np.finfo(np.float32).eps)


def g23_params(g):
    from conftest import stt_default_params
    return stt_default_params(volume=float(g["volume"]))


def g23_tables(g, k):
    """step k of G23 -> (current, field) as wave_step_ref.step takes them (N = 1), built as the envs build them: tau_k * T, J * s_k"""
    kj, kh = int(g["kj"][k]), int(g["kh"][k])
    J, T = float(g["J"][k]), float(g["T"][k])
    cur = (g["tau"][k, :kj][None] * T, J * g["scale"][k, :kj][None]) if kj else None
    fld = (g["th"][k, :kh][None], g["hk"][k, :kh][None]) if kh else None
    return cur, fld


def g23_action(g, k):
    return np.array([g["action"][k]], dtype=np.float64 if g["act_f64"][k] else np.float32)


def g23_shape_and_field(g, k):
    """step k -> (pulse_shape, applied_field) constructor arguments"""
    from spin_torque_gym_amd.physics import PiecewiseLinear
    kj, kh = int(g["kj"][k]), int(g["kh"][k])
    shape = PiecewiseLinear(g["tau"][k, :kj], g["scale"][k, :kj]) if kj else None
    if kh == 0:
        return shape, None
    if kh == 2 and np.array_equal(g["hk"][k, 0], g["hk"][k, 1]) and g["th"][k, 0] == 0.0 and g["th"][k, 1] == float(g["max_duration"]):
        return shape, g["hk"][k, 0].copy()                       # the constant form
    return shape, PiecewiseLinear(g["th"][k, :kh], g["hk"][k, :kh])


def check_step_against_g23(g, k, got, tol_m, where):
    """`got`: dict(m [3], obs [12], reward, terminated, truncated, energy) of step k.  Everything but the energy (and what hangs on it:
    obs[9] and the reward's energy term) against the file; the energy against the closed form."""
    cur, _ = g23_tables(g, k)
    p = g23_params(g)
    r = resistance(g["m_before"][k][None], p)[0]
    if cur is None:
        e_ref = float(g["energy_rect"][k])
    else:
        ra = r * p["area"]
        e_ref = float((ra * ra) / r * pulse_sq_integral(cur[0], cur[1], [float(g["T"][k])])[0])
    err = float(np.abs(got["m"] - g["m_after"][k]).max())
    assert err <= tol_m, (where, k, err)
    assert bool(got["terminated"]) == bool(g["terminated"][k]) and bool(got["truncated"]) == bool(g["truncated"][k]), (where, k)
    idx = [i for i in range(12) if i != 9]
    o, og = np.asarray(got["obs"], dtype=np.float32)[idx], g["obs"][k][idx]
    # (one float32 ulp, on values that themselves follow m to tol_m)
    assert np.all(np.abs(o - og) <= F32_ULP * np.abs(og) + tol_m), (where, k, o, og)
    assert abs(float(got["energy"]) - e_ref) <= 1e-12 * abs(e_ref), (where, k, float(got["energy"]), e_ref)
    w = DEFAULT_CFG["energy_penalty_weight"]
    base_ref = float(g["reward"][k]) - w * (float(g["energy_rect"][k]) / 1e-12)
    base_got = float(got["reward"]) - w * (float(got["energy"]) / 1e-12)
    assert abs(base_got - base_ref) <= 1e-9, (where, k, base_got, base_ref)
    return err

#!/usr/bin/env python3
"""Generate tests/golden/G24_wave_config.npz from the UNMODIFIED Python reference: waveform solves and env steps away from the default
configuration -- solver constants (rtol, atol, max_step, gamma), temperatures, the thermal field, the episode fields.

Same bootstrap as make_golden_waveforms.py / make_golden_wave_step.py (gymnasium stand-in, result cache cleared before every fixed-step
solve, wall-clock guard lifted, physics.PiecewiseLinear callables).  Nothing of the reference is copied: the file holds inputs and the
outputs the reference computed for them.

The thermal field.  Both reference solvers draw np.random.normal(0, 1, 3) exactly once per RHS call (simple_solver.py:384,
llgs_solver.py:112).  For the length of one solve np.random.normal is replaced by a callable that hands out
oracle.thermal_normals(seed, env_id, env_step, call) in call order -- the stream the kernels draw -- and put back afterwards.  Before
anything is recorded the generator proves that wiring where it is made: rectangular pulses through the patched reference against
oracle.simple_solve / oracle.llgs_solve on the same stream, <= 1e-12 with equal point counts.
The Brown field goes with 1 / sqrt(volume): in the rescaled volumes of the current-driven cases (8.75e-11, 9.7e-6) it is ~1e-9 A/m and
would show nothing, so the thermal cases use volume 1e-26 (RK45, whose tolerance is a hundred times wider: 4e-30) with the currents
scaled by the volume ratio, which keeps the spin torque per unit of action as it was.

Arrays (K = knots, padded with NaN to 8):
  sv_*  one row per solve: sv_solver (0 rk4, 1 euler: RobustLLGSSolver; 2: LLGSSolver RK45), sv_rtol, sv_atol, sv_max_step, sv_gamma,
        sv_temperature, sv_thermal, sv_seed, sv_env_id, sv_env_step (the stream key), sv_volume, sv_m0, sv_T, sv_kj / sv_tj / sv_jk
        (current knots; kj = 0: no current), sv_kh / sv_th / sv_hk (field knots); results sv_success, sv_n_points (sub-steps or accepted
        points), sv_attempts (RK45 attempts, counted from the current_func calls as make_golden_waveforms.py counts them; 0 for the
        fixed-step rows), sv_m_final.
  sv_traj_case, sv_traj_t, sv_traj_m, sv_traj_energy, sv_traj_torques: the whole result of one RK45 row.
  ev_*  one row per env step (SpinTorqueEnv driven through the shim of make_golden_wave_step.py, every episode field off its default:
        ev_max_current, max_duration, success_threshold, energy_penalty_weight, max_steps, temperature, targets): ev_episode, ev_solver,
        ev_thermal, ev_seed, ev_env_id (stream key; env_step = ev_step_before), ev_volume, ev_max_step, ev_kj / ev_tau / ev_scale (pulse
        shape over normalised time), ev_kh / ev_th / ev_hk, ev_action, ev_act_f64, ev_J, ev_T (parsed), ev_m_before, ev_target,
        ev_step_before, ev_etot_before; results ev_m_after, ev_obs, ev_reward, ev_terminated, ev_truncated, ev_energy_rect (the
        reference charges its own rectangular energy: the tests take energy, obs[9] and the reward's energy term from the closed form of
        include/spintorque_hip.h), ev_total_energy, ev_alignment.

The generator asserts about its own cases: every case is well conditioned (m0 moved by 1e-13 gives the same flags, with the thermal
field off the same counts, and rows within 1/100 of the tolerance the GPU test applies), no recorded |alignment - threshold| is below
1e-6, at least one RK45 case has rejected attempts, actions beyond both limits and a float64 action that float32 cannot carry occur.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wave_config.py
"""
import logging
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gym_stub  # noqa: E402

gym_stub.install()
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "spin-torque-rl-gym_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
warnings.simplefilter("ignore")
logging.disable(logging.CRITICAL)

import numpy as np  # noqa: E402

from spin_torque_gym.devices import DeviceFactory  # noqa: E402
from spin_torque_gym.envs.spin_torque_env import SpinTorqueEnv  # noqa: E402
from spin_torque_gym.physics.llgs_solver import LLGSSolver  # noqa: E402
from spin_torque_gym.utils.performance import get_optimizer  # noqa: E402
from spin_torque_gym.utils.robust_solver import RobustLLGSSolver  # noqa: E402

from spin_torque_gym_amd.physics import PiecewiseLinear  # noqa: E402

import oracle  # noqa: E402
from env_config_cases import FIXED_MAX_STEPS, RK45_SETTINGS, TARGETS5, THERMAL_FACTOR, TOL_RK4, TOL_RK45  # noqa: E402

KMAX = 8
PERTURB = 1e-13 * np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
VOL_RK4, VOL_RK45, VOL_THERMAL, VOL_THERMAL45 = 8.75e-11, 9.7e-6, 1e-26, 4e-30
EPISODE = dict(max_current=1.5e6, max_duration=2e-9, success_threshold=0.6, energy_penalty_weight=0.25, max_steps=3, temperature=250.0)

# the knot sets of G22 (make_golden_waveforms.py)
TRAPEZOID = ([0, 1e-10, 7e-10, 9e-10, 1.2e-9], [0, 2e6, 2e6, -1e6, 0])
BIPOLAR = ([1e-11, 3e-10, 3.5e-10, 8e-10], [-2e6, -2e6, 2e6, 2e6])
RAMP_H = ([0, 2e-10, 1.2e-9], [[0, 0, 0], [5e4, 0, -1e5], [5e4, 2e4, -1e5]])
CONST_H = ([0, 1e-9], [[1e5, 0, 0], [1e5, 0, 0]])
# pulse shapes over normalised time and fields of the env level (make_golden_wave_step.py)
SHAPES = {"trapezoid": ([0.0, 0.1, 0.8, 1.0], [0.0, 1.0, 1.0, 0.0]), "bipolar": ([0.0, 0.45, 0.55, 0.9, 1.0], [1.0, 1.0, -0.5, -0.5, 0.0])}
FIELDS = {"const": ([0.0, EPISODE["max_duration"]], [[1e5, 0.0, 0.0], [1e5, 0.0, 0.0]]), "ramp": RAMP_H}


def unit(v):
    v = np.array(v, dtype=float)
    return v / np.linalg.norm(v)


def stt_params(**over):
    p = DeviceFactory().get_default_parameters("stt_mram")
    p.update(over)
    return p


def robust_solver(method, max_step=1e-12):
    # the env's constructor arguments (envs/spin_torque_env.py:93-102) plus max_step, wall-clock guard lifted
    return RobustLLGSSolver(method=method, rtol=1e-3, atol=1e-6, max_step=max_step, timeout=1e9, max_retries=2, fallback_method="euler",
                            enable_monitoring=True, enable_validation=True)


def scaled(cur, s):
    return None if cur is None else (list(cur[0]), [s * x for x in cur[1]])


def pack(knots, width):
    t = np.full(KMAX, np.nan)
    v = np.full((KMAX,) if width == 1 else (KMAX, 3), np.nan)
    if knots is None:
        return 0, t, v
    k = len(knots[0])
    t[:k] = knots[0]
    v[:k] = knots[1]
    return k, t, v


class Stream:
    """np.random.normal for the length of one solve: oracle.thermal_normals(seed, env_id, env_step, call) in call order.  The oracle
    replays the stream from 0 on every call, so the draws are fetched one after the other and kept."""
    cache = {}

    def __init__(self, key):
        self.key, self.calls = tuple(int(x) for x in key), 0

    def __call__(self, loc, scale, size):
        assert (loc, scale, size) == (0, 1, 3)
        have = Stream.cache.setdefault(self.key, [])
        while len(have) <= self.calls:
            have.append(oracle.thermal_normals(*self.key, len(have)))
        self.calls += 1
        return have[self.calls - 1].copy()

    def __enter__(self):
        self.saved, np.random.normal = np.random.normal, self
        return self

    def __exit__(self, *exc):
        np.random.normal = self.saved


class Unpatched:
    calls = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


class Counted:
    def __init__(self, f):
        self.f, self.calls = f, 0

    def __call__(self, t):
        self.calls += 1
        return self.f(t)


def solve_case(c, m0):
    """one solve of the reference -> (success, n_points, attempts, m_final, whole result, normals drawn)"""
    params = stt_params(volume=c["volume"])
    cur = PiecewiseLinear(*c["cur"]) if c["cur"] is not None else None
    fld = PiecewiseLinear(*c["fld"]) if c["fld"] is not None else None
    with (Stream((c["seed"], c["env_id"], c["env_step"])) if c["thermal"] else Unpatched()) as st:
        if c["solver"] == "rk45":
            solver = LLGSSolver(rtol=c["rtol"], atol=c["atol"], max_step=c["max_step"], gamma=c["gamma"])
            cf = Counted(cur if cur is not None else (lambda t: 0.0))
            r = solver.solve(m0.copy(), (0, c["T"]), params, cf, fld, thermal_noise=c["thermal"], temperature=c["temperature"])
            npts = len(r["t"])
            # current_func calls: f(t0), select_initial_step's second call, six per attempt, one per accepted point (by-products)
            attempts, rest = divmod(cf.calls - npts - 2, 6)
            assert rest == 0 and attempts >= npts - 1, (cf.calls, npts)
            if c["thermal"]:
                assert st.calls == 2 + 6 * attempts, (st.calls, attempts)      # one draw per RHS call
            return bool(r["success"]), npts - 1, attempts, r["m"][-1], r, st.calls
        get_optimizer().cache.clear()               # the cache key does not hold the drive
        r = robust_solver(c["solver"], c["max_step"]).solve(m0.copy(), (0, c["T"]), params, cur, fld, c["thermal"], c["temperature"])
        if c["thermal"]:
            assert st.calls == r["n_steps"] * (4 if c["solver"] == "rk4" else 1), (st.calls, r["n_steps"])
        return bool(r["success"]), int(r["n_steps"]), 0, r["m"][-1], r, st.calls


def case(solver, m0, T, cur, fld, volume, thermal=False, temperature=300.0, key=(0, 0, 0), rtol=1e-6, atol=1e-9, max_step=1e-12, gamma=2.21e5):
    return dict(solver=solver, m0=unit(m0), T=T, cur=cur, fld=fld, volume=volume, thermal=thermal, temperature=temperature, seed=key[0],
                env_id=key[1], env_step=key[2], rtol=rtol, atol=atol, max_step=max_step, gamma=gamma)


def solve_cases():
    m_up, m_r, m_r2 = [0.02, -0.01, 0.9997], [0.5, -0.6, 0.3], [-0.3, 0.4, -0.7]
    c = []
    # (a) thermal off: the four RK45 settings, a current-plus-field and a field-only case each; the fixed-step solvers at three max_step
    for s in RK45_SETTINGS:
        c.append(case("rk45", m_up, 1e-9, TRAPEZOID, RAMP_H, VOL_RK45, **s))
        c.append(case("rk45", m_r, 3e-10, None, CONST_H, VOL_RK45, **s))
    for method in ("rk4", "euler"):
        for ms in FIXED_MAX_STEPS:
            c.append(case(method, m_r, 3e-10, TRAPEZOID, RAMP_H, VOL_RK4, max_step=ms))
            c.append(case(method, m_r2, float(np.float32(2.2e-10)), None, CONST_H, VOL_RK4, max_step=ms))
    # (b) thermal on: three temperatures, non-zero stream keys, two of the RK45 settings
    js4, js45 = VOL_THERMAL / VOL_RK4, VOL_THERMAL45 / VOL_RK45
    for j, (method, temp, ms) in enumerate([("rk4", 77.0, 2.5e-12), ("rk4", 250.0, 3e-13), ("rk4", 450.0, 1e-10),
                                            ("euler", 77.0, 3e-13), ("euler", 250.0, 1e-10), ("euler", 450.0, 2.5e-12)]):
        cur, fld = ((TRAPEZOID, RAMP_H), (BIPOLAR, CONST_H), (None, RAMP_H))[j % 3]
        c.append(case(method, (m_r, m_r2)[j % 2], (3e-10, 1.3e-10, 2e-10)[j % 3], scaled(cur, js4), fld, VOL_THERMAL, True, temp,
                      (4321 + j, 7 + 64 * j, 3 + j), max_step=ms))
    for j, (s, temp) in enumerate([(0, 77.0), (2, 450.0), (0, 250.0)]):
        cur, fld = ((TRAPEZOID, RAMP_H), (None, CONST_H), (BIPOLAR, None))[j]
        c.append(case("rk45", (m_up, m_r, m_r2)[j], (4e-10, 3e-10, 2e-10)[j], scaled(cur, js45), fld, VOL_THERMAL45, True, temp,
                      (99 + j, 130 + j, 11 + j), **RK45_SETTINGS[s]))
    return c


def stream_self_check():
    """rectangular pulses in zero field through the patched reference against the oracle's thermal solves"""
    m0 = unit([0.5, -0.6, 0.3])
    worst = 0.0
    for solver, T, kw in (("rk4", 1.3e-10, {}), ("euler", 1.3e-10, {}), ("rk45", 1.2e-10, {}),
                          ("rk45", 1.2e-10, dict(rtol=1e-4, atol=1e-7, max_step=5e-12, gamma=1.9e5))):
        vol = VOL_THERMAL45 if solver == "rk45" else VOL_THERMAL
        J = 1.5e6 * vol / (VOL_RK45 if solver == "rk45" else VOL_RK4)
        c = case(solver, m0, T, ([0.0, T], [J, J]), None, vol, True, 250.0, (1234, 5, 7), **kw)
        ok, npts, att, mf, r, calls = solve_case(c, c["m0"])
        cfg = oracle.make_config(solver=solver, thermal=True, temperature=250.0, seed=1234, rtol=c["rtol"], atol=c["atol"],
                                 max_step=c["max_step"], gamma=c["gamma"])
        p = oracle.make_params(stt_params(volume=vol))
        if solver == "rk45":
            o = oracle.llgs_solve(c["m0"], T, p, cfg, J, env_id=5, env_step=7)
            assert o["n_points"] - 1 == npts and o["n_attempts"] == att, (o["n_points"], npts, o["n_attempts"], att)
        else:
            o = oracle.simple_solve(c["m0"], T, p, cfg, J, env_id=5, env_step=7)
            assert o["n_steps"] == npts
        d = float(np.abs(o["m_final"] - mf).max())
        worst = max(worst, d)
        print(f"    stream self-check {solver} {kw or ''}: {calls} draws, |reference - oracle| = {d:.1e}")
        assert ok and o["success"] and d <= 1e-12, (solver, d)
    return worst


def solves(out):
    cases = solve_cases()
    cols = {k: [] for k in ("solver", "rtol", "atol", "max_step", "gamma", "temperature", "thermal", "seed", "env_id", "env_step", "volume", "m0",
                            "T", "kj", "tj", "jk", "kh", "th", "hk", "success", "n_points", "attempts", "m_final")}
    rejected_somewhere, loose = False, []
    for idx, c in enumerate(cases):
        ok, npts, att, mf, r, calls = solve_case(c, c["m0"])
        ok2, npts2, att2, mf2, _, _ = solve_case(c, c["m0"] + PERTURB)
        tol = (TOL_RK45 if c["solver"] == "rk45" else TOL_RK4) * (THERMAL_FACTOR if c["thermal"] else 1)
        d = float(np.abs(mf - mf2).max())
        good = ok and ok2 and d <= tol / 100 and (c["thermal"] or (npts == npts2 and att == att2))
        if not good:
            loose.append((idx, c["solver"], c["thermal"], d, npts, npts2, att, att2))
        if c["thermal"]:                               # the field matters: the same solve without it ends elsewhere
            _, _, _, mf0, _, _ = solve_case(dict(c, thermal=False), c["m0"])
            assert np.abs(mf0 - mf).max() > 20 * tol, (idx, float(np.abs(mf0 - mf).max()), tol)
        rejected_somewhere |= c["solver"] == "rk45" and att > npts
        print(f"    solve {idx}: {c['solver']} thermal={c['thermal']} T={c['temperature']:g} max_step={c['max_step']:g} gamma={c['gamma']:g}: "
              f"{npts} points, {att} attempts, {calls} draws; perturbed solve differs by {d:.1e} (tolerance / 100 = {tol / 100:.0e})")
        for k, v in zip(("kj", "tj", "jk"), pack(c["cur"], 1)):
            cols[k].append(v)
        for k, v in zip(("kh", "th", "hk"), pack(c["fld"], 3)):
            cols[k].append(v)
        for k in ("rtol", "atol", "max_step", "gamma", "temperature", "thermal", "seed", "env_id", "env_step", "volume", "m0", "T"):
            cols[k].append(c[k])
        cols["solver"].append(("rk4", "euler", "rk45").index(c["solver"]))
        cols["success"].append(ok); cols["n_points"].append(npts); cols["attempts"].append(att); cols["m_final"].append(mf)
        if c["solver"] == "rk45" and not c["thermal"] and c["cur"] is not None and c["rtol"] == 1e-3:
            out["sv_traj_case"] = np.int64(idx)
            for k in ("t", "m", "energy", "torques"):
                out["sv_traj_" + k] = np.asarray(r[k])
    assert not loose, ("ill-conditioned cases", loose)
    assert rejected_somewhere, "no RK45 case contains a rejected attempt"
    assert "sv_traj_case" in out
    for k, v in cols.items():
        out["sv_" + k] = np.array(v)


# ---- env level -----------------------------------------------------------------------------------------------------
def episodes():
    """(solver, thermal, max_step, shape or None, field or None, m0, target index, [(J, T, dtype)]): J in units of max_current"""
    f4, f8 = np.float32, np.float64
    t64 = 1.2345678901234567e-10                   # a duration float32 cannot carry
    assert float(np.float32(t64)) != t64
    gen, gen2 = [0.5, -0.6, 0.3], [-0.3, 0.4, -0.7]
    # (short pulses through off-axis states, as in make_golden_wave_step.py: a pulse that switches a settled state amplifies a
    # perturbation beyond the conditioning bound)
    return [
        ("rk4", False, 2.5e-12, "trapezoid", "const", gen, 1, [(-0.4, 1e-10, f4), (-1.7, 1.2e-10, f4), (-0.9, t64, f8)]),
        ("rk4", False, 3e-13, "bipolar", "ramp", gen2, 3, [(1.0, 1.5e-10, f4), (-2.5, 1e-10, f8), (0.6, 3e-9, f4)]),
        ("euler", False, 1e-10, None, "ramp", gen, 4, [(0.8, 1e-10, f4), (-1.3, 1.1e-10, f4), (0.5, 9e-11, f8)]),
        ("rk4", False, 1e-10, "trapezoid", None, [0.2, -0.5, 0.6], 3, [(-0.7, 1.4e-10, f4), (0.5, 6e-11, f8), (-1.4, 1.5e-10, f4)]),
        ("rk4", True, 2.5e-12, "trapezoid", "ramp", gen, 1, [(-0.4, 1e-10, f4), (1.7, 1.2e-10, f4), (-0.9, t64, f8)]),
        ("rk4", True, 1e-10, "bipolar", None, gen2, 3, [(1.0, 1.5e-10, f4), (-2.5, 1e-10, f8), (0.6, 3e-10, f4)]),
        ("euler", True, 3e-13, None, "const", [0.2, -0.5, 0.6], 4, [(0.8, 1e-10, f4), (-1.3, 1.1e-10, f4), (0.5, 9e-11, f8)]),
    ]


ENV_SEED, ENV_ID = 2024, 1


def make_env(solver, thermal, max_step, shape, field):
    volume = VOL_THERMAL if thermal else VOL_RK4
    cfg = dict(EPISODE)
    # (the thermal episodes: the smaller volume with max_current scaled by the volume ratio, see the head of the file)
    cfg["max_current"] = EPISODE["max_current"] * volume / VOL_RK4
    params = stt_params(volume=volume)
    env = SpinTorqueEnv(device_params=params, include_thermal_fluctuations=thermal, target_states=[np.array(t, dtype=float) for t in TARGETS5],
                        **cfg)
    env.cache_observations = False               # H2
    env.solver = robust_solver(solver, max_step)
    real = env.solver.solve

    def shim(m_initial, t_span, device_params, current_func=None, field_func=None, thermal_noise=False, temperature=300.0, **kw):
        J, T = float(env.last_action[0]), float(env.last_action[1])
        assert tuple(t_span) == (0, T) and thermal_noise == thermal and temperature == EPISODE["temperature"]
        if shape is not None:
            tau, s = np.asarray(SHAPES[shape][0]), np.asarray(SHAPES[shape][1])
            current_func = PiecewiseLinear(tau * T, J * s)
        if field is not None:
            field_func = PiecewiseLinear(*FIELDS[field])
        get_optimizer().cache.clear()            # H1
        with (Stream((ENV_SEED, ENV_ID, env.step_count)) if thermal else Unpatched()):
            return real(m_initial=m_initial, t_span=t_span, device_params=device_params, current_func=current_func, field_func=field_func,
                        thermal_noise=thermal_noise, temperature=temperature, **kw)

    env.solver.solve = shim
    return env, cfg["max_current"], volume


def env_steps(out):
    cols = {k: [] for k in ("episode", "solver", "thermal", "volume", "max_step", "max_current", "kj", "tau", "scale", "kh", "th", "hk", "action",
                            "act_f64", "J", "T", "m_before", "target", "step_before", "etot_before", "m_after", "obs", "reward", "terminated",
                            "truncated", "energy_rect", "total_energy", "alignment")}
    targets = np.array(TARGETS5, dtype=float)
    targets /= np.linalg.norm(targets, axis=1, keepdims=True)
    loose, margin = [], np.inf
    for e, (solver, thermal, ms, shape, field, m0, ti, actions) in enumerate(episodes()):
        env, jmax, volume = make_env(solver, thermal, ms, shape, field)
        env.reset(seed=0, options={"initial_state": unit(m0), "target_state": targets[ti].copy()})
        tol = TOL_RK4 * (THERMAL_FACTOR if thermal else 1)
        for (j, T, dt) in actions:
            act = np.array([j * jmax, T], dtype=np.float64)
            if dt is np.float64:
                act[0] = act[0] * (1 + 2.0 ** -30)                       # float32 cannot carry it
                assert T > EPISODE["max_duration"] or float(np.float32(act[1])) != act[1] or float(np.float32(act[0])) != act[0]
            m_before, step_before, etot_before = env.current_magnetization.copy(), env.step_count, env.total_energy
            twin, _, _ = make_env(solver, thermal, ms, shape, field)
            twin.reset(seed=0, options={"initial_state": m_before + PERTURB, "target_state": targets[ti].copy()})
            twin.step_count, twin.total_energy = step_before, etot_before
            o2, r2, te2, tr2, i2 = twin.step(act.astype(dt))
            obs, reward, term, trunc, info = env.step(act.astype(dt))
            assert "error" not in info and info["simulation_success"], (e, info.get("error"))
            d = float(np.abs(env.current_magnetization - twin.current_magnetization).max())
            if not (d <= tol / 100 and term == te2 and trunc == tr2):
                loose.append((e, j, T, d))
            align = float(np.dot(env.current_magnetization, env.target_magnetization))
            margin = min(margin, abs(align - env.success_threshold))
            for k, v in zip(("kj", "tau", "scale"), pack(None if shape is None else SHAPES[shape], 1)):
                cols[k].append(v)
            for k, v in zip(("kh", "th", "hk"), pack(None if field is None else FIELDS[field], 3)):
                cols[k].append(v)
            row = dict(episode=e, solver=0 if solver == "rk4" else 1, thermal=thermal, volume=volume, max_step=ms, max_current=jmax,
                       action=act, act_f64=dt is np.float64, J=float(env.last_action[0]), T=float(env.last_action[1]), m_before=m_before,
                       target=env.target_magnetization.copy(), step_before=step_before, etot_before=etot_before,
                       m_after=env.current_magnetization.copy(), obs=obs, reward=float(reward), terminated=bool(term), truncated=bool(trunc),
                       energy_rect=float(info["energy_consumed"]), total_energy=float(env.total_energy), alignment=align)
            for k, v in row.items():
                cols[k].append(v)
            print(f"    episode {e} ({solver}, thermal={thermal}, {shape}, {field}): J = {row['J']:+.3g}, T = {row['T']:.3g}: alignment "
                  f"{align:+.6f}, terminated {bool(term)}, truncated {bool(trunc)}, perturbed twin differs by {d:.1e}")
            if term or trunc:
                break
    assert not loose, ("ill-conditioned steps", loose)
    assert margin > 1e-6, margin
    o = {k: np.array(v) for k, v in cols.items()}
    assert (np.abs(o["action"][:, 0]) > o["max_current"]).any() and (o["action"][:, 1] > EPISODE["max_duration"]).any()
    assert (np.abs(o["J"]) == o["max_current"]).any() and (o["T"] == EPISODE["max_duration"]).any()
    f64 = o["act_f64"]
    assert f64.any() and (o["action"][f64].astype(np.float32).astype(np.float64) != o["action"][f64]).any(axis=1).all()
    assert o["truncated"].any() and o["terminated"].any() and not o["terminated"].all()
    for k, v in o.items():
        out["ev_" + k] = v
    for k, v in EPISODE.items():
        if k != "max_current":                   # (per row: the thermal episodes scale it)
            out["ev_" + k] = np.float64(v)
    out["ev_targets"] = np.array(TARGETS5, dtype=float)
    out["ev_seed"], out["ev_env_id"] = np.int64(ENV_SEED), np.int64(ENV_ID)
    print(f"  {len(o['T'])} env steps; smallest |alignment - threshold| = {margin:.3g}")


def main():
    oracle.build()
    out = {}
    worst = stream_self_check()
    print(f"  stream wiring: patched reference against the oracle's thermal solves, worst {worst:.1e}")
    solves(out)
    env_steps(out)
    path = os.path.join(HERE, "G24_wave_config.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"  wrote {path} ({size} bytes)")
    assert size <= 100_000


if __name__ == "__main__":
    main()

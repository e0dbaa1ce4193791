"""NumPy restatement of the fixed-step solve and of one env step under noise_model='brown' (include/spintorque_hip.h, cfg.noise_model = 2):
the thermal field of every stage of sub-step i is (strength / sqrt(dt)) xi_i, xi_i the sub-step's one draw of three standard normals.

A thin wrapper over tests/waveform_ref.py: that file's Ornstein-Uhlenbeck branch with corr_time <= 0 has d = 0 and w = 1, so the field it
forms is `strength` times the sub-step's draw, and the 1/sqrt(dt) goes into `strength`, per problem.  dt is recomputed here in the
solver's own roundings.  The strength s is the C oracle's (oracle.thermal_strength), never the library's; the normals are the caller's:
NumPy's generator for the statistics tests, the device's own stream (stg_thermal_normals) where the arithmetic is compared.

The env step reuses the pieces of tests/wave_step_ref.py (action parse, resistance, energy, observation, reward, flags)."""
import numpy as np

import wave_step_ref as wsr
import waveform_ref

K_B = 1.380649e-23
MU0 = waveform_ref.MU0


def substeps(T, max_step=1e-12):
    """(n [N], dt [N]) of the fixed-step solve over (0, T), in its roundings; a T the input gate rejects counts as 1 s (n is unused)"""
    T = np.array(T, dtype=float).reshape(-1)
    with np.errstate(all="ignore"):
        Tn = np.where(T > 0, T, 1.0)
    dt0 = np.minimum(max_step, Tn / 100)
    n = np.maximum(10, (Tn / dt0).astype(np.int64))
    return n, Tn / n


def strength(oracle, params, device_type="stt_mram", gamma=waveform_ref.GAMMA, temperature=300.0):
    """s: the fixed-step solvers' dt-free Brown field strength of this class"""
    return oracle.thermal_strength(oracle.make_params(params, device_type), gamma, temperature, 0)


def solve(m0, T, params, s, normals, method="rk4", J=None, current=None, field=None, max_step=1e-12, temperature=300.0,
          gamma=waveform_ref.GAMMA, trajectory=False, physical=True):
    """waveform_ref.solve under the Brown field.  s: scalar strength; normals [N, >= n, 3]: draw i of problem j is sub-step i's xi.
    physical=False leaves the 1/sqrt(dt) out: the reference's strength on the same one-draw-per-sub-step schedule."""
    T = np.array(T, dtype=float).reshape(-1)
    _, dt = substeps(T, max_step)
    st = (s / np.sqrt(dt))[:, None] if physical else np.full((len(T), 1), float(s))
    return waveform_ref.solve(m0, T, params, method, current=current, J=J, field=field, max_step=max_step, temperature=temperature,
                              gamma=gamma, trajectory=trajectory, thermal=dict(noise="ou", corr_time=0.0, strength=st, normals=normals))


def step(state, actions, params, s, normals, method="rk4", current=None, field=None, cfg=None, cls=None, dev_types=None):
    """One env step of N envs (autoreset off, every env stepped) under the Brown field: wave_step_ref.step's arithmetic with the solve
    above.  params: one dict or a list with cls [N]; s: the strength of each class (scalar or list); normals [N, >= n, 3] per env.
    Returns wave_step_ref.step's dict."""
    cfg = dict(wsr.DEFAULT_CFG, **(cfg or {}))
    m0 = np.array(state["m"], dtype=float)
    target = np.array(state["target"], dtype=float)
    etot = np.array(state["total_energy"], dtype=float)
    steps = np.array(state["step_count"], dtype=np.int64)
    N = len(m0)
    plist = [params] if isinstance(params, dict) else list(params)
    slist = [s] * len(plist) if np.ndim(s) == 0 else list(s)
    dev_types = ["stt_mram"] * len(plist) if dev_types is None else list(dev_types)
    cls = np.zeros(N, dtype=np.int64) if cls is None else np.asarray(cls, dtype=np.int64)
    normals = np.asarray(normals)
    J, T = wsr.parse_actions(actions, cfg["max_current"], cfg["max_duration"])
    success, m_new, n_sub, r_before = np.zeros(N, dtype=bool), m0.copy(), np.zeros(N, dtype=np.int64), np.zeros(N)
    for c, p in enumerate(plist):
        run = np.nonzero(cls == c)[0]
        if not len(run):
            continue
        r_before[run] = wsr.resistance(m0[run], p, dev_types[c])
        cur = None if current is None else (np.asarray(current[0])[run], np.asarray(current[1])[run])
        fld = None if field is None else (np.asarray(field[0])[run], np.asarray(field[1])[run])
        res = solve(m0[run], T[run], p, slist[c], normals[run], method, J=J[run] if current is None else None, current=cur, field=fld,
                    max_step=cfg["max_step"], temperature=cfg["temperature"], gamma=cfg["gamma"])
        success[run], n_sub[run] = res["success"], res["n_steps"]
        mf = res["m_final"]
        mf = mf / np.sqrt((mf[:, 0] * mf[:, 0] + mf[:, 1] * mf[:, 1]) + mf[:, 2] * mf[:, 2])[:, None]
        m_new[run] = np.where(res["success"][:, None], mf, m0[run])
    area = np.array([p.get("area", 1e-14) for p in plist])[cls]
    if current is None:
        v = J * r_before * area
        energy = np.where(np.abs(J) > 1e-12, (v * v) / r_before * T, 0.0)
    else:
        ra = r_before * area
        energy = (ra * ra) / r_before * wsr.pulse_sq_integral(current[0], current[1], T)
    prev_align = wsr._dot(m0, target)
    etot = etot + energy
    steps = steps + 1
    align = wsr._dot(m_new, target)
    is_success = align >= cfg["success_threshold"]
    reward = 10.0 * np.where(is_success, 10.0, 0.0)
    reward = reward + (-cfg["energy_penalty_weight"]) * (-energy / 1e-12)
    reward = reward + (align - prev_align)
    reward = np.where(np.isnan(reward) | np.isinf(reward), -1.0, reward)
    reward = np.minimum(np.maximum(reward, -1e6), 1e6)
    obs = np.zeros((N, 12), dtype=np.float32)
    for c, p in enumerate(plist):
        sel = np.nonzero(cls == c)[0]
        if len(sel):
            obs[sel] = wsr.observation(m_new[sel], target[sel], wsr.resistance(m_new[sel], p, dev_types[c]), p, cfg, steps[sel], etot[sel],
                                       J[sel], T[sel])
    return dict(m=m_new, total_energy=etot, step_count=steps, obs=obs, reward=reward, terminated=is_success, truncated=steps >= cfg["max_steps"],
                energy=energy, status=np.where(success, wsr.STATUS_OK, wsr.STATUS_NOOP).astype(np.uint8), J=J, T=T, n_sub=n_sub)


# ------------------------------------------------------------------------------------------------
# the physics cases shared by the host and the GPU tests
# ------------------------------------------------------------------------------------------------
def volume_for(delta, ku=1e6, ms=8e5, temperature=300.0):
    """V with barrier Delta = (Ku - mu0 Ms^2 / 2) V / (k_B T): the thin-film demagnetising term -Ms m_z lowers the barrier"""
    return delta * K_B * temperature / (ku - MU0 * ms * ms / 2)


def physics_params(volume, damping):
    from conftest import stt_default_params
    return stt_default_params(volume=float(volume), damping=float(damping), saturation_magnetization=8e5, uniaxial_anisotropy=1e6)


def boltzmann_mz2(delta, n=200001):
    """<m_z^2> of the density exp(Delta x^2) on [-1, 1] (composite Simpson)"""
    x = np.linspace(-1.0, 1.0, n)
    w = np.ones(n)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    e = np.exp(delta * (x * x - 1.0))
    return float((w * x * x * e).sum() / (w * e).sum())


def sphere(rng, n):
    v = rng.normal(0, 1, (n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


# Discretisation bias of THIS restatement (RK4, uniform start, J = 0, alpha = 0.1, 1.5 ns): <m_z^2> minus boltzmann_mz2(Delta), measured
# once on the CPU with NumPy's generator and the sample size next to it; profiles/NOTEBOOK.md has the run.  delta -> (max_step, b, samples)
# (standard errors of the two measurements: 0.0006 and 0.0005)
EQUILIBRIUM_BIAS = {2.0: (1e-12, +0.0023, 262144), 4.0: (1e-12, +0.0018, 262144)}

SWITCH = dict(volume=1.3856e-25, damping=0.02, J=1.2482e-9, T=5e-10)          # thermally assisted switching from +z, P ~ 0.39

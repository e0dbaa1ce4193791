"""Cases, inputs and reference answers shared by tests/test_gpu_brown_config.py (the HIP kernels under noise_model='brown' off their
defaults, `-m gpu`) and tests/test_brown_config_conditioning.py (the references against themselves, CPU): one definition, so that the
conditioning test sees exactly the inputs the GPU test uses.

The Brown field's one line of its own is w = 1 / sqrt(dt), with dt per lane: min(max_step, T / 100), then T / n.  At the defaults only
one branch of that minimum is ever taken, with dt within 1 % of 1 ps.  Here max_step is 2.5e-12, 3e-13 and 1e-10 (wave_config_cases'
reduced cross with gamma), durations are wave_config_cases.durations, so that

  max_step = 3e-13            T / 100 = 2e-13 ... 6e-13: lanes with n = 100 and dt = T / 100 next to lanes with n = floor(T / max_step)
                              up to 200 and dt = T / n in [max_step, 1.01 max_step) -- both branches in one launch;
  max_step = 2.5e-12, 1e-10   T / 100 = 1.05e-12 ... 1.6e-12 decides (n = 100, now and then 99 by the quotient's rounding): dt is up to
                              60 % away from the 1 ps a solver stuck at the default max_step would use.

Every case: temperature 77 or 450 K, gamma 1.9e5 or 2.5e5, wave_config_cases.EPISODE's fields, the five-target list, the class table
STT / SOT / VCMA under the reference torque model (volumes 1e-23, 1e-23, 0.8e-23 with currents scaled by the volume ratio as in
wave_config_cases: the field turns m by 6e-3 ... 0.1 rad over a pulse, far above the tolerance, while the chains stay as well conditioned
as without it -- at 1e-26 the field moves m by order one and an ulp of the start rows grows to 1e-11), float32 and float64 actions alternating, the stream key (SEED, ENV_ID0 = 37), N = 130 and one case
with n = 1.

Two references, both fed the caller's normals (the device's own on the GPU, the oracle's stream on the CPU):
  'restatement'   tests/brown_ref.py (NumPy; rectangular pulses and waveform tables);
  'oracle'        the C oracle's fed-normals env step (oracle/stg_oracle.c: stgo_env_step_fed; rectangular pulses; also the device
                  torque model).
run_chain() chains steps on a reference's own state.  With autoreset an env whose episode ends takes the redrawn (m, target) its
caller hands in -- on the GPU the device's own redraw, whose fp32 normals differ from libm's by 1e-7 (tests/test_gpu_env_config.py) --
with energy and step count back at zero."""
import itertools

import numpy as np

import brown_ref as br
import knots_ref as kr
import wave_config_cases as wcc
import wave_step_ref as wsr
from conftest import sot_default_params, stt_default_params, vcma_default_params
from env_config_cases import TARGETS5, TOL_RK4, unit_targets

N = wcc.N
SEED, ENV_ID0, ENV_STEP = wcc.SEED, wcc.ENV_ID0, wcc.ENV_STEP
SETTINGS = ((2.5e-12, 1.9e5), (3e-13, 2.5e5), (1e-10, 1.9e5))
TEMPERATURES = (77.0, 450.0)
VOL = 1e-23
JS = VOL / wcc.VOL                       # currents scale with the volume (the spin torque goes with J / V)
DEV_TYPES = wcc.DEV_TYPES
STEPS = 2                                # chained steps of every entry point
K_MANY = 3                               # the fused launch with autoreset
TOL = TOL_RK4                            # no thermal factor: the references take the device's own normals
P_KNOTS, KNOT_LIMIT = wcc.P_KNOTS, wcc.KNOT_LIMIT
# applied-field knots at a tenth of wave_config_cases' +-1e5 A/m: the bound on the conditioning is 1e-12 here (no thermal factor of 50),
# and at the full amplitude single lanes of the long pulses (1.05e-10 ... 1.6e-10 s, two chained) moved by 1e-12 ... 2e-11 per ulp of
# the start rows -- with the field knots at zero the same cases move by 1e-13.  +-1e4 A/m still turns m by ~ gamma H T = 0.2 rad
FIELD_SCALE = 0.1
VCMA_AREA_DEVICE = 1e-2                  # device torque model: V = J R A reaches ~ 5e-9 V at these currents, K_eff 0.3 ... 1 K_u


def cases():
    out = []
    for method in ("rk4", "euler"):
        for j, ((ms, gamma), temp) in enumerate(itertools.product(SETTINGS, TEMPERATURES)):
            out.append(dict(method=method, max_step=ms, gamma=gamma, temperature=temp, n=N, seed=8000 + 10 * j + (500 if method == "euler" else 0),
                            knots=wcc.KNOTS[j % 3], f64=bool((j + (method == "euler")) % 2)))
    out.append(dict(method="rk4", max_step=3e-13, gamma=2.5e5, temperature=450.0, n=1, seed=8902, knots=wcc.KNOTS[0], f64=False))
    for c in out:
        c["name"] = f"{c['method']}-ms{c['max_step']:g}-g{c['gamma']:g}-{c['temperature']:g}K-n{c['n']}" + ("-f64" if c["f64"] else "")
    return out


def device_cases():
    """the device torque model: both methods at the two settings whose gamma differ"""
    out = [dict(method=m, max_step=ms, gamma=g, temperature=t, n=N, seed=9100 + 10 * j, knots=wcc.KNOTS[0], f64=bool(j % 2), device=True)
           for j, (m, (ms, g), t) in enumerate((("rk4", SETTINGS[0], 450.0), ("euler", SETTINGS[1], 77.0), ("rk4", SETTINGS[1], 77.0),
                                                ("euler", SETTINGS[2], 450.0)))]
    for c in out:
        c["name"] = f"device-{c['method']}-ms{c['max_step']:g}-g{c['gamma']:g}-{c['temperature']:g}K" + ("-f64" if c["f64"] else "")
    return out


def case(cs, name):
    return wcc.case(cs, name)


def class_table(device=False):
    v = [stt_default_params(volume=VOL), sot_default_params(polarization=0.7, volume=VOL), vcma_default_params(polarization=0.6, volume=0.8 * VOL)]
    if device:
        v[2]["area"] = VCMA_AREA_DEVICE
    return v


def config(c):
    return dict(wcc.EPISODE, temperature=c["temperature"], max_step=c["max_step"], gamma=c["gamma"], max_current=wcc.EPISODE["max_current"] * JS)


PROBLEMS = {}


def problem(c):
    """start state, K_MANY action sets (a quarter of the currents beyond max_current), per-env current and field tables for each step
    (stg_step_wave), a pulse shape and field knots (stg_step_shaped), knot times and amplitudes (stg_step_knots)"""
    if c["name"] in PROBLEMS:
        return PROBLEMS[c["name"]]
    from spin_torque_gym_amd.physics import PiecewiseLinear
    rng = np.random.default_rng(c["seed"])
    n, cfg = c["n"], config(c)
    m0 = wcc.unit_rows(rng, n)
    tgt = unit_targets(TARGETS5)[np.arange(n) % 5]
    acts, cur, fld = [], [], []
    kj, kh = c["knots"]
    for _ in range(K_MANY):
        J = rng.uniform(-2e6, 2e6, n) * JS
        if c.get("device"):
            J = np.where(np.abs(J) < 1e5 * JS, 1e5 * JS, J)               # J != 0 in every lane: each class's own torque is at work
        a = np.stack([J, wcc.durations(rng, n, c["max_step"])], axis=1)
        if c["f64"]:
            assert np.all(a.astype(np.float32).astype(np.float64) != a)
        else:
            a = a.astype(np.float32)
        _, T = wsr.parse_actions(a, cfg["max_current"], cfg["max_duration"])
        tj, jk = wcc.tables(rng, n, kj, T, 1)
        th, hk = wcc.tables(rng, n, kh, T, 3)
        acts.append(a); cur.append((tj, 0.5 * jk * JS)); fld.append((th, FIELD_SCALE * hk))      # (currents at half amplitude: wave_config_cases.step_problem)
    acts = np.stack(acts)
    state = dict(m=m0, target=tgt, total_energy=rng.uniform(0, 1e-21, n) * JS * JS, step_count=rng.integers(0, 2, n))
    shape = PiecewiseLinear([0.0, 0.15, 0.7, 0.9, 1.0], [0.0, 0.25, 0.25, -0.15, 0.0])                  # (wave_config_cases.shaped_problem's)
    span = float(acts[:, :, 1].max())
    fk = (np.array([-0.1 * span, 0.3 * span, 1.2 * span]), FIELD_SCALE * rng.uniform(-1e5, 1e5, (3, 3)))
    tau = np.concatenate([[0.0], np.sort(rng.uniform(0.05, 0.95, P_KNOTS - 2)), [1.0]])
    amp = rng.uniform(-1.6, 1.6, (K_MANY, n, P_KNOTS)) * KNOT_LIMIT
    kacts = np.concatenate([acts.astype(np.float64), amp], axis=2)
    kacts = kacts if c["f64"] else kacts.astype(np.float32)
    p = dict(plist=class_table(c.get("device", False)), cls=(np.arange(n) % 3).astype(np.uint8), cfg=cfg, state=state, acts=acts, cur=cur, fld=fld,
             shape=shape, fk=fk, tau=tau, limit=KNOT_LIMIT, kacts=kacts)
    PROBLEMS[c["name"]] = p
    return p


def strengths(oracle, c, p):
    """the dt-free field strength of every class at the case's gamma and temperature (the oracle's, never the library's)"""
    return [br.strength(oracle, d, t, gamma=c["gamma"], temperature=c["temperature"]) for d, t in zip(p["plist"], DEV_TYPES)]


def oracle_normals(oracle, n):
    """normals_of for run_chain on the CPU: the oracle's own stream of envs ENV_ID0 .. ENV_ID0 + n - 1 at stream position rng_step"""
    import waveform_ref
    return lambda rng_step, count: np.stack([waveform_ref.normals(oracle, SEED, ENV_ID0 + i, rng_step, count) for i in range(n)])


def oracle_resets(p):
    """reset_of for run_chain on the CPU: the kernels' device-side reset draw through its oracle restatement"""
    from helpers import device_reset_draw
    targets = unit_targets(p["cfg"]["target_states"])

    def reset_of(k, ids, rng_step):
        rows = [device_reset_draw(SEED, ENV_ID0 + int(i), int(rng_step), targets) for i in ids]
        return np.array([r[0] for r in rows]).reshape(-1, 3), np.array([r[1] for r in rows]).reshape(-1, 3)
    return reset_of


def max_substeps(p, a):
    _, T = wsr.parse_actions(np.asarray(a)[:, :2], p["cfg"]["max_current"], p["cfg"]["max_duration"])
    return int(br.substeps(T, p["cfg"]["max_step"])[0].max())


# ---------------------------------------------------------------------------------------------------------------------
# the drives of the waveform entry points, as tables (current, field) of one step's parsed actions
# ---------------------------------------------------------------------------------------------------------------------
def wave_tables(p, k, sel=slice(None)):
    """stg_step_wave: the per-env tables of step k"""
    return (p["cur"][k][0][sel], p["cur"][k][1][sel]), (p["fld"][k][0][sel], p["fld"][k][1][sel])


def field_table(p, n):
    return np.tile(p["fk"][0], (n, 1)), np.tile(p["fk"][1], (n, 1, 1))


def shaped_tables(p, k, sel=slice(None)):
    """stg_step_shaped: the knots (tau_j T, J s_j) the shape gives step k's parsed actions, and the env-level field knots"""
    a = p["acts"][k][sel]
    J, T = wsr.parse_actions(a, p["cfg"]["max_current"], p["cfg"]["max_duration"])
    return (p["shape"].times[None, :] * T[:, None], J[:, None] * p["shape"].values[None, :]), field_table(p, len(a))


def knots_tables(p, k, sel=slice(None)):
    """stg_step_knots: the knots (tau_j T, J s_j) of step k's parsed knot actions, and the env-level field knots"""
    a = p["kacts"][k][sel]
    return kr.knot_tables_np(p["tau"], *kr.parse_np(a, p["cfg"]["max_current"], p["cfg"]["max_duration"], p["limit"])), field_table(p, len(a))


DRIVES = {"rect": None, "wave": wave_tables, "shaped": shaped_tables, "knots": knots_tables}


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
def _restatement_step(c, p, oracle, state, a, z, cls, tables, field_on=True):
    cur, fld = tables if tables is not None else (None, None)
    r = br.step(state, a, p["plist"], [x if field_on else 0.0 for x in strengths(oracle, c, p)], z, c["method"], current=cur, field=fld, cfg=p["cfg"], cls=cls, dev_types=DEV_TYPES)
    r["alignment"] = wsr._dot(r["m"], np.asarray(state["target"], dtype=float))
    return r


def oracle_config(oracle, c, p, torque_model=0):
    cfg = p["cfg"]
    return oracle.make_config(solver=c["method"], thermal=True, temperature=cfg["temperature"], gamma=cfg["gamma"], max_step=cfg["max_step"],
                              max_steps=cfg["max_steps"], max_current=cfg["max_current"], max_duration=cfg["max_duration"],
                              success_threshold=cfg["success_threshold"], energy_penalty_weight=cfg["energy_penalty_weight"], seed=SEED,
                              torque_model=torque_model, noise_model=2)


def _oracle_step(c, p, oracle, state, a, z, cls, torque_model):
    """the C oracle's fed-normals env step per env (its own action parse, resistance, energy, observation, reward and flags)"""
    ocfg = oracle_config(oracle, c, p, torque_model)
    po = [oracle.make_params(d, t) for d, t in zip(p["plist"], DEV_TYPES)]
    n = len(a)
    step = oracle.env_step_f64 if a.dtype == np.float64 else oracle.env_step
    out = dict(m=np.zeros((n, 3)), total_energy=np.zeros(n), step_count=np.zeros(n, dtype=np.int64), obs=np.zeros((n, 12), dtype=np.float32),
               reward=np.zeros(n), terminated=np.zeros(n, dtype=bool), truncated=np.zeros(n, dtype=bool), energy=np.zeros(n),
               status=np.zeros(n, dtype=np.uint8), n_sub=np.zeros(n, dtype=np.int64))
    for i in range(n):
        st = oracle.EnvState()
        st.m[:] = [float(x) for x in state["m"][i]]
        st.target[:] = [float(x) for x in state["target"][i]]
        st.total_energy, st.step_count = float(state["total_energy"][i]), int(state["step_count"][i])
        o = step(st, a[i], po[int(cls[i])], ocfg, normals=z[i])
        out["m"][i], out["total_energy"][i], out["step_count"][i] = list(st.m), st.total_energy, st.step_count
        out["obs"][i], out["reward"][i], out["energy"][i] = list(o.obs), o.reward, o.energy
        out["terminated"][i], out["truncated"][i], out["status"][i], out["n_sub"][i] = bool(o.terminated), bool(o.truncated), o.status, o.n_sub
    out["alignment"] = wsr._dot(out["m"], np.asarray(state["target"], dtype=float))
    return out


def reset_observation(p, m, target, cls):
    """the first observation of a new episode (energy, step count and last action at zero), each env with its class's resistance form"""
    obs = np.zeros((len(m), 12), dtype=np.float32)
    zero = np.zeros(len(m))
    for ci, (d, t) in enumerate(zip(p["plist"], DEV_TYPES)):
        s = np.nonzero(np.asarray(cls) == ci)[0]
        if len(s):
            obs[s] = wsr.observation(m[s], target[s], wsr.resistance(m[s], d, t), d, p["cfg"], zero[s].astype(np.int64), zero[s], zero[s], zero[s])
    return obs


def run_chain(c, p, oracle, normals_of, engine="restatement", drive="rect", K=STEPS, sel=None, rng_step0=0, autoreset=False, reset_of=None,
              ulp=False, ulp_normals=False, torque_model=0, field_on=True):
    """K chained steps of the envs `sel` (None: all) on the reference `engine`, each from the reference's own state.
    normals_of(rng_step, count) -> [n_all, count, 3]: the draws of every env at that stream position; every stepped env is at
    rng_step0 + k in step k.  drive: 'rect' (the actions' rectangular pulses) or one of the waveform drives ('restatement' only).
    autoreset: an env whose step terminates or truncates takes reset_of(k, ids, rng_step after the step) -> (m, target) rows as its
    next state (ids: indices into `sel`); its observation row becomes the new episode's first (the terminal one goes to 'final_obs').
    ulp / ulp_normals: the largest component of every start row / every normal moved by one ulp (the conditioning test);
    field_on=False: the restatement with strength 0 (what the field is measured against).
    Returns the per-step dicts of brown_ref.step plus 'alignment', 'done' and, with autoreset, 'final_obs'."""
    assert engine in ("restatement", "oracle") and (engine == "restatement" or drive == "rect")
    sel = np.arange(c["n"]) if sel is None else np.asarray(sel)
    st0 = p["state"]
    state = dict(m=st0["m"][sel], target=st0["target"][sel], total_energy=st0["total_energy"][sel], step_count=st0["step_count"][sel])
    if ulp:
        state["m"] = wcc.ulp_moved(state["m"])
    cls = p["cls"][sel]
    acts = p["kacts"] if drive == "knots" else p["acts"]
    refs = []
    for k in range(K):
        a = acts[k][sel]
        z = normals_of(rng_step0 + k, max_substeps(p, a))[sel]
        if ulp_normals:
            z = np.nextafter(z, np.inf)
        if engine == "oracle":
            r = _oracle_step(c, p, oracle, state, a, z, cls, torque_model)
        else:
            assert torque_model == 0
            tables = DRIVES[drive](p, k, sel) if drive != "rect" else None
            r = _restatement_step(c, p, oracle, state, kr.wave_rows(a) if drive == "knots" else a, z, cls, tables, field_on)
        r["done"] = r["terminated"] | r["truncated"]
        state = dict(m=r["m"], target=state["target"], total_energy=r["total_energy"], step_count=r["step_count"])
        if autoreset:
            ids = np.nonzero(r["done"])[0]
            r["final_obs"] = r["obs"].copy()
            if len(ids):
                m_new, t_new = reset_of(k, ids, rng_step0 + k + 1)
                state = {key: np.array(v, copy=True) for key, v in state.items()}
                state["m"][ids], state["target"][ids], state["total_energy"][ids], state["step_count"][ids] = m_new, t_new, 0.0, 0
                r["obs"] = r["obs"].copy()
                r["obs"][ids] = reset_observation(p, state["m"][ids], state["target"][ids], cls[ids])
            r["state_after"] = state
        refs.append(r)
    return refs


def rect_energy(p, a, m_before, cls):
    """the energy a rectangular step charges envs in the states m_before: (J R A)^2 / R T with each class's resistance form
    (spin_torque_env.py:474-480), zero where |J| <= 1e-12"""
    J, T = wsr.parse_actions(a, p["cfg"]["max_current"], p["cfg"]["max_duration"])
    e = np.zeros(len(T))
    for ci, (d, t) in enumerate(zip(p["plist"], DEV_TYPES)):
        s = np.asarray(cls) == ci
        r = wsr.resistance(m_before[s], d, t)
        v = J[s] * r * d["area"]
        e[s] = np.where(np.abs(J[s]) > 1e-12, (v * v) / r * T[s], 0.0)
    return e


def compare_step(got, ref, tol, tag, first=True):
    """one step's outputs (and state, where `got` holds it) against a reference step, the way tests/test_gpu_wave_config.py:
    _compare_step does it: m within tol; status bytes, flags and step counts exactly; observations one float32 ulp plus 2 tol; the fp64
    reward 1e-9 + 2 tol.  The energy goes with the resistance of the state BEFORE the step: 1e-13 relative in a first step (the given
    state), 10 tol relative in a later one, where the start rows are the kernels' own, within tol of the reference's
    (tests/env_config_cases.py: compare).  got: numpy arrays, env-major.  Returns the worst |m - m_ref| (0 without m)."""
    err = 0.0
    if got.get("m") is not None:
        err = float(np.abs(got["m"] - ref["m"]).max())
        assert err <= tol, (tag, "m", err)
    for key in ("status", "terminated", "truncated"):
        assert np.array_equal(np.asarray(got[key]).astype(ref[key].dtype), ref[key]), (tag, key, np.flatnonzero(np.asarray(got[key]).astype(ref[key].dtype) != ref[key])[:8])
    e_tol = 1e-13 if first else 10 * tol
    assert np.all(np.abs(got["energy"] - ref["energy"]) <= e_tol * np.abs(ref["energy"])), (tag, "energy")
    ob, ob_ref = got["obs"], ref["obs"]
    bad = np.abs(ob - ob_ref) > wsr.F32_ULP * np.abs(ob_ref) + 2 * tol
    assert not bad.any(), (tag, "obs", np.argwhere(bad)[:4])
    assert np.all(np.abs(got["reward_f64"] - ref["reward"]) <= 1e-9 + 2 * tol), (tag, "reward")
    if got.get("step_count") is not None:
        assert np.array_equal(got["step_count"], ref["step_count"]), (tag, "step_count")
    if got.get("total_energy") is not None:
        assert np.all(np.abs(got["total_energy"] - ref["total_energy"]) <= e_tol * np.abs(ref["total_energy"])), (tag, "total_energy")
    return err


# ---------------------------------------------------------------------------------------------------------------------
# the launch forms at full size (tests/test_gpu_noise_launch_forms.py): one RK4 step, T <= 0.3 ns
# ---------------------------------------------------------------------------------------------------------------------
LF_MAX_CURRENT = 2e6 * JS
LF_TMIN, LF_TMAX = 1e-10, 3e-10


def launch_slices(n):
    """the three 64-env slices whose values are checked: the first wavefront, one in the middle, the end (with the ragged tail)"""
    return (0, (n // 2) // 64 * 64, n - 64)


def launch_inputs(n, seed, steps=1):
    """m0 uniform on the sphere, targets +-z, float32 actions with J ~ U[-2e6, 2e6] JS and T ~ U[0.1, 0.3] ns.  The first slice of
    launch_slices takes the longest duration and the middle one the shortest, so that the two sit at opposite ends of the
    duration-sorted schedule (the hybrid launch gives its producer / consumer pairs to the longest blocks and runs the shortest with
    inline normals); the last slice keeps its random durations."""
    rng = np.random.default_rng(seed)
    m0 = wcc.unit_rows(rng, n)
    tgt = np.where(rng.integers(0, 2, (n, 1)) == 0, 1.0, -1.0) * np.array([[0.0, 0.0, 1.0]])
    acts = np.empty((steps, n, 2), dtype=np.float32)
    acts[..., 0] = rng.uniform(-2e6, 2e6, (steps, n)) * JS
    acts[..., 1] = rng.uniform(LF_TMIN, LF_TMAX, (steps, n))
    first, mid, _ = launch_slices(n)
    acts[:, first:first + 64, 1] = LF_TMAX
    acts[:, mid:mid + 64, 1] = LF_TMIN
    return m0, tgt, acts


def launch_slice_ref(oracle, m0, tgt, acts0, s0, z, ulp=False, ulp_normals=False):
    """brown_ref.step of the 64 envs from s0 on (one class, the default configuration but for max_current), fed normals z [64, n, 3]"""
    sl = slice(s0, s0 + 64)
    p = stt_default_params(volume=VOL)
    state = dict(m=wcc.ulp_moved(m0[sl]) if ulp else m0[sl], target=tgt[sl], total_energy=np.zeros(64), step_count=np.zeros(64, dtype=np.int64))
    return br.step(state, acts0[sl], p, br.strength(oracle, p), np.nextafter(z, np.inf) if ulp_normals else z, "rk4", cfg=dict(max_current=LF_MAX_CURRENT))

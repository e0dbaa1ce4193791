"""Cases, inputs and restatement answers shared by test_gpu_wave_config.py and test_gpu_knots_config.py (the waveform kernels against
tests/waveform_ref.py / tests/wave_step_ref.py, `-m gpu`) and test_wave_config_conditioning.py (the restatement against itself, CPU): one definition, so that the
conditioning test sees exactly the inputs the GPU tests use.

Everything runs away from the defaults: max_step in FIXED_MAX_STEPS, gamma 1.9e5 / 2.5e5, temperatures 77 / 450 K, the thermal field off,
white and Ornstein-Uhlenbeck (correlation time 7e-13), and -- at the env level -- every episode field of EPISODE, the five-target list,
and a three-class table STT / SOT / VCMA under the reference torque model.  The env-level sweep is a reduced cross of max_step
and gamma (step_cases says which pairings and why).

Durations are chosen so that max_step decides the sub-step count: with max_step = 3e-13, T / 100 is above it (n = T / 3e-13 up to
200); with 2.5e-12 and 1e-10, T / 100 is below them but above the default 1e-12 (n = 100, where a solver stuck at the default would take
up to 160).  The thermal cases use volume 1e-26 with currents scaled by the volume ratio (tests/golden/make_golden_wave_config.py says
why): there the thermal field moves m by 1e-7 ... 1e-5, far above the tolerance, so a field that is dropped, misplaced or decayed
with the wrong dt shows.

The knots cases (knots_problem, knots_ref; tests/test_gpu_knots_config.py) are the shaped cases with the fixed shape replaced by actions
[J, T, s_0 ... s_4] that carry the knot amplitudes: the configuration, the class table, the start state, the field knots and the
(J, T) rows are shaped_problem's, to which come five knot times, the amplitude limit KNOT_LIMIT = 0.25 and amplitudes drawn in
+-1.6 KNOT_LIMIT, so that the clamp works on three amplitudes in eight.  The restatement's answer is wave_step_ref.step under the tables
tests/knots_ref.py builds from the parsed actions (with_knots, run_knots_ref); tests/test_wave_config_host.py pins these two functions
against shaped_ref, tests/test_wave_config_conditioning.py checks the conditioning of the cases and that they are not vacuous."""
import itertools

import numpy as np

from conftest import sot_default_params, stt_default_params, vcma_default_params
from env_config_cases import FIXED_MAX_STEPS, TARGETS5, tol_for, unit_targets  # noqa: F401  (tol_for: for the tests that import this module)
import wave_step_ref
import waveform_ref

N = 130                          # two full wavefronts and a two-lane tail
VOL, VOL_THERMAL = 8.75e-11, 1e-26
J_THERMAL = VOL_THERMAL / VOL
GAMMAS = (1.9e5, 2.5e5)
NOISES = (None, "white", "ou")
CORR_TIME = 7e-13
SEED, ENV_ID0, ENV_STEP = 4242, 37, 5          # the stream key of the solve-level cases; the step cases start at rng_step 0
EPISODE = dict(max_current=1.5e6, max_duration=2e-9, success_threshold=0.6, energy_penalty_weight=0.25, max_steps=3, temperature=250.0,
               target_states=TARGETS5)
DEV_TYPES = ("stt_mram", "sot_mram", "vcma_mram")
KNOTS = ((4, 3), (2, 17), (9, 2))
STEPS = 2


def _name(c):
    return f"{c['method']}-ms{c['max_step']:g}-g{c['gamma']:g}-{c['noise'] or 'T0'}-{c['temperature']:g}K-n{c['n']}" + ("-f64" if c.get("f64") else "")


def solve_cases():
    out = []
    for method in ("rk4", "euler"):
        for j, (ms, gamma, noise) in enumerate(itertools.product(FIXED_MAX_STEPS, GAMMAS, NOISES)):
            out.append(dict(method=method, max_step=ms, gamma=gamma, noise=noise, temperature=(77.0, 450.0)[j % 2], n=N, seed=3000 + j,
                            knots=KNOTS[j % 3]))
    out.append(dict(method="rk4", max_step=3e-13, gamma=1.9e5, noise="white", temperature=450.0, n=1, seed=3100, knots=KNOTS[0]))
    for c in out:
        c["name"] = _name(c)
    return out


def step_cases():
    out = []
    # A REDUCED cross: three of the six (max_step, gamma) pairings of the solve-level sweep, each with every noise model, so that every
    # max_step and every gamma meets every noise model at N = 130.  The other three pairings -- (2.5e-12, 2.5e5), (3e-13, 1.9e5),
    # (1e-10, 2.5e5) -- run at the solve level only: with two chained steps their thermal-off cases moved by 1.2e-12 ... 5e-12 per ulp
    # of the start rows at every input tried, above the tolerance / 100 that tests/test_wave_config_conditioning.py asks for.
    settings = ((2.5e-12, 1.9e5), (3e-13, 2.5e5), (1e-10, 1.9e5))
    for method in ("rk4", "euler"):
        for j, ((ms, gamma), noise) in enumerate(itertools.product(settings, NOISES)):
            out.append(dict(method=method, max_step=ms, gamma=gamma, noise=noise, temperature=(77.0, 450.0)[j % 2], n=N, seed0=5000 + 40 * j,
                            knots=KNOTS[j % 3], f64=bool((j + (method == "euler")) % 2)))
    out.append(dict(method="rk4", max_step=2.5e-12, gamma=2.5e5, noise=None, temperature=77.0, n=1, seed0=5900, knots=KNOTS[0], f64=False))
    for c in out:
        c["name"] = _name(c)
    return out


def case(cases, name):
    for c in cases:
        if c["name"] == name:
            return c
    raise KeyError(name)


def tables(rng, n, K, T, width):
    """per-problem knots as tests/test_gpu_step_wave.py draws them: some tables stop before T, some go beyond it, some start after
    t = 0, some before it.  A copy of that file's _tables (a GPU test module is no place to import from on the CPU), which has to stay in
    step with it: tests/test_wave_config_host.py compares the two draw for draw."""
    span = np.where(rng.random(n) < 0.5, 0.6, 1.5) * T
    start = np.select([rng.random(n) < 0.3, rng.random(n) < 0.3], [0.1 * T, -0.2 * T], 0.0)
    tk = start[:, None] + np.sort(rng.uniform(0, 1, (n, K)), axis=1) * (span - start)[:, None]
    assert (np.diff(tk, axis=1) > 0).all()
    if width == 1:
        vk = rng.uniform(-2e6, 2e6, (n, K))
        vk[rng.random((n, K)) < 0.2] = 0.0                   # exact zeros: ramps cross the |J| = 1e-12 gate
    else:
        vk = rng.uniform(-1e5, 1e5, (n, K, 3))
    return tk, vk


def durations(rng, n, max_step):
    return rng.uniform(2e-11, 6e-11, n) if max_step < 1e-12 else rng.uniform(1.05e-10, 1.6e-10, n)


def unit_rows(rng, n):
    v = rng.normal(0, 1, (n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def ulp_moved(m0):
    """the largest component of every row moved by one ulp"""
    m = m0.copy()
    rows = np.arange(len(m))
    big = np.abs(m).argmax(axis=1)
    m[rows, big] = np.nextafter(m[rows, big], np.inf)
    return m


# ---------------------------------------------------------------------------------------------------------------------
# solve level
# ---------------------------------------------------------------------------------------------------------------------
def solve_problem(c):
    rng = np.random.default_rng(c["seed"])
    n, thermal = c["n"], c["noise"] is not None
    m0 = unit_rows(rng, n)
    T = durations(rng, n, c["max_step"])
    kj, kh = c["knots"]
    cur, fld = tables(rng, n, kj, T, 1), tables(rng, n, kh, T, 3)
    if thermal:
        cur = (cur[0], cur[1] * J_THERMAL)
    return dict(params=stt_default_params(volume=VOL_THERMAL if thermal else VOL), m0=m0, T=T, cur=cur, fld=fld)


SOLVE_REF = {}


def solve_ref(c, oracle, ulp=False):
    """the restatement's answer to a solve case, computed once and shared"""
    key = (c["name"], ulp)
    if key not in SOLVE_REF:
        p = solve_problem(c)
        m0 = ulp_moved(p["m0"]) if ulp else p["m0"]
        thermal = None
        if c["noise"]:
            thermal = waveform_ref.thermal_field(oracle, p["params"], "stt_mram", c["gamma"], c["temperature"], SEED, ENV_ID0 + np.arange(c["n"]),
                                                 ENV_STEP, c["noise"], CORR_TIME)
        SOLVE_REF[key] = (p, waveform_ref.solve(m0, p["T"], p["params"], c["method"], current=p["cur"], field=p["fld"], max_step=c["max_step"],
                                                temperature=c["temperature"], gamma=c["gamma"], thermal=thermal))
    return SOLVE_REF[key]


# ---------------------------------------------------------------------------------------------------------------------
# env level
# ---------------------------------------------------------------------------------------------------------------------
def class_table(thermal):
    """STT / SOT / VCMA under the reference torque model (which takes the polarization of every class)"""
    v = VOL_THERMAL if thermal else VOL
    return [stt_default_params(volume=v), sot_default_params(polarization=0.7, volume=v), vcma_default_params(polarization=0.6, volume=0.8 * v)]


def step_cfg(c):
    thermal = c["noise"] is not None
    cfg = dict(EPISODE, temperature=c["temperature"], max_step=c["max_step"], gamma=c["gamma"])
    if thermal:
        cfg["max_current"] = EPISODE["max_current"] * J_THERMAL
    return cfg


def step_problem(c, seed):
    """start state, STEPS action sets (a quarter of the currents beyond max_current) and per-env tables for each step"""
    rng = np.random.default_rng(seed)
    n, thermal = c["n"], c["noise"] is not None
    js = J_THERMAL if thermal else 1.0
    cfg = step_cfg(c)
    m0 = unit_rows(rng, n)
    tgt = unit_targets(TARGETS5)[np.arange(n) % 5]
    acts, cur, fld = [], [], []
    kj, kh = c["knots"]
    for _ in range(STEPS):
        a = np.stack([rng.uniform(-2e6, 2e6, n) * js, durations(rng, n, c["max_step"])], axis=1)
        if c["f64"]:
            assert np.all(a.astype(np.float32).astype(np.float64) != a)
        else:
            a = a.astype(np.float32)
        _, T = wave_step_ref.parse_actions(a, cfg["max_current"], cfg["max_duration"])
        tj, jk = tables(rng, n, kj, T, 1)
        # (half the amplitude of the solve-level tables: the spin torque amplifies a perturbation of the state exponentially in J t, and
        # two steps chain here; at the full amplitude single lanes move by more than tolerance / 100 per ulp)
        acts.append(a); cur.append((tj, 0.5 * jk * js)); fld.append(tables(rng, n, kh, T, 3))
    state = dict(m=m0, target=tgt, total_energy=rng.uniform(0, 1e-21, n) * js * js, step_count=rng.integers(0, 2, n))
    return dict(plist=class_table(thermal), cls=(np.arange(n) % 3).astype(np.uint8), cfg=cfg, state=state, acts=acts, cur=cur, fld=fld)


def run_steps_ref(c, p, oracle, ulp=False):
    state = dict(p["state"])
    if ulp:
        state["m"] = ulp_moved(state["m"])
    refs = []
    for k in range(STEPS):
        thermal = None
        if c["noise"]:
            thermal = dict(oracle=oracle, seed=SEED, env_id0=ENV_ID0, rng_step=np.full(c["n"], k), noise=c["noise"], corr_time=CORR_TIME)
        r = wave_step_ref.step(state, p["acts"][k], p["plist"], c["method"], current=p["cur"][k], field=p["fld"][k], cfg=p["cfg"], cls=p["cls"],
                               dev_types=DEV_TYPES, thermal=thermal)
        refs.append(r)
        state = dict(m=r["m"], target=state["target"], total_energy=r["total_energy"], step_count=r["step_count"])
    return refs


def pulse_energy(p, k, m_before):
    """the energy step k of problem p charges envs in the states m_before [N,3]: (R A)^2 / R times the closed-form integral of j^2, with
    the resistance form of each env's class (what wave_step_ref.step computes, from given start rows)"""
    _, T = wave_step_ref.parse_actions(p["acts"][k], p["cfg"]["max_current"], p["cfg"]["max_duration"])
    I = wave_step_ref.pulse_sq_integral(p["cur"][k][0], p["cur"][k][1], T)
    e = np.zeros(len(T))
    for c, (d, t) in enumerate(zip(p["plist"], DEV_TYPES)):
        sel = p["cls"] == c
        r = wave_step_ref.resistance(m_before[sel], d, t)
        ra = r * d["area"]
        e[sel] = (ra * ra) / r * I[sel]
    return e


STEP_REF = {}


def step_ref(c, oracle, ulp=False):
    """inputs and the restatement's answer to both steps, computed once and shared; the inputs are drawn again (at most 20 seeds) until
    no alignment of the restatement is within 1e-6 of the threshold, so that no flag rests on rounding.  Every env stays in."""
    key = (c["name"], ulp)
    if key in STEP_REF:
        return STEP_REF[key]
    if ulp:
        p, _ = step_ref(c, oracle)
        STEP_REF[key] = (p, run_steps_ref(c, p, oracle, ulp=True))
        return STEP_REF[key]
    for seed in range(c["seed0"], c["seed0"] + 20):
        p = step_problem(c, seed)
        refs = run_steps_ref(c, p, oracle)
        if all((np.abs(r["alignment"] - p["cfg"]["success_threshold"]) > 1e-6).all() for r in refs):
            break
    else:
        raise AssertionError(f"{c['name']}: no seed of 20 keeps every alignment 1e-6 away from the threshold")
    STEP_REF[key] = (p, refs)
    return STEP_REF[key]


# ---------------------------------------------------------------------------------------------------------------------
# stg_step_shaped: one launch of K_SHAPED steps under an env-level pulse shape
# ---------------------------------------------------------------------------------------------------------------------
K_SHAPED = 3
VOL_RK45, VOL_THERMAL45 = 9.7e-6, 4e-30
SHAPED_DIRECT = [("rk4", None), ("euler", "white"), ("rk4", "ou")]          # the launches compared with the restatement directly


def shaped_problem(solver, noise, f64, seed):
    """the non-default episode configuration, three device classes, K_SHAPED action sets, a pulse shape and field knots"""
    from env_config_cases import RK45_SETTINGS
    from spin_torque_gym_amd.physics import PiecewiseLinear
    rng = np.random.default_rng(seed)
    n, thermal = N, noise is not None
    if solver == "rk45":
        v = VOL_THERMAL45 if thermal else VOL_RK45
        js = v / VOL_RK45
        plist = [dict(p, volume=v * f) for p, f in zip(class_table(False), (1.0, 1.0, 0.8))]
        over = dict(RK45_SETTINGS[1])              # (gamma 1.9e5, rtol 1e-8, max_step 2e-13)
        T = rng.uniform(1e-11, 3e-11, (K_SHAPED, n))
    else:
        js = J_THERMAL if thermal else 1.0
        plist = class_table(thermal)
        over = dict(max_step=3e-13, gamma=1.9e5)         # (short pulses: three steps chain here)
        T = np.stack([durations(rng, n, 3e-13) for _ in range(K_SHAPED)])
    cfg = dict(EPISODE, temperature=450.0, max_current=EPISODE["max_current"] * js, **over)
    J = rng.uniform(-2e6, 2e6, (K_SHAPED, n)) * js
    J[:, ::7] = 0.0
    acts = np.stack([J, T], axis=2)
    acts = acts if f64 else acts.astype(np.float32)
    # (factors of at most a quarter: three steps chain here, and the spin torque amplifies a perturbation exponentially in J t)
    shape = PiecewiseLinear([0.0, 0.15, 0.7, 0.9, 1.0], [0.0, 0.25, 0.25, -0.15, 0.0])
    span = float(T.max())
    fk = (np.array([-0.1 * span, 0.3 * span, 1.2 * span]), rng.uniform(-1e5, 1e5, (3, 3)))
    state = dict(m=unit_rows(rng, n), target=unit_targets(TARGETS5)[np.arange(n) % 5], total_energy=rng.uniform(0, 1e-21, n) * js * js,
                 step_count=rng.integers(0, 2, n))
    # the knots (tau_j T, J s_j) the shape gives each step's parsed action, as pulse_energy and the restatement take them
    cur = []
    for k in range(K_SHAPED):
        Jp, Tp = wave_step_ref.parse_actions(acts[k], cfg["max_current"], cfg["max_duration"])
        cur.append((shape.times[None, :] * Tp[:, None], Jp[:, None] * shape.values[None, :]))
    return dict(plist=plist, cls=(np.arange(n) % 3).astype(np.uint8), cfg=cfg, state=state, acts=acts, shape=shape, fk=fk, cur=cur)


SHAPED_REF = {}


def shaped_ref(method, noise, oracle, ulp=False):
    """the inputs of a direct case and the restatement's K_SHAPED steps under the knots (tau_j T, J s_j), computed once and shared"""
    key = (method, noise, ulp)
    if key in SHAPED_REF:
        return SHAPED_REF[key]
    s = shaped_problem(method, noise, False, 7100)
    n, cfg = N, s["cfg"]
    state, refs = dict(s["state"]), []
    if ulp:
        state["m"] = ulp_moved(state["m"])
    fld = (np.tile(s["fk"][0], (n, 1)), np.tile(s["fk"][1], (n, 1, 1)))
    for k in range(K_SHAPED):
        th = dict(oracle=oracle, seed=SEED, env_id0=ENV_ID0, rng_step=np.full(n, k), noise=noise, corr_time=CORR_TIME) if noise else None
        r = wave_step_ref.step(state, s["acts"][k], s["plist"], method, current=s["cur"][k], field=fld,
                               cfg=cfg, cls=s["cls"], dev_types=DEV_TYPES, thermal=th)
        assert (np.abs(r["alignment"] - cfg["success_threshold"]) > 1e-6).all()        # no flag rests on rounding
        refs.append(r)
        state = dict(m=r["m"], target=state["target"], total_energy=r["total_energy"], step_count=r["step_count"])
    SHAPED_REF[key] = (s, refs)
    return SHAPED_REF[key]


# ---------------------------------------------------------------------------------------------------------------------
# stg_step_knots: one launch of K_SHAPED steps whose actions [J, T, s_0 ... s_4] carry the knot amplitudes
# ---------------------------------------------------------------------------------------------------------------------
P_KNOTS = 5
# (at most a quarter, for the reason shaped_problem gives: three steps chain, and the spin torque amplifies a perturbation exponentially
# in J t)
KNOT_LIMIT = 0.25
KNOTS_SEED = 7300


def knots_problem(solver, noise, f64, seed):
    """shaped_problem(solver, noise, f64, seed) -- its configuration, class table, start state, field knots and (J, T) rows -- with the
    fixed shape replaced by P_KNOTS knot times tau (0, three sorted draws in (0.05, 0.95), 1), the limit KNOT_LIMIT and amplitudes drawn
    uniform in +-1.6 KNOT_LIMIT per env and per step (three in eight beyond the limit: the clamp is at work), from generator seed + 1.
    acts [K_SHAPED, N, 2 + P_KNOTS] float32 or float64; cur: the knots (tau_j T, J s_j) of each step's parsed action."""
    s = shaped_problem(solver, noise, f64, seed)
    rng = np.random.default_rng(seed + 1)
    tau = np.concatenate([[0.0], np.sort(rng.uniform(0.05, 0.95, P_KNOTS - 2)), [1.0]])
    assert (np.diff(tau) > 0).all()
    amp = rng.uniform(-1.6, 1.6, (K_SHAPED, N, P_KNOTS)) * KNOT_LIMIT
    acts = np.concatenate([s["acts"].astype(np.float64), amp], axis=2)
    if f64:
        assert np.all(amp.astype(np.float32).astype(np.float64) != amp)
    else:
        acts = acts.astype(np.float32)                     # (the (J, T) columns were float32 already)
    return with_knots(s, tau, KNOT_LIMIT, acts)


def with_knots(s, tau, limit, acts):
    """the shaped problem s under knot times tau, the amplitude limit and knot actions acts [K_SHAPED, N, 2 + P] instead of its shape"""
    import knots_ref as kr
    p = {k: v for k, v in s.items() if k != "shape"}
    cfg = s["cfg"]
    cur = [kr.knot_tables_np(tau, *kr.parse_np(acts[k], cfg["max_current"], cfg["max_duration"], limit)) for k in range(K_SHAPED)]
    return dict(p, tau=np.asarray(tau, dtype=np.float64), limit=float(limit), acts=acts, cur=cur)


def run_knots_ref(p, method, noise, oracle, ulp=False):
    """the restatement's K_SHAPED steps of a knots problem: wave_step_ref.step under each step's tables p['cur'][k], the (J, T) rows
    through knots_ref.wave_rows, the field table replicated and the thermal stream keyed as in shaped_ref"""
    import knots_ref as kr
    n, cfg = N, p["cfg"]
    state, refs = dict(p["state"]), []
    if ulp:
        state["m"] = ulp_moved(state["m"])
    fld = (np.tile(p["fk"][0], (n, 1)), np.tile(p["fk"][1], (n, 1, 1)))
    for k in range(K_SHAPED):
        th = dict(oracle=oracle, seed=SEED, env_id0=ENV_ID0, rng_step=np.full(n, k), noise=noise, corr_time=CORR_TIME) if noise else None
        r = wave_step_ref.step(state, kr.wave_rows(p["acts"][k]), p["plist"], method, current=p["cur"][k], field=fld,
                               cfg=cfg, cls=p["cls"], dev_types=DEV_TYPES, thermal=th)
        refs.append(r)
        state = dict(m=r["m"], target=state["target"], total_energy=r["total_energy"], step_count=r["step_count"])
    return refs


KNOTS_REF = {}


def knots_ref(method, noise, oracle, ulp=False):
    """the inputs of a direct knots case and the restatement's K_SHAPED steps, computed once and shared"""
    key = (method, noise, ulp)
    if key not in KNOTS_REF:
        p = knots_problem(method, noise, False, KNOTS_SEED)
        refs = run_knots_ref(p, method, noise, oracle, ulp)
        for r in refs:
            assert (np.abs(r["alignment"] - p["cfg"]["success_threshold"]) > 1e-6).all()        # no flag rests on rounding
        KNOTS_REF[key] = (p, refs)
    return KNOTS_REF[key]


# ---------------------------------------------------------------------------------------------------------------------
# tests/golden/G24_wave_config.npz
# ---------------------------------------------------------------------------------------------------------------------
def g24_solve_knots(g, k):
    kj, kh = int(g["sv_kj"][k]), int(g["sv_kh"][k])
    cur = (g["sv_tj"][k, :kj][None], g["sv_jk"][k, :kj][None]) if kj else None
    fld = (g["sv_th"][k, :kh][None], g["sv_hk"][k, :kh][None]) if kh else None
    return cur, fld


def g24_solver(g, k):
    return ("rk4", "euler", "rk45")[int(g["sv_solver"][k])]


def g24_env_cfg(g, k):
    return dict(max_current=float(g["ev_max_current"][k]), max_duration=float(g["ev_max_duration"]), success_threshold=float(g["ev_success_threshold"]),
                energy_penalty_weight=float(g["ev_energy_penalty_weight"]), max_steps=int(g["ev_max_steps"]), temperature=float(g["ev_temperature"]),
                max_step=float(g["ev_max_step"][k]), target_states=g["ev_targets"].tolist())


def g24_env_tables(g, k):
    """step k of the env rows -> (current, field) as wave_step_ref.step takes them (N = 1), built as the envs build them"""
    kj, kh = int(g["ev_kj"][k]), int(g["ev_kh"][k])
    J, T = float(g["ev_J"][k]), float(g["ev_T"][k])
    cur = (g["ev_tau"][k, :kj][None] * T, J * g["ev_scale"][k, :kj][None]) if kj else None
    fld = (g["ev_th"][k, :kh][None], g["ev_hk"][k, :kh][None]) if kh else None
    return cur, fld


def g24_env_action(g, k):
    return np.array([g["ev_action"][k]], dtype=np.float64 if g["ev_act_f64"][k] else np.float32)


def g24_shape_and_field(g, k):
    """step k -> (pulse_shape, applied_field knots (times, values) or None)"""
    from spin_torque_gym_amd.physics import PiecewiseLinear
    kj, kh = int(g["ev_kj"][k]), int(g["ev_kh"][k])
    shape = PiecewiseLinear(g["ev_tau"][k, :kj], g["ev_scale"][k, :kj]) if kj else None
    return shape, ((g["ev_th"][k, :kh], g["ev_hk"][k, :kh]) if kh else None)


def check_step_against_g24(g, k, got, tol_m, where):
    """`got`: dict(m [3], obs [12], reward, terminated, truncated, energy) of env row k.  Everything but the energy (and what hangs on
    it: obs[9] and the reward's energy term) against the file; the energy against the closed form (wave_step_ref.check_step_against_g23
    with this file's configuration)."""
    cfg = g24_env_cfg(g, k)
    cur, _ = g24_env_tables(g, k)
    p = stt_default_params(volume=float(g["ev_volume"][k]))
    r = wave_step_ref.resistance(g["ev_m_before"][k][None], p)[0]
    if cur is None:
        e_ref = float(g["ev_energy_rect"][k])
    else:
        ra = r * p["area"]
        e_ref = float((ra * ra) / r * wave_step_ref.pulse_sq_integral(cur[0], cur[1], [float(g["ev_T"][k])])[0])
    err = float(np.abs(got["m"] - g["ev_m_after"][k]).max())
    assert err <= tol_m, (where, k, err)
    assert bool(got["terminated"]) == bool(g["ev_terminated"][k]) and bool(got["truncated"]) == bool(g["ev_truncated"][k]), (where, k)
    idx = [i for i in range(12) if i != 9]
    o, og = np.asarray(got["obs"], dtype=np.float32)[idx], g["ev_obs"][k][idx]
    assert np.all(np.abs(o - og) <= wave_step_ref.F32_ULP * np.abs(og) + 2 * tol_m), (where, k, o, og)
    assert abs(float(got["energy"]) - e_ref) <= 1e-13 * abs(e_ref), (where, k, float(got["energy"]), e_ref)
    w = cfg["energy_penalty_weight"]
    base_ref = float(g["ev_reward"][k]) - w * (float(g["ev_energy_rect"][k]) / 1e-12)
    base_got = float(got["reward"]) - w * (float(got["energy"]) / 1e-12)
    assert abs(base_got - base_ref) <= 1e-9 + 2 * tol_m, (where, k, base_got, base_ref)
    return err

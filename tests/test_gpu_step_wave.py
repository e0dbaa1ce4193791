"""Shaped current pulses and an applied field on the env step path (stg_step_wave), on the GPU: `pytest -m gpu`.

  1. no tables at all is stg_step, bit for bit: state, every output and the counters, for RK4, Euler and RK45, thermal field off and on
     (same seed), float32 durations, two classes, the easy-axis specialisation and the general form;
  2. the steps the reference env computed under shaped pulses and fields (tests/golden/G23_wave_step.npz) through the C-ABI and through
     SpinTorqueVecEnv / SpinTorqueEnv(pulse_shape=, applied_field=): m within the tolerance tests/test_gpu_waveforms.py applies to the same
     device function, fp32 observations within one float32 ulp, flags exact, the energy against the closed form;
  3. a random sweep against the NumPy restatement (tests/wave_step_ref.py): two full wavefronts and a 2-lane tail, per-env tables;
  4. RK45 against the GPU's own stg_solve_wave of the same tables (pinned by G22) plus the NumPy tail -- against the C oracle's waveform
     solve plus the same tail, two chained steps at N = 130: tests/test_gpu_wave_rk45_oracle.py;
  5. thermal: the same seed twice, and a partition of the envs over two contexts;
  6. autoreset with final_obs, skip_done, records against SoA, a bad table in one lane, the write footprint, the checked errors.
Sizes are N = 1, 64, 65 and 130 (two full wavefronts plus two lanes)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import stt_default_params
from helpers import Guarded
import wave_step_ref
from wave_step_ref import check_step_against_g23, g23_action, g23_params, g23_shape_and_field, g23_tables

pytestmark = pytest.mark.gpu

TOL_RK4 = 1e-10                  # tests/test_gpu_waveforms.py, tests/test_gpu_parity.py: the fixed-step solvers against the reference
TOL_RK45 = 1e-8
F32, F64, U8, I32 = torch.float32, torch.float64, torch.uint8, torch.int32
VOL = {"rk4": (8.75e-11, 2e-11), "euler": (8.75e-11, 2e-11), "rk45": (9.7e-6, 2e-6)}
STATE_KEYS = ("m", "target", "total_energy", "step_count", "rng_step", "done")
NO_TABLES = {"current": None, "field": None}
# The thermal tests use the factory's own volume (in the rescaled volumes of the current-driven cases the Brown field is ~1e-9 A/m and
# would show nothing); the spin torque goes with J / volume, so currents are scaled down with it.
THERMAL_J = 1e-13


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _flat(stg, d):
    return stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", d))


def _backend(stg, n, plist, cls=None, env_id0=0, **cfg):
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    b = HipBackend(n, EnvConfig(**{"diagnostics": True, **cfg}), 0, env_id0)
    b.set_params([_flat(stg, p) for p in plist], cls)
    return b


def _unit_rows(rng, n):
    v = rng.normal(0, 1, (n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _wave(cur=None, fld=None):
    """per-env knots in the tests' layout -- cur = (tj [N,K], jk [N,K]), fld = (th [N,K], hk [N,K,3]) -- as HipBackend.step_wave takes them"""
    w = {"current": None, "field": None}
    if cur is not None:
        w["current"] = (_dev(np.asarray(cur[0]).T), _dev(np.asarray(cur[1]).T))
    if fld is not None:
        w["field"] = (_dev(np.asarray(fld[0]).T), _dev(np.transpose(np.asarray(fld[1]), (1, 2, 0))))
    return w


def _bits(t):
    t = t.contiguous()
    return t.view({F32: torch.int32, F64: torch.int64}.get(t.dtype, t.dtype))


def _same(x, y, what):
    """bit for bit (floats compared as integers)"""
    assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape, x.dtype, y.dtype)
    bad = (_bits(x) != _bits(y)).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements differ, first at {bad[:4].tolist()}"


OUT_NAMES = ("obs", "reward", "reward_f64", "terminated", "truncated", "status")


def _outs(b, res):
    """the six tensors a step returns plus the energy, cloned"""
    torch.cuda.synchronize()
    d = {k: v.clone() for k, v in zip(OUT_NAMES, res)}
    d["energy"] = b.energy.clone()
    return d


def _state(b):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in b.get_state().items()}


def _same_run(a, b, what):
    for k in a:
        _same(a[k], b[k], (what, k))


def _problem(n, solver, seed, f64=False):
    """unit rows, +-z targets, actions with mixed J (zeros and both signs) and float32 durations"""
    rng = np.random.default_rng(seed)
    m0 = _unit_rows(rng, n)
    tgt = np.where(rng.integers(0, 2, (n, 1)) == 0, 1.0, -1.0) * np.array([[0.0, 0.0, 1.0]])
    T = rng.uniform(1e-11, 3e-11, n) if solver == "rk45" else rng.uniform(2e-11, 1.2e-10, n)
    J = rng.uniform(-2e6, 2e6, n)
    J[::5] = 0.0
    act = np.stack([J, T], axis=1).astype(np.float64 if f64 else np.float32)
    return m0, tgt, act


def _start(b, m0, tgt):
    b.reset(init_m=_dev(m0.T), target=_dev(tgt.T))


# ------------------------------------------------------------------------------------------------
# 1. zero tables are the existing step
# ------------------------------------------------------------------------------------------------
# (solver, thermal field: None, "white" or the Ornstein-Uhlenbeck field of the fixed-step solvers)
FIELDS = [(s, f) for s in ("rk4", "euler", "rk45") for f in (None, "white")] + [("rk4", "ou"), ("euler", "ou")]


@pytest.mark.parametrize("axis", ("z", "tilted"))
@pytest.mark.parametrize("solver,noise,n", [(s, f, 130) for s, f in FIELDS] + [("rk4", f, n) for n in (1, 64, 65) for f in (None, "white")])
def test_zero_tables_are_stg_step_bit_for_bit(stg, solver, noise, n, axis):
    thermal = noise is not None
    noise_kw = dict(noise_model="ou") if noise == "ou" else {}
    extra = {} if axis == "z" else dict(easy_axis=np.array([0.15, -0.1, 1.0]), demag_factors=np.array([0.1, 0.2, 0.7]))
    # (the factory's own volume with the thermal field: in the rescaled volumes the Brown field is too small to show)
    plist = [stt_default_params(volume=v, **extra) for v in VOL[solver]] if not thermal else \
        [stt_default_params(**extra), stt_default_params(damping=0.02, **extra)]
    cls = torch.tensor((np.arange(n) % 2).astype(np.uint8))
    m0, tgt, act = _problem(n, solver, 11)
    if thermal:
        act[:, 0] *= THERMAL_J                # (a current the factory's volume integrates)
    runs = []
    for wave in (False, True):
        b = _backend(stg, n, plist, cls, solver=solver, include_thermal_fluctuations=thermal, seed=77, **noise_kw)
        _start(b, m0, tgt)
        steps = []
        for k in range(2):                    # (two steps: the second one's stream position is 1)
            a = _dev(np.roll(act, k, axis=0).T)
            res = b.step_wave(a, NO_TABLES) if wave else b.step(a)
            steps.append(_outs(b, res))
        runs.append((steps, _state(b), b.counters()))
        b.close()
    (sa, sta, ca), (sb, stb, cb) = runs
    for k in range(2):
        _same_run(sa[k], sb[k], (solver, n, thermal, axis, "step", k))
    _same_run(sta, stb, (solver, n, thermal, axis, "state"))
    assert ca == cb and ca["env_steps"] == 2 * n and ca["work_units"] > 0, (ca, cb)
    assert bool((sta["rng_step"] == 2).all())


@pytest.mark.parametrize("solver,noise", FIELDS)
def test_zero_field_table_on_a_general_axis_is_stg_step_bit_for_bit(stg, solver, noise):
    """The waveform solvers themselves, pinned exactly: with a tilted easy axis stg_step runs the general form of its solvers, which is
    the form the waveform solvers are written in, and kj = 0 with an all-zero field table is the rectangular pulse in zero field.  So
    stg_step_wave(kj = 0, kh = 2, hk = 0) -- simple_solve_wave / llgs_solve_wave -- must give stg_step's state, outputs and counters
    (work_units: every sub-step / RK45 attempt) bit for bit, and so must stg_step_wave without tables."""
    thermal = noise is not None
    n = 130
    tilt = dict(easy_axis=np.array([0.15, -0.1, 1.0]), demag_factors=np.array([0.1, 0.2, 0.7]))
    plist = [stt_default_params(volume=v, **tilt) for v in VOL[solver]] if not thermal else \
        [stt_default_params(**tilt), stt_default_params(damping=0.02, **tilt)]
    cls = torch.tensor((np.arange(n) % 2).astype(np.uint8))
    m0, tgt, act = _problem(n, solver, 12)
    if thermal:
        act[:, 0] *= THERMAL_J
    zero_field = {"current": None, "field": (_dev(np.tile([[0.0], [1e-9]], (1, n))), torch.zeros((2, 3, n), dtype=F64, device="cuda"))}
    runs = {}
    for form in ("stg_step", "no tables", "zero field table"):
        b = _backend(stg, n, plist, cls, solver=solver, include_thermal_fluctuations=thermal, seed=78, **(dict(noise_model="ou") if noise == "ou" else {}))
        _start(b, m0, tgt)
        steps = []
        for k in range(2):
            a = _dev(np.roll(act, k, axis=0).T)
            steps.append(_outs(b, b.step(a) if form == "stg_step" else b.step_wave(a, NO_TABLES if form == "no tables" else zero_field)))
        runs[form] = (steps, _state(b), b.counters())
        b.close()
    sa, sta, ca = runs["stg_step"]
    assert bool((sa[0]["status"] == 0).all()) and ca["work_units"] > 2 * n
    for form in ("no tables", "zero field table"):
        sb, stb, cb = runs[form]
        for k in range(2):
            _same_run(sa[k], sb[k], (solver, thermal, form, "step", k))
        _same_run(sta, stb, (solver, thermal, form, "state"))
        assert ca == cb, (form, ca, cb)


# ------------------------------------------------------------------------------------------------
# 2. golden steps of the reference env
# ------------------------------------------------------------------------------------------------
def test_golden_steps_through_the_c_abi(stg, golden):
    g = golden("G23_wave_step")
    backends, worst = {}, 0.0
    for k in range(len(g["T"])):
        solver = ("rk4", "euler")[int(g["solver"][k])]
        if solver not in backends:
            backends[solver] = _backend(stg, 1, [g23_params(g)], solver=solver, include_thermal_fluctuations=False)
            _start(backends[solver], g["m_before"][k][None], g["target"][k][None])
        b = backends[solver]
        b.set_state(dict(m=g["m_before"][k][:, None], target=g["target"][k][:, None], total_energy=np.array([g["etot_before"][k]]),
                         step_count=np.array([g["step_before"][k]], dtype=np.int32), done=np.zeros(1, dtype=np.uint8)))
        cur, fld = g23_tables(g, k)
        o = _outs(b, b.step_wave(_dev(g23_action(g, k).T), _wave(cur, fld)))
        m = _state(b)["m"][:, 0].cpu().numpy()
        got = dict(m=m, obs=o["obs"][:, 0].cpu().numpy(), reward=float(o["reward_f64"][0]), terminated=int(o["terminated"][0]),
                   truncated=int(o["truncated"][0]), energy=float(o["energy"][0]))
        err = check_step_against_g23(g, k, got, TOL_RK4, "C-ABI")
        worst = max(worst, err)
        print(f"G23 step {k} ({solver}, kj={g['kj'][k]}, kh={g['kh'][k]}, T={g['T'][k]:g}): |m - m_ref| = {err:.2e}")
        assert int(o["status"][0]) == 0
    print(f"G23 through the C-ABI: worst |m - m_ref| = {worst:.2e}")
    for b in backends.values():
        b.close()


@pytest.mark.parametrize("facade", (False, True), ids=("SpinTorqueVecEnv", "SpinTorqueEnv"))
def test_golden_episodes_through_the_envs(stg, golden, facade):
    g = golden("G23_wave_step")
    for e in np.unique(g["episode"]):
        ks = np.nonzero(g["episode"] == e)[0]
        shape, field = g23_shape_and_field(g, ks[0])
        kw = dict(device_params=g23_params(g), include_thermal_fluctuations=False, solver=("rk4", "euler")[int(g["solver"][ks[0]])],
                  pulse_shape=shape, applied_field=field)
        m0, tgt = g["m_before"][ks[0]], g["target"][ks[0]]
        if facade:
            env = stg.SpinTorqueEnv(**kw)
            env.reset(options={"initial_state": m0, "target_state": tgt})
        else:
            env = stg.SpinTorqueVecEnv(2, diagnostics=True, out_layout="records" if e % 2 else "soa", **kw)
            env.reset(options={"initial_state": m0, "target_state": tgt})
        for k in ks:
            a = g23_action(g, k)
            if facade:
                obs, reward, term, trunc, info = env.step(a[0])
                assert "error" not in info, info
                rows = [dict(m=env.current_magnetization, obs=obs, reward=reward, terminated=term, truncated=trunc, energy=info["energy_consumed"])]
                assert info["current_density"] == g["J"][k] and info["pulse_duration"] == g["T"][k]
            else:
                obs, rew, term, trunc, info = env.step(torch.from_numpy(np.repeat(a, 2, axis=0)))
                torch.cuda.synchronize()
                m = env.get_state()["m"].cpu().numpy()
                rows = [dict(m=m[:, i], obs=obs[i].cpu().numpy(), reward=float(info["reward_f64"][i]), terminated=bool(term[i]),
                             truncated=bool(trunc[i]), energy=float(info["energy"][i])) for i in range(2)]
                assert abs(float(rew[0]) - float(info["reward_f64"][0])) <= 1e-6 * max(1.0, abs(float(rew[0])))
            for row in rows:                  # (the steps chain; the generator's perturbed twins show that the bound covers it)
                check_step_against_g23(g, k, row, TOL_RK4, f"episode {e}")
        env.close()


# ------------------------------------------------------------------------------------------------
# 3. random sweep against the restatement
# ------------------------------------------------------------------------------------------------
SWEEP = {}


def _tables(rng, n, K, T, width):
    """per-env knots: some tables stop before T, some go beyond it, some start after t = 0, some before it"""
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


def _sweep_case(n, kj, kh, method):
    """inputs and the restatement's answer, computed once per case and shared; drawn again until no flag of the reference rests on rounding"""
    key = (n, kj, kh, method)
    if key in SWEEP:
        return SWEEP[key]
    plist = [stt_default_params(volume=v) for v in VOL[method]]
    cls = (np.arange(n) % 2).astype(np.uint8)
    for seed in range(2000 + kj * 40 + kh, 2000 + kj * 40 + kh + 20):
        rng = np.random.default_rng(seed)
        m0, tgt, act = _problem(n, method, seed)
        _, T = wave_step_ref.parse_actions(act, 2e6, 5e-9)
        cur = _tables(rng, n, kj, T, 1) if kj else None
        fld = _tables(rng, n, kh, T, 3) if kh else None
        state = dict(m=m0, target=tgt, total_energy=rng.uniform(0, 1e-21, n), step_count=rng.integers(0, 50, n))
        ref = wave_step_ref.step(state, act, plist, method, current=cur, field=fld, cls=cls)
        if (np.abs(ref["alignment"] - 0.9) > 1e-6).all():
            break
    SWEEP[key] = (plist, cls, m0, tgt, act, cur, fld, state, ref)
    return SWEEP[key]


@pytest.mark.parametrize("method", ("rk4", "euler"))
@pytest.mark.parametrize("n,kj,kh", [(130, 2, 32), (130, 17, 3), (130, 32, 17), (130, 5, 0), (130, 0, 4), (1, 3, 2)])
def test_random_sweep_vs_restatement(stg, n, kj, kh, method):
    plist, cls, m0, tgt, act, cur, fld, state, ref = _sweep_case(n, kj, kh, method)
    assert (np.abs(ref["alignment"] - 0.9) > 1e-6).all()                     # no flag of the reference rests on rounding
    assert (ref["status"] == 0).all()
    b = _backend(stg, n, plist, torch.tensor(cls), solver=method, include_thermal_fluctuations=False)
    _start(b, m0, tgt)
    b.set_state(dict(total_energy=state["total_energy"], step_count=state["step_count"].astype(np.int32)))
    o = _outs(b, b.step_wave(_dev(act.T), _wave(cur, fld)))
    st = _state(b)
    m = st["m"].cpu().numpy().T
    err = float(np.abs(m - ref["m"]).max())
    e, e_ref = o["energy"].cpu().numpy(), ref["energy"]
    e_err = float(np.max(np.abs(e - e_ref) / np.maximum(np.abs(e_ref), 1e-300)))
    print(f"sweep n={n} kj={kj} kh={kh} {method}: worst |m - m_ref| = {err:.2e}, worst relative energy difference {e_err:.1e}")
    assert err <= TOL_RK4
    # the energy: the closed form in the same order of operations; the resistance goes through the kernels' reciprocal square root
    # (<= 2 ulp per component of m / |m|), so a few ulp
    assert np.all(np.abs(e - e_ref) <= 1e-13 * np.abs(e_ref))
    assert np.array_equal(o["terminated"].cpu().numpy().astype(bool), ref["terminated"])
    assert np.array_equal(o["truncated"].cpu().numpy().astype(bool), ref["truncated"])
    assert np.array_equal(o["status"].cpu().numpy(), ref["status"])
    ob, ob_ref = o["obs"].cpu().numpy().T, ref["obs"]
    # fp32 observations: one float32 ulp, plus what TOL_RK4 on m allows in the components that follow m (m itself and the resistance)
    assert np.all(np.abs(ob - ob_ref) <= wave_step_ref.F32_ULP * np.abs(ob_ref) + 2 * TOL_RK4)
    assert np.all(np.abs(o["reward_f64"].cpu().numpy() - ref["reward"]) <= 1e-9)
    assert np.array_equal(st["step_count"].cpu().numpy(), ref["step_count"])
    assert np.all(np.abs(st["total_energy"].cpu().numpy() - ref["total_energy"]) <= 1e-13 * np.abs(ref["total_energy"]))
    assert b.counters() == {"env_steps": n, "work_units": int(ref["n_sub"].sum()), "noop_steps": 0}
    b.close()


# ------------------------------------------------------------------------------------------------
# 4. RK45: the step is the GPU's own stg_solve_wave plus the tail
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thermal", (False, True), ids=("T0", "thermal"))
def test_rk45_step_is_solve_wave_plus_the_tail(stg, thermal):
    n, kj, kh = 66, 5, 3
    rng = np.random.default_rng(8)
    m0, tgt, act = _problem(n, "rk45", 8)
    act[:, 1] = rng.uniform(5e-11, 3e-10, n).astype(np.float32)
    J, T = wave_step_ref.parse_actions(act, 2e6, 5e-9)
    cur, fld = _tables(rng, n, kj, T, 1), _tables(rng, n, kh, T, 3)
    p = stt_default_params(volume=VOL["rk45"][0])
    b = _backend(stg, n, [p], solver="rk45", include_thermal_fluctuations=thermal, seed=5)
    _start(b, m0, tgt)
    start = _state(b)
    sol = b.solve(start["m"], None, _dev(T), env_step=0, wave=_wave(cur, fld))
    o = _outs(b, b.step_wave(_dev(act.T), _wave(cur, fld)))
    st = _state(b)
    assert bool(sol["success"].all()) and bool((o["status"] == 0).all())
    # (What pins this path exactly is test_zero_field_table_on_a_general_axis_is_stg_step_bit_for_bit; this comparison is an extra.)
    # The solve hands back the last accepted point, normalised; the step's tail normalises that row once more with the kernels'
    # reciprocal square root (seed + one correction, <= 2 ulp per component: csrc/stg_physics.hpp), which NumPy cannot restate bit for
    # bit.  Of a row that is already of unit length to 2 ulp the second normalisation moves a component by at most 4 ulp of 1.
    d = (st["m"] - sol["m_final"]).abs()
    print(f"rk45 step vs solve (thermal={thermal}): {int((d == 0).sum())} of {d.numel()} components bit-equal, worst difference {float(d.max()):.2e}")
    assert float(d.max()) <= 4 * 2.220446049250313e-16
    c = b.counters()
    assert c["env_steps"] == n and c["noop_steps"] == 0 and c["work_units"] >= int(sol["n_points"].sum())       # attempts >= accepted points
    # the tail in NumPy, from the solve's rows
    m = st["m"].cpu().numpy().T
    m_before = start["m"].cpu().numpy().T
    align = (m[:, 0] * tgt[:, 0] + m[:, 1] * tgt[:, 1]) + m[:, 2] * tgt[:, 2]
    r = wave_step_ref.resistance(m_before, p)
    ra = r * p["area"]
    e_ref = (ra * ra) / r * wave_step_ref.pulse_sq_integral(cur[0], cur[1], T)
    assert np.all(np.abs(o["energy"].cpu().numpy() - e_ref) <= 1e-13 * np.abs(e_ref))
    assert (np.abs(align - 0.9) > 1e-6).all()                                    # no flag rests on rounding
    assert np.array_equal(o["terminated"].cpu().numpy().astype(bool), align >= 0.9)
    ob = wave_step_ref.observation(m, tgt, wave_step_ref.resistance(m, p), p, wave_step_ref.DEFAULT_CFG, np.ones(n), st["total_energy"].cpu().numpy(), J, T)
    assert np.all(np.abs(o["obs"].cpu().numpy().T - ob) <= wave_step_ref.F32_ULP * np.abs(ob) + 1e-37)
    b.close()


# ------------------------------------------------------------------------------------------------
# 5. thermal field
# ------------------------------------------------------------------------------------------------
def _thermal_run(stg, solver, lo, hi, noise="white", seed=99):
    """envs [lo, hi) of a 130-env problem under shaped pulses and a field, two steps, thermal field on"""
    n_all = 130
    rng = np.random.default_rng(21)
    m0, tgt, act = _problem(n_all, solver, 21)
    act[:, 0] *= THERMAL_J
    _, T = wave_step_ref.parse_actions(act, 2e6, 5e-9)
    cur, fld = _tables(rng, n_all, 4, T, 1), _tables(rng, n_all, 3, T, 3)
    cur = (cur[0], cur[1] * THERMAL_J)
    sl = slice(lo, hi)
    kw = dict(noise_model=noise) if noise != "white" else {}
    b = _backend(stg, hi - lo, [stt_default_params()], env_id0=lo, solver=solver, include_thermal_fluctuations=True, seed=seed, **kw)
    _start(b, m0[sl], tgt[sl])
    w = _wave((cur[0][sl], cur[1][sl]), (fld[0][sl], fld[1][sl]))
    outs = [_outs(b, b.step_wave(_dev(act[sl].T), w)) for _ in range(2)]
    st = _state(b)
    b.close()
    return outs, st


@pytest.mark.parametrize("solver,noise", [("rk4", "white"), ("euler", "white"), ("rk45", "white"), ("rk4", "ou"), ("euler", "ou")])
def test_thermal_same_seed_twice_and_partition_invariance(stg, solver, noise):
    full, st_full = _thermal_run(stg, solver, 0, 130, noise)
    again, st_again = _thermal_run(stg, solver, 0, 130, noise)
    part, st_part = _thermal_run(stg, solver, 64, 130, noise)
    for k in range(2):
        _same_run(full[k], again[k], (solver, "same seed twice, step", k))
        for name in full[k]:
            _same(full[k][name][..., 64:], part[k][name], (solver, "partition, step", k, name))
    for name in STATE_KEYS:
        _same(st_full[name], st_again[name], (solver, "state", name))
        _same(st_full[name][..., 64:], st_part[name], (solver, "partition, state", name))
    assert bool((full[0]["status"] == 0).all())
    # the field is on: another seed ends elsewhere by far more than rounding
    _, st_other = _thermal_run(stg, solver, 0, 130, noise, seed=100)
    assert float((st_other["m"] - st_full["m"]).abs().max()) > 1e-10


# ------------------------------------------------------------------------------------------------
# 6. other behaviour
# ------------------------------------------------------------------------------------------------
def _shaped_problem(n, seed=4):
    rng = np.random.default_rng(seed)
    m0, tgt, act = _problem(n, "rk4", seed)
    _, T = wave_step_ref.parse_actions(act, 2e6, 5e-9)
    return m0, tgt, act, _tables(rng, n, 4, T, 1), _tables(rng, n, 3, T, 3)


def test_autoreset_with_final_obs(stg):
    n = 130
    m0, tgt, act, cur, fld = _shaped_problem(n)
    p = [stt_default_params(volume=VOL["rk4"][0])]
    kw = dict(solver="rk4", include_thermal_fluctuations=False, seed=3, success_threshold=0.0)       # about half the envs end at once
    plain = _backend(stg, n, p, **kw)
    auto = _backend(stg, n, p, **kw)
    for b in (plain, auto):
        _start(b, m0, tgt)
    o_plain = _outs(plain, plain.step_wave(_dev(act.T), _wave(cur, fld)))
    auto.final_obs = None
    o_auto = _outs(auto, auto.step_wave(_dev(act.T), _wave(cur, fld), autoreset=True))
    final = auto.final_obs.clone()
    done = (o_plain["terminated"] | o_plain["truncated"]) != 0
    assert 10 < int(done.sum()) < n - 10
    for k in ("reward", "reward_f64", "terminated", "truncated", "status", "energy"):
        _same(o_auto[k], o_plain[k], ("autoreset", k))
    _same(final[:, done], o_plain["obs"][:, done], "final_obs = the terminal observation")
    assert bool((final[:, ~done] == 0).all())                                     # rows of other envs untouched (allocated as zeros)
    _same(o_auto["obs"][:, ~done], o_plain["obs"][:, ~done], "obs of the envs that go on")
    st = _state(auto)
    assert bool((st["step_count"][done] == 0).all()) and bool((st["total_energy"][done] == 0).all()) and not bool(st["done"].any())
    assert bool((o_auto["obs"][8, done] == 1.0).all()) and bool((o_auto["obs"][10:, done] == 0).all())  # a new episode's first observation
    # the same reset the step kernels draw
    ref = _backend(stg, n, p, **kw)
    _start(ref, m0, tgt)
    ref.step(_dev(act.T), autoreset=True)
    st_ref = _state(ref)
    both = done & (st_ref["step_count"] == 0)                                     # (the rectangular pulse ends other episodes)
    assert int(both.sum()) > 10
    _same(st["target"][:, both], st_ref["target"][:, both], "targets drawn by the auto-reset")
    _same(st["m"][:, both], st_ref["m"][:, both], "states drawn by the auto-reset")
    for b in (plain, auto, ref):
        b.close()


def test_skip_done(stg):
    n = 130
    m0, tgt, act, cur, fld = _shaped_problem(n)
    p = [stt_default_params(volume=VOL["rk4"][0])]
    kw = dict(solver="rk4", include_thermal_fluctuations=False, success_threshold=0.0)
    b = _backend(stg, n, p, skip_done=True, **kw)
    ref = _backend(stg, n, p, **kw)
    for x in (b, ref):
        _start(x, m0, tgt)
        x.step_wave(_dev(act.T), _wave(cur, fld))
    done = _state(b)["done"] != 0
    assert 10 < int(done.sum()) < n - 10
    before = _state(b)
    o = _outs(b, b.step_wave(_dev(act.T), _wave(cur, fld)))
    o_ref = _outs(ref, ref.step_wave(_dev(act.T), _wave(cur, fld)))
    after = _state(b)
    assert bool((o["status"][done] == 3).all()) and bool((o["reward_f64"][done] == 0).all()) and bool((o["energy"][done] == 0).all())
    for k in STATE_KEYS:
        _same(after[k][..., done], before[k][..., done], ("skip_done: a finished env is not stepped", k))
    for k in o:
        _same(o[k][..., ~done], o_ref[k][..., ~done], ("skip_done: the others step as always", k))
    assert b.counters()["env_steps"] == n + int((~done).sum())
    b.close()
    ref.close()


@pytest.mark.parametrize("n", (1, 64, 65, 130))
def test_records_layout_equals_soa(stg, n):
    from spin_torque_gym_amd.backend import record_views
    m0, tgt, act, cur, fld = _shaped_problem(n)
    p = [stt_default_params(volume=VOL["rk4"][0])]
    outs = {}
    for layout in ("soa", "records"):
        b = _backend(stg, n, p, solver="rk4", include_thermal_fluctuations=False, out_layout=layout, success_threshold=0.0, seed=3)
        _start(b, m0, tgt)
        b.step_wave(_dev(act.T), _wave(cur, fld), autoreset=True)
        torch.cuda.synchronize()
        if layout == "records":
            obs, reward, term, trunc, status = record_views(b.packed)
            outs[layout] = dict(obs=obs.t().contiguous(), reward=reward.contiguous(), terminated=term.contiguous(), truncated=trunc.contiguous(),
                                status=status.contiguous(), final=b.final_obs.contiguous())
            assert bool((b.packed[:, 55] == 0).all())
            _same(status.contiguous(), b.status, "status byte of the records")
            other = torch.zeros_like(b.packed)
            b2 = _backend(stg, n, p, solver="rk4", include_thermal_fluctuations=False, out_layout=layout, success_threshold=0.0, seed=3)
            _start(b2, m0, tgt)
            b2.step_wave(_dev(act.T), _wave(cur, fld), autoreset=True, out=other)       # out=: another record array
            torch.cuda.synchronize()
            _same(other, b.packed, "out= record array")
            b2.close()
        else:
            outs[layout] = dict(obs=b.obs.clone(), reward=b.reward.clone(), terminated=b.terminated.clone(), truncated=b.truncated.clone(),
                                status=b.status.clone(), final=b.final_obs.clone())
        outs[layout].update(reward_f64=b.reward64.clone(), energy=b.energy.clone())
        b.close()
    _same_run(outs["soa"], outs["records"], ("records vs soa", n))


BAD_LANES = {3: "equal times", 64: "decreasing times", 70: "NaN time", 100: "inf field value", 129: "NaN current value"}


def _spoil(cur, fld):
    cur = (cur[0].copy(), cur[1].copy())
    fld = (fld[0].copy(), fld[1].copy())
    cur[0][3, 1] = cur[0][3, 0]
    fld[0][64, 2] = fld[0][64, 0]
    cur[0][70, 0] = np.nan
    fld[1][100, 1, 2] = np.inf
    cur[1][129, 2] = np.nan
    return cur, fld


@pytest.mark.parametrize("solver", ("rk4", "rk45"))
def test_bad_tables_fail_their_lane_only(stg, solver):
    n = 130
    m0, tgt, act, cur, fld = _shaped_problem(n)
    if solver == "rk45":
        act[:, 1] *= 0.25
        cur, fld = (cur[0] * 0.25, cur[1]), (fld[0] * 0.25, fld[1])
    p = [stt_default_params(volume=VOL[solver][0])]
    good = _backend(stg, n, p, solver=solver, include_thermal_fluctuations=False)
    bad = _backend(stg, n, p, solver=solver, include_thermal_fluctuations=False)
    for b in (good, bad):
        _start(b, m0, tgt)
    before = _state(bad)
    o_good = _outs(good, good.step_wave(_dev(act.T), _wave(cur, fld)))
    o_bad = _outs(bad, bad.step_wave(_dev(act.T), _wave(*_spoil(cur, fld))))
    lanes = torch.tensor(sorted(BAD_LANES), device="cuda")
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[lanes] = False
    assert bool((o_good["status"] == 0).all())
    for k in o_bad:
        _same(o_bad[k][..., keep], o_good[k][..., keep], ("neighbours of a bad table", k))
    sg, sb = _state(good), _state(bad)
    for k in STATE_KEYS:
        _same(sb[k][..., keep], sg[k][..., keep], ("neighbours of a bad table, state", k))
    # the failed-solve path: no-op, m unchanged, no energy, the step still counts
    assert bool((o_bad["status"][lanes] == 1).all()) and bool((o_bad["energy"][lanes] == 0).all())
    _same(sb["m"][:, lanes], before["m"][:, lanes], "m of a lane with a bad table")
    assert bool((sb["step_count"][lanes] == 1).all()) and bool((sb["rng_step"][lanes] == 1).all()) and bool((sb["total_energy"][lanes] == 0).all())
    cg, cb = good.counters(), bad.counters()
    assert cb["env_steps"] == n and cb["noop_steps"] == len(BAD_LANES) and cg["noop_steps"] == 0 and cb["work_units"] < cg["work_units"]
    good.close()
    bad.close()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _guards(n, layout, final, nulls=()):
    g = {}
    if layout == "records":
        g["records"] = Guarded("records", (n, 14), I32, n_axis=0)        # 56-byte records as 14 words
        if final:
            g["final_obs"] = Guarded("final_obs", (n, 12), F32, n_axis=0)
    else:
        g["obs"] = Guarded("obs", (12, n), F32)
        g["reward"], g["terminated"], g["truncated"] = Guarded("reward", (n,), F32), Guarded("terminated", (n,), U8), Guarded("truncated", (n,), U8)
        if final:
            g["final_obs"] = Guarded("final_obs", (12, n), F32)
    for name, dt in (("reward_f64", F64), ("energy", F64), ("status", U8)):
        if name not in nulls:
            g[name] = Guarded(name, (n,), dt)
    return g


def _gargs(g):
    p = lambda k: _ptr(g[k].interior) if k in g else None               # noqa: E731
    return (p("records") if "records" in g else p("obs"), p("final_obs"), p("reward"), p("reward_f64"), p("energy"), p("terminated"),
            p("truncated"), p("status"))


@pytest.mark.parametrize("layout", ("soa", "records"))
@pytest.mark.parametrize("solver,n", [("rk4", 1), ("rk4", 65), ("rk4", 130), ("rk45", 130)])
def test_step_wave_write_footprint(stg, solver, n, layout):
    """Every output of stg_step_wave between sentinels: all of obs / reward / flags (or the records) and of the optional arrays that
    are given is written, final_obs exactly where an episode ended, nothing outside; values equal the plain run's; the optional
    outputs may be NULL."""
    m0, tgt, act, cur, fld = _shaped_problem(n)
    if solver == "rk45":
        act[:, 1] *= 0.25
        cur, fld = (cur[0] * 0.25, cur[1]), (fld[0] * 0.25, fld[1])
    if n > 9:
        cur[0][9, 2] = cur[0][9, 1]                                      # a lane with a bad table writes its outputs all the same
    p = [stt_default_params(volume=VOL[solver][0])]
    kw = dict(solver=solver, include_thermal_fluctuations=False, out_layout=layout, success_threshold=0.0, seed=3)
    a, w = _dev(act.T), _wave(cur, fld)
    for autoreset, nulls in ((1, ()), (0, ()), (1, ("reward_f64", "energy", "status"))):
        plain = _backend(stg, n, p, **kw)
        _start(plain, m0, tgt)
        plain.final_obs = None
        plain.step_wave(a, w, autoreset=bool(autoreset))
        torch.cuda.synchronize()
        b = _backend(stg, n, p, **kw)
        _start(b, m0, tgt)
        g = _guards(n, layout, bool(autoreset), nulls)
        rc = b.lib.stg_step_wave(b._ctx, _ptr(a), 0, autoreset, 4, _ptr(w["current"][0]), _ptr(w["current"][1]), 3, _ptr(w["field"][0]),
                                 _ptr(w["field"][1]), *_gargs(g), b._stream())
        assert rc == 0, b.lib.stg_last_error()
        torch.cuda.synchronize()
        if layout == "records":
            rec = g["records"].check().view(U8)                          # [n, 56]: every word of every record written
            _same(rec, plain.packed, ("records", autoreset))
            term, trunc = rec[:, 52], rec[:, 53]
        else:
            for k, want in (("obs", plain.obs), ("reward", plain.reward), ("terminated", plain.terminated), ("truncated", plain.truncated)):
                _same(g[k].check(), want, (k, autoreset))
            term, trunc = plain.terminated, plain.truncated
        for k, want in (("reward_f64", plain.reward64), ("energy", plain.energy), ("status", plain.status)):
            if k in g:
                _same(g[k].check(), want, (k, autoreset))
        if autoreset:
            done = (term | trunc) != 0
            if n > 9:
                assert 0 < int(done.sum()) < n
            mask = done[:, None] if layout == "records" else done[None, :]
            fo = g["final_obs"].check(written=mask)
            fo = fo.t() if layout == "records" else fo
            _same(fo[:, done], plain.final_obs[:, done].contiguous(), "final_obs")
        _same_run(_state(b), _state(plain), ("state", autoreset, nulls))
        plain.close()
        b.close()


def test_checked_errors_launch_nothing(stg):
    from spin_torque_gym_amd import _lib
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    from spin_torque_gym_amd.devices import per_env_param_block_multi
    n = 4
    m0, tgt, act, cur, fld = _shaped_problem(n)
    a = _dev(act.T)
    tk = _dev(np.tile(np.linspace(0, 1e-10, 40)[:, None], (1, n)))
    jk, hk = torch.zeros((40, n), dtype=F64, device="cuda"), torch.zeros((40, 3, n), dtype=F64, device="cuda")

    def call(b, g, a_=a, kj=0, tj=None, jk_=None, kh=0, th=None, hk_=None, obs=True):
        args = list(_gargs(g))
        if not obs:
            args[0] = None
        return b.lib.stg_step_wave(b._ctx, _ptr(a_), 0, 0, kj, _ptr(tj), _ptr(jk_), kh, _ptr(th), _ptr(hk_), *args, b._stream())

    def untouched(b, g, before):
        torch.cuda.synchronize()
        for k in g:
            g[k].check(written=False)
        _same_run(_state(b), before, "state after a refused call")
        assert b.counters()["env_steps"] == 0

    p = [stt_default_params(volume=VOL["rk4"][0])]
    # (a) bad knot counts, missing pointers
    b = _backend(stg, n, p, solver="rk4", include_thermal_fluctuations=False)
    g = _guards(n, "soa", False)
    assert call(b, g) == _lib.STG_E_STATE                                # before the first reset
    _start(b, m0, tgt)
    before = _state(b)
    for kw in (dict(kj=1, tj=tk, jk_=jk), dict(kj=33, tj=tk, jk_=jk), dict(kj=-1, tj=tk, jk_=jk), dict(kh=1, th=tk, hk_=hk), dict(kh=33, th=tk, hk_=hk),
               dict(kj=2, tj=None, jk_=jk), dict(kj=2, tj=tk, jk_=None), dict(kh=2, th=None, hk_=hk), dict(kh=2, th=tk, hk_=None),
               dict(a_=None), dict(obs=False)):
        assert call(b, g, **kw) == _lib.STG_E_INVALID, kw
        assert b.lib.stg_last_error()
    untouched(b, g, before)
    assert call(b, g, kj=32, tj=tk, jk_=jk, kh=2, th=tk, hk_=hk) == 0    # the largest table
    torch.cuda.synchronize()
    for k in g:
        g[k].check()
    b.close()
    # (b) the device-physics torque model
    b = _backend(stg, n, p, solver="rk4", include_thermal_fluctuations=False, torque_model="device")
    _start(b, m0, tgt)
    before = _state(b)
    assert call(b, g := _guards(n, "soa", False), kj=2, tj=tk, jk_=jk) == _lib.STG_E_INVALID and b"torque" in b.lib.stg_last_error()
    untouched(b, g, before)
    with pytest.raises(_lib.StgError):
        b.step_wave(a, _wave(cur, fld))
    b.close()
    # (c) per-env parameter records
    b = HipBackend(n, EnvConfig(solver="rk4", include_thermal_fluctuations=False, diagnostics=True))
    b.set_params_per_env(*per_env_param_block_multi([_flat(stg, p[0])], None, n, {"volume": np.full(n, VOL["rk4"][0])}))
    _start(b, m0, tgt)
    before = _state(b)
    assert call(b, g := _guards(n, "soa", False), kj=2, tj=tk, jk_=jk) == _lib.STG_E_STATE and b"per-env" in b.lib.stg_last_error()
    untouched(b, g, before)
    b.close()

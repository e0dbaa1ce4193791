"""The knot-amplitude entry points (stg_set_pulse_knots, stg_step_knots, stg_step_knots_ids) off their defaults, on the GPU:
`pytest -m gpu`.  tests/test_gpu_step_knots.py runs them at EnvConfig's max_current and max_duration, an amplitude limit of 1 and STT
classes; here every episode field, max_step, gamma (the RK45 constants), the temperature, the five-target list and the amplitude
limit are moved, and the class table is STT / SOT / VCMA -- the configuration and the cases of tests/test_gpu_wave_config.py
(tests/wave_config_cases.py: knots_problem, knots_ref), whose helpers this file imports.

  a. the env steps the reference recorded under shaped pulses (tests/golden/G24_wave_config.npz, the 15 rows with a current table)
     through the knot entry -- the recorded scale factors go in as the action's amplitudes -- and the recorded episodes through
     SpinTorqueVecEnv(pulse_knots=), step() and step_many();
  b. one K = 3 launch of stg_step_knots against the NumPy restatement under the tables of knots_ref.parse_np / knot_tables_np, T = 0 K,
     white and Ornstein-Uhlenbeck, every step's energy at the kernels' own start rows; obs[6] is each class's own resistance form;
  c. stg_step_knots (out_every 1 and 0) and stg_step_knots_ids (100 of 130, permuted) bit for bit K calls of stg_step_wave on
     test-built tables, per solver, noise model and layout, three void lanes among the envs;
  d. SpinTorqueVecEnv(pulse_knots=, amplitude_limit=, the class list, the configuration): step(), step_many() and step_ids() give the
     bits of the backend-level launch.

Tolerances are those of tests/test_gpu_wave_config.py (tol_for, _compare_step); tests/test_wave_config_conditioning.py shows on the CPU
that the cases of (b) move by less than tolerance / 100 per ulp of the start rows.  N = 130 (two full wavefronts and a two-lane
tail) or 1, K = 3.

Measured on an MI355X, worst |m - m_ref| (each test prints its own): the G24 rows through stg_step_knots 1.8e-15, thermal 5.1e-13,
through the envs 7.5e-13; the last of three steps of a launch against the restatement rk4 at 0 K 7.9e-14, euler white 1.3e-11, rk4 OU
1.5e-11 (bound 5e-9); energies at most 3.7e-16 relative.  profiles/NOTEBOOK.md (round 16) also says which of these tests fail when the
kernel clips against the default max_current or clamps against 1."""
import numpy as np
import pytest
import torch

from conftest import stt_default_params
from env_config_cases import backend_factory, tol_for
from knots_ref import parse_np, wave_rows
from test_gpu_wave_config import (OUT_KEYS, OUT_NAMES, SHAPED, STATE_KEYS, _backend, _compare_step, _dev, _g24_env_backend_cfg, _noise_cfg, _outs,
                                  _same, _state, _step_backend, _wave)
import wave_config_cases as wcc
import wave_step_ref

pytestmark = pytest.mark.gpu

K = wcc.K_SHAPED
VOID = ((0, 0, 0), (1, 63, 2), (1, 64, 4), (2, 64, 1))          # (step, lane, amplitude) given a NaN in the chain test


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _knots_backend(stg, c, p, **extra):
    """a context at the start state of knots problem p under its configuration and class table, the knots set"""
    b = _step_backend(stg, c, p, **extra)
    b.set_pulse_knots(p["tau"], p["limit"], p["fk"])
    return b


def _soa(acts):
    """[K,N,2+P] -> the kernel's [K,2+P,N] on the device"""
    return _dev(np.ascontiguousarray(acts.transpose(0, 2, 1)))


def _launch(b, acts, out_every=True):
    """one stg_step_knots launch: dict of OUT_KEYS with a leading [K or 1]"""
    res = b.step_knots_many(_soa(acts), out_every=out_every)
    torch.cuda.synchronize()
    f = {key: v.clone() for key, v in zip(OUT_NAMES, res)}
    f["energy"] = b.energy_many.clone()
    return f


# ------------------------------------------------------------------------------------------------
# a. G24 through the knot entries
# ------------------------------------------------------------------------------------------------
def _g24_knot_action(g, k, dtype=None):
    """[1, 2+kj]: the recorded action of env row k with the recorded scale factors as its amplitudes, in the row's dtype"""
    kj = int(g["ev_kj"][k])
    a = wcc.g24_env_action(g, k)
    a = a if dtype is None else a.astype(dtype)
    s = g["ev_scale"][k, :kj]
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s) and np.abs(s).max() <= 1.0          # float32 carries them; a limit of 1 keeps them
    return np.concatenate([a, s[None].astype(a.dtype)], axis=1)


def test_env_steps_of_g24_through_the_knot_entry(stg, golden):
    g = golden("G24_wave_config")
    rows = np.nonzero(g["ev_kj"] >= 2)[0]
    assert len(rows) == 15 and len(set(g["ev_thermal"][rows])) == 2 and len(set(g["ev_act_f64"][rows])) == 2
    worst = {False: 0.0, True: 0.0}
    for k in rows:
        kj, thermal = int(g["ev_kj"][k]), bool(g["ev_thermal"][k])
        b = _backend(stg, 1, [stt_default_params(volume=float(g["ev_volume"][k]))], env_id0=int(g["ev_env_id"]), **_g24_env_backend_cfg(g, k))
        b.reset(init_m=_dev(g["ev_m_before"][k][:, None]), target=_dev(g["ev_target"][k][:, None]))
        b.set_state(dict(m=g["ev_m_before"][k][:, None], target=g["ev_target"][k][:, None], total_energy=np.array([g["ev_etot_before"][k]]),
                         step_count=np.array([g["ev_step_before"][k]], dtype=np.int32), rng_step=np.array([g["ev_step_before"][k]], dtype=np.int32),
                         done=np.zeros(1, dtype=np.uint8)))
        _, fk = wcc.g24_shape_and_field(g, k)
        b.set_pulse_knots(g["ev_tau"][k, :kj], 1.0, fk)
        f = _launch(b, _g24_knot_action(g, k)[None])
        m = _state(b)["m"][:, 0].cpu().numpy()
        b.close()
        got = dict(m=m, obs=f["obs"][0, :, 0].cpu().numpy(), reward=float(f["reward_f64"][0, 0]), terminated=int(f["terminated"][0, 0]),
                   truncated=int(f["truncated"][0, 0]), energy=float(f["energy"][0, 0]))
        err = wcc.check_step_against_g24(g, k, got, tol_for("rk4", thermal), "stg_step_knots")
        worst[thermal] = max(worst[thermal], err)
        print(f"G24 env step {k} through stg_step_knots (episode {g['ev_episode'][k]}, thermal={thermal}, P={kj}, kh={g['ev_kh'][k]}, "
              f"T={g['ev_T'][k]:g}, f64={bool(g['ev_act_f64'][k])}): |m - m_ref| = {err:.2e}")
        assert int(f["status"][0, 0]) == 0
    print(f"G24 env steps through stg_step_knots: worst |m - m_ref| thermal off {worst[False]:.2e}, thermal on {worst[True]:.2e}")


@pytest.mark.parametrize("how", ("step", "step_many"))
def test_episodes_of_g24_through_the_vec_env_with_pulse_knots(stg, golden, how):
    """tests/test_gpu_wave_config.py: test_episodes_of_g24_through_the_vec_env with the recorded shape handed over as pulse_knots=tau and
    as amplitudes in every action.  Step j of an episode is checked on the launch of its first j + 1 steps; lane 1 is the env whose
    stream the thermal episodes were recorded on, without the thermal field both lanes are checked."""
    from spin_torque_gym_amd.physics import PiecewiseLinear
    g = golden("G24_wave_config")
    worst, seen = 0.0, 0
    for e in np.unique(g["ev_episode"]):
        ks = np.nonzero(g["ev_episode"] == e)[0]
        k0 = ks[0]
        kj = int(g["ev_kj"][k0])
        if kj < 2:
            continue
        seen += len(ks)
        thermal = bool(g["ev_thermal"][k0])
        _, fk = wcc.g24_shape_and_field(g, k0)
        cfg = wcc.g24_env_cfg(g, k0)
        max_step = cfg.pop("max_step")
        lanes = [int(g["ev_env_id"])] if thermal else [0, 1]

        def make():
            env = stg.SpinTorqueVecEnv(2, diagnostics=True, out_layout="records" if e % 2 else "soa", device_params=stt_default_params(volume=float(g["ev_volume"][k0])),
                                       include_thermal_fluctuations=thermal, solver=("rk4", "euler")[int(g["ev_solver"][k0])], seed=int(g["ev_seed"]),
                                       pulse_knots=g["ev_tau"][k0, :kj], amplitude_limit=1.0, applied_field=None if fk is None else PiecewiseLinear(*fk),
                                       backend=backend_factory(None, max_step=max_step), **cfg)
            env.reset(options={"initial_state": g["ev_m_before"][k0], "target_state": g["ev_target"][k0]})
            return env
        tol = tol_for("rk4", thermal)
        if how == "step":
            env = make()
            for k in ks:
                obs, rew, term, trunc, info = env.step(torch.from_numpy(np.repeat(_g24_knot_action(g, k), 2, axis=0)))
                torch.cuda.synchronize()
                m = env.get_state()["m"].cpu().numpy()
                for i in lanes:
                    got = dict(m=m[:, i], obs=obs[i].cpu().numpy(), reward=float(info["reward_f64"][i]), terminated=bool(term[i]),
                               truncated=bool(trunc[i]), energy=float(info["energy"][i]))
                    worst = max(worst, wcc.check_step_against_g24(g, k, got, tol, f"pulse_knots, episode {e}"))
            env.close()
            continue
        # one launch takes one action dtype: the float32 actions widened parse to the same (J, T) (checked against the file)
        acts = np.stack([np.repeat(_g24_knot_action(g, k, np.float64), 2, axis=0) for k in ks])
        for j, k in enumerate(ks):
            J, T, s = parse_np(acts[j], cfg["max_current"], cfg["max_duration"], 1.0)
            assert J[0] == g["ev_J"][k] and T[0] == g["ev_T"][k] and np.array_equal(s[0], g["ev_scale"][k, :kj])
        for j, k in enumerate(ks):
            env = make()
            obs, rew, term, trunc, info = env.step_many(torch.from_numpy(acts[:j + 1]), out_every=False)
            torch.cuda.synchronize()
            m = env.get_state()["m"].cpu().numpy()
            for i in lanes:
                got = dict(m=m[:, i], obs=obs[0, i].cpu().numpy(), reward=float(info["reward_f64"][0, i]), terminated=bool(term[0, i]),
                           truncated=bool(trunc[0, i]), energy=float(info["energy"][0, i]))
                worst = max(worst, wcc.check_step_against_g24(g, k, got, tol, f"pulse_knots, episode {e}, launch of {j + 1} steps"))
            env.close()
    assert seen == 15
    print(f"G24 episodes through SpinTorqueVecEnv(pulse_knots=).{how}: worst |m - m_ref| = {worst:.2e}")


# ------------------------------------------------------------------------------------------------
# b. one launch against the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,noise", wcc.SHAPED_DIRECT)
def test_knots_launch_vs_restatement(stg, oracle_mod, method, noise):
    """The knots twin of tests/test_gpu_wave_config.py: test_shaped_launch_vs_restatement -- one K = 3 launch of stg_step_knots against K
    steps of the restatement under the tables (tau_j T, J s_j) of the amplitudes clamped to KNOT_LIMIT.  A launch hands back the fp64
    state of its last step only, so the start rows of step k -- the energy goes with their resistance -- come from a launch of the
    first k steps on a twin context: every step's energy and the final total_energy are held to 1e-13 at the kernels' own start rows."""
    n = wcc.N
    p, refs = wcc.knots_ref(method, noise, oracle_mod)
    c = dict(method=method, noise=noise, n=n)
    thermal = noise is not None
    assert all((r["status"] == 0).all() for r in refs)
    starts = []                                                  # the kernels' own state before step k
    for k in range(K):
        twin = _knots_backend(stg, c, p)
        if k:
            twin.step_knots_many(_soa(p["acts"][:k]), out_every=False)
        starts.append(_state(twin))
        twin.close()
    e_refs = [wcc.pulse_energy(p, k, starts[k]["m"].cpu().numpy().T) for k in range(K)]
    b = _knots_backend(stg, c, p)
    f = _launch(b, p["acts"])
    st = _state(b)
    tol = tol_for(method, thermal)
    assert np.all(np.abs(e_refs[0] - refs[0]["energy"]) <= 1e-14 * np.abs(refs[0]["energy"]))       # (the reset normalises the given rows once more)
    for k in range(K):
        o = {key: f[key][k] for key in OUT_KEYS}
        e = o["energy"].cpu().numpy()
        assert np.all(np.abs(e - e_refs[k]) <= 1e-13 * np.abs(e_refs[k])), k
        for key in ("terminated", "truncated"):
            assert np.array_equal(o[key].cpu().numpy().astype(bool), refs[k][key]), (k, key)
        assert np.array_equal(o["status"].cpu().numpy(), refs[k]["status"])
        ob, ob_ref = o["obs"].cpu().numpy().T, refs[k]["obs"]
        assert np.all(np.abs(ob - ob_ref) <= wave_step_ref.F32_ULP * np.abs(ob_ref) + 2 * tol), k
        assert np.all(np.abs(o["reward_f64"].cpu().numpy() - refs[k]["reward"]) <= 1e-9 + 2 * tol), k
    _compare_step({key: f[key][K - 1] for key in OUT_KEYS}, st, refs[-1], n, tol, f"knots launch {method} {noise}, last step", e_ref=e_refs[K - 1],
                  etot_ref=starts[K - 1]["total_energy"].cpu().numpy() + e_refs[K - 1])
    assert b.counters() == {"env_steps": K * n, "work_units": int(sum(r["n_sub"].sum() for r in refs)), "noop_steps": 0}
    b.close()
    # obs[6] is each class's own resistance form at the kernels' own rows
    m_after, o6 = st["m"].cpu().numpy().T, f["obs"][K - 1][6].cpu().numpy()
    for ci, (d, t) in enumerate(zip(p["plist"], wcc.DEV_TYPES)):
        sel = p["cls"] == ci
        want = (wave_step_ref.resistance(m_after[sel], d, t) / d["resistance_parallel"]).astype(np.float32)
        assert np.all(np.abs(o6[sel] - want) <= wave_step_ref.F32_ULP * np.abs(want)), (t, np.abs(o6[sel] - want).max())
        if t == "sot_mram":                                      # (the heavy-metal line: the STT form in its place would show)
            stt_form = (wave_step_ref.resistance(m_after[sel], d, "stt_mram") / d["resistance_parallel"]).astype(np.float32)
            assert np.all(np.abs(stt_form - want) > 0.5 * np.abs(want))


# ------------------------------------------------------------------------------------------------
# c. the chain, in every solver and field
# ------------------------------------------------------------------------------------------------
def _chain_problem(solver, noise, layout):
    """the knots problem of a (solver, field, layout) pairing with the void lanes of VOID: float64 actions where the layout is records"""
    p = wcc.knots_problem(solver, noise, layout == "records", 7400 + len(solver) + len(noise or ""))
    acts = p["acts"].copy()
    for k, lane, j in VOID:
        acts[k, lane, 2 + j] = np.nan
    return wcc.with_knots(p, p["tau"], p["limit"], acts)


def _yardstick(stg, c, p, **extra):
    """K calls of stg_step_wave on tables built here (knots_ref.knot_tables_np through wave_config_cases.with_knots; the (J, T) rows
    through knots_ref.wave_rows): (per-step outputs, the state after each step, counters)"""
    n = c["n"]
    ref = _step_backend(stg, c, p, **extra)
    fld = (np.tile(p["fk"][0], (n, 1)), np.tile(p["fk"][1], (n, 1, 1)))
    steps, states = [], []
    for k in range(K):
        steps.append(_outs(ref, ref.step_wave(_dev(wave_rows(p["acts"][k]).T), _wave(p["cur"][k], fld))))
        states.append(_state(ref))
    cnt = ref.counters()
    ref.close()
    # a comparison of no-ops proves nothing: the yardstick's own run solved every env at every step
    assert all(bool((x["status"] == 0).all()) for x in steps) and cnt["work_units"] > K * n and cnt["noop_steps"] == 0
    return steps, states, cnt


@pytest.mark.parametrize("solver,noise,layout", SHAPED)
def test_knot_entries_are_k_calls_of_step_wave_bit_for_bit(stg, solver, noise, layout):
    n = wcc.N
    p = _chain_problem(solver, noise, layout)
    c = dict(method=solver, noise=noise, n=n)
    extra = dict(out_layout=layout)
    assert p["acts"].dtype == (np.float64 if layout == "records" else np.float32)
    # what a kernel at the defaults would do differently is in the inputs
    amp = np.abs(p["acts"][:, :, 2:].astype(np.float64))
    assert (amp > p["limit"]).mean() > 0.2 and (np.abs(p["acts"][:, :, 0].astype(np.float64)) > p["cfg"]["max_current"]).mean() > 0.1
    steps, states, cnt_ref = _yardstick(stg, c, p, **extra)
    for k, lane, _ in VOID:                                      # a void action: a step of no current over 1e-12 s
        assert float(steps[k]["energy"][lane]) == 0.0 and float(steps[k]["obs"][10, lane]) == 0.0
    for every in (True, False):
        b = _knots_backend(stg, c, p, **extra)
        f = _launch(b, p["acts"], out_every=every)
        assert f["obs"].shape[0] == (K if every else 1)
        for k in (range(K) if every else [K - 1]):
            for key in OUT_KEYS:
                _same(f[key][k if every else 0], steps[k][key], (solver, noise, layout, "out_every", every, "step", k, key))
        st = _state(b)
        for key in STATE_KEYS:
            _same(st[key], states[-1][key], (solver, noise, layout, "state", key))
        assert b.counters() == cnt_ref, (b.counters(), cnt_ref)
        b.close()
    # stg_step_knots_ids: 100 of the 130 envs in a permuted order take step 1 after a full step 0
    ids = np.random.default_rng(3).permutation(n)[:100]
    b = _knots_backend(stg, c, p, **extra)
    b.step_knots_many(_soa(p["acts"][:1]))
    before = _state(b)
    out = b.step_knots_ids(_dev(np.ascontiguousarray(p["acts"][1][ids].T)), _dev(ids))
    torch.cuda.synchronize()
    idt = _dev(ids)
    for key, name in (("obs", "obs"), ("reward", "reward"), ("reward_f64", "reward64"), ("terminated", "terminated"), ("truncated", "truncated"),
                      ("status", "status"), ("energy", "energy")):
        _same(out[name].contiguous(), steps[1][key][..., idt].contiguous(), (solver, noise, layout, "ids", key))
    after = _state(b)
    listed = torch.zeros(n, dtype=torch.bool, device="cuda")
    listed[idt] = True
    for key in STATE_KEYS:
        _same(after[key][..., listed], states[1][key][..., listed], (solver, noise, layout, "ids: listed envs", key))
        _same(after[key][..., ~listed], before[key][..., ~listed], (solver, noise, layout, "ids: unlisted envs", key))
    assert b.counters()["env_steps"] == n + len(ids)
    b.close()


# ------------------------------------------------------------------------------------------------
# d. the env layer under the same configuration
# ------------------------------------------------------------------------------------------------
ENV_KEYS = ("max_current", "max_duration", "success_threshold", "energy_penalty_weight", "max_steps", "temperature", "target_states")


def _env(stg, solver, noise, layout, p, start):
    """SpinTorqueVecEnv under the configuration of knots problem p -- the episode fields as keyword arguments, the solver constants
    through the backend seam (tests/env_config_cases.py) -- at the state `start` of a backend-level context"""
    from spin_torque_gym_amd.physics import PiecewiseLinear
    cfg = p["cfg"]
    over = {k: v for k, v in cfg.items() if k not in ENV_KEYS}
    assert set(over) <= {"max_step", "gamma", "rtol", "atol"} and {"max_step", "gamma"} <= set(over)
    env = stg.SpinTorqueVecEnv(wcc.N, device_type=list(wcc.DEV_TYPES), device_params=p["plist"], class_index=p["cls"], solver=solver, seed=wcc.SEED,
                               env_id0=wcc.ENV_ID0, diagnostics=True, out_layout=layout, pulse_knots=p["tau"], amplitude_limit=p["limit"],
                               applied_field=PiecewiseLinear(*p["fk"]), backend=backend_factory(None, **over), **_noise_cfg(noise),
                               **{k: cfg[k] for k in ENV_KEYS})
    env.reset(options={"initial_state": p["state"]["m"], "target_state": p["state"]["target"]})
    env.backend.set_state({k: start[k] for k in STATE_KEYS})
    return env


def _same_env_step(res, f, k, tag, cols=None):
    """the five values an env entry returns (obs [M,12] ...) against step k of a backend-level launch f, at the envs cols"""
    obs, rew, term, trunc, info = res
    pick = (lambda x: x) if cols is None else (lambda x: x[..., cols])
    for x, y, what in ((obs.t(), f["obs"][k], "obs"), (rew, f["reward"][k], "reward"), (term, f["terminated"][k].bool(), "terminated"),
                       (trunc, f["truncated"][k].bool(), "truncated"), (info["status"], f["status"][k], "status"),
                       (info["reward_f64"], f["reward_f64"][k], "reward_f64"), (info["energy"], f["energy"][k], "energy")):
        _same(x.contiguous(), pick(y).contiguous(), tag + (what,))


@pytest.mark.parametrize("solver,noise,layout", [("rk4", None, "records"), ("euler", "white", "soa"), ("rk45", "white", "soa")])
def test_env_entries_give_the_bits_of_the_backend_launch(stg, solver, noise, layout):
    """what catches a configuration field lost between the env's keyword arguments and stg_set_pulse_knots / the knot entries"""
    n = wcc.N
    p = _chain_problem(solver, noise, layout)
    c = dict(method=solver, noise=noise, n=n)
    b = _knots_backend(stg, c, p, out_layout=layout)
    start = _state(b)
    f = _launch(b, p["acts"])
    final = _state(b)
    b.close()
    assert bool((f["status"] == 0).all())
    b = _knots_backend(stg, c, p, out_layout=layout)
    b.step_knots_many(_soa(p["acts"][:2]), out_every=False)
    after2 = _state(b)
    b.close()
    acts = torch.from_numpy(p["acts"])
    # step(): K calls
    env = _env(stg, solver, noise, layout, p, start)
    for k in range(K):
        res = env.step(acts[k])
        torch.cuda.synchronize()
        _same_env_step(res, f, k, (solver, noise, "step()", k))
    st = _state(env.backend)
    for key in STATE_KEYS:
        _same(st[key], final[key], (solver, noise, "step(): state", key))
    env.close()
    # step_many(): one launch
    env = _env(stg, solver, noise, layout, p, start)
    obs, rew, term, trunc, info = env.step_many(acts)
    torch.cuda.synchronize()
    for k in range(K):
        _same_env_step((obs[k], rew[k], term[k], trunc[k], {key: info[key][k] for key in ("status", "reward_f64", "energy")}), f, k,
                       (solver, noise, "step_many()", k))
    st = _state(env.backend)
    for key in STATE_KEYS:
        _same(st[key], final[key], (solver, noise, "step_many(): state", key))
    env.close()
    # step_ids(): 100 of the 130 envs in a permuted order take step 1 after a full step 0
    ids = np.random.default_rng(3).permutation(n)[:100]
    env = _env(stg, solver, noise, layout, p, start)
    env.step(acts[0])
    before = _state(env.backend)
    res = env.step_ids(acts[1][torch.from_numpy(ids)], ids)
    torch.cuda.synchronize()
    idt = _dev(ids)
    assert res[4]["env_id"].tolist() == ids.tolist()
    _same_env_step(res, f, 1, (solver, noise, "step_ids()"), cols=idt)
    st = _state(env.backend)
    listed = torch.zeros(n, dtype=torch.bool, device="cuda")
    listed[idt] = True
    for key in STATE_KEYS:
        _same(st[key][..., listed], after2[key][..., listed], (solver, noise, "step_ids(): listed envs", key))
        _same(st[key][..., ~listed], before[key][..., ~listed], (solver, noise, "step_ids(): unlisted envs", key))
    env.close()

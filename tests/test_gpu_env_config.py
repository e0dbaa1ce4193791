"""The HIP env kernels under non-default env configuration (`pytest -m gpu`): every result-deciding field of `stg_config` besides the
solver choice -- rtol, atol, max_step, gamma, temperature, max_steps, the target list, max_current, max_duration, success_threshold,
energy_penalty_weight, noise_corr_time -- away from its default, against the CPU oracle (which tests/golden/G21_env_config.npz pins to
the reference at these settings, test_oracle_golden.py: test_g21_*) and against G21 directly.

Every case applies the non-default episode fields (env_config_cases.EPISODE: limits, threshold, weight, max_steps = 1, temperature 250 K, a
five-target list with a non-unit and an off-axis row); the cases differ in the solver constants, the temperature, the parameter path (one
class / class table / per-env records), the kernel form and the entry point (step, step_many, step_ids; float32 and float64 actions).

Sizes, the smallest that reach each kernel form: 192 envs for the step matrix (three wavefronts, two classes alternating in the class-table
runs), 256 for the forced lane-refill form (a fourth block in the queue), 8192 for the target-draw counts.  The four-wavefront workgroup
instantiations (65 536 envs and more) read the same CfgView through the same code and are deliberately left out.

Tolerances are the project's (TOL_RK4 = 1e-10, TOL_RK45 = 1e-8, x 50 with the thermal field, observations rtol 3e-7); statuses, flags, step
counts and work counters are exact.  They hold because every (configuration, input batch) used here is well conditioned, which
test_env_config_conditioning.py checks on the CPU on the same inputs (env_config_cases.matrix_cases).

Producer / consumer wavefront pairs and max_step.  A non-default max_step changes the sub-step count of the fixed-step solvers
(dt = min(max_step, T / 100)) and with it the number of thermal chunks a producer wavefront feeds its consumer.  Read in the code before
these tests first ran: the producer (stg_kernels.hpp, the `producer` branch of stg_step_kernel -> stg_physics.hpp: produce_normals) never
computes a sub-step or chunk count of its own.  It fills chunk after chunk and ends on the consumer's signal alone: in the barrier form
(RK45, Euler) on the "continues" flag the consumer writes in SharedNormalsT::chunk_end_go before the rendezvous both take once per chunk,
in the handshake-word form (RK4) on PC_STOP in hs[1].  The consumer's count comes from simple_solve's own `n` (a wave-wide ballot of
`i + 1 < n`); a wavefront whose lanes all have n = 0 (temperature = 0: every solve is rejected) walks one chunk and signals the end.
"""
import numpy as np
import pytest
import torch

import env_config_cases as ecc
from conftest import stt_default_params

pytestmark = pytest.mark.gpu

FORMS = {"pairs": dict(wave_spec=True, lane_refill=False), "inline": dict(wave_spec=False, lane_refill=False),
         "refill": dict(wave_spec=False, lane_refill=2)}            # as test_gpu_attempt_slots.py
_ORACLE = {}                                                         # case name -> the oracle's run (computed once, never changed)
_WORST = {}


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _oracle(stg, name):
    if name not in _ORACLE:
        from helpers import OracleBackend
        name_, n, seed, f64, over, kw = ecc.case(name)
        m0, tgt, acts = ecc.inputs(n, seed, f64=f64)
        _ORACLE[name] = ecc.run_steps(stg, n, m0, tgt, acts, B=OracleBackend, over=over, **kw)
    return _ORACLE[name]


def _hip(stg, name, n=None, **form):
    name_, n_case, seed, f64, over, kw = ecc.case(name)
    m0, tgt, acts = ecc.inputs(n_case, seed, f64=f64)
    rec, counters, _ = ecc.run_steps(stg, n or n_case, m0, tgt, acts, over=over, **{**kw, **form})
    return rec, counters


def _oracle_counters(ora, n, rk45):
    """The oracle's work counters over its first n envs: env steps, failed solves, and (RK45) attempts."""
    rec, counters, attempts = ora
    c = dict(env_steps=len(rec) * n, noop_steps=int(sum((r["status"][:n] == 1).sum() for r in rec)))
    if rk45:
        c["work_units"] = int(attempts[:, :n].sum())
    return c


def _check(stg, name, tag, n=None, **form):
    """One HIP run of case `name` (its first n envs) against the oracle's; returns the HIP records."""
    name_, n_case, seed, f64, over, kw = ecc.case(name)
    n = n or n_case
    ora = _oracle(stg, name)
    hip, c = _hip(stg, name, n, **form)
    rk45 = kw["solver"] == "rk45"
    tol = ecc.tol_for(kw["solver"], kw["include_thermal_fluctuations"])
    worst = ecc.compare(hip, ora[0], tol, (name, tag), cols=None if n == n_case else slice(0, n))
    want = _oracle_counters(ora, n, rk45)
    print(f"env-config {name} [{tag}, {n} envs]: worst |dm| vs oracle = {worst:.3e} (tolerance {tol:.1e}); counters {c}")
    _WORST[(kw["solver"], name)] = max(_WORST.get((kw["solver"], name), 0.0), worst)
    assert {k: c[k] for k in want} == want, (name, tag, c, want)
    return hip, c


# ------------------------------------------------------------------------------------------------------------------------------
# step matrix
# ------------------------------------------------------------------------------------------------------------------------------
RK45_CASES = [c[0] for c in ecc.matrix_cases() if c[0].startswith("rk45-s")]
FIXED_CASES = [c[0] for c in ecc.matrix_cases() if c[0].split("-")[0] in ("rk4", "euler") and c[0].split("-")[1].startswith(("ms", "ou", "device"))]


@pytest.mark.parametrize("name", RK45_CASES)
def test_rk45_controller_constants_in_every_loop_form_vs_oracle(stg, name):
    """rtol, atol, max_step and gamma of the four G21 settings in the RK45 attempt loop: T = 0 K in the inline and lane-refill forms, thermal in
    the pair, inline and lane-refill forms.  State, outputs, flags and the work counters (env steps, attempts, failed solves) against the
    oracle; the forms among themselves bit for bit."""
    thermal = ecc.case(name)[5]["include_thermal_fluctuations"]
    runs = {}
    for form in (("pairs", "inline", "refill") if thermal else ("inline", "refill")):
        n = ecc.N_REFILL if form == "refill" else ecc.N_MATRIX
        runs[form], _ = _check(stg, name, form, n=n, **FORMS[form])
    first = [{k: (v[:ecc.N_MATRIX] if k == "obs" else v[..., :ecc.N_MATRIX]) for k, v in r.items()} for r in runs["refill"]]
    for form in runs:
        if form != "refill":
            ecc.same_bits(runs[form], first, (name, form, "refill"))


@pytest.mark.parametrize("name", FIXED_CASES)
def test_fixed_step_max_step_and_gamma_vs_oracle(stg, name):
    """max_step in {2.5e-12, 3e-13, 1e-10} (120, 1000 and 100 sub-steps for a 0.3 ns pulse) with gamma = 1.9e5 in the RK4 and Euler kernels,
    one class and a class table; the Ornstein-Uhlenbeck field with correlation_time = 7e-13; the device-physics torque model on a mixed
    STT / SOT / VCMA table.  Thermal: both wave_spec values, bit-identical."""
    thermal = ecc.case(name)[5]["include_thermal_fluctuations"]
    if not thermal:
        _check(stg, name, "one wavefront")
        return
    a, ca = _check(stg, name, "pairs", wave_spec=True)
    b, cb = _hip(stg, name, wave_spec=False)
    ecc.same_bits(a, b, (name, "wave_spec on / off"))
    assert ca == cb, (name, ca, cb)


@pytest.mark.parametrize("solver", ["rk45", "rk4", "euler"])
@pytest.mark.parametrize("temperature", [0.0, 77.0, 450.0])
def test_temperature_vs_oracle(stg, solver, temperature, oracle_mod):
    """temperature = 0 with the thermal field on: RobustLLGSSolver's input validation rejects every solve, so every fixed-step step is a no-op
    with status 1 (golden tag temperature_zero_noop on the CPU side), while RK45 integrates with a zero field.  77 K and 450 K: the Brown
    strengths of both classes equal the oracle's under the non-default gamma, and the steps agree."""
    name = f"{solver}-temperature{temperature:g}"
    name_, n, seed, f64, over, kw = ecc.case(name)
    a, ca = _check(stg, name, "pairs", wave_spec=True)
    b, cb = _hip(stg, name, wave_spec=False)
    ecc.same_bits(a, b, (name, "wave_spec on / off"))
    assert ca == cb
    m0, tgt, acts = ecc.inputs(n, seed)
    if temperature == 0.0 and solver != "rk45":
        assert ca["noop_steps"] == 2 * n
        for rec in a:
            assert (rec["status"] == 1).all() and np.abs(rec["m"] - m0.T).max() <= 4e-16       # (reset normalises the unit rows once more)
            assert np.array_equal(rec["m"], a[0]["m"]) and rec["trunc"].all() and (rec["energy"] > 0).any()
    else:
        assert ca["noop_steps"] == 0 and (a[0]["status"] == 0).all()
    env = ecc.make_env(stg, 64, None, over, **kw)
    for cls, (dev, d) in enumerate(zip(kw["device_type"], kw["device_params"])):
        want = oracle_mod.thermal_strength(oracle_mod.make_params(d, dev), over["gamma"], temperature, 1 if solver == "rk45" else 0)
        got = env.backend.thermal_strength(cls)
        assert np.isclose(got, want, rtol=1e-15, atol=0) and (got > 0) == (temperature > 0), (name, cls, got, want)
    env.close()


def test_episode_fields_change_what_a_default_configuration_gives(stg):
    """The non-default limits, threshold, weight, max_steps, temperature and target list are not a no-op: against a run of the same inputs under
    the default configuration (targets +-z), observation components 3-5, 7, 8, 10 and 11, the reward and both flags differ."""
    name = "rk4-ms2.5e-12-T0-one"
    name_, n, seed, f64, over, kw = ecc.case(name)
    hip, _ = _hip(stg, name)
    m0, tgt, acts = ecc.inputs(n, seed)
    env = stg.SpinTorqueVecEnv(n, diagnostics=True, **kw)
    env.reset(options={"initial_state": m0, "target_state": np.where(np.arange(n)[:, None] % 2 == 0, 1.0, -1.0) * np.array([[0.0, 0.0, 1.0]])})
    dflt = [ecc.snapshot(env, *env.step(torch.from_numpy(a))) for a in acts]
    env.close()
    h, d = hip[0], dflt[0]
    for comp in (3, 4, 5, 7, 8, 10, 11):
        assert (h["obs"][:, comp] != d["obs"][:, comp]).any(), comp
    assert (h["obs"][:, 7] == np.float32(250.0 / 300.0)).all() and (h["obs"][:, 8] == 0.0).all()
    assert (h["reward"] != d["reward"]).any() and (h["term"] != d["term"]).any()
    assert h["trunc"].all() and not d["trunc"].any()


@pytest.mark.parametrize("name", ["rk45-s1-T0-table", "rk45-temperature77", "rk4-ms2.5e-12-T0-table", "rk4-temperature450",
                                  "euler-ms2.5e-12-thermal-table", "euler-temperature77"])
def test_per_env_records_equal_the_class_table_bit_for_bit(stg, name):
    """stg_set_params_per_env with every env's record holding its class's values: the lane derives its constants from the per-env copy of
    gamma and temperature (a.ep), the class-table path from the host's.  Non-default gamma and temperature: identical bits."""
    name_, n_case, seed, f64, over, kw = ecc.case(name)
    n = ecc.N_MATRIX
    m0, tgt, acts = ecc.inputs(n_case, seed)
    table, ct = _hip(stg, name, n)
    per_env_kw = {**kw, **ecc.device_kwargs(kw["solver"], "per_env")}
    per_env, cp, _ = ecc.run_steps(stg, n, m0, tgt, acts, over=over, **per_env_kw)
    ecc.same_bits(table, per_env, (name, "class table / per-env records"))
    assert ct == cp, (name, ct, cp)
    assert over["gamma"] != 2.21e5 and {**ecc.EPISODE, **kw}["temperature"] != 300.0


# ------------------------------------------------------------------------------------------------------------------------------
# entry points: step_many, step_ids, both output layouts; float32 and float64 actions
# ------------------------------------------------------------------------------------------------------------------------------
def _cpu(t):
    return torch.as_tensor(t).cpu().numpy().copy()


def _entry_points(stg, name):
    from helpers import OracleBackend
    name_, n_case, seed, f64, over, kw = ecc.case(name)
    n, solver = ecc.N_MATRIX, kw["solver"]
    tol = ecc.tol_for(solver, kw["include_thermal_fluctuations"])
    m0, tgt, acts = ecc.inputs(n_case, seed, f64=f64)
    m0, tgt, acts = m0[:n], tgt[:n], acts[:, :n]
    ora = _oracle(stg, name)[0]
    # both output layouts (the env's default is 'records'): the same bits
    rec, _ = _hip(stg, name, n)
    soa, _ = _hip(stg, name, n, out_layout="soa")
    ecc.same_bits(rec, soa, (name, "records / soa"))
    # step_ids: 100 of the 192 ids, shuffled; outputs in list order, against the oracle's full step
    ids = np.random.default_rng(5).permutation(n)[:ecc.N_IDS]
    env = ecc.make_env(stg, n, None, over, **kw)
    env.reset(options={"initial_state": m0, "target_state": tgt})
    sub = []
    for a in acts:
        o, r, te, tr, info = env.step_ids(torch.from_numpy(a[ids]), ids)
        assert np.array_equal(_cpu(info["env_id"]), ids)
        st = env.get_state()
        sub.append(dict(obs=_cpu(o), reward=_cpu(info["reward_f64"]), energy=_cpu(info["energy"]), term=_cpu(te), trunc=_cpu(tr),
                        status=_cpu(info["status"]), m=_cpu(st["m"])[:, ids], target=_cpu(st["target"])[:, ids],
                        step_count=_cpu(st["step_count"])[ids]))
    rest = np.setdiff1d(np.arange(n), ids)
    assert np.abs(_cpu(env.get_state()["m"])[:, rest] - m0.T[:, rest]).max() <= 4e-16 and (_cpu(env.get_state()["step_count"])[rest] == 0).all()
    env.close()
    worst = ecc.compare(sub, ora, tol, (name, "step_ids"), cols=ids)
    # step_many(K = 3, autoreset) with max_steps = 1: every env ends and redraws at every step.  Step 0 is the step above: terminal
    # observation, reward, energy tight.  Later steps start from states redrawn from fp32 device normals (1e-7 from libm's): loose, but the
    # redrawn targets are table rows, bit for bit, and flags / statuses exact.
    acts3 = np.concatenate([acts, acts[:1]])
    many = []
    for B in (None, OracleBackend):
        env = ecc.make_env(stg, n, B, over, autoreset=True, **kw)
        env.reset(options={"initial_state": m0, "target_state": tgt})
        o, r, te, tr, info = env.step_many(torch.from_numpy(acts3))
        st = env.get_state()
        many.append(dict(obs=_cpu(o), reward=_cpu(info["reward_f64"]), energy=_cpu(info["energy"]), term=_cpu(te), trunc=_cpu(tr),
                         status=_cpu(info["status"]), final_obs=_cpu(info["final_obs"]), m=_cpu(st["m"]), target=_cpu(st["target"]),
                         step_count=_cpu(st["step_count"])))
        env.close()
    h, o = many
    assert h["obs"].shape == (3, n, 12) and h["trunc"].all() and (h["step_count"] == 0).all()
    for key in ("status", "trunc", "step_count", "target"):
        assert np.array_equal(h[key], o[key]), (name, "step_many", key)
    # (success flags of the later steps: where the oracle's terminal alignment is not within 1e-4 of the threshold -- the redrawn start rows
    # differ by 1e-7 -- and everywhere at step 0)
    align = (o["final_obs"][:, :, :3].astype(np.float64) * o["final_obs"][:, :, 3:6]).sum(axis=2)
    clear = np.abs(align - ecc.EPISODE["success_threshold"]) > 1e-4
    clear[0] = True
    assert np.array_equal(h["term"][clear], o["term"][clear]) and clear.mean() > 0.99, (name, "step_many", "term")
    assert np.array_equal(h["obs"][:, :, 3:6], o["obs"][:, :, 3:6])                       # the redrawn targets, as float32
    assert np.allclose(h["final_obs"][0], o["final_obs"][0], rtol=3e-7, atol=max(1e-12, 10 * tol)), (name, "step_many: terminal observation")
    assert np.allclose(h["final_obs"][0], ora[0]["obs"][:n], rtol=3e-7, atol=max(1e-12, 10 * tol))   # ... which is the plain step's observation
    assert np.allclose(h["reward"][0], o["reward"][0], rtol=1e-10, atol=max(1e-12, 10 * tol)), (name, "step_many: reward")
    assert np.allclose(h["energy"][0], o["energy"][0], rtol=max(1e-12, 10 * tol), atol=0)
    assert np.abs(h["obs"][:, :, :3] - o["obs"][:, :, :3]).max() < 2e-6 and np.abs(h["m"] - o["m"]).max() < 2e-6      # fresh draws
    assert np.allclose(h["final_obs"][1:], o["final_obs"][1:], rtol=1e-3, atol=1e-3)
    assert len({tuple(t) for t in h["target"].T}) == 5                                       # all five targets are drawn
    print(f"env-config {name} [entry points]: step_ids worst |dm| vs oracle = {worst:.3e} (tolerance {tol:.1e})")
    _WORST[(solver, name + " step_ids")] = worst


@pytest.mark.parametrize("name", ["rk45-s1-thermal-table", "rk4-ms3e-13-thermal-table", "euler-ms1e-10-thermal-table"])
def test_entry_points_and_layouts_float32(stg, name):
    _entry_points(stg, name)


@pytest.mark.parametrize("solver", ["rk45", "rk4", "euler"])
def test_float64_actions_random_batch_vs_oracle(stg, solver):
    """The AT = double instantiations on values float32 cannot carry (and, for a quarter of them, beyond max_current): step, step_many and
    step_ids against the oracle's float64 entry.  The same values rounded to float32 give other results."""
    name = f"{solver}-float64"
    hip, _ = _check(stg, name, "step, float64 actions")
    _entry_points(stg, name)
    name_, n, seed, f64, over, kw = ecc.case(name)
    m0, tgt, acts = ecc.inputs(n, seed, f64=True)
    f32, _, _ = ecc.run_steps(stg, n, m0, tgt, acts.astype(np.float32), over=over, **kw)
    # (float32 moves T by <= 6e-8 relative: |dm| <= gamma' H_k T x 6e-8 ~ 5e11 / s x 0.3 ns x 6e-8 ~ 1e-5 for the typical env; a few RK4 / Euler
    # envs change their sub-step count with it)
    d = np.abs(hip[0]["m"] - f32[0]["m"]).max(axis=0)
    assert (d > 0).sum() > n // 2 and np.median(d) < 1e-5, (name, np.median(d))


def test_float64_and_target_list_episodes_vs_golden_g21(stg, golden):
    """The five G21 episodes through the SpinTorqueEnv facade: 5 / 1 / 8 target_states with non-default threshold, weight, limits and
    temperature, two of them stepped with float64 action arrays beyond the env's limits and the safety wrapper's.  Tolerances of
    test_gpu_parity.py: test_env_episodes_vs_golden_g6."""
    from test_oracle_golden import G21_EPISODE_CFG
    g = golden("G21_env_config")
    for k, tag in enumerate(str(t) for t in g["episode_tags"]):
        env = stg.SpinTorqueEnv(device_params=stt_default_params(volume=float(g[f"ep{k}_volume"])), include_thermal_fluctuations=False,
                                target_states=list(g[f"ep{k}_target_states"]), **G21_EPISODE_CFG[tag])
        assert np.abs(np.array(env.target_states) - g[f"ep{k}_target_states"]).max() <= 2e-16
        obs0, _ = env.reset(seed=0, options={"initial_state": g[f"ep{k}_m0"], "target_state": g[f"ep{k}_target"]})
        assert np.allclose(obs0, g[f"ep{k}_obs"][0], rtol=2e-7, atol=1e-12), tag
        acts = g[f"ep{k}_actions"]
        assert (acts.dtype == np.float64) == tag.startswith("float64")
        for j, a in enumerate(acts):
            obs, r, te, tr, info = env.step(a.copy())
            assert "error" not in info, (tag, j, info)
            assert np.allclose(obs, g[f"ep{k}_obs"][j + 1], rtol=2e-7, atol=1e-12), (tag, j, obs, g[f"ep{k}_obs"][j + 1])
            rr = g[f"ep{k}_reward"][j]
            assert abs(r - rr) <= 1e-10 * max(1.0, abs(rr)), (tag, j, r, rr)
            assert te == bool(g[f"ep{k}_terminated"][j]) and tr == bool(g[f"ep{k}_truncated"][j]), (tag, j)
            assert info["simulation_success"] == bool(g[f"ep{k}_success"][j]), (tag, j)
            re_ = g[f"ep{k}_energy"][j]
            assert abs(info["energy_consumed"] - re_) <= 1e-12 * max(abs(re_), 1e-300), (tag, j)
            assert np.abs(env.current_magnetization - g[f"ep{k}_m"][j + 1]).max() <= ecc.TOL_RK4, (tag, j)
        env.close()


def test_rk45_solve_api_vs_golden_g21_and_oracle(stg, golden):
    """LLGSSolver at the four G21 settings through the solve API: accepted points, times and states against the recorded reference and
    against the oracle (tolerances of test_gpu_parity.py: test_rk45_solver_vs_golden)."""
    from helpers import OracleBackend
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    g = golden("G21_env_config")
    rows = g["llgs_cases"]
    table = [stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", stt_default_params(volume=float(g["llgs_volume"]))))]
    for s in sorted(set(rows[:, 0].astype(int))):
        sel = rows[rows[:, 0] == s]
        rtol, atol, max_step, gamma = sel[0, 1:5]
        assert dict(rtol=rtol, atol=atol, max_step=max_step, gamma=gamma) == ecc.RK45_SETTINGS[s]
        cap = max(len(g[f"llgs_t_{s}_{k}"]) for k in range(len(sel))) + 8
        res = []
        for B in (HipBackend, OracleBackend):
            b = B(len(sel), EnvConfig(diagnostics=True, solver="rk45", include_thermal_fluctuations=False, rtol=rtol, atol=atol, max_step=max_step,
                                      gamma=gamma))
            b.set_params(table, None)
            out = b.solve(torch.tensor(sel[:, 5:8].T.copy()), torch.tensor(sel[:, 8].copy()), torch.tensor(sel[:, 9].copy()), traj_cap=cap)
            res.append({key: _cpu(out[key]) for key in ("m_final", "n_points", "success", "t", "m")})
            b.close()
        h, o = res
        assert np.array_equal(h["n_points"], o["n_points"]) and np.array_equal(h["success"], o["success"])
        for k in range(len(sel)):
            rt, rm = g[f"llgs_t_{s}_{k}"], g[f"llgs_m_{s}_{k}"]
            kk = len(rt)
            assert bool(h["success"][k]) == bool(sel[k, 10]) and int(h["n_points"][k]) == kk - 1, (s, k, int(h["n_points"][k]), kk - 1)
            assert np.abs(h["t"][:kk, k] - rt).max() <= 1e-9 * rt[-1]
            d = np.abs(h["m"][:kk, :, k] - rm).max()
            assert d <= ecc.TOL_RK45 and np.abs(h["m_final"][:, k] - rm[-1]).max() <= ecc.TOL_RK45, (s, k, d)
            assert np.abs(h["m"][:kk, :, k] - o["m"][:kk, :, k]).max() <= ecc.TOL_RK45 and np.abs(h["t"][:kk, k] - o["t"][:kk, k]).max() <= 1e-9 * rt[-1]
            _WORST[("rk45", f"solve API setting {s}")] = max(_WORST.get(("rk45", f"solve API setting {s}"), 0.0), float(d))
        print(f"env-config solve API, setting {s} {ecc.RK45_SETTINGS[s]}: worst |dm| vs G21 = {_WORST[('rk45', f'solve API setting {s}')]:.3e}")


# ------------------------------------------------------------------------------------------------------------------------------
# target selection: a per-lane dynamic index into the kernel-argument target table
# ------------------------------------------------------------------------------------------------------------------------------
TARGETS8 = ecc.unit_targets([[1.0, 2.0, 2.0], [2.0, -1.0, 2.0], [-2.0, 2.0, 1.0], [0.6, 0.0, -0.8], [0.0, -0.28, 0.96], [3.0, 4.0, 12.0],
                             [-1.0, -1.0, -1.0], [0.36, 0.48, -0.8]])
DRAW_SEED, DRAW_N = 77, 8192


@pytest.mark.parametrize("n_targets", [1, 3, 5, 8])
def test_target_draws_are_the_rows_the_oracle_names(stg, n_targets):
    """reset without a target_state, then step_many(K = 2) with autoreset and max_steps = 1 (every env redraws at every step): each env's target
    -- in the state and as observation components 3-5 -- is bit for bit the row helpers.device_reset_draw names for (seed, env id, stream
    position), and over 8192 envs every row's count lies within 4 sigma of N / n (the oracle alone, seed 77, position 0: 1.6 sigma at most)."""
    from helpers import device_reset_draw
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    n, K = DRAW_N, 2
    targets = TARGETS8[:n_targets]
    assert len({tuple(np.float32(t)) for t in targets}) == n_targets and (np.abs(targets) < 0.999).all()
    cfg = EnvConfig(solver="rk4", include_thermal_fluctuations=False, target_states=[list(t) for t in targets], max_steps=1, seed=DRAW_SEED,
                    diagnostics=True, **{k: v for k, v in ecc.EPISODE.items() if k not in ("max_steps", "target_states")})
    b = HipBackend(n, cfg)
    b.set_params([stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", stt_default_params(volume=8.75e-11)))])
    obs = _cpu(b.reset(None, None, None, DRAW_SEED))                # [12, n]
    st = {k: _cpu(v) for k, v in b.get_state().items()}

    def expect(seed, pos):
        return np.array([device_reset_draw(seed, i, pos, targets)[1] for i in range(n)])       # [n, 3]

    def check(tgt, obs_tgt, want, tag):
        assert tgt is None or np.array_equal(tgt, want.T), (n_targets, tag, "state")
        assert np.array_equal(obs_tgt, want.T.astype(np.float32)), (n_targets, tag, "observation")
        idx = np.array([int(np.flatnonzero((targets == row).all(axis=1))[0]) for row in want])
        counts = np.bincount(idx, minlength=n_targets)
        sigma = np.sqrt(n * (1.0 / n_targets) * (1.0 - 1.0 / n_targets))
        dev = np.abs(counts - n / n_targets).max() / sigma if n_targets > 1 else 0.0
        print(f"target draws n = {n_targets} ({tag}): counts {counts.tolist()}, largest deviation {dev:.2f} sigma")
        assert counts.sum() == n and dev <= 4.0, (n_targets, tag, counts)

    check(st["target"], obs[3:6], expect(DRAW_SEED, 0), "reset")
    rng = np.random.default_rng(3)
    a = np.empty((K, 2, n), dtype=np.float32)
    a[:, 0] = rng.uniform(-2e6, 2e6, (K, n))
    a[:, 1] = rng.uniform(1e-12, 5e-11, (K, n))
    o, r, r64, te, tr, status = b.step_many(torch.from_numpy(a), out_every=True, autoreset=True)
    o = _cpu(o)                                                     # [K, 12, n]
    assert _cpu(tr).all()
    for k in range(K):       # the redraw after step k reads the env's stream at position k + 1, keyed with the configuration's seed
        check(_cpu(b.get_state()["target"]) if k == K - 1 else None, o[k, 3:6], expect(DRAW_SEED, k + 1), f"redraw {k}")
    b.close()


def test_zz_worst_differences_summary():
    """(prints what the tests above measured, per solver and configuration)"""
    for (solver, name), d in sorted(_WORST.items()):
        print(f"env-config worst |dm| {solver:5s} {name}: {d:.3e}")

"""Configurations, input batches and the runner shared by test_gpu_env_config.py (HIP kernels against the oracle, `-m gpu`) and
test_env_config_conditioning.py (the oracle against itself, CPU): one definition, so that the conditioning test sees exactly the
inputs the GPU tests use.

`stg_config` carries the solver constants (rtol, atol, max_step, gamma), the temperature and the episode fields (limits, threshold,
weight, max_steps, target list).  SpinTorqueVecEnv takes the episode fields as keyword arguments; the solver constants reach the
backends through `backend_factory`, which rewrites the EnvConfig the env hands to its backend -- the HIP one and the oracle alike.
"""
import dataclasses

import numpy as np
import torch

from conftest import sot_default_params, stt_default_params, vcma_default_params

TOL_RK4 = 1e-10
TOL_RK45 = 1e-8
THERMAL_FACTOR = 50          # test_gpu_parity.py: test_randomised_configurations_vs_oracle (the normals carry fp32 device transcendentals)

# distinguishable targets, one non-unit and one off-axis among them (the G21 list); the env normalises them
TARGETS5 = [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.6, 0.0, 0.8], [0.0, -2.0, 0.0], [1.0, 1.0, 1.0]]
# every episode field away from its default, in every case (temperature: overridden by the temperature cases)
EPISODE = dict(max_current=1.5e6, max_duration=2e-9, success_threshold=0.6, energy_penalty_weight=0.25, max_steps=1,
               temperature=250.0, target_states=TARGETS5)
# (rtol, atol, max_step, gamma) of LLGSSolver: the four G21 settings
RK45_SETTINGS = [dict(rtol=1e-4, atol=1e-7, max_step=5e-12, gamma=2.21e5), dict(rtol=1e-8, atol=1e-11, max_step=2e-13, gamma=1.9e5),
                 dict(rtol=1e-3, atol=1e-6, max_step=1e-11, gamma=2.5e5), dict(rtol=1e-5, atol=0.0, max_step=1e-9, gamma=2.21e5)]
FIXED_MAX_STEPS = (2.5e-12, 3e-13, 1e-10)
VOLUME = {"rk45": 9.7e-6, "rk4": 8.75e-11, "euler": 8.75e-11}
N_MATRIX, N_REFILL, N_IDS = 192, 256, 100


def tol_for(solver, thermal):
    return (TOL_RK45 if solver == "rk45" else TOL_RK4) * (THERMAL_FACTOR if thermal else 1)


def unit_targets(rows):
    t = np.asarray(rows, dtype=np.float64)
    return t / np.linalg.norm(t, axis=1, keepdims=True)


def inputs(n, seed, steps=2, f64=False):
    """Random unit rows, explicit targets cycling through the five-target list, J ~ U[-2e6, 2e6] (a quarter beyond max_current),
    T ~ U[1 ps, 0.3 ns].  float32 actions, or float64 values that float32 cannot carry."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (n, 3))
    m0 = v / np.linalg.norm(v, axis=1, keepdims=True)
    tgt = unit_targets(TARGETS5)[np.arange(n) % 5]
    acts = np.empty((steps, n, 2), dtype=np.float64)
    acts[..., 0] = rng.uniform(-2e6, 2e6, (steps, n))
    acts[..., 1] = rng.uniform(1e-12, 3e-10, (steps, n))
    if f64:
        assert np.all(acts.astype(np.float32).astype(np.float64) != acts)
        return m0, tgt, acts
    return m0, tgt, acts.astype(np.float32)


def device_kwargs(solver, params):
    """'one': one class.  'table': two classes alternating (STT, VCMA).  'per_env': the same two classes, every env with a record of its
    own that holds its class's values.  'mixed_device': STT / SOT / VCMA with the device-physics torque model."""
    vol = VOLUME[solver]
    if params == "one":
        return dict(device_params=stt_default_params(volume=vol))
    if params == "mixed_device":
        return dict(device_type=["stt_mram", "sot_mram", "vcma_mram"], torque_model="device",
                    device_params=[stt_default_params(volume=vol), sot_default_params(polarization=0.7, volume=vol),
                                   vcma_default_params(polarization=0.7, volume=vol)])
    table = [stt_default_params(volume=vol), vcma_default_params(polarization=0.6, volume=vol * 0.8)]
    kw = dict(device_type=["stt_mram", "vcma_mram"], device_params=table)
    if params == "per_env":
        kw["per_env_params"] = "damping"          # (filled in by class_kwargs, which knows the batch size)
    else:
        assert params == "table"
    return kw


def class_kwargs(kw, n):
    """The per-batch-size parts of device_kwargs: the class index, and the per-env values equal to the class table's."""
    kw = dict(kw)
    k = len(kw["device_type"]) if isinstance(kw.get("device_type"), list) else 1
    if k > 1:
        cls = (np.arange(n) % k).astype(np.uint8)
        kw["class_index"] = cls
        if kw.get("per_env_params") == "damping":
            kw["per_env_params"] = {"damping": np.array([kw["device_params"][c]["damping"] for c in cls], dtype=np.float64)}
    return kw


def backend_factory(B=None, **over):
    """A backend constructor that builds backend class `B` (None: the HIP backend) on the env's EnvConfig with `over` written over it."""
    def make(n, cfg, device_index=0, env_id0=0):
        cls = B
        if cls is None:
            from spin_torque_gym_amd.backend import HipBackend
            cls = HipBackend
        return cls(n, dataclasses.replace(cfg, **over), device_index, env_id0)
    return make


def parsed_actions(b, a):
    """What the oracle's action parser makes of actions `a` [n,2] (float32 or float64) under oracle backend `b`'s configuration."""
    import oracle
    parse = oracle.parse_action_f64 if a.dtype == np.float64 else oracle.parse_action
    return [parse(a[i], b.ocfg) for i in range(b.n)]


def oracle_attempts(b, a):
    """RK45 attempts per env of the step oracle backend `b` is about to take with actions `a` [n,2]: the oracle's solver on each env's
    own state row, parsed action, class and stream position (test_gpu_attempt_slots.py: _oracle_attempts, with class tables)."""
    import oracle
    out = np.zeros(b.n, dtype=np.int64)
    for i, (J, T) in enumerate(parsed_actions(b, a)):
        s = b.states[i]
        r = oracle.llgs_solve(np.array([s.m[0], s.m[1], s.m[2]]), T, b._p(i), b.ocfg, J, env_id=b.env_id0 + i, env_step=int(s.rng_step), cap=4)
        out[i] = r["n_attempts"]
    return out


def make_env(stg, n, B=None, over=None, **kw):
    kw = class_kwargs({**EPISODE, **kw}, n)
    return stg.SpinTorqueVecEnv(n, diagnostics=True, backend=backend_factory(B, **(over or {})), **kw)


def snapshot(env, o, r, te, tr, info):
    st = env.get_state()
    cpu = lambda t: torch.as_tensor(t).cpu().numpy().copy()
    return dict(obs=cpu(o), reward=cpu(info["reward_f64"]), energy=cpu(info["energy"]), term=cpu(te), trunc=cpu(tr), status=cpu(info["status"]),
                m=cpu(st["m"]), target=cpu(st["target"]), step_count=cpu(st["step_count"]), reward32=cpu(r))


def run_steps(stg, n, m0, tgt, acts, B=None, over=None, ulp=False, **kw):
    """Resets to (m0, tgt) and steps through `acts` [steps,n,2].  Returns the per-step snapshots and the work counters; with an oracle RK45
    backend also `attempts` [steps,n] (and the counters' work_units are their sum, as the HIP library counts attempts).
    `ulp`: the largest component of every start row is moved by one ulp after the reset (the conditioning test)."""
    env = make_env(stg, n, B, over, **kw)
    env.reset(options={"initial_state": m0[:n], "target_state": tgt[:n]})
    if ulp:
        st = {k: torch.as_tensor(v).clone() for k, v in env.get_state().items()}
        m = st["m"].numpy()
        big = np.abs(m).argmax(axis=0)
        cols = np.arange(n)
        m[big, cols] = np.nextafter(m[big, cols], np.inf)
        env.backend.set_state(st)
    rec, attempts = [], []
    count = B is not None and kw.get("solver") == "rk45"
    for a in acts:
        a = a[:n]
        if count:
            attempts.append(oracle_attempts(env.backend, a))
        rec.append(snapshot(env, *env.step(torch.from_numpy(a))))
    counters = env.backend.counters()
    if count:
        counters["accepted_points"] = counters["work_units"]       # (what the oracle's env step reports as its work)
        counters["work_units"] = int(np.sum(attempts))
    env.close()
    return rec, counters, np.array(attempts)


def compare(hip, ora, tol_m, tag, cols=None):
    """Statuses, flags and step counts exactly; state within tol_m; observations, rewards and energies as test_gpu_parity.py: _compare.
    `cols`: the envs of the oracle run that the HIP records hold, in their order (None: the same envs).  Returns the worst |dm|."""
    worst = 0.0
    for k, (h, full) in enumerate(zip(hip, ora)):
        # (observations are [n,12], everything else has the env index last)
        o = full if cols is None else {key: (v[cols] if key == "obs" else v[..., cols]) for key, v in full.items()}
        for key in ("status", "term", "trunc"):
            assert np.array_equal(h[key], o[key]), (tag, k, key, np.flatnonzero(h[key] != o[key]))
        if "step_count" in h:
            assert np.array_equal(h["step_count"], o["step_count"]), (tag, k)
        if "m" in h:
            # (an explicit target_state is normalised on the device with a fused sum of squares: an ulp or two from the host's)
            assert np.abs(h["target"] - o["target"]).max() <= 5e-16, (tag, k, "target")
            d = float(np.abs(h["m"] - o["m"]).max())
            worst = max(worst, d)
            assert d <= tol_m, (tag, k, d)
        assert np.allclose(h["obs"], o["obs"], rtol=3e-7, atol=max(1e-12, 10 * tol_m)), (tag, k, "obs")
        assert np.allclose(h["reward"], o["reward"], rtol=1e-10, atol=max(1e-12, 10 * tol_m)), (tag, k, "reward")
        assert np.allclose(h["energy"], o["energy"], rtol=max(1e-12, 10 * tol_m), atol=0), (tag, k, "energy")
    return worst


def same_bits(a, b, tag):
    for k, (x, y) in enumerate(zip(a, b)):
        for key in x:
            assert np.array_equal(x[key].view(np.uint8), y[key].view(np.uint8)), (tag, k, key)


# ---------------------------------------------------------------------------------------------------------------------
# the (configuration, input batch) pairs of the step matrix; test_gpu_env_config.py runs each on the HIP kernels and the oracle, the
# conditioning test runs each twice on the oracle
# ---------------------------------------------------------------------------------------------------------------------
def matrix_cases():
    """-> [(name, n, seed, f64, over, kw)]: `over` the solver constants, `kw` the env's keyword arguments (without the kernel-form
    options, which do not change results)."""
    cases = []
    for s, over in enumerate(RK45_SETTINGS):
        for thermal in (False, True):
            for params in (("one", "table") if s == 1 else ("one",)):
                cases.append((f"rk45-s{s}-{'thermal' if thermal else 'T0'}-{params}", N_REFILL, 2100 + s, False, over,
                              dict(solver="rk45", include_thermal_fluctuations=thermal, seed=77, **device_kwargs("rk45", params))))
    for solver in ("rk4", "euler"):
        for j, ms in enumerate(FIXED_MAX_STEPS):
            for thermal in (False, True):
                for params in (("one", "table") if j == 0 else ("table",)):
                    cases.append((f"{solver}-ms{ms:g}-{'thermal' if thermal else 'T0'}-{params}", N_MATRIX, 2200 + j, False,
                                  dict(max_step=ms, gamma=1.9e5),
                                  dict(solver=solver, include_thermal_fluctuations=thermal, seed=78, **device_kwargs(solver, params))))
        cases.append((f"{solver}-ou", N_MATRIX, 2300, False, dict(max_step=2.5e-12, gamma=1.9e5),
                      dict(solver=solver, include_thermal_fluctuations=True, seed=79, noise_model="ou", correlation_time=7e-13,
                           **device_kwargs(solver, "one"))))
        cases.append((f"{solver}-device-torque", N_MATRIX, 2301, False, dict(max_step=2.5e-12, gamma=1.9e5),
                      dict(solver=solver, include_thermal_fluctuations=False, seed=80, **device_kwargs(solver, "mixed_device"))))
    for solver in ("rk45", "rk4", "euler"):
        over = RK45_SETTINGS[2] if solver == "rk45" else dict(max_step=2.5e-12, gamma=2.5e5)
        for temperature in (0.0, 77.0, 450.0):
            cases.append((f"{solver}-temperature{temperature:g}", N_MATRIX, 2400, False, over,
                          dict(solver=solver, include_thermal_fluctuations=True, seed=81, temperature=temperature, **device_kwargs(solver, "table"))))
        cases.append((f"{solver}-float64", N_MATRIX, 2500, True, RK45_SETTINGS[0] if solver == "rk45" else dict(max_step=2.5e-12, gamma=1.9e5),
                      dict(solver=solver, include_thermal_fluctuations=False, seed=82, **device_kwargs(solver, "table"))))
    return cases


def case(name):
    for c in matrix_cases():
        if c[0] == name:
            return c
    raise KeyError(name)

"""The ends of an RK45 solve, in all three forms of the attempt loop (`pytest -m gpu`; csrc/stg_physics.hpp: llgs_lane_attempt, llgs_solve,
SharedNormalsT::open / close, produce_normals).

A producer/consumer pair's continue flag is written twice per solve: both copies say 1 from before the solve's first rendezvous, and the one
0 follows the loop (copy n & 1 after n attempts).  Every attempt still clamps its step to the pulse's end and tests the pulse gate for the
stage times that can pass it.  The cases put the clamped step and the end of the loop wherever they can fall: a wavefront whose 64 lanes
have pulses of k ps, k = 1 ... 64 (every lane's last step in another iteration; the same a rounding above and below k ps), all lanes at 1 ps
(one attempt each, every one of them clamped), one lane of 1 ns beside 63 of 1 ps, actions of J = 0 / NaN / +-inf, envs that do not integrate
(skip_done), attempt budgets of 1, 2 and 5 (lanes active when the loop ends) and K = 3 fused env-steps with auto-reset.  Shapes: 64, 100 and
192 envs -- one wavefront, one and a part (inert lanes walk every barrier), three.  Each case runs the pairs (wave_spec=True), the inline
loop (wave_spec=False) and the forced lane-refill kernel (lane_refill=2): identical bits for state, obs, reward, flags, status and the work
counters; and the oracle: TOL_RK45 of test_gpu_parity.py on the state, status / flags / step counts and the attempts exactly, accepted
points per env exactly (through the solve API: see test_accepted_points_per_env_vs_oracle for what that covers).  Thermal field on and off (off: no pairs exist)."""
import numpy as np
import pytest
import torch

from conftest import stt_default_params
from test_gpu_attempt_slots import FORMS, KW, _assert_same_bits, _cmp_oracle
from test_gpu_fullsize import _inputs
from test_gpu_parity import TOL_RK45
import test_gpu_attempt_slots as slots

pytestmark = pytest.mark.gpu

assert TOL_RK45 == slots.TOL_RK45          # (_cmp_oracle's bound is the parity suite's)

PS = 1e-12
FACTORS = {"k ps": 1.0, "k ps (1 + 2^-52)": 1.0 + 2.0 ** -52, "k ps (1 - 2^-53)": 1.0 - 2.0 ** -53}


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _parsed(b, a, i):
    """The env's parse of action row i (csrc/stg_physics.hpp: parse_action): the safety clamp in the action's own dtype -- an infinity is
    clamped like any number, a NaN in either component replaces the action by (0, 1 ps) -- then the env's limits in float64."""
    AT = a.dtype.type
    a0, a1 = AT(a[i, 0]), AT(a[i, 1])
    cmax, dmin, dmax = AT(1e8), AT(1e-12), AT(1e-6)
    if not np.isnan(a0):
        a0 = min(max(a0, -cmax), cmax)
    if not np.isnan(a1):
        a1 = min(max(a1, dmin), dmax)
    if np.isnan(a0) or np.isnan(a1):
        a0, a1 = AT(0), dmin
    return min(max(float(a0), -b.cfg.max_current), b.cfg.max_current), min(max(float(a1), 1e-12), b.cfg.max_duration)


def _oracle_attempts(b, a):
    """Attempts of the oracle's RK45 solver for the step oracle backend `b` is about to take with actions `a` (as
    test_gpu_attempt_slots._oracle_attempts, for either action dtype and for actions that are no numbers)."""
    import oracle
    total = 0
    for i in range(b.n):
        s = b.states[i]
        J, T = _parsed(b, a, i)
        r = oracle.llgs_solve(np.array([s.m[0], s.m[1], s.m[2]]), T, b.params[0], b.ocfg, J, env_id=b.env_id0 + i, env_step=int(s.rng_step), cap=4)
        total += int(r["n_attempts"])
    return total


def _run(stg, n, m0, tgt, acts, done=None, backend=None, **kw):
    env = stg.SpinTorqueVecEnv(n, diagnostics=True, **({} if backend is None else dict(backend=backend)), **kw)
    env.reset(options={"initial_state": m0, "target_state": tgt})
    if done is not None:
        st = env.get_state()
        st["done"][torch.from_numpy(done).to(st["done"].device)] = 1
        env.backend.set_state(st)
    rec, attempts = [], 0
    for a in acts:
        if backend is not None:
            attempts += _oracle_attempts(env.backend, a)
        before = env.get_state()["m"].clone()
        o, r, te, tr, info = env.step(torch.from_numpy(a))
        st = env.get_state()
        rec.append(dict(m_before=before, obs=o.t().clone(), reward=info["reward_f64"].clone(), energy=info["energy"].clone(), term=te.clone(), trunc=tr.clone(),
                        status=info["status"].clone(), m=st["m"].clone(), step_count=st["step_count"].clone()))
    counters = env.backend.counters()
    if backend is not None:
        counters["work_units"] = attempts
    env.close()
    return rec, counters


def _three_forms_and_oracle(stg, n, m0, tgt, acts, thermal, tag, done=None, **kw):
    """Pairs (thermal only), inline and refill on the same inputs: the same bits and counters; then the oracle.  Returns the counters."""
    from helpers import OracleBackend
    kw = dict(KW, include_thermal_fluctuations=thermal, **kw)
    forms = FORMS if thermal else {k: v for k, v in FORMS.items() if k != "pairs"}
    runs = {name: _run(stg, n, m0, tgt, acts, done=done, **kw, **form) for name, form in forms.items()}
    ref, c_ref = runs["inline"]
    for name, (rec, c) in runs.items():
        _assert_same_bits(rec, ref, (tag, name, "against inline"))
        assert c == c_ref, (tag, name, c, c_ref)
    _cmp_oracle(ref, c_ref, _run(stg, n, m0, tgt, acts, done=done, backend=OracleBackend, **kw), tag)
    return c_ref


def _ladder(n, factor, steps, seed):
    """Pulses of (lane + 1) ps times `factor`, as float64 actions (a float32 could not hold the factor)."""
    m0, tgt, a32 = _inputs(n, seed=seed, steps=steps)
    acts = a32.astype(np.float64)
    acts[..., 1] = ((np.arange(n) % 64) + 1) * PS * factor
    return m0, tgt, acts


@pytest.mark.parametrize("thermal", [True, False])
@pytest.mark.parametrize("factor", list(FACTORS))
@pytest.mark.parametrize("n", [64, 100, 192])
def test_every_lane_ends_in_another_iteration(stg, n, factor, thermal):
    m0, tgt, acts = _ladder(n, FACTORS[factor], steps=2, seed=5100 + n)
    c = _three_forms_and_oracle(stg, n, m0, tgt, acts, thermal, f"ladder {factor}, n = {n}, thermal {thermal}", lane_sort=False)
    assert c["noop_steps"] == 0 and c["work_units"] >= 2 * n


@pytest.mark.parametrize("thermal", [True, False])
@pytest.mark.parametrize("n", [64, 100, 192])
def test_every_attempt_is_the_clamped_one(stg, n, thermal):
    """All lanes at 1 ps: one step that ends at T (a few lanes retry it after a rejection)."""
    m0, tgt, acts = _inputs(n, seed=5200 + n, steps=2)
    acts[..., 1] = np.float32(PS)
    c = _three_forms_and_oracle(stg, n, m0, tgt, acts, thermal, f"all 1 ps, n = {n}, thermal {thermal}")
    assert c["noop_steps"] == 0 and 2 * n <= c["work_units"] <= 6 * n


@pytest.mark.parametrize("thermal", [True, False])
def test_one_long_lane_beside_63_short_ones(stg, thermal):
    n = 64
    m0, tgt, acts = _inputs(n, seed=5300, steps=2)
    acts[..., 1] = np.float32(PS)
    acts[:, 17, 1] = np.float32(1e-9)
    c = _three_forms_and_oracle(stg, n, m0, tgt, acts, thermal, f"1 ns beside 1 ps, thermal {thermal}", lane_sort=False)
    assert c["noop_steps"] == 0 and c["work_units"] > 1000


@pytest.mark.parametrize("thermal", [True, False])
def test_actions_that_are_zero_or_no_numbers(stg, thermal):
    """J = 0 (no torque terms); NaN in either component (the safety wrapper's replacement: J = 0, 1 ps); J = +-inf and a pulse of -inf
    (clamped like numbers: the current limit, 1 ps).  (A pulse of +inf is the longest pulse: a microsecond, a million attempts.)"""
    n = 100
    m0, tgt, acts = _inputs(n, seed=5400, steps=2, tlo=1e-12, thi=5e-11)
    acts[:, 0::10, 0] = 0.0
    acts[:, 1::10, 0] = np.nan
    acts[:, 2::10, 0] = np.inf
    acts[:, 3::10, 0] = -np.inf
    acts[:, 4::10, 1] = np.nan
    acts[:, 6::10, 1] = -np.inf
    c = _three_forms_and_oracle(stg, n, m0, tgt, acts, thermal, f"J = 0 / NaN / inf, thermal {thermal}", lane_sort=False)
    assert c["noop_steps"] == 0


@pytest.mark.parametrize("thermal", [True, False])
def test_envs_that_do_not_integrate(stg, thermal):
    """skip_done: wavefront 0 integrates nothing (no solve, no rendezvous but H1), wavefront 1 has idle lanes beside integrating ones.  The
    oracle backend steps every env it is given, so it gets no finished envs and is compared on the envs that were stepped."""
    from helpers import OracleBackend
    n = 192
    m0, tgt, acts = _ladder(n, 1.0, steps=1, seed=5500)
    done = np.zeros(n, dtype=bool)
    done[:64] = True
    done[64:128:3] = True
    kw = dict(KW, include_thermal_fluctuations=thermal, lane_sort=False)
    forms = FORMS if thermal else {k: v for k, v in FORMS.items() if k != "pairs"}
    runs = {name: _run(stg, n, m0, tgt, acts, done=done, skip_done=True, **kw, **form) for name, form in forms.items()}
    ref, c_ref = runs["inline"]
    for name, (rec, c) in runs.items():
        _assert_same_bits(rec, ref, ("skip_done", thermal, name))
        assert c == c_ref, (name, c, c_ref)
    ora, c_ora = _run(stg, n, m0, tgt, acts, backend=OracleBackend, **kw)
    stepped = ~done
    h, o = ref[0], ora[0]
    for key in ("status", "term", "trunc"):
        assert np.array_equal(h[key].cpu().numpy()[stepped], o[key].cpu().numpy()[stepped]), key
    d = np.abs(h["m"].cpu().numpy()[:, stepped] - o["m"].cpu().numpy()[:, stepped]).max()
    print("skip_done, thermal", thermal, ": worst |dm| vs oracle on the stepped envs =", d, c_ref)
    assert d <= TOL_RK45
    # a finished env keeps its row and is not counted; the attempts are those of the stepped envs
    assert np.array_equal(h["m"].cpu().numpy()[:, done], h["m_before"].cpu().numpy()[:, done])
    assert bool((h["step_count"].cpu().numpy()[done] == 0).all())
    assert c_ref["env_steps"] == int(stepped.sum()) and c_ref["noop_steps"] == 0
    env = stg.SpinTorqueVecEnv(n, diagnostics=True, backend=OracleBackend, **kw)
    env.reset(options={"initial_state": m0, "target_state": tgt})
    import oracle
    b = env.backend
    want = 0
    for i in np.flatnonzero(stepped):
        J, T = _parsed(b, acts[0], i)
        s_ = b.states[i]
        want += int(oracle.llgs_solve(np.array([s_.m[0], s_.m[1], s_.m[2]]), T, b.params[0], b.ocfg, J, env_id=b.env_id0 + int(i),
                                      env_step=int(s_.rng_step), cap=4)["n_attempts"])
    env.close()
    assert c_ref["work_units"] == want, (c_ref, want)


@pytest.mark.parametrize("thermal", [True, False])
@pytest.mark.parametrize("budget", [1, 2, 5])
@pytest.mark.parametrize("n", [100, 192])
def test_lanes_still_active_when_the_loop_ends(stg, n, budget, thermal):
    m0, tgt, acts = _ladder(n, 1.0, steps=2, seed=5600 + budget)
    c = _three_forms_and_oracle(stg, n, m0, tgt, acts, thermal, f"budget {budget}, n = {n}, thermal {thermal}", max_attempts=budget, lane_sort=False)
    assert c["noop_steps"] > 0 and c["work_units"] <= budget * 2 * n


def _oracle_fused(stg, n, m0, tgt, acts, **kw):
    """The oracle env stepped through the K action rows one env-step at a time (auto-reset on): per env-step its outputs, the attempts
    of its solver over the envs that had not been reset before that env-step, and which envs those are."""
    from helpers import OracleBackend
    env = stg.SpinTorqueVecEnv(n, diagnostics=True, backend=OracleBackend, **kw)
    env.reset(seed=9, options={"initial_state": m0, "target_state": tgt})
    import oracle
    b = env.backend
    redrawn = np.zeros(n, dtype=bool)
    rec = []
    for a in acts:
        attempts = 0
        for i in np.flatnonzero(~redrawn):
            J, T = _parsed(b, a, i)
            s_ = b.states[i]
            attempts += int(oracle.llgs_solve(np.array([s_.m[0], s_.m[1], s_.m[2]]), T, b.params[0], b.ocfg, J, env_id=b.env_id0 + int(i),
                                              env_step=int(s_.rng_step), cap=4)["n_attempts"])
        o, r, te, tr, info = env.step(torch.from_numpy(a))
        st = env.get_state()
        ended = (te.numpy() | tr.numpy()).astype(bool)
        rec.append(dict(obs=o.t().numpy().copy(), reward=info["reward_f64"].numpy().copy(), energy=info["energy"].numpy().copy(),
                        term=te.numpy().copy(), trunc=tr.numpy().copy(), status=info["status"].numpy().copy(),
                        final_obs=info["final_obs"].t().numpy().copy(), m=st["m"].numpy().copy(), clean=~redrawn, ended=ended,
                        attempts_clean=attempts))
        redrawn = redrawn | ended
    env.close()
    return rec


@pytest.mark.parametrize("thermal", [True, False])
@pytest.mark.parametrize("max_steps", [2, 3])
@pytest.mark.parametrize("out_every", [True, False])
def test_three_fused_env_steps_with_autoreset(stg, out_every, max_steps, thermal):
    """step_many, K = 3, with same-step auto-reset inside the launch: episodes of two steps (every env is reset after env-step 2 and takes
    env-step 3 from a redrawn state) and of three (every env is reset after the launch's last env-step).  The three forms bit for bit.
    Against the oracle, for every env-step whose outputs the launch returns (all three with out_every, the last one without): flags and
    status exactly; for the envs that had not been reset before that env-step -- a redrawn state comes from fp32 device normals, 1e-7
    from libm's -- the fp64 reward, the energy, the observation or terminal observation and, where the episode goes on, the state, at
    the bounds of test_gpu_fullsize._cmp_slice (TOL_RK45 on the state, 10 TOL_RK45 on what is derived from it).
    Attempts: the counters are totals of the launch.  With episodes of three steps no env-step of the launch starts from a redrawn state
    (premise, asserted: nobody terminates early), and the total must equal the oracle's exactly.  With episodes of two, a third of the
    launch's attempts are made from redrawn states, which the oracle redraws 1e-7 away: there the total cannot be had from the oracle,
    and the three forms' equal counters are what is checked."""
    n, K = 100, 3
    m0, tgt, acts = _ladder(n, 1.0, steps=K, seed=5702)
    # (targets in the other hemisphere, and a seed with which the ORACLE's episodes all last max_steps steps -- with others a lane of
    # 60 ps at a large current terminates in env-step 2 --, so that every reset of the launch is a truncation; asserted below)
    tgt = np.where(m0[:, 2:3] > 0, -1.0, 1.0) * np.array([[0.0, 0.0, 1.0]])
    kw = dict(KW, include_thermal_fluctuations=thermal, autoreset=True, max_steps=max_steps, lane_sort=False)
    forms = FORMS if thermal else {k: v for k, v in FORMS.items() if k != "pairs"}
    outs = {}
    for name, form in forms.items():
        env = stg.SpinTorqueVecEnv(n, diagnostics=True, **kw, **form)
        env.reset(seed=9, options={"initial_state": m0, "target_state": tgt})
        o, r, te, tr, info = env.step_many(torch.from_numpy(acts), out_every=out_every)
        st = env.get_state()
        outs[name] = ([dict(obs=o.clone(), reward=info["reward_f64"].clone(), reward32=r.clone(), energy=info["energy"].clone(), term=te.clone(),
                            trunc=tr.clone(), status=info["status"].clone(), final_obs=info["final_obs"].clone(), m=st["m"].clone(),
                            step_count=st["step_count"].clone(), rng_step=st["rng_step"].clone())], env.backend.counters())
        env.close()
    ref, c_ref = outs["inline"]
    for name in forms:
        _assert_same_bits(outs[name][0], ref, ("fused K = 3", out_every, max_steps, thermal, name))
        assert outs[name][1] == c_ref and c_ref["env_steps"] == K * n
    ora = _oracle_fused(stg, n, m0, tgt, acts, **kw)
    h = {key: v.cpu().numpy() for key, v in ref[0].items()}
    for key in ("obs", "final_obs"):             # (step_many hands out [K, n, 12]; the oracle rows below are [12, n])
        if h[key].shape[-2:] == (n, 12):
            h[key] = h[key].transpose(0, 2, 1)
        assert h[key].shape[-2:] == (12, n), (key, h[key].shape)
    tol = TOL_RK45
    worst = dict(m=0.0, reward=0.0, energy=0.0)
    for k in (range(K) if out_every else [K - 1]):
        j = k if out_every else 0
        o = ora[k]
        tag = ("fused K = 3 against the oracle", out_every, max_steps, thermal, "env-step", k)
        for key in ("term", "trunc", "status"):
            assert np.array_equal(h[key][j], o[key]), (tag, key)
        clean, ended = o["clean"], o["ended"] & o["clean"]
        if not clean.any():          # (episodes of two steps: env-step 3 starts from redrawn states throughout)
            continue
        worst["reward"] = max(worst["reward"], np.abs(h["reward"][j][clean] - o["reward"][clean]).max())
        worst["energy"] = max(worst["energy"], np.abs(h["energy"][j][clean] - o["energy"][clean]).max())
        assert np.allclose(h["reward"][j][clean], o["reward"][clean], rtol=1e-10, atol=10 * tol), tag
        assert np.allclose(h["energy"][j][clean], o["energy"][clean], rtol=10 * tol, atol=0), tag
        going = clean & ~ended
        if going.any():
            assert np.allclose(h["obs"][j][:, going], o["obs"][:, going], rtol=3e-7, atol=10 * tol), tag
        if ended.any():
            assert np.allclose(h["final_obs"][j][:, ended], o["final_obs"][:, ended], rtol=3e-7, atol=10 * tol), tag
        if k == K - 1 and going.any():
            dm = np.abs(h["m"][:, going] - o["m"][:, going]).max()
            worst["m"] = max(worst["m"], dm)
            assert dm <= tol, (tag, dm)
    print("fused K = 3", out_every, max_steps, thermal, "worst against the oracle before a reset:", worst, c_ref)
    if max_steps == 3:
        assert all(o["clean"].all() for o in ora), "premise: no env ends before the launch's last env-step"
        assert c_ref["work_units"] == sum(o["attempts_clean"] for o in ora), (c_ref, [o["attempts_clean"] for o in ora])


def test_accepted_points_per_env_vs_oracle(stg):
    """Accepted points per env through the solve API (thermal field on): the ladder, J = 0 lanes among them.  env.step returns no
    accepted points per env, so this is the one place they meet the oracle's, and it is the solve kernel -- llgs_solve with the normals
    inline -- that is measured here.  The pair kernel's accepted points are covered only indirectly: they decide the state, which the
    cases above hold bit-identical between the pairs and the inline form."""
    from helpers import OracleBackend
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    n = 64
    rng = np.random.default_rng(58)
    v = rng.normal(0, 1, (n, 3))
    m0 = v / np.linalg.norm(v, axis=1, keepdims=True)
    J = rng.uniform(-2e6, 2e6, n)
    J[::7] = 0.0
    T = (np.arange(n) + 1) * PS
    table = [stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", stt_default_params(volume=9.7e-6)))]
    res = []
    for B in (HipBackend, OracleBackend):
        b = B(n, EnvConfig(diagnostics=True, solver="rk45", include_thermal_fluctuations=True, temperature=300.0, seed=5))
        b.set_params(table, None)
        out = b.solve(torch.tensor(m0.T.copy()), torch.tensor(J), torch.tensor(T))
        res.append({key: torch.as_tensor(out[key]).cpu().numpy().copy() for key in ("m_final", "n_points", "success")})
        b.close()
    h, o = res
    assert h["success"].all() and o["success"].all()
    assert np.array_equal(h["n_points"], o["n_points"])
    assert np.abs(h["m_final"] - o["m_final"]).max() <= TOL_RK45

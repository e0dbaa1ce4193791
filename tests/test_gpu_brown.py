"""noise_model='brown' -- the Brown field with its 1/sqrt(dt) factor (include/spintorque_hip.h, cfg.noise_model = 2) -- on the GPU:
`pytest -m gpu`.

  1. arithmetic parity: every fixed-step path against the NumPy restatement (tests/brown_ref.py) FED THE DEVICE'S OWN NORMALS
     (stg_thermal_normals at the env's stream position), final m within TOL_RK4 = 1e-10 with exact status bytes and sub-step counts.
     (The device's normals differ from the oracle's by ~1e-7 relative -- tests/test_gpu_parity.py pins them -- and at this field
     strength that alone moves m by 3-4e-5, while rounding-level perturbations of the normals move it by less than 1e-12: with the
     device's normals 1e-10 tests the arithmetic.)  N = 130 (two wavefronts and a 2-lane tail), T ~ U[0.1, 0.3] ns (<= 300 sub-steps),
     two regimes: equilibrium (alpha = 0.1, Delta = 4, J = 0, random m0) and switching (alpha = 0.02, V = 1.3856e-25, J = 1.2482e-9,
     m0 near +z);
  2. Boltzmann's <m_z^2> on the device, 16 384 envs;
  3. thermally assisted switching against the restatement run with NumPy's own generator, and switching_probability;
  4. stg_create with noise_model = 2.

Every test here fails without the feature with "ValueError: noise_model must be ..." (4: with STG_E_INVALID from stg_create)."""
import ctypes as C

import numpy as np
import pytest
import torch

import brown_ref as br
import wave_step_ref as wsr
from spin_torque_gym_amd import physics
from conftest import sot_default_params, vcma_default_params

pytestmark = pytest.mark.gpu

TOL_RK4 = 1e-10                  # tests/test_gpu_parity.py: the fixed-step solvers against the reference
N = 130
MAX_CURRENT = 1e-8
SEED = 41
REGIMES = ("equilibrium", "switching")
SOLVERS = ("rk4", "euler")
CFG = dict(max_current=MAX_CURRENT)          # of the restatement's env step; everything else is the default of both sides


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _regime(name):
    if name == "equilibrium":
        return dict(damping=0.1, volume=br.volume_for(4.0), J=0.0)
    return dict(damping=br.SWITCH["damping"], volume=br.SWITCH["volume"], J=br.SWITCH["J"])


def _problem(regime, seed, K=1, n=N):
    """m0 [n,3] (uniform on the sphere / near +z), targets -z, actions [K,n,2] float32 with the regime's J and T ~ U[0.1, 0.3] ns"""
    rng = np.random.default_rng(seed)
    if regime == "equilibrium":
        m0 = br.sphere(rng, n)
    else:
        m0 = np.array([0.0, 0.0, 1.0]) + 0.05 * rng.normal(0, 1, (n, 3))
        m0 /= np.linalg.norm(m0, axis=1, keepdims=True)
    tgt = np.tile([0.0, 0.0, -1.0], (n, 1))
    a = np.stack([np.full((K, n), _regime(regime)["J"]), rng.uniform(1e-10, 3e-10, (K, n))], axis=2).astype(np.float32)
    return m0, tgt, a


def _params(regime, **over):
    r = _regime(regime)
    return dict(br.physics_params(r["volume"], r["damping"]), **over)


def _normals(backend, rng_step, n_calls):
    """the device's own draws for sub-steps 0 .. n_calls-1 of every env at its stream position rng_step [N] -> [N, n_calls, 3]"""
    rng_step = np.asarray(rng_step)
    out = np.zeros((backend.n, n_calls, 3))
    for s in np.unique(rng_step):
        z = backend.thermal_normals(int(s), 0, int(n_calls)).permute(2, 0, 1).cpu().numpy()
        out[rng_step == s] = z[rng_step == s]
    return out


def _np_state(env):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in env.get_state().items()}


def _ref_state(st, sel=slice(None)):
    return dict(m=st["m"].T[sel], target=st["target"].T[sel], total_energy=st["total_energy"][sel], step_count=st["step_count"][sel])


def _check_against_ref(what, before, after, outs, acts, ref_kw, sel=None, rows=None, tables=None):
    """one env step against brown_ref.step.  before / after: _np_state; outs = (obs [M,12], reward_f64 [M], terminated, truncated,
    status) of the stepped envs `sel` (None: all, in order); acts [M,2(+P)]; ref_kw: params, s, method, cls, dev_types of ALL envs' classes
    (cls per env); rows: the stepped envs whose m the restatement covers (None: all); tables(J, T) -> (current, field) or None."""
    n = before["m"].shape[1]
    sel = np.arange(n) if sel is None else np.asarray(sel)
    J, T = wsr.parse_actions(acts[:, :2], MAX_CURRENT, 5e-9)
    n_max = int(br.substeps(T)[0].max())
    z = ref_kw.pop("normals")(before["rng_step"], n_max)[sel]
    cur, fld = tables(J, T) if tables is not None else (None, None)
    kw = dict(ref_kw)
    if kw.get("cls") is not None:
        kw["cls"] = np.asarray(kw["cls"])[sel]
    ref = br.step(_ref_state(before, sel), acts[:, :2], normals=z, current=cur, field=fld, cfg=CFG, **kw)
    obs, r64, te, tr, status = (np.asarray(x.cpu() if torch.is_tensor(x) else x) for x in outs)
    rows = np.arange(len(sel)) if rows is None else np.asarray(rows)
    m_after = after["m"].T[sel]
    err = float(np.abs(m_after[rows] - ref["m"][rows]).max())
    print(f"{what}: |m - m_ref| = {err:.2e} over {len(rows)} envs, sub-steps {int(ref['n_sub'].min())}..{int(ref['n_sub'].max())}")
    assert err <= TOL_RK4, (what, err)
    assert np.array_equal(status[rows], ref["status"][rows]) and (status == wsr.STATUS_OK).all(), (what, status)
    assert np.array_equal(after["step_count"][sel], ref["step_count"]) and np.array_equal(after["rng_step"][sel], before["rng_step"][sel] + 1)
    assert np.array_equal(te.astype(bool)[rows], ref["terminated"][rows]) and np.array_equal(tr.astype(bool)[rows], ref["truncated"][rows]), what
    assert np.allclose(obs[rows], ref["obs"][rows], rtol=3e-7, atol=1e-9), (what, np.abs(obs[rows] - ref["obs"][rows]).max())
    assert np.allclose(r64[rows], ref["reward"][rows], rtol=1e-9, atol=1e-9), (what, np.abs(r64[rows] - ref["reward"][rows]).max())
    assert np.allclose(after["total_energy"][sel], ref["total_energy"], rtol=1e-12, atol=0.0), what
    return ref


def _step_outs(res):
    obs, r, te, tr, info = res
    return obs, info["reward_f64"], te, tr, info["status"]


def _make_env(stg, solver, n=N, noise="brown", **kw):
    return stg.SpinTorqueVecEnv(n, diagnostics=True, include_thermal_fluctuations=True, solver=solver, seed=SEED, noise_model=noise,
                                max_current=MAX_CURRENT, **kw)


def _reset(env, m0, tgt):
    env.reset(options={"initial_state": m0, "target_state": tgt})


def _same_bits(x, y, what):
    x, y = x.contiguous(), y.contiguous()
    assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape)
    view = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bool: torch.uint8}
    bad = (x.view(view.get(x.dtype, x.dtype)) != y.view(view.get(y.dtype, y.dtype))).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements differ, first at {bad[:4].tolist()}"


def _same_state(e1, e2, what):
    torch.cuda.synchronize()
    s1, s2 = e1.get_state(), e2.get_state()
    for k in s1:
        _same_bits(s1[k], s2[k], (what, "state", k))


# ------------------------------------------------------------------------------------------------
# 1. arithmetic parity
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("regime", REGIMES)
def test_solve_and_trajectory_vs_restatement(stg, oracle_mod, regime, solver):
    """stg_solve and stg_solve_traj (every row of the trajectories of six problems, among them both lanes of the tail; the final m of
    all) at stream position 3"""
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    p = _params(regime)
    m0, _, a = _problem(regime, 5)
    J, T = a[0, :, 0].astype(np.float64), a[0, :, 1].astype(np.float64)
    b = HipBackend(N, EnvConfig(solver=solver, include_thermal_fluctuations=True, noise_model="brown", seed=SEED, max_current=MAX_CURRENT))
    b.set_params([stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", p))])
    n, _ = br.substeps(T)
    assert n.max() <= 300
    z = _normals(b, np.full(N, 3), int(n.max()))
    s = br.strength(oracle_mod, p)
    assert abs(b.thermal_strength(0) - s) <= 1e-14 * s                      # dt-free, as for 'white' and 'ou'
    ref = br.solve(m0, T, p, s, z, solver, J=J)
    assert ref["success"].all()
    cap = int(n.max()) + 1
    for traj_cap in (0, cap):
        out = b.solve(torch.from_numpy(m0.T.copy()), torch.from_numpy(J), torch.from_numpy(T), env_step=3, traj_cap=traj_cap)
        torch.cuda.synchronize()
        mf = out["m_final"].cpu().numpy().T
        err = float(np.abs(mf - ref["m_final"]).max())
        print(f"{regime} {solver} traj_cap={traj_cap}: |m - m_ref| = {err:.2e}")
        assert err <= TOL_RK4, (regime, solver, traj_cap, err)
        assert np.array_equal(out["n_points"].cpu().numpy(), ref["n_steps"]) and bool((out["success"] == 1).all())
        assert float(np.abs(mf - m0).max()) > 1e-2                           # the field and the torque did move the states
    t, m = out["t"].cpu().numpy(), out["m"].cpu().numpy()
    for j in (0, 63, 64, 127, 128, 129):
        rj = br.solve(m0[j:j + 1], T[j:j + 1], p, s, z[j:j + 1], solver, J=J[j:j + 1], trajectory=True)
        k = int(n[j]) + 1
        assert np.array_equal(t[:k, j], rj["t"]), (regime, solver, j)
        err = float(np.abs(m[:k, :, j] - rj["m"]).max())
        assert err <= TOL_RK4, (regime, solver, j, err)
        assert not t[k:, j].any() and not m[k:, :, j].any()
    b.close()


def _forms(regime, oracle_mod):
    """the env forms of the step test: name -> (constructor keywords, restatement keywords, rows the restatement covers)"""
    r = _regime(regime)
    p0 = _params(regime)
    cls2 = (np.arange(N) % 2).astype(np.uint8)
    s_of = lambda p, t="stt_mram": br.strength(oracle_mod, p, t)               # noqa: E731
    forms = {"one class": (dict(device_params=p0), dict(params=p0, s=s_of(p0)), None)}
    pv = vcma_default_params(volume=0.8 * r["volume"], damping=r["damping"], saturation_magnetization=8e5, uniaxial_anisotropy=1e6,
                             polarization=0.6)
    forms["class table STT + VCMA"] = (dict(device_type=["stt_mram", "vcma_mram"], device_params=[p0, pv], class_index=cls2),
                                       dict(params=[p0, pv], s=[s_of(p0), s_of(pv, "vcma_mram")], cls=cls2, dev_types=["stt_mram", "vcma_mram"]),
                                       None)
    p1 = dict(p0, volume=1.3 * r["volume"])
    forms["per-env records"] = (dict(device_params=p0, per_env_params=dict(volume=np.where(cls2 == 0, p0["volume"], p1["volume"]))),
                                dict(params=[p0, p1], s=[s_of(p0), s_of(p1)], cls=cls2), None)
    ps = sot_default_params(volume=r["volume"], damping=r["damping"], saturation_magnetization=8e5, uniaxial_anisotropy=1e6, polarization=0.7)
    # device torque model: an STT lane keeps the reference RHS; a SOT lane's own torque scales with J, so the restatement (reference
    # torque model) covers the SOT lanes at J = 0 only
    forms["torque_model='device', STT + SOT"] = (
        dict(device_type=["stt_mram", "sot_mram"], device_params=[p0, ps], class_index=cls2, torque_model="device"),
        dict(params=[p0, ps], s=[s_of(p0), s_of(ps, "sot_mram")], cls=cls2, dev_types=["stt_mram", "sot_mram"]),
        None if r["J"] == 0.0 else np.nonzero(cls2 == 0)[0])
    return forms


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("regime", REGIMES)
def test_step_forms_vs_restatement(stg, oracle_mod, regime, solver):
    """step() for one class, a class table of STT + VCMA (two volumes), per-env parameter records (two volumes) and the device torque
    model with an STT + SOT table: state, status, sub-step count, observation, reward and flags of one step"""
    m0, tgt, a = _problem(regime, 6)
    for name, (env_kw, ref_kw, rows) in _forms(regime, oracle_mod).items():
        env = _make_env(stg, solver, **env_kw)
        _reset(env, m0, tgt)
        env.backend.counters(reset=True)
        before = _np_state(env)
        outs = _step_outs(env.step(torch.from_numpy(a[0])))
        after = _np_state(env)
        ref = _check_against_ref((regime, solver, name), before, after, outs, a[0],
                                 dict(ref_kw, method=solver, normals=lambda rs, k, b=env.backend: _normals(b, rs, k)), rows=rows)
        cnt = env.backend.counters()
        assert cnt["work_units"] == int(ref["n_sub"].sum()) and cnt["env_steps"] == N and cnt["noop_steps"] == 0, (name, cnt)
        if rows is not None:                       # the SOT lanes under their own torque: stepped, finite, unit
            m = after["m"].T
            assert np.isfinite(m).all() and np.abs(np.linalg.norm(m, axis=1) - 1).max() < 1e-12
        env.close()


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("regime", REGIMES)
def test_step_many_advances_the_stream(stg, oracle_mod, regime, solver):
    """step_many with K = 2: bit for bit two step() calls, each of which matches the restatement at its own stream position (0, then 1)
    from the state the device was in before it"""
    p = _params(regime)
    m0, tgt, a = _problem(regime, 7, K=2)
    ref_kw = dict(params=p, s=br.strength(oracle_mod, p), method=solver)
    one, many = _make_env(stg, solver, device_params=p), _make_env(stg, solver, device_params=p)
    _reset(one, m0, tgt), _reset(many, m0, tgt)
    single = []
    for k in range(2):
        before = _np_state(one)
        assert (before["rng_step"] == k).all()
        res = one.step(torch.from_numpy(a[k]))
        outs = tuple(x.clone() for x in _step_outs(res)) + (res[1].clone(), res[4]["energy"].clone())
        _check_against_ref((regime, solver, "step", k), before, _np_state(one), outs[:5], a[k],
                           dict(ref_kw, normals=lambda rs, c, b=one.backend: _normals(b, rs, c)))
        single.append(outs)
    zs = [_normals(one.backend, np.full(N, k), 8) for k in range(2)]
    assert np.abs(zs[0] - zs[1]).max() > 0.1                                  # the two positions are different draws
    obs, r, te, tr, info = many.step_many(torch.from_numpy(a))
    for k in range(2):
        got = (obs[k], info["reward_f64"][k], te[k], tr[k], info["status"][k], r[k], info["energy"][k])
        for x, y, key in zip(got, single[k], ("obs", "reward_f64", "terminated", "truncated", "status", "reward", "energy")):
            _same_bits(x, y, (regime, solver, "step_many", k, key))
    _same_state(one, many, (regime, solver, "step_many"))
    one.close(), many.close()


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("regime", REGIMES)
def test_step_ids_subset(stg, oracle_mod, regime, solver):
    """step_ids on a pair-closed subset of 66 ids, twice: the listed envs match the restatement at their own stream positions, every
    other env stays bit for bit"""
    p = _params(regime)
    m0, tgt, a = _problem(regime, 8, K=2)
    rng = np.random.default_rng(9)
    pairs = np.concatenate([rng.permutation(N // 2 - 1)[:32], [N // 2 - 1]])    # (the pair of the 2-lane tail among them)
    ids = rng.permutation(np.concatenate([2 * pairs, 2 * pairs + 1]))           # list order is not env order
    assert len(np.unique(ids)) == 66 and ids.max() == N - 1
    others = np.setdiff1d(np.arange(N), ids)
    env = _make_env(stg, solver, device_params=p)
    _reset(env, m0, tgt)
    start = _np_state(env)
    for k in range(2):
        before = _np_state(env)
        obs, r, te, tr, info = env.step_ids(torch.from_numpy(a[k][ids]), ids)
        assert np.array_equal(info["env_id"].cpu().numpy(), ids)
        after = _np_state(env)
        _check_against_ref((regime, solver, "step_ids", k), before, after, (obs, info["reward_f64"], te, tr, info["status"]), a[k][ids],
                           dict(params=p, s=br.strength(oracle_mod, p), method=solver,
                                normals=lambda rs, c, b=env.backend: _normals(b, rs, c)), sel=ids)
        for key in start:
            assert np.array_equal(after[key][..., others], start[key][..., others]), (regime, solver, k, key)
    assert (after["rng_step"][ids] == 2).all() and (after["rng_step"][others] == 0).all()
    env.close()


def _shape_and_field(stg):
    from spin_torque_gym_amd.physics import PiecewiseLinear
    shape = PiecewiseLinear([0.0, 0.2, 0.7, 1.0], [0.0, 1.0, 1.0, 0.4])
    field = PiecewiseLinear([0.0, 1.5e-10, 3e-10], [[2e4, 0.0, 0.0], [0.0, 2e4, -1e4], [-1e4, 0.0, 3e4]])
    return shape, field


def _field_tables(field, n):
    return np.tile(field.times, (n, 1)), np.tile(field.values, (n, 1, 1))


@pytest.mark.parametrize("regime", REGIMES)
def test_solve_batch_with_knots_vs_restatement(stg, oracle_mod, regime):
    """SimpleLLGSSolver(noise_model='brown').solve_batch(current_knots=, field_knots=): the waveform copy of the fixed-step solve
    (stg_solve_wave), per-problem current tables and one field table, at stream position 2"""
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    p = _params(regime)
    m0, _, a = _problem(regime, 10)
    T = a[0, :, 1].astype(np.float64)
    Jp = 1.2482e-9                                                    # (a current in both regimes: the tables are what is tested)
    tk = np.array([0.0, 0.2, 0.7, 1.0])[None, :] * T[:, None]         # [N,K]
    jk = np.tile(Jp * np.array([0.0, 1.0, 1.0, 0.4]), (N, 1)) * np.linspace(0.5, 1.5, N)[:, None]
    _, field = _shape_and_field(stg)
    solver = physics.SimpleLLGSSolver(method="rk4", noise_model="brown", seed=SEED)
    got = solver.solve_batch(m0, None, T, p, thermal_noise=True, env_step=2, current_knots=(tk.T.copy(), jk.T.copy()),
                             field_knots=(field.times, field.values))
    b = HipBackend(N, EnvConfig(solver="rk4", include_thermal_fluctuations=True, noise_model="brown", seed=SEED))
    n, _ = br.substeps(T)
    z = _normals(b, np.full(N, 2), int(n.max()))
    b.close()
    ref = br.solve(m0, T, p, br.strength(oracle_mod, p), z, "rk4", current=(tk, jk), field=_field_tables(field, N))
    err = float(np.abs(got["m_final"] - ref["m_final"]).max())
    print(f"{regime} solve_batch with knots: |m - m_ref| = {err:.2e}")
    assert err <= TOL_RK4 and got["success"].all() and np.array_equal(got["n_points"], ref["n_steps"])
    plain = solver.solve_batch(m0, np.full(N, Jp), T, p, thermal_noise=True, env_step=2)
    assert float(np.abs(plain["m_final"] - got["m_final"]).max()) > 1e-3                 # the tables do drive the solve


@pytest.mark.parametrize("regime", REGIMES)
def test_shaped_steps_vs_restatement_and_fused(stg, oracle_mod, regime):
    """pulse_shape + applied_field (rk4): step() (stg_step_wave) against the restatement, and step_many with K = 2 (stg_step_shaped) bit
    for bit two step() calls"""
    p = _params(regime)
    m0, tgt, a = _problem(regime, 11, K=2)
    a[:, :, 0] = np.float32(1.2482e-9)
    shape, field = _shape_and_field(stg)
    kw = dict(device_params=p, pulse_shape=shape, applied_field=field)
    one, many = _make_env(stg, "rk4", **kw), _make_env(stg, "rk4", **kw)
    _reset(one, m0, tgt), _reset(many, m0, tgt)

    def tables(J, T):
        return (shape.times[None, :] * T[:, None], J[:, None] * shape.values[None, :]), _field_tables(field, N)
    single = []
    for k in range(2):
        before = _np_state(one)
        res = one.step(torch.from_numpy(a[k]))
        outs = tuple(x.clone() for x in _step_outs(res)) + (res[1].clone(), res[4]["energy"].clone())
        if k == 0:
            _check_against_ref((regime, "shaped step"), before, _np_state(one), outs[:5], a[k],
                               dict(params=p, s=br.strength(oracle_mod, p), method="rk4",
                                    normals=lambda rs, c, b=one.backend: _normals(b, rs, c)), tables=tables)
        single.append(outs)
    obs, r, te, tr, info = many.step_many(torch.from_numpy(a))
    for k in range(2):
        got = (obs[k], info["reward_f64"][k], te[k], tr[k], info["status"][k], r[k], info["energy"][k])
        for x, y, key in zip(got, single[k], ("obs", "reward_f64", "terminated", "truncated", "status", "reward", "energy")):
            _same_bits(x, y, (regime, "shaped step_many", k, key))
    _same_state(one, many, (regime, "shaped step_many"))
    one.close(), many.close()


@pytest.mark.parametrize("regime", REGIMES)
def test_knot_amplitude_steps_vs_restatement_and_fused(stg, oracle_mod, regime):
    """pulse_knots (rk4; the action carries the amplitudes): step() (stg_step_knots, K = 1) against the restatement, and step_many with
    K = 2 bit for bit two step() calls"""
    p = _params(regime)
    m0, tgt, a2 = _problem(regime, 12, K=2)
    a2[:, :, 0] = np.float32(1.2482e-9)
    rng = np.random.default_rng(13)
    tau = np.array([0.0, 0.3, 0.6, 1.0])
    a = np.concatenate([a2, rng.uniform(-1.3, 1.3, (2, N, 4)).astype(np.float32)], axis=2)        # (some amplitudes beyond the clamp)
    kw = dict(device_params=p, pulse_knots=tau, amplitude_limit=1.0)
    one, many = _make_env(stg, "rk4", **kw), _make_env(stg, "rk4", **kw)
    _reset(one, m0, tgt), _reset(many, m0, tgt)
    single = []
    for k in range(2):
        before = _np_state(one)
        res = one.step(torch.from_numpy(a[k]))
        outs = tuple(x.clone() for x in _step_outs(res)) + (res[1].clone(), res[4]["energy"].clone())
        if k == 0:
            s = np.clip(a[k][:, 2:].astype(np.float64), -1.0, 1.0)
            _check_against_ref((regime, "knots step"), before, _np_state(one), outs[:5], a[k],
                               dict(params=p, s=br.strength(oracle_mod, p), method="rk4",
                                    normals=lambda rs, c, b=one.backend: _normals(b, rs, c)),
                               tables=lambda J, T: ((tau[None, :] * T[:, None], J[:, None] * s), None))
        single.append(outs)
    obs, r, te, tr, info = many.step_many(torch.from_numpy(a))
    for k in range(2):
        got = (obs[k], info["reward_f64"][k], te[k], tr[k], info["status"][k], r[k], info["energy"][k])
        for x, y, key in zip(got, single[k], ("obs", "reward_f64", "terminated", "truncated", "status", "reward", "energy")):
            _same_bits(x, y, (regime, "knots step_many", k, key))
    _same_state(one, many, (regime, "knots step_many"))
    one.close(), many.close()


@pytest.mark.parametrize("solver", SOLVERS)
def test_wave_specialised_pairs_bit_identical(stg, solver):
    """N = 320: the producer / consumer wavefront pairs (wave_spec=True) and the one-wavefront kernels (False) agree bit for bit, one
    class and a class table, two steps (the form of test_ornstein_uhlenbeck_noise_model_vs_oracle)"""
    n = 320
    m0, tgt, a = _problem("switching", 14, K=2, n=n)
    p0 = _params("switching")
    pv = vcma_default_params(volume=0.8 * p0["volume"], damping=0.02, saturation_magnetization=8e5, uniaxial_anisotropy=1e6, polarization=0.6)
    for kw in (dict(device_params=p0),
               dict(device_type=["stt_mram", "vcma_mram"], device_params=[p0, pv], class_index=(np.arange(n) % 2).astype(np.uint8))):
        res = []
        for ws in (False, True):
            env = _make_env(stg, solver, n=n, wave_spec=ws, **kw)
            _reset(env, m0, tgt)
            out = []
            for k in range(2):
                o, r, te, tr, info = env.step(torch.from_numpy(a[k]))
                out.append((o.clone(), info["reward_f64"].clone(), info["status"].clone(), env.get_state()["m"].clone()))
            res.append(out)
            env.close()
        for k in range(2):
            for x, y, key in zip(res[0][k], res[1][k], ("obs", "reward_f64", "status", "m")):
                _same_bits(x, y, (solver, "wave_spec", k, key))
            assert bool((res[0][k][2] == 0).all())
        assert float((res[0][1][3] - torch.from_numpy(m0.T).cuda()).abs().max()) > 1e-2


@pytest.mark.parametrize("solver", SOLVERS)
def test_brown_is_neither_white_nor_ou(stg, solver):
    m0, tgt, a = _problem("equilibrium", 15)
    p = _params("equilibrium")
    m = {}
    for noise in ("brown", "white", "ou"):
        env = _make_env(stg, solver, noise=noise, device_params=p)
        _reset(env, m0, tgt)
        env.step(torch.from_numpy(a[0]))
        m[noise] = _np_state(env)["m"]
        env.close()
    assert np.abs(m["brown"] - m["white"]).max() > 1e-3 and np.abs(m["brown"] - m["ou"]).max() > 1e-3


# ------------------------------------------------------------------------------------------------
# 2. Boltzmann on the device
# ------------------------------------------------------------------------------------------------
def test_boltzmann_on_the_device(stg):
    """16 384 envs, rk4, alpha = 0.1, Delta = 4: device-side random reset, one step at J = 0 over 1.5 ns; <m_z^2> within the restatement's
    measured bias (tests/brown_ref.py, a CPU constant) plus four standard errors of Boltzmann's value, <m_z> within four of zero"""
    n = 16384
    max_step, b, _ = br.EQUILIBRIUM_BIAS[4.0]
    assert max_step == 1e-12
    env = _make_env(stg, "rk4", n=n, device_params=_params("equilibrium"))
    env.reset(seed=3)
    mz0 = _np_state(env)["m"][2]
    assert abs(float((mz0 * mz0).mean()) - 1.0 / 3.0) < 4 * np.sqrt(4.0 / 45.0 / n)           # uniform on the sphere: var(m_z^2) = 4/45
    a = np.tile(np.array([0.0, 1.5e-9], dtype=np.float32), (n, 1))
    _, _, _, _, info = env.step(torch.from_numpy(a))
    assert bool((info["status"] == 0).all())
    mz = _np_state(env)["m"][2]
    env.close()
    exact = br.boltzmann_mz2(4.0)
    mz2, se2 = float((mz * mz).mean()), float((mz * mz).std() / np.sqrt(n))
    mz1, se1 = float(mz.mean()), float(mz.std() / np.sqrt(n))
    print(f"device: <m_z^2> = {mz2:.4f} +- {se2:.4f} against {exact:.4f} (bias {b:+.4f}); <m_z> = {mz1:+.4f} +- {se1:.4f}")
    assert abs(mz2 - exact) <= abs(b) + 4 * se2
    assert abs(mz1) <= 4 * se1


# ------------------------------------------------------------------------------------------------
# 3. thermally assisted switching, independent streams
# ------------------------------------------------------------------------------------------------
SW_ACTION = np.array([br.SWITCH["J"], br.SWITCH["T"]], dtype=np.float32)


def test_switching_statistics_independent_streams(stg, oracle_mod):
    """m0 = +z exactly, target -z, float32 action (1.2482e-9, 5e-10): P(m_z < 0) of 16 384 envs on Philox against 4096 samples of the
    restatement on NumPy's generator, within four binomial standard errors of the smaller sample (+ 1e-3); the same launch with the
    white field switches no env"""
    p = _params("switching")
    n_cpu, n = 4096, 16384
    J, T = wsr.parse_actions(SW_ACTION[None, :], MAX_CURRENT, 5e-9)
    steps = int(br.substeps(T)[0][0])
    assert steps == 499                                                      # float32(5e-10) is just below 5e-10
    rng = np.random.default_rng(2024)
    ref = br.solve(np.tile([0.0, 0.0, 1.0], (n_cpu, 1)), np.full(n_cpu, T[0]), p, br.strength(oracle_mod, p),
                   rng.standard_normal((n_cpu, steps, 3)), "rk4", J=np.full(n_cpu, J[0]))
    assert ref["success"].all()
    p_cpu = float((ref["m_final"][:, 2] < 0).mean())
    frac = {}
    for noise in ("brown", "white"):
        env = _make_env(stg, "rk4", n=n, noise=noise, device_params=p)
        _reset(env, np.tile([0.0, 0.0, 1.0], (n, 1)), np.tile([0.0, 0.0, -1.0], (n, 1)))
        _, _, _, _, info = env.step(torch.from_numpy(np.tile(SW_ACTION, (n, 1))))
        assert bool((info["status"] == 0).all())
        frac[noise] = float((_np_state(env)["m"][2] < 0).mean())
        env.close()
    print(f"switched: HIP {frac['brown']:.4f} CPU {p_cpu:.4f}; white field {frac['white']:.4f}")
    assert 0.05 < p_cpu < 0.95                                               # the regime is genuinely stochastic
    assert abs(frac["brown"] - p_cpu) <= 4 * np.sqrt(p_cpu * (1 - p_cpu) / n_cpu) + 1e-3, (frac["brown"], p_cpu)
    assert frac["white"] == 0.0


def test_switching_probability_counts_equal_a_host_reduction(stg):
    """three conditions x 4096 trials in one launch: the counts reduced on the device equal those of solve_batch on the replicated
    problems reduced on the host, exactly"""
    p = _params("switching")
    G, R = 3, 4096
    J = float(SW_ACTION[0]) * np.array([0.85, 1.0, 1.15])
    T = np.full(G, float(SW_ACTION[1]))
    m0 = np.tile([0.0, 0.0, 1.0], (G, 1))
    solver = physics.SimpleLLGSSolver(method="rk4", noise_model="brown", seed=SEED)
    got = solver.switching_probability(m0, J, T, p, R)
    full = solver.solve_batch(np.repeat(m0, R, axis=0), np.repeat(J, R), np.repeat(T, R), p, thermal_noise=True)
    want = (-full["m_final"][:, 2] > 0.0).reshape(G, R).sum(axis=1)
    print("switching_probability:", got["p_switch"], "+-", got["stderr"], "failed", got["n_failed"])
    assert np.array_equal(got["n_switched"], want) and np.array_equal(got["n_failed"], (~full["success"]).reshape(G, R).sum(axis=1))
    assert np.array_equal(got["p_switch"], want / R) and not got["n_failed"].any()
    assert got["p_switch"][0] < got["p_switch"][2] and 0.05 < got["p_switch"][1] < 0.95       # more current switches more often
    assert physics.SimpleLLGSSolver(method="rk4", noise_model="white", seed=SEED).switching_probability(m0, J, T, p, 64)["n_switched"].sum() == 0


# ------------------------------------------------------------------------------------------------
# 4. stg_create
# ------------------------------------------------------------------------------------------------
def test_stg_create_with_noise_model_2(stg):
    from spin_torque_gym_amd import _lib
    from spin_torque_gym_amd.backend import EnvConfig
    lib = _lib.load()
    for solver in ("rk4", "euler"):
        cfg = EnvConfig(solver=solver).to_abi()
        cfg.noise_model = 2
        cfg.noise_corr_time = 0.0                                            # ignored for model 2
        ctx = C.c_void_p()
        assert lib.stg_create(C.byref(ctx), 0, 64, 0, C.byref(cfg)) == 0, lib.stg_last_error()
        lib.stg_destroy(ctx)
    ctx = C.c_void_p()
    bad = EnvConfig(solver="rk45").to_abi()
    bad.noise_model = 2
    assert lib.stg_create(C.byref(ctx), 0, 64, 0, C.byref(bad)) == _lib.STG_E_INVALID and b"fixed-step" in lib.stg_last_error()
    bad = EnvConfig(solver="rk4").to_abi()
    bad.noise_model = 3
    assert lib.stg_create(C.byref(ctx), 0, 64, 0, C.byref(bad)) == _lib.STG_E_INVALID and b"noise_model" in lib.stg_last_error()
    assert _lib.ABI_VERSION == 5 and lib.stg_abi_version() == 5

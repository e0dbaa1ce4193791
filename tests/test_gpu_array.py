"""The SpinTorqueArray-v0 kernels (csrc/stg_array.hip) on the MI355X beyond 4 x 4: every launch branch of stg_array_step against the
CPU oracle on non-square, single-row / single-column, 5 x 5, 8 x 8 and 2 x 32 arrays with many lanes; every output element written and
nothing else; masked and device-side random resets; NaN / infinite actions in a batch against the recorded reference (G20).

Tolerances are the ones of the 4 x 4 tests in test_gpu_parity.py: pattern <= 1e-11, observation rtol 3e-7 / atol 1e-10, reward 1e-9 / 1e-9,
energy rtol 1e-10, flags and step counts equal."""
import numpy as np
import pytest
import torch

from conftest import sot_default_params, vcma_default_params

pytestmark = pytest.mark.gpu

SOT = dict(device_type="sot_mram", device_params=sot_default_params(aspect_ratio=2.0), max_current=5e3)
VCMA = dict(device_type="vcma_mram", max_current=5e3,
            device_params=vcma_default_params(aspect_ratio=0.5, reference_magnetization=np.array([0.0, 0.2, 1.0])))
STT = dict(device_type="stt_mram")
DEVICES = {"stt": STT, "sot": SOT, "vcma": VCMA}
FLAG_SENTINEL = 0xA5


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as stg
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return stg


def _unit(rng, *shape):
    v = rng.normal(0, 1, shape + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _limit(shape, mode):
    return {"individual": shape[0] * shape[1] - 1, "row": shape[0] - 1, "column": shape[1] - 1, "global": 0}[mode]


def _actions(rng, n, shape, mode, step, max_current=2e6):
    """[n, 3] ([n, 2] in 'global' mode).  The first half of the batch (whole wavefronts of it when there are several) addresses index
    (lane + step) mod (limit + 1), so neighbouring lanes of one wavefront touch different cells, rows and columns; the other lanes get
    fractional indices in [-1, limit + 1].  J reaches 1.5 x max_current, T runs from below 1e-12 to above max_duration; lanes
    8, 17, 26, ... are undriven (J = 0)."""
    J = rng.uniform(-1.5 * max_current, 1.5 * max_current, n)
    J[8::9] = 0.0
    if mode == "global":        # action[1] is what 'global' mode reads as the current
        return np.stack([rng.uniform(-2e6, 2e6, n), J], axis=1).astype(np.float32)
    lim = _limit(shape, mode)
    idx = rng.uniform(-1.0, lim + 1.0, n)
    k = (n + 1) // 2
    idx[:k] = (np.arange(k) + step) % (lim + 1)
    return np.stack([idx, J, rng.uniform(-1e-10, 6e-9, n)], axis=1).astype(np.float32)


def _snap(env, out):
    obs, r, te, tr, info = out
    st = env.get_state()
    c = lambda t: t.cpu().numpy().copy()
    return dict(obs=c(obs), reward=c(info["reward_f64"]), reward32=c(r), term=c(te), trunc=c(tr), energy=c(info["energy"]),
                pattern=c(st["pattern"]), target=c(st["target"]), total_energy=c(st["total_energy"]), step_count=c(st["step_count"]))


def _max_diff(a, b, ctx):
    """max |a - b| over the entries that are not NaN; NaN exactly where the other side has NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), ctx
    ok = ~np.isnan(a)
    return float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0


def _compare(h, o, ctx):
    """One step's outputs and state, HIP against oracle, at the project's tolerances.  Returns the worst |dm|."""
    dm = _max_diff(h["pattern"], o["pattern"], ctx)
    assert dm <= 1e-11, (ctx, dm)
    assert np.allclose(h["obs"], o["obs"], rtol=3e-7, atol=1e-10, equal_nan=True), ctx
    assert np.allclose(h["reward"], o["reward"], rtol=1e-9, atol=1e-9, equal_nan=True), ctx
    assert np.array_equal(h["reward32"], h["reward"].astype(np.float32), equal_nan=True), ctx
    assert np.array_equal(h["term"], o["term"]) and np.array_equal(h["trunc"], o["trunc"]), ctx
    assert np.allclose(h["energy"], o["energy"], rtol=1e-10, atol=0, equal_nan=True), ctx
    assert np.allclose(h["total_energy"], o["total_energy"], rtol=1e-10, atol=0, equal_nan=True), ctx
    assert np.array_equal(h["step_count"], o["step_count"]) and np.array_equal(h["target"], o["target"]), ctx
    return dm


def _similarity(snap, n_dev):
    return (snap["pattern"] * snap["target"]).reshape(n_dev, 3, -1).sum(axis=1).mean(axis=0)


def _threshold(n_dev):
    """About 0.3 standard deviations of the similarity of a random pattern with a +-z target: roughly four arrays in ten start above it."""
    return 0.3 / np.sqrt(3.0 * n_dev)


# ------------------------------------------------------------------------------------------------
# a. shape x mode x kernel table against the oracle
# ------------------------------------------------------------------------------------------------
# (shape, action mode, coupling type or None, observation mode, device, STG_ARRAY_VARIANT or None, N).  N is ragged for the kernel the
# case runs: 64-lane workgroups (LDS kernels) 1 / 65 / 130, 256-lane workgroups ('individual' kernel, 4 x 4 'global' register kernel)
# 1 / 257 / 300.
TABLE = [
    ((1, 1), "individual", "dipolar", "array", "stt", None, 257),
    ((1, 1), "individual", None, "vector", "stt", None, 1),
    ((1, 7), "column", "exchange", "vector", "stt", None, 65),
    ((1, 7), "row", "stray_field", "array", "stt", None, 130),
    ((7, 1), "row", "dipolar", "vector", "stt", None, 130),
    ((7, 1), "column", None, "array", "stt", None, 65),
    ((5, 3), "row", "dipolar", "vector", "sot", None, 130),
    ((5, 3), "column", "exchange", "array", "stt", None, 65),
    ((5, 3), "individual", "stray_field", "array", "vcma", None, 257),
    ((3, 5), "row", "exchange", "array", "vcma", None, 65),
    ((3, 5), "column", "stray_field", "vector", "stt", None, 130),
    ((3, 5), "individual", "dipolar", "vector", "sot", None, 300),
    ((2, 3), "individual", None, "vector", "vcma", None, 1),
    ((5, 5), "global", "stray_field", "vector", "stt", None, 130),
    ((5, 5), "global", None, "array", "sot", None, 1),
    ((8, 8), "row", "dipolar", "array", "stt", None, 65),
    ((8, 8), "column", "exchange", "vector", "stt", None, 130),
    ((8, 8), "global", "stray_field", "array", "sot", None, 65),
    ((8, 8), "individual", "dipolar", "vector", "stt", None, 257),
    ((2, 32), "column", "dipolar", "vector", "vcma", None, 130),
    ((2, 32), "row", "exchange", "array", "stt", None, 65),
    ((2, 32), "individual", "stray_field", "array", "stt", None, 300),
    ((4, 4), "row", "dipolar", "array", "stt", "0", 130),
    ((4, 4), "column", "exchange", "vector", "sot", "0", 65),
    ((4, 4), "row", "stray_field", "vector", "vcma", "1", 65),
    ((4, 4), "column", "dipolar", "array", "stt", "1", 130),
    ((4, 4), "row", None, "array", "sot", "2", 1),
    ((4, 4), "column", "stray_field", "vector", "stt", "2", 130),
    ((4, 4), "global", "dipolar", "vector", "stt", None, 257),
    ((4, 4), "global", None, "array", "vcma", None, 300),
    ((4, 4), "global", "exchange", "array", "sot", "1", 1),
    ((4, 4), "global", "stray_field", "vector", "stt", "2", 130),
    ((4, 4), "global", "dipolar", "array", "stt", "0", 65),
    ((4, 4), "individual", "exchange", "array", "stt", None, 300),
]


def _case_id(c):
    (r, cc), mode, coup, obs, dev, variant, n = c
    return f"{r}x{cc}-{mode}-{coup or 'nocoupling'}-{obs}-{dev}-v{variant or 'default'}-N{n}"


def test_table_covers_what_it_claims():
    """The table itself (no GPU work): every shape of G20 plus 4 x 4 under the three variants in 'row' and 'column' mode, all modes,
    coupling types, observation modes and device types, every N of both workgroup sizes."""
    shapes = {c[0] for c in TABLE}
    assert shapes >= {(1, 1), (1, 7), (7, 1), (5, 3), (3, 5), (5, 5), (8, 8), (2, 32), (4, 4)}
    assert {(c[1], c[5]) for c in TABLE if c[0] == (4, 4) and c[1] in ("row", "column")} == {(m, v) for m in ("row", "column") for v in "012"}
    assert {c[1] for c in TABLE} == {"individual", "row", "column", "global"}
    assert {c[2] for c in TABLE} == {"dipolar", "exchange", "stray_field", None}
    assert {c[3] for c in TABLE} == {"array", "vector"} and {c[4] for c in TABLE} == {"stt", "sot", "vcma"}
    wide = [c for c in TABLE if c[1] == "individual" or (c[1] == "global" and c[0] == (4, 4) and c[5] in (None, "1"))]
    assert {c[6] for c in wide} == {1, 257, 300} and {c[6] for c in TABLE if c not in wide} == {1, 65, 130}
    assert 30 <= len(TABLE) <= 40


@pytest.mark.parametrize("case", TABLE, ids=_case_id)
def test_array_kernels_vs_oracle(stg, case, monkeypatch):
    from helpers import OracleArrayBackend
    shape, mode, coup, obs_mode, dev, variant, n = case
    if variant is None:
        monkeypatch.delenv("STG_ARRAY_VARIANT", raising=False)
    else:
        monkeypatch.setenv("STG_ARRAY_VARIANT", variant)
    n_dev = shape[0] * shape[1]
    seed = 1000 + TABLE.index(case)
    rng = np.random.default_rng(seed)
    init = _unit(rng, n, *shape)
    devkw = DEVICES[dev]
    acts = [_actions(rng, n, shape, mode, s, devkw.get("max_current", 2e6)) for s in range(4)]
    thr = _threshold(n_dev)
    kw = dict(action_mode=mode, include_coupling=coup is not None, coupling_type=coup or "dipolar", coupling_strength=0.2,
              observation_mode=obs_mode, success_threshold=thr, max_steps=3, **devkw)
    runs = []
    for backend in (OracleArrayBackend, None):
        env = stg.SpinTorqueArrayVecEnv(n, shape, backend=backend, **kw)
        obs, _ = env.reset(options={"initial_pattern": init})
        rec = [obs.cpu().numpy().copy()]
        for a in acts:
            rec.append(_snap(env, env.step(torch.from_numpy(a))))
        env.close()
        runs.append(rec)
    ora, hip = runs
    # no similarity within 1e-9 of the threshold (oracle alone): a flipped flag below is a wrong flag, not a tie
    for s in range(1, 5):
        assert np.abs(_similarity(ora[s], n_dev) - thr).min() > 1e-9, (s, "pick another seed")
    assert np.allclose(hip[0], ora[0], rtol=2e-7, atol=1e-12)
    worst = max(_compare(hip[s], ora[s], (_case_id(case), s)) for s in range(1, 5))
    print(f"array-dm {_case_id(case)} worst |dm| = {worst:.3e}")
    assert not hip[2]["trunc"].any() and hip[3]["trunc"].all() and hip[4]["trunc"].all()          # max_steps = 3
    assert np.array_equal(hip[4]["step_count"], np.full(n, 4, dtype=np.int32))
    if n > 1:
        t = np.concatenate([hip[s]["term"] for s in range(1, 5)])
        assert t.any() and not t.all()
        moved = np.abs(hip[1]["pattern"] - init.reshape(n, -1).T).max(axis=0) > 1e-6
        assert moved[np.arange(n) % 9 != 8].all() and not moved[8::9].any()                       # driven arrays move, undriven do not


# ------------------------------------------------------------------------------------------------
# a2. non-default env configuration
# ------------------------------------------------------------------------------------------------
CONFIG_CASES = [((1, 1), "individual", 257), ((4, 4), "global", 257)]
CONFIG_KW = dict(temperature=250.0, max_duration=2e-9, energy_penalty_weight=0.3, observation_mode="vector")


@pytest.mark.parametrize("case", CONFIG_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1]}-N{c[2]}")
def test_non_default_temperature_duration_limit_and_energy_weight_vs_oracle(stg, case):
    """temperature = 250, max_duration = 2e-9, energy_penalty_weight = 0.3 in 'vector' observations, on the smallest 'individual' and 'global'
    shapes of the table: four steps one at a time and the same four in one step_many launch, against the oracle stepped one at a time.  The
    configuration is not a no-op: the oracle under the default configuration gives other observations and rewards."""
    from helpers import OracleArrayBackend
    shape, mode, n = case
    n_dev, K = shape[0] * shape[1], 4
    rng = np.random.default_rng(3000 + CONFIG_CASES.index(case))
    init = _unit(rng, n, *shape)
    acts = [_actions(rng, n, shape, mode, s) for s in range(K)]
    thr = _threshold(n_dev)
    base = dict(action_mode=mode, coupling_strength=0.2, success_threshold=thr, max_steps=3)

    def stepped(backend, **kw):
        env = stg.SpinTorqueArrayVecEnv(n, shape, backend=backend, **base, **kw)
        obs, _ = env.reset(options={"initial_pattern": init})
        rec = [obs.cpu().numpy().copy()] + [_snap(env, env.step(torch.from_numpy(a))) for a in acts]
        env.close()
        return rec
    ora, hip = stepped(OracleArrayBackend, **CONFIG_KW), stepped(None, **CONFIG_KW)
    for s in range(1, K + 1):
        assert np.abs(_similarity(ora[s], n_dev) - thr).min() > 1e-9, (s, "pick another seed")
    assert np.allclose(hip[0], ora[0], rtol=2e-7, atol=1e-12)
    worst = max(_compare(hip[s], ora[s], (case, s)) for s in range(1, K + 1))
    print(f"array-dm non-default configuration {shape} {mode} worst |dm| = {worst:.3e}")
    env = stg.SpinTorqueArrayVecEnv(n, shape, **base, **CONFIG_KW)
    env.reset(options={"initial_pattern": init})
    obs, r, te, tr, info = env.step_many(torch.from_numpy(np.stack(acts)))
    c = lambda t: t.cpu().numpy().copy()
    many = dict(obs=c(obs), reward=c(info["reward_f64"]), reward32=c(r), term=c(te), trunc=c(tr), energy=c(info["energy"]))
    last = _snap(env, (obs[-1], r[-1], te[-1], tr[-1], dict(reward_f64=info["reward_f64"][-1], energy=info["energy"][-1])))
    env.close()
    for s in range(K):
        ctx = (case, "step_many", s)
        o = ora[s + 1]
        assert np.allclose(many["obs"][s], o["obs"], rtol=3e-7, atol=1e-10, equal_nan=True), ctx
        assert np.allclose(many["reward"][s], o["reward"], rtol=1e-9, atol=1e-9, equal_nan=True), ctx
        assert np.array_equal(many["term"][s], o["term"]) and np.array_equal(many["trunc"][s], o["trunc"]), ctx
        assert np.allclose(many["energy"][s], o["energy"], rtol=1e-10, atol=0, equal_nan=True), ctx
    _compare(last, ora[K], (case, "step_many", "state"))
    # what the configuration changes: the temperature entry of the vector observation, the energy term of the reward, the duration clamp
    dflt = stepped(OracleArrayBackend, observation_mode="vector")
    assert not np.allclose(ora[1]["obs"], dflt[1]["obs"], rtol=1e-3, atol=1e-6) and (ora[1]["reward"] != dflt[1]["reward"]).any()
    if mode != "global":            # ('global' mode has no duration in its action -- the pulse is 1 ns -- and its energy term is ~1e-9 of the reward)
        assert not np.allclose(ora[1]["energy"], dflt[1]["energy"], rtol=1e-3, atol=0)
        assert not np.allclose(ora[1]["reward"], dflt[1]["reward"], rtol=1e-3, atol=1e-6)


# ------------------------------------------------------------------------------------------------
# b. every output written, nothing else touched
# ------------------------------------------------------------------------------------------------
GUARD_CASES = [
    ((8, 8), "row", "array", None, 130),            # general LDS kernel, > 48 KB of LDS
    ((3, 5), "column", "vector", None, 130),        # general LDS kernel, 'vector' rows with n != 16
    ((3, 5), "individual", "vector", None, 300),    # streaming kernel, n != 16
    ((8, 8), "individual", "array", None, 300),
    ((4, 4), "row", "vector", None, 130),           # 4 x 4 LDS kernel
    ((4, 4), "global", "vector", None, 300),        # register kernel: buffer stores, which drop out-of-range stores silently
    ((4, 4), "global", "array", None, 300),
]


@pytest.mark.parametrize("case", GUARD_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1]}-{c[2]}-N{c[4]}")
def test_step_writes_every_output_and_nothing_else(stg, case, monkeypatch):
    """The step's outputs point into the middle of larger, sentinel-filled tensors (NaN; 0xA5 for the byte flags): after one step every
    element inside is overwritten, with what a plain run writes, and every guard element is untouched."""
    shape, mode, obs_mode, variant, n = case
    monkeypatch.delenv("STG_ARRAY_VARIANT", raising=False)
    rng = np.random.default_rng(77)
    init = _unit(rng, n, *shape)
    a = torch.from_numpy(_actions(rng, n, shape, mode, 0))
    kw = dict(action_mode=mode, coupling_strength=0.2, observation_mode=obs_mode, success_threshold=_threshold(shape[0] * shape[1]), max_steps=1)
    plain = stg.SpinTorqueArrayVecEnv(n, shape, **kw)
    plain.reset(options={"initial_pattern": init})
    want = _snap(plain, plain.step(a))
    plain.close()
    env = stg.SpinTorqueArrayVecEnv(n, shape, **kw)
    env.reset(options={"initial_pattern": init})
    b = env.backend
    pad_rows, pad = 3, 96
    big = dict(obs=torch.full((b.obs_dim + 2 * pad_rows, n), float("nan"), dtype=torch.float32, device="cuda"))
    inner = dict(obs=big["obs"][pad_rows:pad_rows + b.obs_dim])
    for name, dtype, fill in (("reward", torch.float32, float("nan")), ("reward64", torch.float64, float("nan")),
                              ("energy", torch.float64, float("nan")), ("terminated", torch.uint8, FLAG_SENTINEL),
                              ("truncated", torch.uint8, FLAG_SENTINEL)):
        big[name] = torch.full((n + 2 * pad,), fill, dtype=dtype, device="cuda")
        inner[name] = big[name][pad:pad + n]
    for name, t in inner.items():
        assert t.is_contiguous()
        setattr(b, name, t)
    got = _snap(env, env.step(a))
    torch.cuda.synchronize()
    env.close()
    for name, t in big.items():
        guard = torch.cat([t[:pad_rows].reshape(-1), t[pad_rows + b.obs_dim:].reshape(-1)]) if name == "obs" else torch.cat([t[:pad], t[pad + n:]])
        if t.dtype == torch.uint8:
            assert bool((guard == FLAG_SENTINEL).all()), name
            assert bool((inner[name] <= 1).all()), name
        else:
            assert bool(torch.isnan(guard).all()), name
            assert not bool(torch.isnan(inner[name]).any()), name
    for key in ("obs", "reward", "reward32", "term", "trunc", "energy", "pattern", "total_energy", "step_count"):
        assert np.array_equal(got[key], want[key]), key
    assert want["trunc"].all() and want["energy"].max() > 0


# ------------------------------------------------------------------------------------------------
# c. masked reset
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("new_target", [False, True], ids=["keep-target", "new-target"])
def test_masked_reset(stg, new_target):
    """3 x 5, N = 130: after two steps every third array restarts from a new pattern (and, second case, a new target).  The others keep
    pattern, target, total energy and step count bit for bit; the returned observation is the oracle's for all arrays; two further steps
    match the oracle, the arrays that did not restart running into max_steps while the others do not."""
    from helpers import OracleArrayBackend
    n, shape = 130, (3, 5)
    rng = np.random.default_rng(41)
    init, init2 = _unit(rng, n, *shape), _unit(rng, n, *shape)
    tgt2 = _unit(rng, n, *shape)
    mask = (np.arange(n) % 3 == 0)
    acts = [_actions(rng, n, shape, "column", s) for s in range(4)]
    thr = _threshold(15)
    opts = {"mask": torch.from_numpy(mask), "initial_pattern": init2}
    if new_target:
        opts["target_pattern"] = tgt2
    runs = []
    for backend in (OracleArrayBackend, None):
        env = stg.SpinTorqueArrayVecEnv(n, shape, action_mode="column", coupling_type="stray_field", coupling_strength=0.2,
                                        observation_mode="vector", success_threshold=thr, max_steps=3, backend=backend)
        env.reset(options={"initial_pattern": init})
        rec = [_snap(env, env.step(torch.from_numpy(a))) for a in acts[:2]]
        obs, _ = env.reset(options=opts)
        st = {k: v.cpu().numpy().copy() for k, v in env.get_state().items()}
        rec.append(dict(obs=obs.cpu().numpy().copy(), **st))
        rec += [_snap(env, env.step(torch.from_numpy(a))) for a in acts[2:]]
        env.close()
        runs.append(rec)
    ora, hip = runs
    for s in (0, 1, 3, 4):
        assert np.abs(_similarity(ora[s], 15) - thr).min() > 1e-9, s
        _compare(hip[s], ora[s], ("masked reset", s))
    before, after = hip[1], hip[2]
    keep = ~mask
    for key in ("pattern", "target", "total_energy", "step_count"):
        assert np.array_equal(after[key][..., keep], before[key][..., keep]), key
    assert np.array_equal(after["pattern"][:, mask], init2.reshape(n, -1).T[:, mask])
    want_t = tgt2.reshape(n, -1).T[:, mask] if new_target else before["target"][:, mask]
    assert np.array_equal(after["target"][:, mask], want_t)
    assert not after["total_energy"][mask].any() and not after["step_count"][mask].any() and (after["step_count"][keep] == 2).all()
    assert np.allclose(after["obs"], ora[2]["obs"], rtol=2e-7, atol=1e-12)
    for key in ("pattern", "target", "total_energy", "step_count"):
        assert np.allclose(after[key], ora[2][key], rtol=1e-10, atol=1e-11), key
    for s in (3, 4):
        assert hip[s]["trunc"][keep].all() and not hip[s]["trunc"][mask].any()
    assert np.array_equal(hip[4]["step_count"], np.where(mask, 2, 4))


# ------------------------------------------------------------------------------------------------
# d. device-side random reset
# ------------------------------------------------------------------------------------------------
def _patterns(env):
    return env.get_state()["pattern"].cpu().numpy().copy()


def _check_draw(oracle, got, seed, env_ids, resets, n_dev, ctx):
    """|m_hip - m_oracle| <= 2 * 2e-5 / |z| per component: the kernel's fp32 Box-Muller normals are within 2e-5 of the oracle's
    (test_thermal_normals_moments_and_oracle_stream), and normalising divides that by the un-normalised norm |z|."""
    worst = 0.0
    for col, (eid, rs) in enumerate(zip(env_ids, resets)):
        m, z = oracle.array_reset_draw(seed, int(eid), int(rs), n_dev)
        err = np.abs(got[:, col].reshape(n_dev, 3) - m)
        bound = 2 * 2e-5 / z
        assert (err <= bound[:, None]).all(), (ctx, int(eid), float((err / bound[:, None]).max()))
        worst = max(worst, float((err / bound[:, None]).max()))
    return worst


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (4, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_random_reset(stg, shape, oracle_mod):
    n, n_dev, seed = 200, shape[0] * shape[1], 0x5EED0000 + shape[1]
    env = stg.SpinTorqueArrayVecEnv(n, shape, action_mode="individual")
    again = stg.SpinTorqueArrayVecEnv(n, shape, action_mode="individual")
    part = stg.SpinTorqueArrayVecEnv(72, shape, action_mode="individual", env_id0=128)
    ids = np.arange(n)
    # first reset: the oracle's draw, unit vectors, the same batch for the same seed, a window of it for env_id0 = 128
    env.backend.reset(None, None, None, seed)
    p1 = _patterns(env)
    w1 = _check_draw(oracle_mod, p1, seed, ids, np.zeros(n), n_dev, "first")
    assert np.abs(np.linalg.norm(p1.reshape(n_dev, 3, n), axis=1) - 1).max() < 1e-12
    again.backend.reset(None, None, None, seed)
    assert np.array_equal(_patterns(again), p1)
    part.backend.reset(None, None, None, seed)
    assert np.array_equal(_patterns(part), p1[:, 128:200])
    again.backend.reset(None, None, None, seed + 1)
    assert np.abs(_patterns(again) - p1).max() > 0.1
    # second reset, masked: the selected arrays draw with resets = 1, the others keep their pattern
    mask = (ids % 3 == 1)
    env.backend.reset(torch.from_numpy(mask), None, None, seed)
    p2 = _patterns(env)
    assert np.array_equal(p2[:, ~mask], p1[:, ~mask])
    assert (np.abs(p2[:, mask] - p1[:, mask]).max(axis=0) > 1e-3).all()
    w2 = _check_draw(oracle_mod, p2[:, mask], seed, ids[mask], np.ones(mask.sum()), n_dev, "second")
    # third reset, all arrays: the counters advanced only where the second one drew
    env.backend.reset(None, None, None, seed)
    p3 = _patterns(env)
    w3 = _check_draw(oracle_mod, p3, seed, ids, np.where(mask, 2, 1), n_dev, "third")
    print(f"array-reset {shape[0]}x{shape[1]} worst error / bound = {max(w1, w2, w3):.3f}")
    # and the oracle backend behind the same host code draws the same thing
    from helpers import OracleArrayBackend
    oenv = stg.SpinTorqueArrayVecEnv(72, shape, action_mode="individual", env_id0=128, backend=OracleArrayBackend)
    oenv.backend.reset(None, None, None, seed)
    assert np.array_equal(_patterns(oenv)[:, 5], oracle_mod.array_reset_draw(seed, 133, 0, n_dev)[0].reshape(-1))
    _check_draw(oracle_mod, p1[:, 128:200], seed, ids[128:200], np.zeros(72), n_dev, "window")
    for e in (env, again, part):
        e.close()


@pytest.mark.parametrize("shape", [(3, 5), (5, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_reset_default_target_is_the_checkerboard(stg, shape):
    """stg_array_reset without a target on a fresh context: the kernel's own checkerboard over (row, column) of a non-square array."""
    n = 70
    env = stg.SpinTorqueArrayVecEnv(n, shape, observation_mode="vector")
    obs = env.backend.reset(None, None, None, 5).cpu().numpy().copy()
    st = env.get_state()
    want = stg.array_env.checkerboard_pattern(*shape).reshape(-1)
    tgt = st["target"].cpu().numpy()
    assert np.array_equal(tgt, np.repeat(want[:, None], n, axis=1))
    n3 = 3 * shape[0] * shape[1]
    assert np.array_equal(obs[n3:2 * n3], tgt.astype(np.float32)) and np.array_equal(obs[:n3], st["pattern"].cpu().numpy().astype(np.float32))
    env.close()


# ------------------------------------------------------------------------------------------------
# e. NaN and infinite actions in a batch
# ------------------------------------------------------------------------------------------------
SPECIAL_LANES = [0, 63, 64, 129]          # first lane, last lane of the first wavefront, first of the second, the last (ragged) lane


@pytest.mark.parametrize("tag", ["nan_2x3_individual", "nan_3x3_global"])
def test_nan_and_infinite_actions_in_a_batch(stg, golden, tag):
    """The recorded NaN / inf episodes of the reference (G20) ride in four lanes of a batch of 130 whose other lanes do ordinary work.
    Those lanes match the recording and the oracle, NaN where they have NaN; every other lane is bit-identical to a run in which the four
    lanes carried ordinary actions."""
    from helpers import OracleArrayBackend
    from test_oracle_golden import G20_EPISODES, g20_check_step
    g = golden("G20_array_edges")
    k = [str(t) for t in g["episode_tags"]].index(tag)
    ckw, coup, dev, over = G20_EPISODES[tag]
    shape, mode = (ckw["rows"], ckw["cols"]), ckw["action_mode"]
    n, n_dev = 130, ckw["rows"] * ckw["cols"]
    rng = np.random.default_rng(5)
    init = _unit(rng, n, *shape)
    init[SPECIAL_LANES] = g[f"ep{k}_pattern"][0]
    g_acts = g[f"ep{k}_actions"]
    ordinary = [_actions(rng, n, shape, mode, s) for s in range(len(g_acts))]
    special = [a.copy() for a in ordinary]
    for a, ga in zip(special, g_acts):
        a[SPECIAL_LANES] = ga
    kw = dict(action_mode=mode, coupling_type=coup[0], coupling_strength=coup[1], observation_mode=ckw.get("obs_mode", "array"))
    runs = {}
    for name, backend, acts in (("hip", None, special), ("oracle", OracleArrayBackend, special), ("plain", None, ordinary)):
        env = stg.SpinTorqueArrayVecEnv(n, shape, backend=backend, **kw)
        env.reset(options={"initial_pattern": init})
        runs[name] = [_snap(env, env.step(torch.from_numpy(a))) for a in acts]
        env.close()
    others = np.setdiff1d(np.arange(n), SPECIAL_LANES)
    saw_nan = False
    for j in range(len(g_acts)):
        h, o, p = runs["hip"][j], runs["oracle"][j], runs["plain"][j]
        for lane in SPECIAL_LANES:
            g20_check_step(g, k, j, h["pattern"][:, lane], h["obs"][lane], h["reward"][lane], h["term"][lane], h["trunc"][lane],
                           h["energy"][lane], (tag, lane), pat_tol=1e-11, obs_tol=(3e-7, 1e-10), r_tol=1e-9, e_tol=1e-10)
        _compare(h, o, (tag, j))
        for key in ("obs", "reward", "reward32", "term", "trunc", "energy", "pattern", "total_energy", "step_count"):
            assert np.array_equal(h[key][others] if key == "obs" else h[key][..., others],
                                  p[key][others] if key == "obs" else p[key][..., others]), (tag, j, key)
        assert not np.isnan(h["pattern"][:, others]).any() and not np.isnan(h["reward"][others]).any()
        saw_nan = saw_nan or bool(np.isnan(h["reward"][SPECIAL_LANES]).any())
    assert saw_nan == (tag == "nan_2x3_individual")          # only a NaN duration leaves NaN behind; 'global' mode has no duration


@pytest.mark.parametrize("mode", ["individual", "row", "column"])
def test_nan_index_addresses_nothing(stg, mode):
    """A NaN index raises in the reference (the N = 1 facade mirrors that); in a batch it addresses nothing: pattern unchanged, energy 0,
    step count advanced, and the other lanes are what they are without it."""
    n, shape = 130, (3, 5)
    rng = np.random.default_rng(8)
    init = _unit(rng, n, *shape)
    ordinary = _actions(rng, n, shape, mode, 0)
    ordinary[SPECIAL_LANES, 1], ordinary[SPECIAL_LANES, 2] = 1.5e6, 1e-9     # (driven, so that an addressed cell would move)
    special = ordinary.copy()
    special[SPECIAL_LANES, 0] = np.nan
    snaps = []
    for a in (special, ordinary):
        env = stg.SpinTorqueArrayVecEnv(n, shape, action_mode=mode, coupling_strength=0.2, observation_mode="vector")
        env.reset(options={"initial_pattern": init})
        snaps.append(_snap(env, env.step(torch.from_numpy(a))))
        env.close()
    h, p = snaps
    start = init.reshape(n, -1).T
    assert np.array_equal(h["pattern"][:, SPECIAL_LANES], start[:, SPECIAL_LANES])
    assert np.abs(p["pattern"][:, SPECIAL_LANES] - start[:, SPECIAL_LANES]).max(axis=0).min() > 1e-6
    assert not h["energy"][SPECIAL_LANES].any() and not h["total_energy"][SPECIAL_LANES].any()
    assert (h["step_count"] == 1).all() and np.isfinite(h["reward"]).all() and np.isfinite(h["obs"]).all()
    assert np.array_equal(h["obs"][SPECIAL_LANES, :45], start[:, SPECIAL_LANES].T.astype(np.float32))
    others = np.setdiff1d(np.arange(n), SPECIAL_LANES)
    for key in ("reward", "term", "trunc", "energy", "pattern", "total_energy"):
        assert np.array_equal(h[key][..., others], p[key][..., others]), key
    assert np.array_equal(h["obs"][others], p["obs"][others])

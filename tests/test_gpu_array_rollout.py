"""stg_array_step_many on the MI355X: K fused steps of the array env with same-step auto-reset (csrc/stg_array.hip,
stg_array_step_many_kernel) against the CPU oracle and against the path that composes the same thing from stg_array_step and a masked
stg_array_reset per step (SpinTorqueArrayVecEnv.step_many(fused=False), itself checked against the oracle in test_array_rollout_host.py);
partition and ordering; every output written and nothing else; NaN lanes; set_state / get_resets; a captured graph.

Tolerances are those of test_gpu_array.py: pattern <= 1e-11, observation rtol 3e-7 / atol 1e-10, reward 1e-9 / 1e-9, energy rtol 1e-10, flags
and step counts equal.  A freshly drawn pattern agrees with stg_array_reset's draw to 1e-15 (same stream, same normalisation: room for
contraction differences only)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_array import DEVICES, FLAG_SENTINEL, SPECIAL_LANES, _actions, _max_diff, _similarity, _snap, _threshold, _unit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as stg
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return stg


def _c(t):
    return t.cpu().numpy().copy()


def _many(env, acts, **kw):
    """One step_many call: outputs with a leading [K] (or 1), and the state after it."""
    obs, r, te, tr, info = env.step_many(torch.from_numpy(acts) if isinstance(acts, np.ndarray) else acts, **kw)
    out = dict(obs=_c(obs), reward=_c(info["reward_f64"]), reward32=_c(r), term=_c(te), trunc=_c(tr), energy=_c(info["energy"]))
    if "final_obs" in info:
        out.update(final_obs=_c(info["final_obs"]), done=_c(info["done"]))
    st = env.get_state()
    out.update({k: _c(v) for k, v in st.items()})
    if hasattr(env.backend, "get_resets"):
        out["resets"] = _c(env.backend.get_resets())
    return out


def _outputs_close(h, o, ctx):
    """Per-step outputs ([K]-leading or one step's) at the project's tolerances."""
    assert np.allclose(h["obs"], o["obs"], rtol=3e-7, atol=1e-10, equal_nan=True), ctx
    assert np.allclose(h["reward"], o["reward"], rtol=1e-9, atol=1e-9, equal_nan=True), ctx
    assert np.array_equal(h["reward32"], h["reward"].astype(np.float32), equal_nan=True), ctx
    assert np.array_equal(h["term"], o["term"]) and np.array_equal(h["trunc"], o["trunc"]), ctx
    assert np.allclose(h["energy"], o["energy"], rtol=1e-10, atol=0, equal_nan=True), ctx


def _state_close(h, o, ctx):
    dm = _max_diff(h["pattern"], o["pattern"], ctx)
    assert dm <= 1e-11, (ctx, dm)
    assert np.allclose(h["total_energy"], o["total_energy"], rtol=1e-10, atol=0, equal_nan=True), ctx
    assert np.array_equal(h["step_count"], o["step_count"]) and np.array_equal(h["target"], o["target"]), ctx
    return dm


BITWISE = ("obs", "reward", "reward32", "term", "trunc", "energy", "final_obs", "done")
STATE = ("pattern", "target", "total_energy", "step_count", "resets")


def _same_bits(a, b, keys, ctx, cols=None):
    for key in keys:
        x, y = a[key], b[key]
        if cols is not None:
            x = x[:, cols] if key in BITWISE else x[..., cols]
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (ctx, key)


# ------------------------------------------------------------------------------------------------
# a. fused against the oracle, autoreset off
# ------------------------------------------------------------------------------------------------
# (shape, action mode, coupling type or None, observation mode, device, N): the NDEV = 16 kernel in every action mode, the generic kernel
# below and above 64 KB of LDS, one wavefront plus one lane / two plus two, a single array, no coupling
ORACLE_CASES = [
    ((4, 4), "individual", "dipolar", "array", "stt", 130),
    ((4, 4), "row", "exchange", "vector", "stt", 130),
    ((4, 4), "column", "stray_field", "array", "vcma", 130),
    ((4, 4), "global", "dipolar", "vector", "stt", 130),
    ((3, 5), "row", "dipolar", "vector", "sot", 65),
    ((8, 8), "global", "stray_field", "array", "stt", 65),
    ((8, 8), "individual", "dipolar", "vector", "stt", 65),
    ((2, 32), "column", "dipolar", "vector", "vcma", 130),
    ((1, 1), "individual", "dipolar", "array", "stt", 1),
    ((3, 5), "column", None, "array", "stt", 130),
]


def _oc_id(c):
    (r, cc), mode, coup, obs, dev, n = c
    return f"{r}x{cc}-{mode}-{coup or 'nocoupling'}-{obs}-{dev}-N{n}"


@pytest.mark.parametrize("case", ORACLE_CASES, ids=_oc_id)
def test_fused_rollout_vs_oracle(stg, case):
    """K = 5 in one launch, out_every, no auto-reset, max_steps = 3: truncation starts mid-rollout and the done arrays keep stepping, as in
    the reference.  The oracle is stepped one step at a time."""
    from helpers import OracleArrayBackend
    shape, mode, coup, obs_mode, dev, n = case
    n_dev, K = shape[0] * shape[1], 5
    rng = np.random.default_rng(2000 + ORACLE_CASES.index(case))
    init = _unit(rng, n, *shape)
    devkw = DEVICES[dev]
    acts = np.stack([_actions(rng, n, shape, mode, s, devkw.get("max_current", 2e6)) for s in range(K)])
    thr = _threshold(n_dev)
    kw = dict(action_mode=mode, include_coupling=coup is not None, coupling_type=coup or "dipolar", coupling_strength=0.2,
              observation_mode=obs_mode, success_threshold=thr, max_steps=3, **devkw)
    oenv = stg.SpinTorqueArrayVecEnv(n, shape, backend=OracleArrayBackend, **kw)
    oenv.reset(options={"initial_pattern": init})
    ora = [_snap(oenv, oenv.step(torch.from_numpy(a))) for a in acts]
    # no similarity within 1e-9 of the threshold (oracle alone): a flipped flag below is a wrong flag, not a tie
    for s in range(K):
        assert np.abs(_similarity(ora[s], n_dev) - thr).min() > 1e-9, (s, "pick another seed")
    env = stg.SpinTorqueArrayVecEnv(n, shape, **kw)
    env.reset(options={"initial_pattern": init})
    hip = _many(env, acts)
    env.close()
    assert hip["obs"].shape == (K, n, oenv.backend.obs_dim)
    for s in range(K):
        _outputs_close({k: hip[k][s] for k in ("obs", "reward", "reward32", "term", "trunc", "energy")}, ora[s], (_oc_id(case), s))
    worst = _state_close(hip, ora[-1], _oc_id(case))
    print(f"array-rollout-dm {_oc_id(case)} worst |dm| after {K} steps = {worst:.3e}")
    assert not hip["trunc"][1].any() and hip["trunc"][2:].all()                                   # max_steps = 3
    assert np.array_equal(hip["step_count"], np.full(n, K, dtype=np.int32)) and not hip["resets"].any()
    if n > 1:
        assert hip["term"].any() and not hip["term"].all()
        moved = np.abs(ora[0]["pattern"] - init.reshape(n, -1).T).max(axis=0) > 1e-6
        assert moved[np.arange(n) % 9 != 8].all() and not moved[8::9].any()                       # driven arrays move, undriven do not


# ------------------------------------------------------------------------------------------------
# b. fused against composed, autoreset on
# ------------------------------------------------------------------------------------------------
AUTORESET_CASES = [((4, 4), "global", "array"), ((4, 4), "row", "vector"), ((3, 5), "individual", "vector"), ((8, 8), "row", "array")]
N_AR, K_AR, SENTINEL = 130, 6, -7.0


def _finish_threshold(n_dev):
    """One standard deviation of the similarity of a random pattern with a random target of unit vectors (1 / sqrt(3 n)): about one fresh
    episode in six starts above it, so over the three to six episodes an array sees in K = 6 steps of max_steps = 2 roughly half the
    arrays terminate at least once.  (Every array also truncates: with max_steps = 2 'finishes at least once' can only discriminate
    through termination.  The targets are random per array because 'global' mode drives all cells of an array to the same pole, where
    the similarity with the +-z checkerboard is zero for every array.)"""
    return 1.0 / np.sqrt(3.0 * n_dev)


def _autoreset_pair(stg, shape, mode, obs_mode, out_every=True, seed=0):
    rng = np.random.default_rng(3000 + 10 * shape[0] + len(mode) + seed)
    init, target = _unit(rng, N_AR, *shape), _unit(rng, N_AR, *shape)
    acts = np.stack([_actions(rng, N_AR, shape, mode, s) for s in range(K_AR)])
    kw = dict(action_mode=mode, coupling_strength=0.2, observation_mode=obs_mode, success_threshold=_finish_threshold(shape[0] * shape[1]),
              max_steps=2)
    runs = []
    for fused in (False, True):
        env = stg.SpinTorqueArrayVecEnv(N_AR, shape, **kw)
        env.reset(seed=17, options={"initial_pattern": init, "target_pattern": target})
        k_out = K_AR if out_every else 1
        fo = torch.full((k_out, env.backend.obs_dim, N_AR), SENTINEL, dtype=torch.float32, device="cuda")
        runs.append(_many(env, acts, autoreset=True, fused=fused, out_every=out_every, out={"final_obs": fo}))
        env.close()
    return runs


@pytest.mark.parametrize("case", AUTORESET_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1]}-{c[2]}")
def test_fused_autoreset_vs_composed(stg, case):
    shape, mode, obs_mode = case
    comp, fus = _autoreset_pair(stg, shape, mode, obs_mode)
    # the composed run alone: resets happen, and not everywhere at once -- the test cannot pass by never (or always) resetting
    frac_term = comp["term"].any(axis=0).mean()
    frac_done = comp["done"].mean()
    print(f"array-autoreset {shape} {mode}: arrays that terminate at least once {frac_term:.2f}, done entries {frac_done:.2f}")
    assert 0.2 <= frac_term <= 0.8 and 0.2 <= frac_done <= 0.8
    assert comp["done"].any(axis=0).all() and comp["resets"].min() >= 3 and comp["resets"].max() > 3
    done = comp["done"]
    for key in ("term", "trunc", "done", "step_count", "resets", "target"):
        assert np.array_equal(fus[key], comp[key]), key
    assert (fus["final_obs"][~done] == SENTINEL).all() and (comp["final_obs"][~done] == SENTINEL).all()
    assert np.allclose(fus["final_obs"][done], comp["final_obs"][done], rtol=3e-7, atol=1e-10)
    _outputs_close(fus, comp, case)
    _state_close(fus, comp, case)
    # arrays that finished at the last step hold a freshly drawn pattern: the same draw as stg_array_reset's
    fresh = done[-1]
    assert fresh.any() and not fresh.all()
    assert np.abs(fus["pattern"][:, fresh] - comp["pattern"][:, fresh]).max() <= 1e-15
    assert np.abs(np.linalg.norm(fus["pattern"][:, fresh].reshape(-1, 3, fresh.sum()), axis=1) - 1).max() < 1e-12
    assert (fus["step_count"][fresh] == 0).all() and not fus["total_energy"][fresh].any()
    if obs_mode == "vector":       # the new episode's first observation: steps-remaining 1, energy 0
        n6 = 6 * shape[0] * shape[1]
        assert (fus["obs"][done][:, n6 + 1] == 1.0).all() and (fus["obs"][done][:, n6 + 2] == 0.0).all()


def test_fused_autoreset_last_step_only(stg):
    """out_every=False: the outputs are the last step's of the out_every=True run and the state is the same, bit for bit."""
    shape, mode, obs_mode = AUTORESET_CASES[1]
    _, every = _autoreset_pair(stg, shape, mode, obs_mode)
    comp, last = _autoreset_pair(stg, shape, mode, obs_mode, out_every=False)
    for key in BITWISE:
        assert last[key].shape[0] == 1
        if key == "final_obs":
            d = every["done"][-1]
            assert np.array_equal(last[key][0][d], every[key][-1][d]) and (last[key][0][~d] == SENTINEL).all()
        else:
            assert np.array_equal(last[key][0], every[key][-1]), key
    _same_bits(last, every, STATE, "state")
    for key in ("term", "trunc", "done", "resets", "step_count"):
        assert np.array_equal(last[key], comp[key]), key


# ------------------------------------------------------------------------------------------------
# c. partition and ordering
# ------------------------------------------------------------------------------------------------
def _partition_env(stg, n, init, env_id0=0, shape=(3, 5)):
    env = stg.SpinTorqueArrayVecEnv(n, shape, action_mode="column", coupling_strength=0.2, observation_mode="vector",
                                    success_threshold=_finish_threshold(shape[0] * shape[1]), max_steps=2, env_id0=env_id0)
    env.reset(seed=23, options={"initial_pattern": init})
    return env


def test_rollout_partitions(stg):
    """K = 4 in one launch equals two launches of K = 2 (the state goes through HBM in between), and an env that holds arrays 64..129
    (env_id0 = 64, N = 66) equals those columns of the N = 130 run -- bit for bit, with auto-reset on."""
    n, shape = 130, (3, 5)
    rng = np.random.default_rng(31)
    init = _unit(rng, n, *shape)
    acts = np.stack([_actions(rng, n, shape, "column", s) for s in range(4)])
    env = _partition_env(stg, n, init)
    whole = _many(env, acts, autoreset=True)
    env.close()
    assert whole["resets"].max() >= 2 and whole["term"].any()
    env = _partition_env(stg, n, init)
    first = _many(env, acts[:2], autoreset=True)
    second = _many(env, acts[2:], autoreset=True)
    env.close()
    for key in BITWISE:
        got = np.concatenate([first[key], second[key]])
        assert np.array_equal(got, whole[key], equal_nan=True), key
    _same_bits(second, whole, STATE, "two launches")
    env = _partition_env(stg, 66, init[64:], env_id0=64)
    part = _many(env, np.ascontiguousarray(acts[:, 64:]), autoreset=True)
    env.close()
    _same_bits(whole, part, BITWISE + STATE, "window", cols=slice(64, 130))


# ------------------------------------------------------------------------------------------------
# d. every output written, nothing else touched
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [((8, 8), "row"), ((4, 4), "global")], ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1]}")
def test_rollout_writes_every_output_and_nothing_else(stg, case):
    """The [K]-leading outputs and final_obs point into the middle of larger sentinel-filled tensors (NaN; 0xA5 for the byte flags): after
    K = 3 steps every element inside is overwritten with what a plain run writes -- final_obs exactly where an array finished -- and every
    guard element is untouched."""
    shape, mode = case
    n, K = 130, 3
    rng = np.random.default_rng(78)
    init = _unit(rng, n, *shape)
    acts = np.stack([_actions(rng, n, shape, mode, s) for s in range(K)])
    kw = dict(action_mode=mode, coupling_strength=0.2, observation_mode="vector", success_threshold=_finish_threshold(shape[0] * shape[1]),
              max_steps=2)
    plain = stg.SpinTorqueArrayVecEnv(n, shape, **kw)
    plain.reset(seed=3, options={"initial_pattern": init})
    want = _many(plain, acts, autoreset=True)
    plain.close()
    env = stg.SpinTorqueArrayVecEnv(n, shape, **kw)
    env.reset(seed=3, options={"initial_pattern": init})
    obs_dim, pad_rows, pad = env.backend.obs_dim, 3, 96
    big, inner = {}, {}
    for name in ("obs", "final_obs"):
        big[name] = torch.full((K * obs_dim + 2 * pad_rows, n), float("nan"), dtype=torch.float32, device="cuda")
        inner[name] = big[name][pad_rows:pad_rows + K * obs_dim].view(K, obs_dim, n)
    for name, dtype, fill in (("reward", torch.float32, float("nan")), ("reward64", torch.float64, float("nan")),
                              ("energy", torch.float64, float("nan")), ("terminated", torch.uint8, FLAG_SENTINEL),
                              ("truncated", torch.uint8, FLAG_SENTINEL)):
        big[name] = torch.full((K * n + 2 * pad,), fill, dtype=dtype, device="cuda")
        inner[name] = big[name][pad:pad + K * n].view(K, n)
    got = _many(env, acts, autoreset=True, out=inner)
    torch.cuda.synchronize()
    env.close()
    done = want["done"]
    assert done.any() and not done.all()
    for name, t in big.items():
        flat = t.reshape(-1)
        lo = pad_rows * n if name in ("obs", "final_obs") else pad
        guard = torch.cat([flat[:lo], flat[flat.numel() - lo:]])
        if t.dtype == torch.uint8:
            assert bool((guard == FLAG_SENTINEL).all()), name
            assert bool((inner[name] <= 1).all()), name
        else:
            assert bool(torch.isnan(guard).all()), name
            if name == "final_obs":
                fo = np.isnan(inner[name].cpu().numpy())                               # [K, obs_dim, n]: a column is written whole or not at all
                assert np.array_equal(fo.all(axis=1), ~done) and np.array_equal(fo.any(axis=1), ~done)
            else:
                assert not bool(torch.isnan(inner[name]).any()), name
    _same_bits(got, want, [k for k in BITWISE if k != "final_obs"] + list(STATE), "guarded run")
    assert np.array_equal(got["final_obs"][done], want["final_obs"][done])


# ------------------------------------------------------------------------------------------------
# e. NaN lanes
# ------------------------------------------------------------------------------------------------
def test_nan_duration_lanes_in_a_rollout(stg):
    """3 x 5 'individual', K = 4, max_steps = 3, auto-reset: four lanes carry a NaN duration at step 2 (they start opposite to the target, so
    none of them terminates before).  Every other lane is bit-identical to a run without them; the four lanes have NaN exactly where the
    composed path has NaN; they truncate at step 3, and what the auto-reset draws is finite."""
    n, shape, K = 130, (3, 5), 4
    rng = np.random.default_rng(9)
    init = _unit(rng, n, *shape)
    init[SPECIAL_LANES] = -stg.array_env.checkerboard_pattern(*shape)
    ordinary = np.stack([_actions(rng, n, shape, "individual", s) for s in range(K)])
    ordinary[:, SPECIAL_LANES, 1] = 1.5e6                  # driven, so that the NaN duration reaches the addressed cell
    special = ordinary.copy()
    special[1, SPECIAL_LANES, 2] = np.nan
    runs = {}
    for name, acts, fused in (("fused", special, True), ("composed", special, False), ("plain", ordinary, True)):
        env = stg.SpinTorqueArrayVecEnv(n, shape, action_mode="individual", coupling_strength=0.2, observation_mode="vector",
                                        success_threshold=_finish_threshold(15), max_steps=3)
        env.reset(seed=4, options={"initial_pattern": init})
        runs[name] = _many(env, acts, autoreset=True, fused=fused)
        env.close()
    f, c, p = runs["fused"], runs["composed"], runs["plain"]
    others = np.setdiff1d(np.arange(n), SPECIAL_LANES)
    _same_bits({k: f[k][:, others] if k in BITWISE else f[k][..., others] for k in BITWISE + STATE},
               {k: p[k][:, others] if k in BITWISE else p[k][..., others] for k in BITWISE + STATE}, BITWISE + STATE, "other lanes")
    for key in ("obs", "reward", "energy", "final_obs", "pattern", "total_energy"):
        assert np.array_equal(np.isnan(f[key]), np.isnan(c[key])), key
    for key in ("term", "trunc", "done", "step_count", "resets"):
        assert np.array_equal(f[key], c[key]), key
    assert np.isnan(f["reward"][1, SPECIAL_LANES]).all() and np.isnan(f["reward"][2, SPECIAL_LANES]).all()
    assert not np.isnan(f["reward"][:, others]).any() and not np.isnan(f["reward"][0]).any()
    sp = np.array(SPECIAL_LANES)
    assert not f["done"][:2, sp].any() and f["trunc"][2, sp].all() and not f["term"][:, sp].any()
    assert np.isnan(f["final_obs"][2, sp]).any(axis=1).all() and np.isnan(f["obs"][1, sp]).any(axis=1).all()
    assert np.isfinite(f["obs"][2:, sp]).all() and np.isfinite(f["reward"][3]).all()              # the draw and what follows it
    assert np.isfinite(f["pattern"]).all() and np.isfinite(f["total_energy"]).all()


def test_nan_index_lanes_in_a_rollout(stg):
    """3 x 5 'row', K = 3, max_steps = 3, auto-reset, N = 65 (one wavefront and one ragged lane): four driven lanes carry a NaN row index at
    step 1.  A NaN index addresses nothing: at that step those lanes' pattern stays as it was and their energy is 0, where the same lanes
    with an ordinary index move and spend energy; nothing is NaN.  The fused launch agrees with the composed path everywhere, and every
    other lane is bit-identical to a run without the NaN indices.  (The four lanes start close to the opposite of the target, so none of
    them finishes before step 2 and no restart hides the comparison.)"""
    n, shape, K = 65, (3, 5), 3
    lanes = [0, 31, 63, 64]
    n3 = 3 * shape[0] * shape[1]
    rng = np.random.default_rng(10)
    init = _unit(rng, n, *shape)
    tilted = -stg.array_env.checkerboard_pattern(*shape) + 0.1 * _unit(rng, len(lanes), *shape)
    init[lanes] = tilted / np.linalg.norm(tilted, axis=-1, keepdims=True)
    ordinary = np.stack([_actions(rng, n, shape, "row", s) for s in range(K)])
    ordinary[:, lanes, 1] = 1.5e6                      # driven: only the index keeps the cells from moving
    ordinary[:, lanes, 2] = 5e-10
    special = ordinary.copy()
    special[1, lanes, 0] = np.nan
    runs = {}
    for name, acts, fused in (("fused", special, True), ("composed", special, False), ("plain", ordinary, True)):
        env = stg.SpinTorqueArrayVecEnv(n, shape, action_mode="row", coupling_strength=0.2, observation_mode="vector",
                                        success_threshold=_finish_threshold(15), max_steps=3)
        env.reset(seed=4, options={"initial_pattern": init})
        runs[name] = _many(env, acts, autoreset=True, fused=fused)
        env.close()
    f, c, p = runs["fused"], runs["composed"], runs["plain"]
    others = np.setdiff1d(np.arange(n), lanes)
    _same_bits({k: f[k][:, others] if k in BITWISE else f[k][..., others] for k in BITWISE + STATE},
               {k: p[k][:, others] if k in BITWISE else p[k][..., others] for k in BITWISE + STATE}, BITWISE + STATE, "other lanes")
    for key in ("term", "trunc", "done", "step_count", "resets", "target"):
        assert np.array_equal(f[key], c[key]), key
    _outputs_close(f, c, "fused against composed")
    _state_close(f, c, "fused against composed")
    sp = np.array(lanes)
    assert not f["done"][:2, sp].any() and f["trunc"][2, sp].all()
    for r in (f, c):
        assert np.array_equal(r["obs"][1, sp, :n3], r["obs"][0, sp, :n3])                         # pattern rows: nothing moved at step 1
        assert (r["energy"][1, sp] == 0.0).all() and (r["energy"][0, sp] > 0.0).all()
        for key in ("obs", "reward", "energy", "pattern", "total_energy"):
            assert np.isfinite(r[key]).all(), key
    assert (p["energy"][1, sp] > 0.0).all() and (p["obs"][1, sp, :n3] != p["obs"][0, sp, :n3]).any(axis=1).all()


# ------------------------------------------------------------------------------------------------
# f. set_state / get_resets, rejected arguments
# ------------------------------------------------------------------------------------------------
def test_set_state_round_trip_and_rejected_arguments(stg):
    from spin_torque_gym_amd import _lib
    n, shape = 70, (3, 5)
    rng = np.random.default_rng(12)
    init = _unit(rng, n, *shape)
    acts = np.stack([_actions(rng, n, shape, "row", s) for s in range(6)])
    kw = dict(action_mode="row", coupling_strength=0.2, observation_mode="vector", success_threshold=_finish_threshold(15), max_steps=2)
    a = stg.SpinTorqueArrayVecEnv(n, shape, **kw)
    b = stg.SpinTorqueArrayVecEnv(n, shape, **kw)
    # before the first reset: an error from the library, nothing launched
    lib, ba = _lib.load(), b.backend
    act = torch.from_numpy(acts[:2]).permute(0, 2, 1).contiguous().cuda()
    o = ba.many_outputs(2)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = lambda K, actions: (ba._ctx, K, actions, 1, 0, 0, ptr(o["obs"]), None, ptr(o["reward"]), None, None, ptr(o["terminated"]),
                               ptr(o["truncated"]), None)
    assert lib.stg_array_step_many(*args(2, ptr(act))) == _lib.STG_E_STATE and b"reset" in lib.stg_last_error()
    with pytest.raises(_lib.StgError, match="reset"):
        ba.step_many(act)
    a.reset(seed=8, options={"initial_pattern": init})
    a.step_many(torch.from_numpy(acts[:3]), autoreset=True)
    sd = a.state_dict()
    assert sd["resets"].dtype == torch.int64 and sd["resets"].max() >= 1 and sd["pattern"].device.type == "cpu"
    b.load_state_dict(sd)
    got = b.state_dict()
    for key in ("pattern", "target", "total_energy", "step_count", "resets"):
        assert torch.equal(got[key], sd[key]), key
    assert got["dev_seed"] == sd["dev_seed"] and got["needs_reset"] is False
    ra, rb = _many(a, acts[3:], autoreset=True), _many(b, acts[3:], autoreset=True)
    _same_bits(ra, rb, BITWISE + STATE, "restored env")
    assert ra["done"].any() and ra["resets"].max() >= 2
    # a partial set_state touches only what it is given
    before = b.state_dict()
    ba.set_state(step_count=torch.zeros(n, dtype=torch.int32))
    after = b.state_dict()
    assert not after["step_count"].any()
    for key in ("pattern", "target", "total_energy", "resets"):
        assert torch.equal(after[key], before[key]), key
    # rejected arguments return before any launch
    assert lib.stg_array_step_many(*args(0, ptr(act))) == _lib.STG_E_INVALID and b"K" in lib.stg_last_error()
    assert lib.stg_array_step_many(*args(-3, ptr(act))) == _lib.STG_E_INVALID
    assert lib.stg_array_step_many(*args(2, None)) == _lib.STG_E_INVALID and b"NULL" in lib.stg_last_error()
    bad = list(args(2, ptr(act)))
    bad[6] = None                   # obs
    assert lib.stg_array_step_many(*bad) == _lib.STG_E_INVALID
    assert lib.stg_array_get_resets(ba._ctx, None, None) == _lib.STG_E_INVALID
    assert lib.stg_array_step_many(None, *args(2, ptr(act))[1:]) == _lib.STG_E_INVALID
    torch.cuda.synchronize()
    still = b.state_dict()
    for key in ("pattern", "total_energy", "step_count", "resets"):
        assert torch.equal(still[key], after[key]), key
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------
# g. a captured graph
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 4), (8, 8)], ids=lambda s: f"{s[0]}x{s[1]}")        # 8 x 8: the launch with more than 64 KB of LDS
def test_rollout_in_a_captured_graph(stg, shape):
    """One step_many(K = 2, autoreset) captured with torch.cuda.graph (static action and output buffers) and replayed twice equals two
    eager calls: the call enqueues kernels only."""
    n, K = 130, 2
    rng = np.random.default_rng(14)
    init = _unit(rng, n, *shape)
    acts = np.stack([_actions(rng, n, shape, "row", s) for s in range(2 * K)])
    kw = dict(action_mode="row", coupling_strength=0.2, observation_mode="vector", success_threshold=_finish_threshold(shape[0] * shape[1]), max_steps=2)
    eager = stg.SpinTorqueArrayVecEnv(n, shape, **kw)
    eager.reset(seed=6, options={"initial_pattern": init})
    want = [_many(eager, acts[:K], autoreset=True), _many(eager, acts[K:], autoreset=True)]
    eager.close()
    env = stg.SpinTorqueArrayVecEnv(n, shape, **kw)
    env.reset(seed=6, options={"initial_pattern": init})
    start = env.state_dict()
    b = env.backend
    static_a = torch.from_numpy(acts[:K]).permute(0, 2, 1).contiguous().cuda()
    static_o = b.many_outputs(K, True, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up outside the capture, then back to the start
        b.step_many(static_a, True, True, env._dev_seed, static_o)
    torch.cuda.current_stream().wait_stream(side)
    env.load_state_dict(start)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.step_many(static_a, True, True, env._dev_seed, static_o)
    for rep in range(2):
        static_a.copy_(torch.from_numpy(acts[rep * K:(rep + 1) * K]).permute(0, 2, 1))
        static_o["final_obs"].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = dict(obs=_c(static_o["obs"].transpose(1, 2)), reward=_c(static_o["reward64"]), reward32=_c(static_o["reward"]),
                   term=_c(static_o["terminated"]).astype(bool), trunc=_c(static_o["truncated"]).astype(bool), energy=_c(static_o["energy"]),
                   final_obs=_c(static_o["final_obs"].transpose(1, 2)))
        got["done"] = got["term"] | got["trunc"]
        got.update({k: _c(v) for k, v in env.get_state().items()}, resets=_c(b.get_resets()))
        _same_bits(got, want[rep], BITWISE + STATE, f"replay {rep}")
    assert want[1]["resets"].max() >= 2
    del graph
    env.close()

"""SpinTorqueArrayVecEnv.step_many / state_dict on the CPU oracle (no GPU): the path that composes K steps with same-step auto-reset from
the single-step calls -- the specification of the fused stg_array_step_many kernel (tests/test_gpu_array_rollout.py) -- checked against the
oracle's own step, reset draw and observation functions; and the three declarations the feature adds to the C header."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import OracleArrayBackend
from test_gpu_array import _actions, _threshold, _unit

N, SHAPE, N_DEV = 12, (3, 5), 15


@pytest.fixture(scope="module")
def stg(oracle_mod):
    import spin_torque_gym_amd as stg
    return stg


class CheckpointOracleBackend(OracleArrayBackend):
    """OracleArrayBackend plus HipArrayBackend's checkpoint calls (set_state, get_resets)."""

    def get_resets(self):
        return torch.from_numpy(self.resets.astype(np.int64))

    def set_state(self, pattern=None, target=None, total_energy=None, step_count=None, resets=None):
        import oracle
        for i in range(self.n):
            if self.states[i] is None:
                self.states[i] = oracle.ArrayEnvState(np.zeros((self.n_dev, 3)), np.zeros((self.n_dev, 3)))
            s = self.states[i]
            if pattern is not None:
                s.pattern[:] = pattern[:, i].numpy().reshape(-1, 3)
            if target is not None:
                s.target[:] = target[:, i].numpy().reshape(-1, 3)
            if total_energy is not None:
                s.total_energy.value = float(total_energy[i])
            if step_count is not None:
                s.step_count.value = int(step_count[i])
        if resets is not None:
            self.resets[:] = resets.numpy().astype(np.uint32)


def _env(stg, backend=OracleArrayBackend, obs_mode="vector", **over):
    kw = dict(action_mode="column", coupling_type="dipolar", coupling_strength=0.2, observation_mode=obs_mode,
              success_threshold=_threshold(N_DEV), max_steps=2, backend=backend)
    kw.update(over)
    return stg.SpinTorqueArrayVecEnv(N, SHAPE, **kw)


def _state(env):
    return {k: v.numpy().copy() for k, v in env.get_state().items()}


def _acts(K, seed=3):
    rng = np.random.default_rng(seed)
    return _unit(rng, N, *SHAPE), np.stack([_actions(rng, N, SHAPE, "column", s) for s in range(K)])


def test_step_many_without_autoreset_is_k_steps(stg):
    """K = 4, autoreset=False: the four step() calls exactly, finished arrays stepping on (max_steps = 2); out_every=False: the last of them."""
    init, acts = _acts(4)
    ref = _env(stg)
    ref.reset(seed=5, options={"initial_pattern": init})
    want = []
    for a in acts:
        obs, r, te, tr, info = ref.step(torch.from_numpy(a))
        want.append([t.numpy().copy() for t in (obs, r, te, tr, info["reward_f64"], info["energy"])])
    for out_every in (True, False):
        env = _env(stg)
        env.reset(seed=5, options={"initial_pattern": init})
        obs, r, te, tr, info = env.step_many(torch.from_numpy(acts), out_every=out_every)
        assert "final_obs" not in info and "done" not in info
        steps = range(4) if out_every else [3]
        assert obs.shape == (len(steps), N, 6 * N_DEV + 4) and r.shape == (len(steps), N) and te.dtype == torch.bool
        for slot, k in enumerate(steps):
            got = [t[slot].numpy() for t in (obs, r, te, tr, info["reward_f64"], info["energy"])]
            for g, w in zip(got, want[k]):
                assert np.array_equal(g, w, equal_nan=True), (out_every, k)
        for key, v in _state(env).items():
            assert np.array_equal(v, _state(ref)[key]), key
        assert (_state(env)["step_count"] == 4).all() and not env.backend.resets.any()
    assert np.array_equal(want[1][3], np.ones(N, dtype=bool)) and not want[0][3].any()          # truncation starts at step 2


def test_step_many_autoreset_against_the_oracle(stg, oracle_mod):
    """3 x 5 'column', N = 12, max_steps = 2, threshold at 0.3 sigma of a random pattern's similarity (so some arrays terminate at step 1):
    every step of a K = 1 chain is checked against the oracle's own functions, then K = 4 in one call equals the chain."""
    init, acts = _acts(4)
    ref = _env(stg)                # stepped by hand, reset by hand
    env = _env(stg)
    for e in (ref, env):
        e.reset(seed=5, options={"initial_pattern": init})
    seed = env._dev_seed
    assert seed == ref._dev_seed and seed != 0
    counts = np.zeros(N, dtype=np.int64)
    chain, saw_term_at_first_step = [], False
    for k in range(4):
        obs_w, r_w, te_w, tr_w, info_w = ref.step(torch.from_numpy(acts[k]))
        obs_w, te_w, tr_w = obs_w.numpy().copy(), te_w.numpy().copy(), tr_w.numpy().copy()
        done = te_w | tr_w
        before = _state(env)
        sentinel = torch.full((1, env.backend.obs_dim, N), -7.0)
        obs, r, te, tr, info = env.step_many(torch.from_numpy(acts[k:k + 1]), autoreset=True, out={"final_obs": sentinel})
        chain.append([t[0].numpy().copy() for t in (obs, r, te, tr, info["reward_f64"], info["energy"], info["final_obs"], info["done"])])
        # flags and reward are the terminal step's
        assert np.array_equal(te[0].numpy(), te_w) and np.array_equal(tr[0].numpy(), tr_w) and np.array_equal(info["done"][0].numpy(), done)
        assert np.array_equal(r[0].numpy(), r_w.numpy()) and np.array_equal(info["reward_f64"][0].numpy(), info_w["reward_f64"].numpy())
        # final_obs: the terminal observation where done, untouched elsewhere; obs: the step's where not done
        fo = info["final_obs"][0].numpy()
        assert np.array_equal(fo[done], obs_w[done]) and (fo[~done] == -7.0).all()
        assert np.array_equal(obs[0].numpy()[~done], obs_w[~done])
        if k == 0:
            saw_term_at_first_step = bool(te_w.any())
            assert te_w.any() and not done.all() and not tr_w.any()
        # the done arrays restart exactly as a masked random reset restarts them: draw (seed, env id, reset count), target kept, zeros
        st = _state(env)
        for i in range(N):
            if done[i]:
                pat, _ = oracle_mod.array_reset_draw(seed, i, counts[i], N_DEV)
                assert np.array_equal(st["pattern"][:, i], pat.reshape(-1)), (k, i)
                assert st["step_count"][i] == 0 and st["total_energy"][i] == 0.0
                fresh = oracle_mod.ArrayEnvState(pat, before["target"][:, i])
                assert np.array_equal(obs[0].numpy()[i], oracle_mod.array_observation(fresh, env.backend.ocfg)), (k, i)
                assert obs[0].numpy()[i, 6 * N_DEV + 1] == 1.0 and obs[0].numpy()[i, 6 * N_DEV + 2] == 0.0
                counts[i] += 1
            else:
                assert st["step_count"][i] == before["step_count"][i] + 1
        assert np.array_equal(st["target"], before["target"])
        assert np.array_equal(env.backend.resets, counts)                       # the counter advances only for done arrays
        # the hand-driven env follows: the same masked reset
        ref.backend.reset(torch.from_numpy(done.astype(np.uint8)), None, None, seed)
        for key, v in _state(ref).items():
            assert np.array_equal(v, st[key]), (k, key)
    assert saw_term_at_first_step and counts.max() >= 2 and counts.min() >= 1   # the draw sequence continued: resets = 0, 1, ...
    # K = 4 in one call: the chain
    one = _env(stg)
    one.reset(seed=5, options={"initial_pattern": init})
    obs, r, te, tr, info = one.step_many(torch.from_numpy(acts), autoreset=True)
    for k in range(4):
        got = [t[k].numpy() for t in (obs, r, te, tr, info["reward_f64"], info["energy"], info["final_obs"], info["done"])]
        d = chain[k][7]
        for j, (g, w) in enumerate(zip(got, chain[k])):
            if j == 6:      # final_obs: NaN in the fresh tensor where not done
                assert np.array_equal(g[d], w[d]) and np.isnan(g[~d]).all()
            else:
                assert np.array_equal(g, w, equal_nan=True), (k, j)
    for key, v in _state(one).items():
        assert np.array_equal(v, _state(env)[key]), key
    # ... and with out_every=False its last step
    last = _env(stg)
    last.reset(seed=5, options={"initial_pattern": init})
    obs1, r1, te1, tr1, info1 = last.step_many(torch.from_numpy(acts), autoreset=True, out_every=False)
    assert obs1.shape[0] == 1 and np.array_equal(obs1[0].numpy(), obs[3].numpy()) and np.array_equal(r1[0].numpy(), r[3].numpy())
    assert np.array_equal(info1["done"][0].numpy(), info["done"][3].numpy())
    assert np.array_equal(last.backend.resets, one.backend.resets)


def test_step_many_rejects_what_it_cannot_do(stg):
    env = _env(stg)
    _, acts = _acts(2)
    with pytest.raises(RuntimeError, match="reset"):
        env.step_many(torch.from_numpy(acts))
    env.reset(seed=1)
    with pytest.raises(ValueError, match="shape"):
        env.step_many(torch.from_numpy(acts[0]))
    with pytest.raises(ValueError, match="shape"):
        env.step_many(torch.from_numpy(acts[:, :, :2]))
    d = _env(stg, obs_mode="dict")
    d.reset(seed=1)
    with pytest.raises(ValueError, match="dict"):
        d.step_many(torch.from_numpy(acts))


def test_state_dict_round_trip_continues_identically(stg):
    """state_dict -> a new env -> load_state_dict: the same continuation, including the next auto-reset draws (reset counters and the
    device seed travel with the state)."""
    init, acts = _acts(6, seed=9)
    a = _env(stg, backend=CheckpointOracleBackend)
    a.reset(seed=11, options={"initial_pattern": init})
    a.step_many(torch.from_numpy(acts[:3]), autoreset=True)
    sd = a.state_dict()
    assert set(sd) == {"pattern", "target", "total_energy", "step_count", "resets", "dev_seed", "needs_reset"}
    assert sd["resets"].numpy().any() and sd["dev_seed"] == a._dev_seed and sd["needs_reset"] is False
    b = _env(stg, backend=CheckpointOracleBackend)
    with pytest.raises(RuntimeError):
        b.step_many(torch.from_numpy(acts[3:]))
    b.load_state_dict(sd)
    outs = [e.step_many(torch.from_numpy(acts[3:]), autoreset=True) for e in (a, b)]
    for x, y in zip(outs[0][:4], outs[1][:4]):
        assert np.array_equal(x.numpy(), y.numpy())
    for key in ("reward_f64", "energy", "final_obs", "done"):
        assert np.array_equal(outs[0][4][key].numpy(), outs[1][4][key].numpy(), equal_nan=key == "final_obs"), key
    assert outs[0][4]["done"].numpy().any()
    for key, v in _state(a).items():
        assert np.array_equal(v, _state(b)[key]), key
    assert np.array_equal(a.backend.resets, b.backend.resets) and a.backend.resets.max() >= 2
    # a fresh env's state_dict says so, and loading it leaves the reset due
    fresh = _env(stg, backend=CheckpointOracleBackend).state_dict()
    assert fresh["needs_reset"] is True and "pattern" not in fresh
    c = _env(stg, backend=CheckpointOracleBackend)
    c.load_state_dict(fresh)
    with pytest.raises(RuntimeError):
        c.step(torch.from_numpy(acts[0]))


def test_header_declares_the_rollout_calls():
    text = open(os.path.join(ROOT, "include", "spintorque_hip.h")).read()
    assert re.search(r"^#define STG_ABI_VERSION 5$", text, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("stg_array_step_many", "stg_array_set_state", "stg_array_get_resets"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*stg_array_ctx\s*\*", code), name
    from spin_torque_gym_amd import _lib
    assert _lib.ABI_VERSION == 5
    for name in ("stg_array_step_many", "stg_array_set_state", "stg_array_get_resets"):
        assert name in _lib.SYMBOLS

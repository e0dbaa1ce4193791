"""Host side of subset stepping and the send/recv pool (no GPU): a fake backend stands in for HipBackend's id launches, streams and
events, so that SpinTorqueVecEnv's bookkeeping -- recv order, the checks on sent ids, async mode -- runs on the CPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT


class _Event:
    def __init__(self):
        self.done = True

    def query(self):
        return self.done

    def synchronize(self):
        self.done = True


class FakeBackend:
    """HipBackend's interface as far as step_ids and the pool use it.  obs row 0 = env id, row 1 = steps taken by that env."""

    def __init__(self, n_envs, cfg, device_index=0, env_id0=0):
        self.n = int(n_envs)
        self.cfg = cfg
        self.device = torch.device("cpu")
        self.steps = np.zeros(self.n, dtype=np.int64)
        self.launches = []                  # (stream, ids)
        self.events = []

    def set_params(self, table, cls=None):
        pass

    def reset(self, mask=None, init_m=None, target=None, seed=0):
        self.steps[:] = 0
        obs = torch.zeros((12, self.n), dtype=torch.float32)
        obs[0] = torch.arange(self.n, dtype=torch.float32)
        return obs

    def step(self, actions, autoreset=False, out=None):
        self.steps += 1
        z = torch.zeros(self.n)
        return torch.zeros((12, self.n)), z, None, z.to(torch.uint8), z.to(torch.uint8), None

    def get_state(self):
        return {"step_count": torch.as_tensor(self.steps.copy())}

    def ids_workspace(self, m):
        return torch.empty(int(m), dtype=torch.uint8)

    def make_streams(self, k):
        return list(range(k))

    def record_event(self, stream):
        ev = _Event()
        self.events.append(ev)
        return ev

    def hand_over(self, out):
        pass

    def step_ids(self, actions, env_ids, autoreset=False, workspace=None, out=None, stream=None):
        ids = torch.as_tensor(env_ids).numpy().astype(np.int64)
        assert workspace is not None and workspace.numel() >= len(ids)
        self.steps[ids] += 1
        self.launches.append((stream, ids.copy()))
        m = len(ids)
        obs = torch.zeros((12, m), dtype=torch.float32)
        obs[0] = torch.as_tensor(ids, dtype=torch.float32)
        obs[1] = torch.as_tensor(self.steps[ids], dtype=torch.float32)
        z = torch.zeros(m, dtype=torch.uint8)
        return dict(obs=obs, reward=torch.as_tensor(actions)[0].to(torch.float32), terminated=z, truncated=z.clone(), status=z.clone(),
                    final_obs=torch.zeros((12, m)), reward64=None, energy=None)

    def close(self):
        pass


def make_env(n=16, **kw):
    import spin_torque_gym_amd as stg
    env = stg.SpinTorqueVecEnv(n, seed=0, backend=FakeBackend, **kw)
    env.reset()
    return env


def _ids(info):
    return info["env_id"].numpy().tolist()


def test_recv_returns_reset_batches_then_oldest_completed_first():
    env = make_env(16)
    env.async_reset(4)
    got = [_ids(env.recv()[4]) for _ in range(4)]
    assert got == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]]
    with pytest.raises(RuntimeError, match="nothing is in flight"):
        env.recv()
    act = np.zeros((4, 2), dtype=np.float32)
    env.send(act, [4, 5, 6, 7])
    env.send(act + 1, [0, 1, 2, 3])
    env.send(act + 2, [8, 9, 10, 11])
    b = env.backend
    b.events[0].done = False          # the first send is still running, the second and third are through
    obs, rew, term, trunc, info = env.recv()
    assert _ids(info) == [0, 1, 2, 3] and rew.tolist() == [1.0] * 4
    assert obs.shape == (4, 12) and obs[:, 1].tolist() == [1.0] * 4
    assert _ids(env.recv()[4]) == [8, 9, 10, 11]
    b.events[0].done = True
    assert _ids(env.recv()[4]) == [4, 5, 6, 7]
    # launches go round the pool's streams, at most four by default
    assert [s for s, _ in b.launches] == [0, 1, 2]
    env.send(act, [0, 1, 2, 3])
    env.send(act, [4, 5, 6, 7])
    assert [s for s, _ in b.launches] == [0, 1, 2, 3, 0]


def test_send_merges_and_splits_batches_along_pairs():
    env = make_env(16)
    env.async_reset(4)
    for _ in range(4):
        env.recv()
    env.send(np.zeros((8, 2), np.float32), [5, 4, 0, 1, 13, 12, 3, 2])           # merged, unsorted
    env.send(np.zeros((2, 2), np.float32), np.array([10, 11]))                     # split off a batch
    obs, _, _, _, info = env.recv()
    assert _ids(info) == [5, 4, 0, 1, 13, 12, 3, 2]                                # list order
    assert obs[:, 0].tolist() == [5.0, 4.0, 0.0, 1.0, 13.0, 12.0, 3.0, 2.0]
    assert _ids(env.recv()[4]) == [10, 11]
    assert env.backend.steps.tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0]


def test_send_rejects_bad_id_sets():
    env = make_env(16)
    env.async_reset(4)
    env.recv()                                                                     # envs 0..3 received
    a2 = np.zeros((2, 2), np.float32)
    with pytest.raises(ValueError, match="received"):
        env.send(a2, [4, 5])                                                       # still in flight (not received)
    with pytest.raises(ValueError, match="duplicate"):
        env.send(np.zeros((4, 2), np.float32), [0, 1, 1, 0])
    with pytest.raises(ValueError, match="in \\[0, 16\\)"):
        env.send(a2, [0, 16])
    with pytest.raises(ValueError, match="in \\[0, 16\\)"):
        env.send(a2, torch.tensor([-1, 0]))
    with pytest.raises(ValueError, match="splits a pair"):
        env.send(np.zeros((3, 2), np.float32), [0, 1, 2])
    with pytest.raises(ValueError, match="splits a pair"):
        env.send(a2, [1, 2])
    with pytest.raises(TypeError):
        env.send(a2, np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="actions"):
        env.send(np.zeros((3, 2), np.float32), [0, 1])
    assert env.backend.launches == []                                              # nothing was launched
    env.send(a2, [0, 1])
    with pytest.raises(ValueError, match="received"):
        env.send(a2, [0, 1])                                                       # sent twice
    env.send(a2, [3, 2])


def test_odd_env_count_last_env_has_no_partner():
    env = make_env(7)
    env.async_reset(2)
    got = [_ids(env.recv()[4]) for _ in range(4)]
    assert got == [[0, 1], [2, 3], [4, 5], [6]]
    env.send(np.zeros((1, 2), np.float32), [6])
    with pytest.raises(ValueError, match="even"):
        env.async_reset(3)


def test_step_while_async_raises_and_reset_ends_async_mode():
    env = make_env(8)
    env.async_reset(4)
    env.recv()
    env.send(np.zeros((4, 2), np.float32), [0, 1, 2, 3])
    env.backend.events[-1].done = False
    for call in (lambda: env.step(np.zeros((8, 2), np.float32)), lambda: env.step_many(np.zeros((2, 8, 2), np.float32)),
                 env.state_dict, lambda: env.step_ids(np.zeros((2, 2), np.float32), [6, 7])):
        with pytest.raises(RuntimeError, match="reset\\(\\) to end async mode"):
            call()
    env.reset()                                                                    # drains the pool (the event completes) and ends async mode
    assert env.backend.events[-1].done
    with pytest.raises(RuntimeError, match="not in async mode"):
        env.recv()
    with pytest.raises(RuntimeError, match="not in async mode"):
        env.send(np.zeros((2, 2), np.float32), [0, 1])
    env.step(np.zeros((8, 2), np.float32))
    assert "step_count" in env.state_dict()


def test_step_ids_checks_on_the_host():
    env = make_env(8)
    obs, rew, term, trunc, info = env.step_ids(np.ones((3, 2), np.float32), torch.tensor([6, 1, 3]))
    assert _ids(info) == [6, 1, 3] and info["env_id"].dtype == torch.int64
    assert obs.shape == (3, 12) and term.dtype == torch.bool
    assert env.backend.steps.tolist() == [0, 1, 0, 1, 0, 0, 1, 0]
    with pytest.raises(ValueError, match="duplicate"):
        env.step_ids(np.ones((2, 2), np.float32), [2, 2])
    with pytest.raises(ValueError, match="in \\[0, 8\\)"):
        env.step_ids(np.ones((1, 2), np.float32), [8])
    with pytest.raises(ValueError, match="empty"):
        env.step_ids(np.ones((0, 2), np.float32), [])


def test_abi_version_5_and_step_ids_symbols():
    from spin_torque_gym_amd import _lib
    assert _lib.ABI_VERSION == 5 and _lib.STATUS_BAD_ID == 4
    text = open(os.path.join(ROOT, "include", "spintorque_hip.h")).read()
    assert re.search(r"#define STG_ABI_VERSION 5\b", text)
    assert re.search(r"STG_STATUS_BAD_ID = 4", text)
    assert {"stg_step_ids", "stg_step_ids_workspace_bytes"} <= set(_lib.SYMBOLS)
    lib = _lib.load()
    assert lib.stg_abi_version() == 5
    # argument checks come before any device work
    assert lib.stg_step_ids_workspace_bytes(None, 16) == 0
    assert lib.stg_step_ids(None, 1, None, None, 0, 0, None, None, None, None, None, None, None, None, None, None) == _lib.STG_E_INVALID
    assert b"ctx" in lib.stg_last_error()

"""Shaped pulses and an applied field in fused K-step rollouts, subset stepping and the send/recv pool, host side (no GPU).

  * the three C-ABI symbols (stg_set_pulse_shape, stg_step_shaped, stg_step_shaped_ids) are bound with the right arity at the unchanged
    ABI version, and their argument errors come back before any device work;
  * SpinTorqueVecEnv with a shape or a field reaches the shaped backend entries from step_many / step_ids / send with the right actions
    and ids, hands the shape over once per backend, and leaves step() on step_wave;
  * without a shape none of the new backend methods is called; a backend without the entries keeps raising NotImplementedError."""
import numpy as np
import pytest
import torch

E_INVALID = -1


# ------------------------------------------------------------------------------------------------
# the C-ABI
# ------------------------------------------------------------------------------------------------
def test_symbols_are_bound_and_the_abi_version_stays():
    from spin_torque_gym_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 5 and lib.stg_abi_version() == 5
    for name, arity in (("stg_set_pulse_shape", 7), ("stg_step_shaped", 15), ("stg_step_shaped_ids", 15)):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert len(_lib.SYMBOLS[name][1]) == arity, name
    # the fused entry has stg_step_many's signature, the id entry stg_step_ids's without the workspace
    assert _lib.SYMBOLS["stg_step_shaped"] == _lib.SYMBOLS["stg_step_many"]
    ids = list(_lib.SYMBOLS["stg_step_ids"][1])
    del ids[6]
    assert _lib.SYMBOLS["stg_step_shaped_ids"][1] == ids


def _dp(x):
    import ctypes as C
    x = np.ascontiguousarray(x, dtype=np.float64)
    return x, C.c_void_p(x.ctypes.data)


def test_argument_errors_come_before_any_device_work():
    """No context exists without a GPU, so every call here ends in STG_E_INVALID; the message tells which check refused it: the table
    checks run first, on host memory only, and a good table gets as far as the NULL context."""
    from spin_torque_gym_amd import _lib
    lib = _lib.load()
    tau, ptau = _dp([0.0, 0.25, 1.0])
    sc, psc = _dp([0.0, 1.0, 0.5])
    th, pth = _dp([0.0, 1e-9])
    hk, phk = _dp([[1e4, 0.0, 0.0], [0.0, 0.0, -1e4]])

    def call(*a):
        rc = lib.stg_set_pulse_shape(None, *a)
        return rc, lib.stg_last_error().decode()

    assert call(3, ptau, psc, 2, pth, phk) == (E_INVALID, "ctx is NULL")                  # everything in order but the context
    assert call(0, None, None, 0, None, None) == (E_INVALID, "ctx is NULL")               # clearing the shape
    for kj in (1, -1, 33):
        rc, msg = call(kj, ptau, psc, 0, None, None)
        assert rc == E_INVALID and msg.startswith("kj must be"), (kj, msg)
    for kh in (1, -2, 33):
        rc, msg = call(0, None, None, kh, pth, phk)
        assert rc == E_INVALID and msg.startswith("kh must be"), (kh, msg)
    for args in ((3, None, psc, 0, None, None), (3, ptau, None, 0, None, None)):
        rc, msg = call(*args)
        assert rc == E_INVALID and "tau/scale must not be NULL" in msg
    for args in ((0, None, None, 2, None, phk), (0, None, None, 2, pth, None)):
        rc, msg = call(*args)
        assert rc == E_INVALID and "th/hk must not be NULL" in msg
    for bad in ([0.0, 0.5, 0.5], [0.0, 0.6, 0.5], [0.5, 0.25, 1.0]):                       # not strictly increasing
        b, pb = _dp(bad)
        rc, msg = call(3, pb, psc, 0, None, None)
        assert rc == E_INVALID and "strictly increasing" in msg, (bad, msg)
    for bad in ([-0.1, 0.5, 1.0], [0.0, 0.5, 1.0 + 2.3e-16], [0.0, 0.5, 1.5]):             # outside [0, 1]
        b, pb = _dp(bad)
        rc, msg = call(3, pb, psc, 0, None, None)
        assert rc == E_INVALID and "[0, 1]" in msg, (bad, msg)
    for bad_tau, bad_sc in (([0.0, np.nan, 1.0], sc), (tau, [0.0, np.inf, 1.0])):
        (b, pb), (c, pc) = _dp(bad_tau), _dp(bad_sc)
        rc, msg = call(3, pb, pc, 0, None, None)
        assert rc == E_INVALID and "finite" in msg
    b, pb = _dp([1e-9, 1e-9])
    rc, msg = call(0, None, None, 2, pb, phk)
    assert rc == E_INVALID and "th must be strictly increasing" in msg
    b, pb = _dp([[1e4, 0.0, 0.0], [0.0, np.nan, 0.0]])
    rc, msg = call(0, None, None, 2, pth, pb)
    assert rc == E_INVALID and "finite" in msg
    # a field table may start anywhere (absolute seconds): a negative first knot passes the table checks
    b, pb = _dp([-1e-9, 1e-9])
    assert call(0, None, None, 2, pb, phk) == (E_INVALID, "ctx is NULL")
    # the step entries
    assert lib.stg_step_shaped(None, 1, None, 0, 1, 0, None, None, None, None, None, None, None, None, None) == E_INVALID
    assert b"ctx" in lib.stg_last_error()
    assert lib.stg_step_shaped_ids(None, 1, None, None, 0, 0, None, None, None, None, None, None, None, None, None) == E_INVALID
    assert b"ctx" in lib.stg_last_error()


# ------------------------------------------------------------------------------------------------
# the env over a recording backend
# ------------------------------------------------------------------------------------------------
class _Event:
    def query(self):
        return True

    def synchronize(self):
        pass


class Recorder:
    """HipBackend's interface as far as the env's launch forms use it, shaped entries included; every call is logged.  obs row 0 = env
    id, reward = the action's current."""
    log = []                                  # (name, ...) per call, shared by the instances of one test

    def __init__(self, n_envs, cfg, device_index=0, env_id0=0):
        self.n, self.cfg, self.device = int(n_envs), cfg, torch.device("cpu")

    def _note(self, *rec):
        type(self).log.append(rec)

    def set_params(self, table, cls=None):
        pass

    def set_pulse_shape(self, shape, field_knots):
        self._note("set_pulse_shape", shape, field_knots)

    def reset(self, mask=None, init_m=None, target=None, seed=0):
        obs = torch.zeros((12, self.n), dtype=torch.float32)
        obs[0] = torch.arange(self.n, dtype=torch.float32)
        return obs

    def _one(self, name, actions):
        self._note(name, torch.as_tensor(actions).clone())
        z = torch.zeros(self.n)
        return torch.zeros((12, self.n)), z, None, z.to(torch.uint8), z.to(torch.uint8), None

    def step(self, actions, autoreset=False, out=None):
        return self._one("step", actions)

    def step_wave(self, actions, wave, autoreset=False, out=None):
        assert (wave["current"] is None) == (self.want_shape is None) and (wave["field"] is None) == (self.want_field is None)
        return self._one("step_wave", actions)

    def _many(self, name, actions, out_every, autoreset):
        a = torch.as_tensor(actions)
        self._note(name, a.clone(), bool(out_every), bool(autoreset))
        ko = a.shape[0] if out_every else 1
        z = torch.zeros((ko, self.n))
        self.final_obs_many = torch.zeros((ko, 12, self.n))
        return torch.zeros((ko, 12, self.n)), z, None, z.to(torch.uint8), z.to(torch.uint8), None

    def step_many(self, actions, out_every=True, autoreset=False):
        return self._many("step_many", actions, out_every, autoreset)

    def step_shaped_many(self, actions, out_every=True, autoreset=False):
        return self._many("step_shaped_many", actions, out_every, autoreset)

    def _ids(self, name, actions, env_ids, stream):
        a = torch.as_tensor(actions)
        ids = torch.as_tensor(env_ids).numpy().astype(np.int64)
        self._note(name, a.clone(), ids.tolist(), stream)
        m = len(ids)
        obs = torch.zeros((12, m), dtype=torch.float32)
        obs[0] = torch.as_tensor(ids, dtype=torch.float32)
        z = torch.zeros(m, dtype=torch.uint8)
        return dict(obs=obs, reward=a[0].to(torch.float32), terminated=z, truncated=z.clone(), status=z.clone(), final_obs=torch.zeros((12, m)),
                    reward64=None, energy=None)

    def step_ids(self, actions, env_ids, autoreset=False, workspace=None, out=None, stream=None):
        assert workspace is not None
        return self._ids("step_ids", actions, env_ids, stream)

    def step_shaped_ids(self, actions, env_ids, autoreset=False, out=None, stream=None):
        return self._ids("step_shaped_ids", actions, env_ids, stream)

    def ids_workspace(self, m):
        self._note("ids_workspace", int(m))
        return torch.empty(int(m), dtype=torch.uint8)

    def make_streams(self, k):
        return list(range(k))

    def record_event(self, stream):
        return _Event()

    def hand_over(self, out):
        pass

    def get_state(self):
        return {}

    def close(self):
        pass


def _recorder(shape=None, field=None):
    class R(Recorder):
        log = []
        want_shape, want_field = shape, field
    return R


def _names(R):
    return [r[0] for r in R.log]


def _shape():
    from spin_torque_gym_amd.physics import PiecewiseLinear
    return PiecewiseLinear([0.0, 0.1, 0.8, 1.0], [0.0, 1.0, 1.0, 0.3])


@pytest.mark.parametrize("kw", ("shape", "field", "both"))
def test_shaped_env_reaches_the_shaped_entries(kw):
    import spin_torque_gym_amd as stg
    shape = _shape() if kw in ("shape", "both") else None
    field = [1e4, 0.0, -2e4] if kw in ("field", "both") else None
    R = _recorder(shape, field)
    n = 8
    env = stg.SpinTorqueVecEnv(n, seed=0, backend=R, pulse_shape=shape, applied_field=field, max_duration=5e-9)
    # the shape goes to the backend once, when the backend is made, as the env holds it
    assert _names(R) == ["set_pulse_shape"]
    _, got_shape, got_field = R.log[0]
    assert got_shape is shape
    if field is None:
        assert got_field is None
    else:
        assert got_field[0].tolist() == [0.0, 5e-9] and got_field[1].tolist() == [field, field]
    env.reset()
    rng = np.random.default_rng(0)
    # step_many: [K,N,2] in, the kernel's [K,2,N] at the backend, flags passed through
    a = rng.uniform(0.0, 1.0, (3, n, 2)).astype(np.float32)
    obs, rew, term, trunc, info = env.step_many(a, out_every=False)
    assert tuple(obs.shape) == (1, n, 12) and term.dtype == torch.bool
    name, got, out_every, autoreset = R.log[-1]
    assert name == "step_shaped_many" and (out_every, autoreset) == (False, False)
    assert np.array_equal(got.numpy(), a.transpose(0, 2, 1))
    env.step_many(torch.from_numpy(a.transpose(0, 2, 1).copy()), actions_soa=True)
    assert R.log[-1][0] == "step_shaped_many" and R.log[-1][2] is True and np.array_equal(R.log[-1][1].numpy(), a.transpose(0, 2, 1))
    # step_ids: list order kept, no workspace asked for
    a2 = rng.uniform(0.0, 1.0, (3, 2)).astype(np.float64)
    obs, rew, term, trunc, info = env.step_ids(a2, [6, 1, 3])
    name, got, ids, stream = R.log[-1]
    assert name == "step_shaped_ids" and ids == [6, 1, 3] and stream is None and np.array_equal(got.numpy(), a2.T)
    assert info["env_id"].tolist() == [6, 1, 3] and obs[:, 0].tolist() == [6.0, 1.0, 3.0] and rew.tolist() == a2[:, 0].astype(np.float32).tolist()
    # step() stays on step_wave
    env.step(rng.uniform(0.0, 1.0, (n, 2)).astype(np.float32))
    assert R.log[-1][0] == "step_wave"
    # the pool: reset batches, then sends on the pool's streams through the shaped id entry
    env.async_reset(4, num_streams=2)
    assert [env.recv()[4]["env_id"].tolist() for _ in range(2)] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    a4 = rng.uniform(0.0, 1.0, (4, 2)).astype(np.float32)
    env.send(a4, [5, 4, 0, 1])
    env.send(a4[:2], [2, 3])
    env.send(a4[:2], [7, 6])
    sends = [r for r in R.log if r[0] == "step_shaped_ids"][1:]
    assert [(r[2], r[3]) for r in sends] == [([5, 4, 0, 1], 0), ([2, 3], 1), ([7, 6], 0)]
    assert np.array_equal(sends[0][1].numpy(), a4.T)
    assert env.recv()[4]["env_id"].tolist() == [5, 4, 0, 1]
    env.reset()
    # nothing plain ran, no workspace was allocated, and the shape was set exactly once
    assert not {"step", "step_many", "step_ids", "ids_workspace"} & set(_names(R))
    assert _names(R).count("set_pulse_shape") == 1
    env.close()


def test_autoreset_reaches_the_shaped_entries():
    import spin_torque_gym_amd as stg
    R = _recorder(_shape(), None)
    env = stg.SpinTorqueVecEnv(4, seed=0, backend=R, pulse_shape=_shape(), autoreset=True)
    env.reset()
    obs, rew, term, trunc, info = env.step_many(np.zeros((2, 4, 2), np.float32))
    assert R.log[-1][0] == "step_shaped_many" and R.log[-1][3] is True and tuple(info["final_obs"].shape) == (2, 4, 12)
    obs, rew, term, trunc, info = env.step_ids(np.zeros((2, 2), np.float32), [2, 3])
    assert R.log[-1][0] == "step_shaped_ids" and tuple(info["final_obs"].shape) == (2, 12)


def test_a_rebuilt_backend_gets_the_shape_again():
    import spin_torque_gym_amd as stg
    R = _recorder(_shape(), None)
    env = stg.SpinTorqueVecEnv(4, seed=0, backend=R, pulse_shape=_shape())
    first = env.backend
    env.cfg.seed += 1                          # what load_state_dict does for a checkpoint of another stream key
    env.backend = env._make_backend()
    assert env.backend is not first and _names(R) == ["set_pulse_shape", "set_pulse_shape"]


def test_without_a_shape_none_of_the_new_methods_is_called():
    import spin_torque_gym_amd as stg

    class Plain(Recorder):
        log = []

        def set_pulse_shape(self, *a, **k):
            raise AssertionError("set_pulse_shape called without a shape or a field")

        def step_shaped_many(self, *a, **k):
            raise AssertionError("step_shaped_many called without a shape or a field")

        def step_shaped_ids(self, *a, **k):
            raise AssertionError("step_shaped_ids called without a shape or a field")

        def step_wave(self, *a, **k):
            raise AssertionError("step_wave called without a shape or a field")
    env = stg.SpinTorqueVecEnv(8, seed=0, backend=Plain)
    env.reset()
    env.step(np.zeros((8, 2), np.float32))
    env.step_many(np.zeros((2, 8, 2), np.float32))
    env.step_ids(np.zeros((2, 2), np.float32), [4, 5])
    env.async_reset(4, num_streams=2)
    env.recv()
    env.send(np.zeros((4, 2), np.float32), [0, 1, 2, 3])
    env.reset()
    names = _names(Plain)
    assert names.count("step") == 1 and names.count("step_many") == 1 and names.count("step_ids") == 2
    assert names.count("ids_workspace") == 3                         # one for step_ids, one per stream of the pool


def test_a_backend_without_the_entries_still_refuses():
    """Capability, not a flag: a backend that only has step_wave (the CPU oracle seam) keeps the NotImplementedError, and gets no
    set_pulse_shape call."""
    import spin_torque_gym_amd as stg

    class WaveOnly:
        def __init__(self, n_envs, cfg, device_index=0, env_id0=0):
            self.n, self.device = int(n_envs), torch.device("cpu")

        def set_params(self, table, cls=None):
            pass

        def reset(self, mask=None, init_m=None, target=None, seed=0):
            return torch.zeros((12, self.n))

        def step_wave(self, actions, wave, autoreset=False, out=None):
            z = torch.zeros(self.n)
            return torch.zeros((12, self.n)), z, None, z.to(torch.uint8), z.to(torch.uint8), None

        def close(self):
            pass
    env = stg.SpinTorqueVecEnv(4, seed=0, backend=WaveOnly, applied_field=[1e4, 0.0, 0.0])
    env.reset()
    act = np.zeros((4, 2), np.float32)
    for call in (lambda: env.step_many(act[None]), lambda: env.step_ids(act[:2], [0, 1]), lambda: env.async_reset(2),
                 lambda: env.send(act[:2], [0, 1]), lambda: env.recv()):
        with pytest.raises(NotImplementedError, match="pulse_shape or applied_field"):
            call()
    assert tuple(env.step(act)[0].shape) == (4, 12)

"""Actions that carry the pulse's knot amplitudes (pulse_knots=, stg_set_pulse_knots / stg_step_knots / stg_step_knots_ids), host side
(no GPU).

  * the torch restatement of the action parse (envs.parse_knot_actions_fp64, envs.knot_tables) equals the NumPy one written from the
    header's four steps (tests/knots_ref.py), bit for bit, on the parse edges: clamp, +-Inf, NaN amplitude, NaN J, zeros, tied knot times;
  * action-space shapes and bounds, pulse_knots + pulse_shape -> ValueError, tau / amplitude_limit validation;
  * over a recording backend: set_pulse_knots once per context and the right backend method per API call; a step_wave-only backend gets
    step() (checked in numbers through the NumPy restatement of the step) and refuses the rest; without pulse_knots no new method runs;
  * the sharded env refuses; the three C-ABI symbols are bound with the header's argument counts at ABI version 5."""
import re

import numpy as np
import pytest
import torch

from conftest import stt_default_params
import wave_step_ref
from knots_ref import edge_actions, knot_tables_np, parse_np, wave_rows
from test_step_shaped_host import Recorder, _names
from test_wave_step_host import WaveOracleBackend

E_INVALID = -1
TAU4 = [0.0, 0.2, 0.7, 1.0]


# ------------------------------------------------------------------------------------------------
# the parse
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
@pytest.mark.parametrize("P,limit", [(4, 1.0), (2, 0.75), (32, 3.0)])
def test_torch_parse_equals_the_numpy_parse_bit_for_bit(dtype, P, limit):
    from spin_torque_gym_amd import envs
    a = edge_actions(dtype, P, limit)
    J, T, s = parse_np(a, 2e6, 5e-9, limit)
    Jt, Tt, st = envs.parse_knot_actions_fp64(torch.from_numpy(a.T.copy()), 2e6, 5e-9, limit)
    for x, y, what in ((Jt.numpy(), J, "J"), (Tt.numpy(), T, "T"), (st.numpy().T, s, "s")):
        assert x.dtype == np.float64 and np.array_equal(x.view(np.int64), np.ascontiguousarray(y).view(np.int64)), what
    # what the parse is meant to do, spelled out on the rows above
    assert (np.abs(s) <= limit).all() and not np.isnan(s).any()
    assert s[1, 0] == limit and s[1, 1] == -limit and s[2, 0] == limit and s[2, 1] == -limit
    for row in (3, 4):
        assert J[row] == 0.0 and T[row] == 1e-12 and (s[row] == 0.0).all() and not np.signbit(s[row]).any()
    for row in (5, 6, 7):                                                    # NaN / Inf in (J, T) alone: stg_step's rule, amplitudes kept
        assert T[row] == 1e-12 or row == 7
        assert (s[row] == (0.5 if row < 7 else -0.5)).all()
    assert J[5] == 0.0 and J[6] == 0.0 and J[7] == 2e6
    # the tables: one rounded product each
    tau = np.linspace(0.0, 1.0, P)
    tj, jk = envs.knot_tables(tau, Jt, Tt, st)
    assert np.array_equal(tj.numpy(), tau[:, None] * T[None, :]) and np.array_equal(jk.numpy().view(np.int64), (J[None, :] * s.T).view(np.int64))


def test_tied_knot_times_are_the_products_the_header_names():
    """two adjacent tau one ulp apart: tau * T ties for T = 1.25 * 2^-34 and not for 1.75 * 2^-34 (tests/test_gpu_step_shaped.py)"""
    from spin_torque_gym_amd import envs
    ta, tb = 1.0 - 2.0 ** -52, 1.0 - 2.0 ** -53
    T = torch.tensor([1.25 * 2.0 ** -34, 1.75 * 2.0 ** -34], dtype=torch.float64)
    tj, _ = envs.knot_tables([0.0, 0.3, ta, tb], torch.ones(2, dtype=torch.float64), T, torch.ones((4, 2), dtype=torch.float64))
    assert tj[2, 0] == tj[3, 0] and tj[2, 1] < tj[3, 1]
    assert wave_step_ref.tables_valid(tj.numpy().T, np.ones((2, 4))).tolist() == [False, True]


# ------------------------------------------------------------------------------------------------
# constructor checks and spaces
# ------------------------------------------------------------------------------------------------
class KnotRecorder(Recorder):
    """tests/test_step_shaped_host.py's recording backend plus the knot entries"""
    log = []

    def set_pulse_knots(self, tau, amplitude_limit, field_knots):
        self._note("set_pulse_knots", np.array(tau), amplitude_limit, field_knots)

    def step_knots_many(self, actions, out_every=True, autoreset=False):
        return self._many("step_knots_many", actions, out_every, autoreset)

    def step_knots_ids(self, actions, env_ids, autoreset=False, out=None, stream=None):
        return self._ids("step_knots_ids", actions, env_ids, stream)

    def _many(self, name, actions, out_every, autoreset):
        res = super()._many(name, actions, out_every, autoreset)
        return res[:5] + (torch.zeros(res[1].shape, dtype=torch.uint8),)


def _krec():
    class R(KnotRecorder):
        log = []
        want_shape = want_field = None
    return R


def test_action_space_shapes_and_bounds():
    import spin_torque_gym_amd as stg
    env = stg.SpinTorqueVecEnv(3, seed=0, backend=_krec(), pulse_knots=TAU4, amplitude_limit=1.5, max_current=1e6, max_duration=2e-9)
    lo, hi = env.single_action_space.low, env.single_action_space.high
    assert lo.shape == hi.shape == (6,) and lo.dtype == np.float32
    assert lo.tolist() == [np.float32(-1e6), 0.0] + [-1.5] * 4 and hi.tolist() == [np.float32(1e6), np.float32(2e-9)] + [1.5] * 4
    assert env.action_space.shape == (3, 6)
    assert env.result_config()["pulse_knots"] == TAU4 and env.result_config()["amplitude_limit"] == 1.5
    one = stg.SpinTorqueEnv(backend=_krec(), pulse_knots=[0.0, 1.0])
    assert one.action_space.shape == (4,) and one.action_space.high[2:].tolist() == [1.0, 1.0]           # amplitude_limit defaults to 1
    assert one.get_device_info()["pulse_knots"] == [0.0, 1.0] and one.get_solver_info()["amplitude_limit"] == 1.0
    plain = stg.SpinTorqueVecEnv(3, seed=0, backend=_krec())
    assert plain.single_action_space.shape == (2,) and "pulse_knots" not in plain.result_config()


def test_pulse_knots_excludes_pulse_shape_and_validates_tau():
    import spin_torque_gym_amd as stg
    from spin_torque_gym_amd.physics import PiecewiseLinear
    R = _krec()
    with pytest.raises(ValueError, match="exclude"):
        stg.SpinTorqueVecEnv(2, backend=R, pulse_knots=TAU4, pulse_shape=PiecewiseLinear([0.0, 1.0], [1.0, 1.0]))
    with pytest.raises(ValueError, match="exclude"):
        stg.SpinTorqueEnv(backend=R, pulse_knots=TAU4, pulse_shape=PiecewiseLinear([0.0, 1.0], [1.0, 1.0]))
    for bad in ([0.5], [], [0.0, 0.5, 0.5], [0.0, 0.6, 0.5], [-0.1, 1.0], [0.0, 1.0 + 2.3e-16], [0.0, np.nan, 1.0], [0.0, np.inf],
                np.linspace(0, 1, 33), [[0.0, 1.0]]):
        with pytest.raises(ValueError, match="pulse_knots"):
            stg.SpinTorqueVecEnv(2, backend=R, pulse_knots=bad)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="amplitude_limit"):
            stg.SpinTorqueVecEnv(2, backend=R, pulse_knots=TAU4, amplitude_limit=bad)
    assert R.log == []
    stg.SpinTorqueVecEnv(2, backend=R, pulse_knots=np.linspace(0, 1, 32))      # STG_MAX_KNOTS knots pass
    # a field goes along with the knots
    env = stg.SpinTorqueVecEnv(2, backend=R, pulse_knots=TAU4, applied_field=[1e4, 0.0, 0.0], max_duration=5e-9)
    name, tau, limit, fk = R.log[-1]
    assert name == "set_pulse_knots" and tau.tolist() == TAU4 and limit == 1.0 and fk[0].tolist() == [0.0, 5e-9]
    assert env.result_config()["applied_field"] is not None


# ------------------------------------------------------------------------------------------------
# the env over a recording backend
# ------------------------------------------------------------------------------------------------
def test_knot_env_reaches_the_knot_entries():
    import spin_torque_gym_amd as stg
    R = _krec()
    n, w = 8, 6
    env = stg.SpinTorqueVecEnv(n, seed=0, backend=R, pulse_knots=TAU4, amplitude_limit=2.0)
    assert _names(R) == ["set_pulse_knots"] and R.log[0][2] == 2.0 and R.log[0][3] is None
    env.reset()
    rng = np.random.default_rng(0)
    # step(): one K = 1 launch of the fused entry, [N,2+P] in, [1,2+P,N] at the backend
    a1 = rng.uniform(0.0, 1.0, (n, w)).astype(np.float32)
    obs, rew, term, trunc, info = env.step(a1)
    name, got, out_every, autoreset = R.log[-1]
    assert name == "step_knots_many" and tuple(got.shape) == (1, w, n) and np.array_equal(got[0].numpy(), a1.T)
    assert tuple(obs.shape) == (n, 12) and tuple(rew.shape) == (n,) and term.dtype == torch.bool and tuple(info["status"].shape) == (n,)
    env.step(torch.from_numpy(a1.T.copy()), actions_soa=True)
    assert np.array_equal(R.log[-1][1][0].numpy(), a1.T)
    # step_many
    a = rng.uniform(0.0, 1.0, (3, n, w)).astype(np.float32)
    obs, rew, term, trunc, info = env.step_many(a, out_every=False)
    name, got, out_every, autoreset = R.log[-1]
    assert name == "step_knots_many" and (out_every, autoreset) == (False, False) and np.array_equal(got.numpy(), a.transpose(0, 2, 1))
    assert tuple(obs.shape) == (1, n, 12)
    # step_ids: list order kept, no workspace
    a2 = rng.uniform(0.0, 1.0, (3, w)).astype(np.float64)
    obs, rew, term, trunc, info = env.step_ids(a2, [6, 1, 3])
    name, got, ids, stream = R.log[-1]
    assert name == "step_knots_ids" and ids == [6, 1, 3] and stream is None and np.array_equal(got.numpy(), a2.T)
    assert info["env_id"].tolist() == [6, 1, 3] and obs[:, 0].tolist() == [6.0, 1.0, 3.0]
    # the action width is checked on the host
    for call in (lambda: env.step(a1[:, :2]), lambda: env.step_many(a[:, :, :2]), lambda: env.step_ids(a2[:, :5], [6, 1, 3])):
        with pytest.raises(ValueError, match="actions must be"):
            call()
    # the pool
    env.async_reset(4, num_streams=2)
    assert [env.recv()[4]["env_id"].tolist() for _ in range(2)] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    a4 = rng.uniform(0.0, 1.0, (4, w)).astype(np.float32)
    env.send(a4, [5, 4, 0, 1])
    env.send(a4[:2], [2, 3])
    with pytest.raises(ValueError, match="actions must be"):
        env.send(a4[:2, :2], [7, 6])
    sends = [r for r in R.log if r[0] == "step_knots_ids"][1:]
    assert [(r[2], r[3]) for r in sends] == [([5, 4, 0, 1], 0), ([2, 3], 1)] and np.array_equal(sends[0][1].numpy(), a4.T)
    assert env.recv()[4]["env_id"].tolist() == [5, 4, 0, 1]
    env.reset()
    assert not {"step", "step_many", "step_ids", "ids_workspace", "step_wave", "step_shaped_many", "step_shaped_ids", "set_pulse_shape"} & set(_names(R))
    assert _names(R).count("set_pulse_knots") == 1
    # a rebuilt backend (what load_state_dict does for another stream key) gets the knots again
    env.backend = env._make_backend()
    assert _names(R).count("set_pulse_knots") == 2
    env.close()


def test_autoreset_reaches_the_knot_entries():
    import spin_torque_gym_amd as stg
    R = _krec()
    env = stg.SpinTorqueVecEnv(4, seed=0, backend=R, pulse_knots=[0.0, 1.0], autoreset=True)
    env.reset()
    obs, rew, term, trunc, info = env.step(np.zeros((4, 4), np.float32))
    assert R.log[-1][0] == "step_knots_many" and R.log[-1][3] is True and tuple(info["final_obs"].shape) == (4, 12)
    obs, rew, term, trunc, info = env.step_many(np.zeros((2, 4, 4), np.float32))
    assert R.log[-1][3] is True and tuple(info["final_obs"].shape) == (2, 4, 12)
    obs, rew, term, trunc, info = env.step_ids(np.zeros((2, 4), np.float32), [2, 3])
    assert R.log[-1][0] == "step_knots_ids" and tuple(info["final_obs"].shape) == (2, 12)


def test_without_pulse_knots_none_of_the_new_methods_is_called():
    import spin_torque_gym_amd as stg
    from spin_torque_gym_amd.physics import PiecewiseLinear

    class Plain(KnotRecorder):
        log = []
        want_field = None

        def set_pulse_knots(self, *a, **k):
            raise AssertionError("set_pulse_knots called without pulse_knots")

        def step_knots_many(self, *a, **k):
            raise AssertionError("step_knots_many called without pulse_knots")

        def step_knots_ids(self, *a, **k):
            raise AssertionError("step_knots_ids called without pulse_knots")
    for shape in (None, PiecewiseLinear([0.0, 1.0], [1.0, 0.5])):
        Plain.want_shape = shape
        env = stg.SpinTorqueVecEnv(8, seed=0, backend=Plain, pulse_shape=shape)
        env.reset()
        env.step(np.zeros((8, 2), np.float32))
        env.step_many(np.zeros((2, 8, 2), np.float32))
        env.step_ids(np.zeros((2, 2), np.float32), [4, 5])
        env.async_reset(4, num_streams=2)
        env.recv()
        env.send(np.zeros((4, 2), np.float32), [0, 1, 2, 3])
        env.reset()
    names = _names(Plain)
    assert names.count("step") == 1 and names.count("step_wave") == 1 and names.count("step_many") == 1 and names.count("step_shaped_many") == 1


def test_a_step_wave_only_backend_gets_step_and_refuses_the_rest():
    """The CPU seam of tests/test_wave_step_host.py has step_wave and nothing newer: step() builds the tables in torch from the parse
    restatement and runs there; the numbers are those of the NumPy step on tables this test builds from its own parse."""
    import spin_torque_gym_amd as stg
    from spin_torque_gym_amd.distributed import ShardedSpinTorqueVecEnv
    p = stt_default_params(volume=8.75e-11)
    n, P, limit = len(edge_actions(np.float32)), 4, 1.0
    tau = np.array(TAU4)
    env = stg.SpinTorqueVecEnv(n, device_params=p, include_thermal_fluctuations=False, backend=WaveOracleBackend, pulse_knots=tau,
                               diagnostics=True, out_layout="soa")
    assert not hasattr(env.backend, "set_pulse_knots")
    env.reset(seed=2)
    act = edge_actions(np.float32, P, limit)
    for call in (lambda: env.step_many(act[None]), lambda: env.step_ids(act[:2], [0, 1]), lambda: env.async_reset(2),
                 lambda: env.send(act[:2], [0, 1]), lambda: env.recv()):
        with pytest.raises(NotImplementedError, match="pulse_knots"):
            call()
    with pytest.raises(NotImplementedError, match=re.compile("ShardedSpinTorqueVecEnv is not implemented with pulse_knots")):
        ShardedSpinTorqueVecEnv(4, pulse_knots=tau)
    st = {k: v.numpy().copy() for k, v in env.backend.get_state().items()}
    obs, rew, term, trunc, info = env.step(torch.from_numpy(act))
    J, T, s = parse_np(act, 2e6, 5e-9, limit)
    cur = knot_tables_np(tau, J, T, s)
    a_in = wave_rows(act)
    Jp, Tp = wave_step_ref.parse_actions(a_in, 2e6, 5e-9)
    assert np.array_equal(Jp, J) and np.array_equal(Tp, T)                    # what step_wave parses from the rows it is handed
    ref = wave_step_ref.step(dict(m=st["m"].T, target=st["target"].T, total_energy=st["total_energy"], step_count=st["step_count"]),
                             a_in, p, "rk4", current=cur)
    assert np.array_equal(obs.numpy(), ref["obs"]) and np.array_equal(info["reward_f64"].numpy(), ref["reward"])
    assert np.array_equal(info["energy"].numpy(), ref["energy"]) and np.array_equal(info["status"].numpy(), ref["status"])
    # the void rows: parsed action (0, 1e-12) in the observation, no energy; zero amplitudes: no energy either
    t_min = np.float32(1e-12 / 5e-9)
    for row in (3, 4):
        assert obs[row, 10] == 0.0 and obs[row, 11] == t_min and info["energy"][row] == 0.0
    assert info["energy"][8] == 0.0 and info["energy"][0] > 0.0
    # the single env over the same seam: Box(2+P,), a wrong-shaped action falls back to the zero action as before
    one = stg.SpinTorqueEnv(device_params=p, include_thermal_fluctuations=False, backend=WaveOracleBackend, pulse_knots=tau)
    one.reset(seed=1)
    o, r, te, tr, inf = one.step(act[0])
    assert o.shape == (12,) and inf["current_density"] == 1.5e6 and inf["energy_consumed"] > 0.0 and "error" not in inf
    o, r, te, tr, inf = one.step(act[3])
    assert (inf["current_density"], inf["pulse_duration"]) == (0.0, 1e-12) and inf["energy_consumed"] == 0.0
    o, r, te, tr, inf = one.step(act[0][:2])
    assert (inf["current_density"], inf["pulse_duration"]) == (0.0, 1e-12)


# ------------------------------------------------------------------------------------------------
# the C-ABI
# ------------------------------------------------------------------------------------------------
def test_symbols_are_bound_with_the_headers_argument_counts():
    import os
    from spin_torque_gym_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 5 and lib.stg_abi_version() == 5
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "spintorque_hip.h")).read()
    for name in ("stg_set_pulse_knots", "stg_step_knots", "stg_step_knots_ids"):
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert decl is not None, name
        assert name in _lib.SYMBOLS and hasattr(lib, name) and len(_lib.SYMBOLS[name][1]) == decl.group(1).count(",") + 1, name
    assert _lib.SYMBOLS["stg_step_knots"] == _lib.SYMBOLS["stg_step_shaped"]
    assert _lib.SYMBOLS["stg_step_knots_ids"] == _lib.SYMBOLS["stg_step_shaped_ids"]
    assert len(_lib.SYMBOLS["stg_set_pulse_knots"][1]) == 7


def test_argument_errors_come_before_any_device_work():
    """no context exists without a GPU: a good call gets as far as the NULL context, a bad one names its check"""
    import ctypes as C
    from spin_torque_gym_amd import _lib
    lib = _lib.load()

    def dp(x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        return x, C.c_void_p(x.ctypes.data)

    def call(*a):
        return lib.stg_set_pulse_knots(None, *a), lib.stg_last_error().decode()
    tau, ptau = dp(TAU4)
    th, pth = dp([0.0, 1e-9])
    hk, phk = dp([[1e4, 0.0, 0.0], [0.0, 0.0, -1e4]])
    assert call(4, ptau, 1.0, 2, pth, phk) == (E_INVALID, "ctx is NULL")
    assert call(0, None, 0.0, 0, None, None) == (E_INVALID, "ctx is NULL")                 # clearing
    for P in (1, -1, 33):
        assert call(P, ptau, 1.0, 0, None, None)[1].startswith("P must be")
    for kh in (1, -2, 33):
        assert call(4, ptau, 1.0, kh, pth, phk)[1].startswith("kh must be")
    assert "tau must not be NULL" in call(4, None, 1.0, 0, None, None)[1]
    assert "th/hk must not be NULL" in call(4, ptau, 1.0, 2, None, phk)[1]
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert "s_limit" in call(4, ptau, bad, 0, None, None)[1], bad
    for bad, word in (([0.0, 0.5, 0.5, 1.0], "strictly increasing"), ([0.0, 0.6, 0.5, 1.0], "strictly increasing"), ([-0.1, 0.2, 0.5, 1.0], "[0, 1]"),
                      ([0.0, 0.2, 0.5, 1.5], "[0, 1]"), ([0.0, np.nan, 0.5, 1.0], "finite")):
        b, pb = dp(bad)
        rc, msg = call(4, pb, 1.0, 0, None, None)
        assert rc == E_INVALID and word in msg, (bad, msg)
    b, pb = dp([1e-9, 1e-9])
    assert "th must be strictly increasing" in call(4, ptau, 1.0, 2, pb, phk)[1]
    assert lib.stg_step_knots(None, 1, None, 0, 1, 0, None, None, None, None, None, None, None, None, None) == E_INVALID
    assert b"ctx" in lib.stg_last_error()
    assert lib.stg_step_knots_ids(None, 1, None, None, 0, 0, None, None, None, None, None, None, None, None, None) == E_INVALID
    assert b"ctx" in lib.stg_last_error()

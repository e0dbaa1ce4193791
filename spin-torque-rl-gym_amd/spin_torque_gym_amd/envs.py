"""Environment level: the Gymnasium-facing mirror of the reference's SpinTorqueEnv.

  SpinTorqueVecEnv ... N independent SpinTorque-v0 environments stepped by one kernel launch; torch tensors in
                       and out (VectorEnv-shaped API).  This is the product.
  SpinTorqueEnv ...... the reference's single-env class as a thin N=1 facade over the same kernels: same
                       constructor keywords, reset/step/render/close, info keys and error behaviour as
                       spin_torque_gym/envs/spin_torque_env.py:26-745, NumPy in and out.

Nothing here computes physics: action clamping, integration, energy, observation, reward and termination all
happen in libspintorque_hip.so.  The host side keeps what is inherently host-side in the reference too:
the seeded PCG64 generator of reset() (gymnasium.utils.seeding), the episode history list and rendering.
"""
import time
import warnings
from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .backend import EnvConfig, HipBackend
from .devices import DeviceFactory, flatten_params

try:  # Gymnasium is optional (it is not part of the build image); the API shape is kept either way.
    import gymnasium as _gym
    from gymnasium import spaces as _spaces
    _EnvBase = _gym.Env
except Exception:  # pragma: no cover - exercised in the build image
    _gym = None
    _spaces = None
    _EnvBase = object


class _Box:
    """Minimal stand-in for gymnasium.spaces.Box when Gymnasium is absent (attributes only)."""

    def __init__(self, low, high, shape=None, dtype=np.float32):
        low = np.asarray(low, dtype=dtype)
        high = np.asarray(high, dtype=dtype)
        self.shape = tuple(shape) if shape is not None else low.shape
        self.low = np.broadcast_to(low, self.shape).astype(dtype)
        self.high = np.broadcast_to(high, self.shape).astype(dtype)
        self.dtype = np.dtype(dtype)
        self._rng = np.random.default_rng()

    def seed(self, seed=None):
        self._rng = np.random.default_rng(seed)

    def sample(self):
        lo = np.where(np.isfinite(self.low), self.low, -1.0)
        hi = np.where(np.isfinite(self.high), self.high, 1.0)
        return self._rng.uniform(lo, hi).astype(self.dtype)

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))

    __contains__ = contains           # `obs in env.observation_space`, as with gymnasium.spaces.Box


def _box(low, high, shape=None, dtype=np.float32):
    if _spaces is not None:
        return _spaces.Box(low=np.asarray(low, dtype=dtype) if shape is None else low,
                           high=np.asarray(high, dtype=dtype) if shape is None else high, shape=shape, dtype=dtype)
    return _Box(low, high, shape, dtype)


def _np_random(seed=None):
    """gymnasium.utils.seeding.np_random: Generator(PCG64(SeedSequence(seed)))."""
    ss = np.random.SeedSequence(seed)
    return np.random.Generator(np.random.PCG64(ss)), ss.entropy


class _TimerTable:
    """Host-side timer table behind get_performance_stats() (the reference's PerformanceProfiler.get_stats shape,
    utils/performance.py:391-474: `<op>_avg_time/_total_time/_count/_min_time/_max_time` plus named counters).  Times are
    host wall-clock around the call: for the vector env that is the enqueue cost of an asynchronous launch, for the N = 1
    facade (which reads the state back every step) the whole step."""

    def __init__(self):
        self._t: Dict[str, List[float]] = {}
        self.counters: Dict[str, int] = {}

    def add(self, name: str, seconds: float) -> None:
        r = self._t.setdefault(name, [0, 0.0, float("inf"), 0.0])
        r[0] += 1
        r[1] += seconds
        r[2] = min(r[2], seconds)
        r[3] = max(r[3], seconds)

    def get_stats(self) -> Dict[str, Any]:
        out: Dict[str, Any] = {}
        for name, (cnt, tot, lo, hi) in self._t.items():
            out.update({f"{name}_avg_time": tot / cnt, f"{name}_total_time": tot, f"{name}_count": cnt,
                        f"{name}_min_time": lo, f"{name}_max_time": hi})
        out.update(self.counters)
        return out

    def reset(self) -> None:
        self._t.clear()
        self.counters.clear()


def _default_env_side_params(device_type: str) -> Dict[str, Any]:
    """SpinTorqueEnv._get_default_device_params (spin_torque_env.py:156-182): the factory's STT defaults, or a
    generic dict for other types (which lacks 'easy_axis', so the factory then rejects it, as in the reference)."""
    if device_type == "stt_mram":
        return DeviceFactory().get_default_parameters("stt_mram")
    return {"volume": 1e-24, "saturation_magnetization": 800e3, "damping": 0.01, "uniaxial_anisotropy": 1e6,
            "polarization": 0.7}


# -- checkpoints across partitions of the envs (shared by SpinTorqueVecEnv and distributed.ShardedSpinTorqueVecEnv) ----------------
# EnvConfig fields that decide results (SpinTorqueVecEnv.result_config adds target_states, autoreset and the device classes)
_RESULT_FIELDS = ("solver", "include_thermal_fluctuations", "temperature", "gamma", "max_step", "rtol", "atol", "max_steps",
                  "max_current", "max_duration", "success_threshold", "energy_penalty_weight", "max_attempts", "skip_done",
                  "torque_model", "noise_model", "correlation_time")
# per-env tensors of a state dict; the env index is the LAST dimension of each (m and target are [3, n])
STATE_TENSORS = ("m", "target", "total_energy", "step_count", "rng_step", "done")


def state_span(st) -> tuple:
    """[lo, hi) of global env ids that a state dict holds: what a sharded checkpoint says, else env_id0 and the tensors' length."""
    if "lo" in st and "hi" in st:
        return int(st["lo"]), int(st["hi"])
    lo = int(st.get("env_id0", 0))
    return lo, lo + int(st["m"].shape[-1])


def check_state_config(st, config) -> None:
    """ValueError naming the first result-deciding field on which the checkpoint's recorded configuration differs from `config`
    (a dict without one -- a plain SpinTorqueVecEnv.state_dict() -- records nothing to compare)."""
    theirs = st.get("config")
    if theirs is None:
        return
    for k, v in config.items():
        if k in theirs and theirs[k] != v:
            raise ValueError(f"checkpoint was taken with {k}={theirs[k]!r}, this env has {k}={v!r}")


def assemble_state(pieces, lo: int, hi: int, tile: bool = True):
    """The state dict of envs [lo, hi) out of `pieces`, state dicts of contiguous spans of global env ids (state_span) saved under any
    partition.  The pieces must agree on n_global, cfg_seed and config; with `tile` they must tile [0, n_global) exactly, otherwise
    they must at least cover [lo, hi).  ValueError names what does not hold.  Slices and at most one torch.cat per tensor."""
    pieces = sorted(pieces, key=state_span)
    if not pieces:
        raise ValueError("an empty list of state dicts")
    first = pieces[0]
    for key in ("n_global", "cfg_seed", "config"):
        for p in pieces[1:]:
            if (key in p) != (key in first):
                raise ValueError(f"some state dicts of the list record {key}, others do not")
            if key == "config":
                check_state_config(p, first.get("config") or {})
            elif key in p and p[key] != first[key]:
                raise ValueError(f"the state dicts disagree on {key}: {first[key]!r} and {p[key]!r}")
    n_global = first.get("n_global")
    cursor = 0 if tile else state_span(first)[0]
    for p in pieces:
        plo, phi = state_span(p)
        if phi - plo != int(p["m"].shape[-1]) or phi < plo:
            raise ValueError(f"a state dict claims lo, hi = [{plo}, {phi}) but holds {int(p['m'].shape[-1])} envs")
        if plo > cursor:
            raise ValueError(f"the lo, hi ranges of the state dicts leave a hole: envs [{cursor}, {plo}) are in none of them")
        if plo < cursor:
            raise ValueError(f"the lo, hi ranges of the state dicts overlap: envs [{plo}, {min(cursor, phi)}) are in two of them")
        cursor = phi
    if tile and n_global is not None and cursor != int(n_global):
        if cursor < int(n_global):
            raise ValueError(f"the lo, hi ranges of the state dicts leave a hole: envs [{cursor}, {int(n_global)}) are in none of them")
        raise ValueError(f"the lo, hi ranges of the state dicts end at {cursor}, past n_global={int(n_global)}")
    if lo < state_span(first)[0] or hi > cursor:
        raise ValueError(f"envs [{lo}, {hi}) asked for, the state dicts hold lo, hi = [{state_span(first)[0]}, {cursor})")
    parts = []                                                   # (piece, first and one-past-last column of it to take)
    for p in pieces:
        plo, phi = state_span(p)
        a, b = max(lo, plo), min(hi, phi)
        if a < b:
            parts.append((p, a - plo, b - plo))
    out = {k: v for k, v in first.items() if k in ("host_rng", "cfg_seed", "config")}
    for key in STATE_TENSORS:
        cols = [torch.as_tensor(p[key])[..., a:b] for p, a, b in parts]
        out[key] = cols[0] if len(cols) == 1 else torch.cat([c.to(cols[0].device) for c in cols], dim=-1)
    out["env_id0"] = int(lo)
    return out


# -- shaped pulses and an applied field on the step path (stg_step_wave, stg_step_shaped) --------------------------------------------
_WAVE_LIMIT = ("{what} is not implemented on this backend while pulse_shape or applied_field is set: step() runs them everywhere "
               "(stg_step_wave); step_many, step_ids and async_reset / send / recv need a backend with the shaped entries "
               "(HipBackend.step_shaped_many / step_shaped_ids: stg_step_shaped, stg_step_shaped_ids), and there is no sharded variant yet")


def check_pulse_shape(shape):
    """pulse_shape= of the envs: a scalar physics.PiecewiseLinear over normalised time tau in [0, 1] (None passes)."""
    from .physics import PiecewiseLinear
    if shape is None:
        return None
    if not isinstance(shape, PiecewiseLinear):
        raise ValueError("pulse_shape must be a physics.PiecewiseLinear (times = normalised tau in [0, 1], scalar values)")
    if shape.vector:
        raise ValueError("pulse_shape takes scalar values [K] (a factor on the action's current density), got [K,3]")
    if float(shape.times[0]) < 0.0 or float(shape.times[-1]) > 1.0:
        raise ValueError("pulse_shape times are normalised: every tau must lie in [0, 1] (tau * pulse duration is the knot time)")
    return shape


def field_knots(applied_field, max_duration):
    """applied_field= of the envs -> (times [K], values [K,3]) in seconds and A/m, or None.  A constant 3-vector becomes the two-knot
    table (0, max_duration) -- the last value holds beyond it --; a physics.PiecewiseLinear with [K,3] values is taken as it is."""
    from .physics import PiecewiseLinear
    if applied_field is None:
        return None
    if isinstance(applied_field, PiecewiseLinear):
        if not applied_field.vector:
            raise ValueError("applied_field as a PiecewiseLinear takes [K,3] values (A/m), got scalar values")
        return applied_field.times.copy(), applied_field.values.copy()
    h = np.asarray(applied_field, dtype=np.float64)
    if h.shape != (3,) or not np.isfinite(h).all():
        raise ValueError("applied_field must be a finite 3-vector in A/m or a physics.PiecewiseLinear with [K,3] values")
    return np.array([0.0, float(max_duration) if max_duration > 0 else 1.0]), np.stack([h, h])


_KNOTS_LIMIT = ("{what} is not implemented on this backend while pulse_knots is set: step() runs everywhere (stg_step_wave on tables "
                "built from the actions); step_many, step_ids and async_reset / send / recv need a backend with the knot entries "
                "(HipBackend.step_knots_many / step_knots_ids: stg_step_knots, stg_step_knots_ids), and there is no sharded variant yet")


def check_pulse_knots(tau, amplitude_limit):
    """pulse_knots= and amplitude_limit= of the envs -> (tau float64 [P], limit): normalised knot times in [0, 1], finite and strictly
    increasing, 2 <= P <= STG_MAX_KNOTS; the limit finite and > 0 (tau None passes as (None, limit))."""
    if tau is None:
        return None, float(amplitude_limit)
    tau = np.array(tau, dtype=np.float64)
    if tau.ndim != 1 or not 2 <= tau.shape[0] <= _lib.STG_MAX_KNOTS:
        raise ValueError(f"pulse_knots takes 2 ... {_lib.STG_MAX_KNOTS} knot times [P], got shape {tau.shape}")
    if not np.isfinite(tau).all() or not (np.diff(tau) > 0).all():
        raise ValueError("pulse_knots must be finite and strictly increasing")
    if float(tau[0]) < 0.0 or float(tau[-1]) > 1.0:
        raise ValueError("pulse_knots times are normalised: every tau must lie in [0, 1] (tau * pulse duration is the knot time)")
    limit = float(amplitude_limit)
    if not (np.isfinite(limit) and limit > 0.0):
        raise ValueError("amplitude_limit must be finite and > 0")
    return tau, limit


def parse_knot_actions_fp64(a: torch.Tensor, max_current: float, max_duration: float, amplitude_limit: float):
    """The action parse of stg_step_knots restated in torch, for actions [2+P,N] float32 or float64: rows 0 and 1 as parse_actions_fp64;
    the amplitude rows in fp64, clamped to +-amplitude_limit (NaN kept); a NaN amplitude voids its env's action to J = 0, T = 1e-12 and
    zero amplitudes.  Returns (J [N], T [N], s [P,N]) float64 -- the values the kernel parses from the same actions, bit for bit."""
    J, T = parse_actions_fp64(a[:2], max_current, max_duration)
    s = a[2:].double().clamp(-amplitude_limit, amplitude_limit)              # (clamp keeps NaN and takes +-Inf to the limit)
    void = torch.isnan(s).any(dim=0)
    J = torch.where(void, torch.zeros_like(J), J)
    T = torch.where(void, torch.full_like(T, 1e-12), T)
    return J, T, torch.where(void[None, :], torch.zeros_like(s), s)


def knot_tables(tau, J: torch.Tensor, T: torch.Tensor, s: torch.Tensor):
    """(tj [P,N], jk [P,N]) of the parsed knot action (J [N], T [N], s [P,N]): knot times tau_j * T, knot values J * s_j, each ONE
    rounded fp64 product."""
    tau = torch.as_tensor(tau, dtype=torch.float64, device=T.device)
    return (tau[:, None] * T[None, :]).contiguous(), (J[None, :] * s).contiguous()


def parse_actions_fp64(a: torch.Tensor, max_current: float, max_duration: float):
    """The kernels' action parse restated in torch, for actions [2,N] float32 or float64: the safety clamp in the action's own dtype
    (current to +-1e8, duration to [1e-12, 1e-6], NaN kept), NaN / Inf in either -> (0, 1e-12), then in fp64 the clips to max_current and
    [1e-12, max_duration].  Returns (J [N], T [N]) float64 -- the values stg_step_wave parses from the same actions, bit for bit."""
    a0, a1 = a[0].clamp(-1e8, 1e8), a[1].clamp(1e-12, 1e-6)                 # (clamp keeps NaN; the bounds are rounded to a's dtype)
    bad = torch.isnan(a0) | torch.isnan(a1) | torch.isinf(a0) | torch.isinf(a1)
    a0 = torch.where(bad, torch.zeros_like(a0), a0)
    a1 = torch.where(bad, torch.full_like(a1, 1e-12), a1)
    return a0.double().clamp(-max_current, max_current), a1.double().clamp(1e-12, max_duration)


def pulse_tables(shape, J: torch.Tensor, T: torch.Tensor):
    """(tj [K,N], jk [K,N]) of a pulse_shape for the parsed (J [N], T [N]): knot times tau_k * T, knot values J * s_k, each ONE rounded
    fp64 product."""
    tau = torch.as_tensor(shape.times, dtype=torch.float64, device=T.device)
    s = torch.as_tensor(shape.values, dtype=torch.float64, device=T.device)
    return (tau[:, None] * T[None, :]).contiguous(), (J[None, :] * s[:, None]).contiguous()


class SpinTorqueVecEnv:
    """N parallel SpinTorque-v0 environments on one MI355X.

    Device classes: pass one ``device_type``/``device_params`` for a homogeneous batch, or lists of both plus
    ``class_index`` (uint8 per env) for mixed batches (up to 64 classes; the per-class constants live in LDS).
    Layout: with ``out_layout='records'`` (default) the kernel writes one 56-byte record per env -- obs[12] f32, reward f32,
    terminated, truncated, status -- and ``obs`` / ``reward`` / the flags are strided *views* of that array (``obs`` is [N,12],
    row stride 14 floats); ``out_layout='soa'`` keeps four separate arrays with a component-major [12,N] obs buffer, of which
    ``obs`` is the transposed view.  No copies either way.  Actions are accepted as [N,2] (Gym convention) or, with
    ``actions_soa=True``, as the kernel's [2,N].
    With ``autoreset`` a step also returns ``info['final_obs']`` -- the terminal observation of the envs whose episode ended on
    this step (their ``obs`` row already holds the new episode's first observation).  ``diagnostics=True`` additionally fills
    ``info['reward_f64']`` (the reward before rounding to fp32) and ``info['energy']`` (the reference's
    info['energy_consumed'], spin_torque_env.py:474-480); by default a step writes the RL-facing outputs only
    (``info['status']`` is then the records' status byte).
    Subsets and asynchronous stepping: ``step_ids(actions, env_ids)`` steps the listed envs only (outputs compact, in list order);
    ``async_reset`` / ``recv`` / ``send`` are the EnvPool contract on top of it (in-flight batches on a small pool of streams).
    Shaped pulses and an applied field: ``pulse_shape`` -- a scalar ``physics.PiecewiseLinear`` over normalised time
    tau in [0, 1]: with the parsed action (J, T) the current is the table of knots (tau_k T, J s_k), last value held beyond the last
    knot -- and ``applied_field`` -- a constant 3-vector in A/m, or a ``PiecewiseLinear`` with [K,3] values in absolute seconds, the
    same for every env, restarted at t = 0 of every pulse.  The step's energy is then (R A)^2 / R times the integral of j(t)^2 over the
    pulse (include/spintorque_hip.h, stg_step_wave).  Class tables work; ``per_env_params`` and ``torque_model='device'`` are refused by
    the library.  ``step()`` runs on stg_step_wave with tables built from the actions; ``step_many``, ``step_ids`` and ``async_reset`` /
    ``send`` / ``recv`` run on stg_step_shaped / stg_step_shaped_ids, which hold the shape on chip (handed to the backend once) and give
    every env the bits ``step()`` gives it.  Only ``ShardedSpinTorqueVecEnv`` still refuses a shape or a field.
    Agent-shaped pulses: ``pulse_knots=tau`` (P normalised knot times in [0, 1]) widens the action to ``[J, T, s_0 ... s_{P-1}]`` -- the
    policy chooses the knot amplitudes per env and per step, clamped to +-``amplitude_limit``; the current is the table of knots
    (tau_j T, J s_j) (include/spintorque_hip.h, stg_step_knots, states the parse: a NaN amplitude voids the action).  Not together with
    ``pulse_shape``; ``applied_field`` works as above.  Actions are [N, 2+P], [K, N, 2+P] for ``step_many`` and [M, 2+P] for
    ``step_ids`` / ``send``; every entry point runs on stg_step_knots / stg_step_knots_ids.
    """

    def __init__(self, num_envs: int, device_type: Union[str, Sequence[str]] = "stt_mram",
                 device_params: Union[None, Dict[str, Any], Sequence[Dict[str, Any]]] = None,
                 class_index=None, target_states: Optional[List[np.ndarray]] = None, max_steps: int = 100,
                 max_current: float = 2e6, max_duration: float = 5e-9, temperature: float = 300.0,
                 include_thermal_fluctuations: bool = True, success_threshold: float = 0.9,
                 energy_penalty_weight: float = 0.1, solver: str = "rk4", seed: Optional[int] = None,
                 autoreset: bool = False, skip_done: bool = False, device_index: int = 0, env_id0: int = 0,
                 max_attempts: int = 200_000, lane_sort: Optional[bool] = None, wave_spec: Optional[bool] = None, torque_model: str = "reference",
                 noise_model: str = "white", correlation_time: float = 1e-12,
                 per_env_params: Optional[Dict[str, Any]] = None, out_layout: str = "records",
                 diagnostics: bool = False, lane_refill: Optional[int] = None, backend=None, pulse_shape=None, applied_field=None,
                 pulse_knots=None, amplitude_limit: float = 1.0):
        self.num_envs = int(num_envs)
        self.pulse_shape = check_pulse_shape(pulse_shape)
        if pulse_knots is not None and pulse_shape is not None:
            raise ValueError("pulse_knots and pulse_shape exclude each other: the action carries the amplitudes, or the shape is fixed")
        self.pulse_knots, self.amplitude_limit = check_pulse_knots(pulse_knots, amplitude_limit)
        self._knots_on = self.pulse_knots is not None
        self._act_w = 2 + (len(self.pulse_knots) if self._knots_on else 0)          # width of one env's action
        self.applied_field = applied_field
        self._field_knots = field_knots(applied_field, max_duration)
        self._wave_on = self.pulse_shape is not None or self._field_knots is not None or self._knots_on
        self._field_tab = None                # the field table on the device, [K,N] / [K,3,N], built on the first shaped step
        factory = DeviceFactory()
        types = [device_type] if isinstance(device_type, str) else list(device_type)
        if device_params is None:
            plist = [_default_env_side_params(t) for t in types]
        elif isinstance(device_params, dict):
            plist = [device_params]
        else:
            plist = list(device_params)
        if len(plist) != len(types):
            raise ValueError("device_type and device_params must have the same length")
        self.devices = [factory.create_device(t, p) for t, p in zip(types, plist)]
        self.device_types = types
        if target_states is None:
            targets = [np.array([0.0, 0.0, 1.0]), np.array([0.0, 0.0, -1.0])]
        else:
            targets = [self.devices[0].validate_magnetization(np.asarray(t, dtype=float)) for t in target_states]
        self.target_states = targets
        self._rng, self._seed = _np_random(seed)
        self.cfg = EnvConfig(solver=solver, include_thermal_fluctuations=include_thermal_fluctuations,
                             temperature=temperature, max_steps=max_steps, max_current=max_current,
                             max_duration=max_duration, success_threshold=success_threshold,
                             energy_penalty_weight=energy_penalty_weight, target_states=[list(t) for t in targets],
                             seed=int(self._rng.integers(0, 2**63 - 1)) if seed is None else int(seed),
                             max_attempts=max_attempts, skip_done=skip_done, lane_sort=lane_sort, wave_spec=wave_spec,
                             torque_model=torque_model, noise_model=noise_model, correlation_time=correlation_time,
                             out_layout=out_layout, diagnostics=bool(diagnostics), lane_refill=lane_refill)
        self.autoreset = bool(autoreset)
        self.diagnostics = bool(diagnostics)
        # `backend` is a test seam: a class/callable with HipBackend's constructor signature (tests inject the CPU
        # oracle for the gloo runs and as the comparator); the product default is the HIP library, nothing else.
        self._backend_factory = HipBackend if backend is None else backend
        self._device_index, self.env_id0 = int(device_index), int(env_id0)
        self._class_index, self._per_env_params = class_index, per_env_params
        if per_env_params and len(self.devices) > 1 and class_index is None:
            raise ValueError("per_env_params with several base device classes needs class_index (the base of each env)")
        self.profiler = _TimerTable()
        self.backend = self._make_backend()
        n_amp = self._act_w - 2
        self.single_action_space = _box([-max_current, 0.0] + [-self.amplitude_limit] * n_amp,
                                        [max_current, max_duration] + [self.amplitude_limit] * n_amp, dtype=np.float32)
        self.single_observation_space = _box(-np.inf, np.inf, shape=(12,), dtype=np.float32)
        self._needs_reset = True
        self._pool = None                     # the send/recv pool while in async mode (async_reset ... reset)
        self._ids_ws = None                   # workspace of synchronous step_ids calls (sized for num_envs)

    # batched spaces of gymnasium.vector.VectorEnv, built on first use (N x 2 / N x 12 bounds)
    @property
    def action_space(self):
        if getattr(self, "_action_space", None) is None:
            lo, hi = self.single_action_space.low, self.single_action_space.high
            self._action_space = _box(np.tile(lo, (self.num_envs, 1)), np.tile(hi, (self.num_envs, 1)), dtype=np.float32)
        return self._action_space

    @property
    def observation_space(self):
        if getattr(self, "_observation_space", None) is None:
            self._observation_space = _box(-np.inf, np.inf, shape=(self.num_envs, 12), dtype=np.float32)
        return self._observation_space

    def _make_backend(self):
        """One context for (num_envs, cfg, env_id0) with this env's device parameters installed."""
        b = self._backend_factory(self.num_envs, self.cfg, self._device_index, self.env_id0)
        if self._per_env_params:
            # device-to-device variation: every env gets its own record, starting from its base device class (one class, or
            # class_index into several -- a mixed STT/SOT/VCMA batch); keys are the reference's device_params keys, values
            # arrays of length num_envs ([num_envs, 3] for vectors)
            from .devices import per_env_param_block_multi
            cls = None if self._class_index is None else torch.as_tensor(self._class_index).cpu().numpy()
            b.set_params_per_env(*per_env_param_block_multi([flatten_params(d) for d in self.devices], cls, self.num_envs,
                                                            self._per_env_params))
        else:
            b.set_params([flatten_params(d) for d in self.devices], self._class_index)
        if self._knots_on:
            if self._shaped(b):
                b.set_pulse_knots(self.pulse_knots, self.amplitude_limit, self._field_knots)      # once per context
        elif self._wave_on and self._shaped(b):
            b.set_pulse_shape(self.pulse_shape, self._field_knots)           # once per context: the fused / subset entries read it
        return b

    def _shaped(self, backend):
        """Does the backend offer the fused / subset entries of this env's drive -- the knot entries with pulse_knots, the shaped ones
        otherwise?  (HipBackend does; a test seam may offer step_wave only.)"""
        return getattr(backend, "step_knots_many" if self._knots_on else "step_shaped_many", None) is not None

    # -- Gymnasium VectorEnv-shaped API ---------------------------------------------------------------
    def reset(self, seed: Optional[int] = None, options: Optional[Dict[str, Any]] = None):
        """options: 'initial_state' / 'target_state' as [N,3] (or [3], broadcast) arrays, 'mask' (bool [N]) to
        reset a subset.  Without them states are drawn on the device from Philox(seed, env_id, ...)."""
        options = options or {}
        self._end_async()
        if seed is not None:
            self._rng, self._seed = _np_random(seed)
        dev_seed = int(self._rng.integers(0, 2**63 - 1))
        init = self._soa3(options.get("initial_state"))
        tgt = self._soa3(options.get("target_state"))
        mask = options.get("mask")
        if mask is not None:
            mask = torch.as_tensor(mask).to(torch.uint8)
        t0 = time.perf_counter()
        obs = self.backend.reset(mask, init, tgt, dev_seed)
        self.profiler.add("reset", time.perf_counter() - t0)
        self._needs_reset = False
        return obs.t(), {}

    def step(self, actions, actions_soa: bool = False, out=None):
        """out (out_layout='records' only): a uint8 [N,56] record array that receives this step's outputs instead of the
        env's own (double buffering; the multi-GPU env passes its slice of the global record array)."""
        if self._needs_reset:
            raise RuntimeError("Environment must be reset before calling step")
        self._no_pool("step")
        a = torch.as_tensor(actions)
        if not actions_soa:
            a = a.t()
        if self._knots_on and (a.dim() != 2 or a.shape[0] != self._act_w):
            raise ValueError(f"actions must be [N, {self._act_w}] (J, T and {self._act_w - 2} knot amplitudes), got {tuple(torch.as_tensor(actions).shape)}")
        t0 = time.perf_counter()
        if self._knots_on and self._shaped(self.backend):
            if out is not None:
                raise NotImplementedError("step(out=) is not implemented with pulse_knots")
            obs, rew, rew64, term, trunc, status = (None if x is None else x[0] for x in
                                                    self.backend.step_knots_many(a.unsqueeze(0), out_every=True, autoreset=self.autoreset))
            self.profiler.add("step", time.perf_counter() - t0)
            info = {} if status is None else {"status": status}
            if self.autoreset:
                info["final_obs"] = self.backend.final_obs_many[0].t()
            if self.diagnostics:
                info.update(reward_f64=rew64, energy=self.backend.energy_many[0])
            return obs.t(), rew, term.bool(), trunc.bool(), info
        if self._wave_on:
            a = a.to(device=self.backend.device, dtype=torch.float64 if a.dtype == torch.float64 else torch.float32)
            kw = {} if out is None else {"out": out}
            wave = self._wave_tables(a)
            if self._knots_on:
                # stg_step_wave parses rows 0 and 1 itself: a void action goes in as a NaN current, which it parses to (0, 1e-12)
                void = torch.isnan(a[2:]).any(dim=0)
                a = torch.stack([torch.where(void, torch.full_like(a[0], float("nan")), a[0]), a[1]])
            obs, rew, rew64, term, trunc, status = self.backend.step_wave(a, wave, autoreset=self.autoreset, **kw)
        elif out is None:
            obs, rew, rew64, term, trunc, status = self.backend.step(a, autoreset=self.autoreset)
        else:
            obs, rew, rew64, term, trunc, status = self.backend.step(a, autoreset=self.autoreset, out=out)
        self.profiler.add("step", time.perf_counter() - t0)
        # diagnostics=False (default): the launch writes the RL-facing outputs only; `status` is then the status byte of the
        # records (a view; absent in the SoA layout).  diagnostics=True adds the fp64 reward and the step's Joule energy (the
        # reference's info['energy_consumed'] etc. at N = 1).
        info = {} if status is None else {"status": status}
        if self.autoreset:
            # same-step auto-reset: rows of `obs` whose episode just ended already hold the new episode's first
            # observation; their terminal observation is in info["final_obs"] (valid where terminated | truncated) --
            # RL-facing data (bootstrapping at truncation), so it is there whatever `diagnostics` says
            info["final_obs"] = self.backend.final_obs.t()
        if self.diagnostics:
            info.update(reward_f64=rew64, energy=self.backend.energy)
        return obs.t(), rew, term.bool(), trunc.bool(), info

    def _wave_tables(self, a):
        """The tables of one shaped step for actions a [2,N] on the device (the `wave` of HipBackend.step_wave): a few elementwise
        ops on [K,N].  The current table follows the parsed action; the field table is the same at every step."""
        wave = {"current": None, "field": None}
        if self._knots_on:
            J, T, s = parse_knot_actions_fp64(a, self.cfg.max_current, self.cfg.max_duration, self.amplitude_limit)
            wave["current"] = knot_tables(self.pulse_knots, J, T, s)
        if self.pulse_shape is not None:
            J, T = parse_actions_fp64(a, self.cfg.max_current, self.cfg.max_duration)
            wave["current"] = pulse_tables(self.pulse_shape, J, T)
        if self._field_knots is not None:
            if self._field_tab is None:
                n, dev = self.num_envs, self.backend.device
                th = torch.as_tensor(self._field_knots[0], dtype=torch.float64, device=dev)
                hk = torch.as_tensor(self._field_knots[1], dtype=torch.float64, device=dev)
                self._field_tab = (th[:, None].expand(-1, n).contiguous(), hk[:, :, None].expand(-1, -1, n).contiguous())
            wave["field"] = self._field_tab
        return wave

    def _no_wave(self, what):
        if self._wave_on and not self._shaped(self.backend):
            raise NotImplementedError((_KNOTS_LIMIT if self._knots_on else _WAVE_LIMIT).format(what=what))

    def step_many(self, actions, out_every: bool = True, actions_soa: bool = False):
        """K env steps in one launch.  actions [K,N,2] (or [K,2,N] with actions_soa); with pulse_knots the 2 is 2+P."""
        self._no_pool("step_many")
        self._no_wave("step_many")
        a = torch.as_tensor(actions)
        if not actions_soa:
            a = a.transpose(1, 2)
        t0 = time.perf_counter()
        if self._knots_on and (a.dim() != 3 or a.shape[1] != self._act_w):
            raise ValueError(f"actions must be [K, N, {self._act_w}], got {tuple(torch.as_tensor(actions).shape)}")
        launch = self.backend.step_knots_many if self._knots_on else (self.backend.step_shaped_many if self._wave_on else self.backend.step_many)
        obs, rew, rew64, term, trunc, status = launch(a, out_every=out_every, autoreset=self.autoreset)
        self.profiler.add("step_many", time.perf_counter() - t0)
        info = {} if status is None else {"status": status}
        if self.autoreset:
            info["final_obs"] = self.backend.final_obs_many.transpose(1, 2)     # [K or 1, N, 12]
        if self.diagnostics:
            info.update(reward_f64=rew64, energy=self.backend.energy_many)
        return obs.transpose(1, 2), rew, term.bool(), trunc.bool(), info

    def _soa3(self, v):
        if v is None:
            return None
        t = torch.as_tensor(np.asarray(v, dtype=np.float64) if not torch.is_tensor(v) else v).to(torch.float64)
        if t.dim() == 1:
            t = t.unsqueeze(0).expand(self.num_envs, 3)
        if tuple(t.shape) != (self.num_envs, 3):
            raise ValueError(f"expected [N,3] or [3], got {tuple(t.shape)}")
        # device.validate_magnetization (base_device.py:108-116) raises for a zero vector; the kernel then normalises
        if not bool(torch.all(torch.linalg.norm(t, dim=1) >= 1e-12)) or not bool(torch.isfinite(t).all()):
            raise ValueError("Magnetization vector cannot be zero")
        return t.t().contiguous()

    # -- checkpoint / resume ---------------------------------------------------------------------------
    # (the second row: the global metadata a ShardedSpinTorqueVecEnv checkpoint adds to the same dict, distributed.py)
    _HOST_KEYS = ("host_rng", "cfg_seed", "env_id0",
                  "n_global", "world", "rank", "lo", "hi", "config")

    def result_config(self) -> Dict[str, Any]:
        """The constructor arguments that decide an env's results, as plain data: what a checkpoint taken under one partition of the
        envs must agree on with the env that loads it (check_state_config).  Not in it: what is bit-identical by construction
        (lane_sort, wave_spec, lane_refill, out_layout, diagnostics) and the per-env tables (class_index, per_env_params)."""
        d = {k: getattr(self.cfg, k) for k in _RESULT_FIELDS}
        d["target_states"] = [[float(x) for x in t] for t in self.cfg.target_states]
        d["autoreset"] = self.autoreset
        d["device_params"] = [bytes(flatten_params(dev)).hex() for dev in self.devices]
        if self._wave_on:                     # (only then: a plain env's dict stays what it was)
            d["pulse_shape"] = None if self.pulse_shape is None else [self.pulse_shape.times.tolist(), self.pulse_shape.values.tolist()]
            d["applied_field"] = None if self._field_knots is None else [x.tolist() for x in self._field_knots]
        if self._knots_on:
            d["pulse_knots"] = self.pulse_knots.tolist()
            d["amplitude_limit"] = self.amplitude_limit
        return d

    def state_dict(self):
        """Device state + everything the random streams hang on: the host PCG64 state (reset seeds), `cfg.seed` (the
        Philox key of the thermal field and of device-side auto-resets) and `env_id0` (its counter offset)."""
        self._no_pool("state_dict")
        st = {k: v.cpu() for k, v in self.backend.get_state().items()}
        st["host_rng"] = self._rng.bit_generator.state
        st["cfg_seed"] = int(self.cfg.seed)
        st["env_id0"] = int(self.env_id0)
        return st

    def load_state_dict(self, st):
        """Resumes bit-for-bit: an env built with another stream key (e.g. seed=None in a new process) or env_id0 gets
        its context rebuilt with the checkpoint's before the state is restored.
        Also takes a LIST of ShardedSpinTorqueVecEnv per-rank dicts (any world size): this env then takes the envs
        [env_id0, env_id0 + num_envs) out of them.  A dict that names its configuration (`config`, the sharded env's) must agree with
        this env's on every field that decides results, else ValueError."""
        self._end_async()
        if isinstance(st, (list, tuple)):
            st = assemble_state(st, self.env_id0, self.env_id0 + self.num_envs)
        check_state_config(st, self.result_config())
        seed, id0 = int(st.get("cfg_seed", self.cfg.seed)), int(st.get("env_id0", self.env_id0))
        if seed != int(self.cfg.seed) or id0 != self.env_id0:
            self.backend.close()
            self.cfg.seed, self.env_id0 = seed, id0
            self.backend = self._make_backend()
        self.backend.set_state({k: v for k, v in st.items() if k not in self._HOST_KEYS})
        if "host_rng" in st:
            self._rng.bit_generator.state = st["host_rng"]
        self._needs_reset = False

    def get_performance_stats(self) -> Dict[str, Any]:
        """Host timer table + on-device counters (the reference's get_performance_stats shape, spin_torque_env.py:711-718;
        its 'optimizer' entry is the result/observation cache, which is deliberately not reproduced -- SURVEY H1/H2)."""
        c = self.backend.counters()
        prof = self.profiler.get_stats()
        prof.update(env_steps=c["env_steps"], solver_work_units=c["work_units"], noop_steps=c["noop_steps"])
        return {"profiler": prof, "optimizer": {"cache": "not reproduced (SURVEY H1/H2)", "cache_hits": 0, "cache_misses": 0},
                "health": self.get_health_report()}

    def get_state(self):
        return self.backend.get_state()

    def get_health_report(self):
        from .harness import health_report
        return health_report(self)

    def close(self):
        self._end_async()
        self.backend.close()

    # -- subset stepping and the EnvPool-style send/recv pool ------------------------------------------------
    def _check_ids(self, env_ids) -> np.ndarray:
        """env_ids (host or device integer tensor, array or sequence) -> host int64 [M].  Range and duplicate checks run on the host:
        device ids cost one small device-to-host copy."""
        if torch.is_tensor(env_ids):
            if env_ids.is_floating_point() or env_ids.is_complex() or env_ids.dtype == torch.bool:
                raise TypeError("env_ids must be integers")
            ids = env_ids.detach().to("cpu", torch.int64).numpy().reshape(-1)
        else:
            ids = np.asarray(env_ids)
            if ids.size and ids.dtype.kind not in "iu":
                raise TypeError("env_ids must be integers")
            ids = ids.astype(np.int64).reshape(-1)
        if ids.size == 0:
            raise ValueError("env_ids is empty")
        if int(ids.min()) < 0 or int(ids.max()) >= self.num_envs:
            raise ValueError(f"env ids must be in [0, {self.num_envs})")
        seen = np.zeros(self.num_envs, dtype=bool)        # (O(N) instead of a sort: the pool checks every send)
        seen[ids] = True
        if int(np.count_nonzero(seen)) != ids.size:
            raise ValueError("env_ids holds duplicate ids")
        return ids

    def _ids_actions(self, actions, m):
        a = torch.as_tensor(actions)
        w = self._act_w
        if a.dim() != 2 or tuple(a.shape) != (m, w):
            raise ValueError(f"actions must be [M, {w}] = [{m}, {w}], got {tuple(a.shape)}")
        return a.t()

    def _ids_result(self, out, env_id):
        info = {"env_id": env_id}
        if out.get("status") is not None:
            info["status"] = out["status"]
        if self.autoreset:
            info["final_obs"] = out["final_obs"].t()
        if self.diagnostics:
            info.update(reward_f64=out["reward64"], energy=out["energy"])
        return out["obs"].t(), out["reward"], out["terminated"].bool(), out["truncated"].bool(), info

    def step_ids(self, actions, env_ids):
        """One env step of the envs `env_ids` only (every other env is left exactly as it is).  actions [M,2], row j for env_ids[j].
        Returns obs [M,12], reward [M], terminated [M], truncated [M], info -- all in list order -- with info['env_id'] (int64 [M]) and
        'status', plus 'final_obs' with autoreset and 'reward_f64' / 'energy' with diagnostics.  An env's results are those a full
        step() would give it with the same action."""
        if self._needs_reset:
            raise RuntimeError("Environment must be reset before calling step_ids")
        self._no_pool("step_ids")
        self._no_wave("step_ids")
        ids = self._check_ids(env_ids)
        a = self._ids_actions(actions, ids.size)
        if self._ids_ws is None and not self._wave_on:
            self._ids_ws = self.backend.ids_workspace(self.num_envs)
        env_id = torch.as_tensor(ids).to(self.backend.device)
        t0 = time.perf_counter()
        if self._knots_on:
            out = self.backend.step_knots_ids(a, env_id, autoreset=self.autoreset)
        elif self._wave_on:
            out = self.backend.step_shaped_ids(a, env_id, autoreset=self.autoreset)
        else:
            out = self.backend.step_ids(a, env_id, autoreset=self.autoreset, workspace=self._ids_ws)
        self.profiler.add("step_ids", time.perf_counter() - t0)
        return self._ids_result(out, env_id)

    def async_reset(self, batch_size: int, seed: Optional[int] = None, num_streams: int = 4):
        """Resets every env and enters async mode (EnvPool's contract): batch k = envs [kB, (k+1)B) is then ready for recv() with its
        reset observation.  batch_size B must be even (envs 2k and 2k+1 share a 128-byte line of state and are always sent together,
        see send).  num_streams (<= 4 by default, the HIP runtime's default hardware-queue count): streams of the pool."""
        self._no_wave("async_reset / send / recv")
        B, N = int(batch_size), self.num_envs
        if B < 2 or B % 2:
            raise ValueError("batch_size must be even (>= 2): envs 2k and 2k+1 are stepped together")
        if B > N:
            raise ValueError(f"batch_size must be <= num_envs ({N})")
        if not 1 <= int(num_streams) <= 32:
            raise ValueError("num_streams must be in [1, 32]")
        obs, _ = self.reset(seed=seed)
        self._pool = _AsyncPool(self, B, int(num_streams), obs)

    def recv(self):
        """Outputs of a completed in-flight batch, the oldest completed first (spin-polls the batches' events): (obs, reward,
        terminated, truncated, info) as step_ids returns them, info['env_id'] naming the envs.  The tensors stay valid until those ids are
        sent again."""
        self._no_wave("recv")
        if self._pool is None:
            raise RuntimeError("recv: not in async mode (call async_reset first)")
        return self._pool.recv()

    def send(self, actions, env_ids):
        """Steps env_ids with actions [M,2] asynchronously, on the next stream of the pool.  The ids must have been received and not sent
        since, and be pair-closed: with env 2k or 2k+1 the set holds its partner too (the last env of an odd num_envs has none) -- the
        two share a 128-byte line of state, which two launches in flight at once must not (include/spintorque_hip.h, stg_step_ids).
        A send may merge received batches or split one along pairs."""
        self._no_wave("send")
        if self._pool is None:
            raise RuntimeError("send: not in async mode (call async_reset first)")
        self._pool.send(actions, env_ids)

    def _no_pool(self, what):
        if self._pool is not None:
            raise RuntimeError(f"{what}: the send/recv pool is active (async_reset); call reset() to end async mode first")

    def _end_async(self):
        if self._pool is not None:
            self._pool.drain()
            self._pool = None


class _AsyncPool:
    """Bookkeeping of SpinTorqueVecEnv's async mode: which envs are in flight, which are received and held by the caller, and the
    in-flight launches (oldest first) with their completion events.  Each stream has its own stg_step_ids workspace (none with a pulse
    shape or an applied field: stg_step_shaped_ids stages nothing); the output arrays of a launch are its own (they stay valid for as
    long as the caller holds them)."""

    def __init__(self, env, batch_size, num_streams, reset_obs):
        self.env = env
        b = env.backend
        n = env.num_envs
        self.streams = b.make_streams(num_streams)
        self.workspaces = [None if env._wave_on else b.ids_workspace(n) for _ in self.streams]
        self.next_stream = 0
        self.held = np.zeros(n, dtype=bool)           # received, not sent since
        self.inflight = []                            # [(ids host int64, event or None, result or None, outputs, env_id)], in send order
        dev = b.device
        for lo in range(0, n, batch_size):            # the reset batches: complete from the start
            hi = min(lo + batch_size, n)
            m = hi - lo
            env_id = torch.arange(lo, hi, dtype=torch.int64, device=dev)
            info = {"env_id": env_id, "status": torch.zeros(m, dtype=torch.uint8, device=dev)}
            if env.autoreset:
                info["final_obs"] = torch.zeros((m, 12), dtype=torch.float32, device=dev)
            if env.diagnostics:
                info.update(reward_f64=torch.zeros(m, dtype=torch.float64, device=dev), energy=torch.zeros(m, dtype=torch.float64, device=dev))
            res = (reset_obs[lo:hi].clone(), torch.zeros(m, dtype=torch.float32, device=dev), torch.zeros(m, dtype=torch.bool, device=dev),
                   torch.zeros(m, dtype=torch.bool, device=dev), info)
            self.inflight.append((np.arange(lo, hi, dtype=np.int64), None, res, None, env_id))

    def recv(self):
        if not self.inflight:
            raise RuntimeError("recv: nothing is in flight (send received envs first)")
        while True:
            for k, (ids, ev, res, out, env_id) in enumerate(self.inflight):
                if ev is None or ev.query():
                    del self.inflight[k]
                    if out is not None:           # (complete: from here on the arrays are read on the current stream)
                        self.env.backend.hand_over(out)
                        res = self.env._ids_result(out, env_id)
                    self.held[ids] = True
                    return res
            time.sleep(0)

    def send(self, actions, env_ids):
        env = self.env
        ids = env._check_ids(env_ids)
        if not self.held[ids].all():
            raise ValueError("send: every id must have been received (recv) and not sent since")
        n = env.num_envs
        in_set = np.zeros(n, dtype=bool)
        in_set[ids] = True
        partner = ids ^ 1
        partner = partner[partner < n]
        if not in_set[partner].all():
            raise ValueError("send: the id set splits a pair (2k, 2k+1); send both envs of a pair together")
        a = env._ids_actions(actions, ids.size)
        k = self.next_stream
        self.next_stream = (k + 1) % len(self.streams)
        b = env.backend
        env_id = torch.as_tensor(ids).to(b.device)
        if env._knots_on:
            out = b.step_knots_ids(a, env_id, autoreset=env.autoreset, stream=self.streams[k])
        elif env._wave_on:
            out = b.step_shaped_ids(a, env_id, autoreset=env.autoreset, stream=self.streams[k])
        else:
            out = b.step_ids(a, env_id, autoreset=env.autoreset, workspace=self.workspaces[k], stream=self.streams[k])
        ev = b.record_event(self.streams[k])
        self.held[ids] = False
        self.inflight.append((ids, ev, None, out, env_id))

    def drain(self):
        for _, ev, _, _, _ in self.inflight:
            if ev is not None:
                ev.synchronize()
        self.inflight = []


class SpinTorqueEnv(_EnvBase):
    """Drop-in for spin_torque_gym.envs.SpinTorqueEnv (spin_torque_env.py:26-745) running on the GPU path.

    Same keyword arguments; two additions select what the reference cannot express: ``solver`` ('rk4' is the
    SimpleLLGSSolver/RobustLLGSSolver pair the reference env really uses, 'rk45' the LLGSSolver the north star
    names) and ``device_index``.  Known reference behaviours are reproduced, not repaired:
    solver failure leaves m unchanged but still charges energy (H3), the energy "penalty" is a bonus (H7),
    action_mode='discrete' and observation_mode='dict' end in the catch-all error return (H8).  Not reproduced:
    the result/observation caches (H1/H2), which return stale data.
    """

    metadata = {"render_modes": ["human", "rgb_array"], "render_fps": 30}

    def __init__(self, device_type: str = "stt_mram", device_params: Optional[Dict[str, Any]] = None,
                 target_states: Optional[List[np.ndarray]] = None, max_steps: int = 100, max_current: float = 2e6,
                 max_duration: float = 5e-9, temperature: float = 300.0, include_thermal_fluctuations: bool = True,
                 reward_components: Optional[Dict[str, Dict]] = None, action_mode: str = "continuous",
                 observation_mode: str = "vector", success_threshold: float = 0.9, energy_penalty_weight: float = 0.1,
                 render_mode: Optional[str] = None, seed: Optional[int] = None, solver: str = "rk4",
                 device_index: int = 0, backend=None, pulse_shape=None, applied_field=None, pulse_knots=None,
                 amplitude_limit: float = 1.0):
        if reward_components is not None:
            raise NotImplementedError("custom reward callables are arbitrary Python and stay on the reference "
                                      "(SURVEY.md section 2); the GPU path implements the default 4-component reward")
        if action_mode not in ("continuous", "discrete"):
            raise ValueError(f"Unknown action mode: {action_mode}")
        if observation_mode not in ("vector", "dict"):
            raise ValueError(f"Unknown observation mode: {observation_mode}")
        self.device_type = device_type
        self.max_steps, self.max_current, self.max_duration = max_steps, max_current, max_duration
        self.temperature, self.include_thermal = temperature, include_thermal_fluctuations
        self.action_mode, self.observation_mode = action_mode, observation_mode
        self.success_threshold, self.energy_penalty_weight = success_threshold, energy_penalty_weight
        self.render_mode = render_mode
        self._np_random = None
        self.seed(seed)
        self._vec = SpinTorqueVecEnv(1, device_type, device_params, None, target_states, max_steps, max_current,
                                     max_duration, temperature, include_thermal_fluctuations, success_threshold,
                                     energy_penalty_weight, solver, seed, False, False,
                                     device_index, 0, diagnostics=True, backend=backend, pulse_shape=pulse_shape,
                                     applied_field=applied_field, pulse_knots=pulse_knots, amplitude_limit=amplitude_limit)
        self.device = self._vec.devices[0]
        self.target_states = self._vec.target_states
        self.solver_name = solver
        if action_mode == "continuous":
            self.action_space = self._vec.single_action_space          # Box(2,), or Box(2+P,) with pulse_knots
        else:
            self.current_levels = np.linspace(-max_current, max_current, 5)
            self.duration_levels = np.array([0.1e-9, 0.5e-9, 1.0e-9, 2.0e-9])
            self.action_space = _spaces.Discrete(20) if _spaces is not None else None
        self.observation_space = _box(-np.inf, np.inf, shape=(12,), dtype=np.float32)
        self.current_magnetization = None
        self.target_magnetization = None
        self.step_count = 0
        self.total_energy = 0.0
        self.episode_history: List[Dict[str, Any]] = []
        self.last_action = np.zeros(2)
        self._solve_count = 0
        self._solve_time = [0.0, 0.0]         # last, total (wall time of the synchronous N = 1 step)
        self.profiler = _TimerTable()
        self.renderer = None                  # the persistent figure of render('human') (spin_torque_env.py:152-154, 570-587)
        if render_mode == "human":
            from .render import HumanFigure
            self.renderer = HumanFigure("macrospin")

    # -- seeding (spin_torque_env.py:694-697) -------------------------------------------------------------
    def seed(self, seed: Optional[int] = None):
        self._np_random, s = _np_random(seed)
        return [s]

    # -- reset (spin_torque_env.py:250-308) -----------------------------------------------------------------
    def reset(self, seed: Optional[int] = None, options: Optional[Dict[str, Any]] = None):
        t_reset = time.perf_counter()
        if seed is not None:
            self._np_random, _ = _np_random(seed)
        options = options or {}
        self.step_count, self.total_energy = 0, 0.0
        self.episode_history = []
        self.last_action = np.zeros(2)
        if "initial_state" in options:
            m0 = self.device.validate_magnetization(options["initial_state"])
        else:
            m0 = self.device.validate_magnetization(self._np_random.normal(0, 1, 3))
        if "target_state" in options:
            tgt = self.device.validate_magnetization(options["target_state"])
        else:
            tgt = self.target_states[self._np_random.integers(len(self.target_states))].copy()
        obs, _ = self._vec.reset(options={"initial_state": np.asarray(m0, dtype=np.float64)[None, :],
                                          "target_state": np.asarray(tgt, dtype=np.float64)[None, :]})
        self._pull_state()
        self.profiler.add("env_reset", time.perf_counter() - t_reset)
        return obs[0].cpu().numpy().copy(), self._get_info()

    def _pull_state(self):
        st = self._vec.get_state()
        self.current_magnetization = st["m"][:, 0].cpu().numpy().copy()
        self.target_magnetization = st["target"][:, 0].cpu().numpy().copy()
        self.total_energy = float(st["total_energy"][0])
        self.step_count = int(st["step_count"][0])

    # -- step (spin_torque_env.py:310-407) ------------------------------------------------------------------
    def step(self, action):
        if self.current_magnetization is None:
            raise RuntimeError("Environment must be reset before calling step")
        try:
            if self.action_mode != "continuous" or self.observation_mode != "vector":
                # H8: the reference's safety wrapper rejects these modes' inputs and the catch-all takes over
                raise TypeError("only length-1 arrays can be converted to Python scalars")
            a = action if isinstance(action, np.ndarray) else np.array(action, dtype=np.float32)
            w = self._vec._act_w
            if a.shape != (w,):                     # monitoring.py:300-302
                a = np.array([0.0, 1e-12] + [0.0] * (w - 2), dtype=np.float32)
            if a.dtype not in (np.float32, np.float64):
                a = a.astype(np.float32)
            prev_alignment = float(np.dot(self.current_magnetization, self.target_magnetization))
            t_step = time.perf_counter()
            obs, rew, term, trunc, info_t = self._vec.step(torch.from_numpy(np.ascontiguousarray(a)).unsqueeze(0))
            obs_np = obs[0].cpu().numpy().copy()
            reward = float(info_t["reward_f64"][0])
            status = int(info_t["status"][0])
            energy = float(info_t["energy"][0])
            self._pull_state()
            self._solve_count += 1
            dt_step = time.perf_counter() - t_step
            self._solve_time = [dt_step, self._solve_time[1] + dt_step]
            self.profiler.add("env_step", dt_step)
            # the kernel's parsed action comes back through the observation; recompute it in fp64 for `info`
            J, T = _parse_action_host(a[:2], self.max_current, self.max_duration)
            if np.isnan(a[2:]).any():               # a NaN amplitude voids the action (stg_step_knots)
                J, T = 0.0, 1e-12
            self.last_action = np.array([J, T])
            alignment = float(np.dot(self.current_magnetization, self.target_magnetization))
            terminated, truncated = bool(term[0]), bool(trunc[0])
            self.episode_history.append({"step": self.step_count, "action": [J, T],
                                         "magnetization": self.current_magnetization.copy(), "reward": reward,
                                         "energy": energy, "alignment": alignment})
            info = self._get_info()
            info.update({"final_magnetization": self.current_magnetization.copy(), "energy_consumed": energy,
                         "pulse_duration": T, "current_density": J,
                         "simulation_success": status != _lib.STATUS_NOOP})
            info.update({"is_success": terminated, "step_energy": energy,
                         "alignment_improvement": alignment - prev_alignment, "current_alignment": alignment})
            success_c = 10.0 if terminated else 0.0
            info.update({"reward_components": {"success": success_c, "energy": -energy / 1e-12,
                                               "progress": alignment - prev_alignment, "stability": 0.0},
                         "total_reward": reward, "solver_status": status})
            return obs_np, reward, terminated, truncated, info
        except Exception as e:                      # spin_torque_env.py:397-407
            obs = self._vec.backend.obs[:, 0].cpu().numpy().copy()
            return obs, -1.0, False, True, {"error": str(e), "step_count": self.step_count}

    def _get_info(self):
        align = float(np.dot(self.current_magnetization, self.target_magnetization)) if self.current_magnetization is not None else 0.0
        return {"step_count": self.step_count, "total_energy": self.total_energy, "current_alignment": align,
                "is_success": align >= self.success_threshold, "target_reached": align >= self.success_threshold,
                "magnetization_magnitude": float(np.linalg.norm(self.current_magnetization)) if self.current_magnetization is not None else 0.0,
                "device_type": self.device_type, "episode_history": self.episode_history.copy()}

    # -- rendering (spin_torque_env.py:556-684): host-side matplotlib, optional (spin_torque_gym_amd/render.py) -------
    def render(self, mode: Optional[str] = None):
        """'human': the reference's four-panel figure (3-D magnetisation arrows in the unit sphere; energy, alignment and current
        histories), one persistent figure redrawn in place, returns None; 'rgb_array': the x-y projection as uint8 [H, W, 3]."""
        mode = self.render_mode if mode is None else mode
        if mode is None:
            return None
        if mode not in ("human", "rgb_array"):
            raise ValueError(f"Unsupported render mode: {mode}")
        from . import render as _render
        if self.current_magnetization is None:
            raise RuntimeError("Environment must be reset before calling render")
        if mode == "rgb_array":
            return _render.macrospin_rgb(self)
        if self.renderer is None:
            self.renderer = _render.HumanFigure("macrospin")
        self.renderer.draw(self)
        return None

    def close(self):
        if self.renderer is not None:
            self.renderer.close()
            self.renderer = None
        self._vec.close()

    # -- introspection (spin_torque_env.py:699-745) ------------------------------------------------------------
    def _drive_info(self):
        """pulse_shape / applied_field as plain data (empty without either)."""
        v = self._vec
        if not v._wave_on:
            return {}
        if v._knots_on:
            return {"pulse_knots": v.pulse_knots.tolist(), "amplitude_limit": v.amplitude_limit,
                    "applied_field": None if v._field_knots is None else {"times": v._field_knots[0].tolist(), "values": v._field_knots[1].tolist()}}
        return {"pulse_shape": None if v.pulse_shape is None else {"tau": v.pulse_shape.times.tolist(), "scale": v.pulse_shape.values.tolist()},
                "applied_field": None if v._field_knots is None else {"times": v._field_knots[0].tolist(), "values": v._field_knots[1].tolist()}}

    def get_device_info(self):
        info = self.device.get_device_info()
        info.update(self._drive_info())
        return info

    def get_solver_info(self):
        info = {"method": self.solver_name, "solve_count": self._solve_count, "timeout_count": 0,
                "last_solve_time": self._solve_time[0], "timeout_rate": 0.0,
                "avg_solve_time": self._solve_time[1] / max(self._solve_count, 1), "backend": "hip/gfx950"}
        info.update(self._drive_info())
        return info

    def get_health_report(self):
        from .harness import health_report
        return health_report(self)

    def get_performance_stats(self):
        """spin_torque_env.py:711-718: {'profiler', 'optimizer', 'solver', 'health'}.  The profiler table carries this
        facade's synchronous step()/reset() wall times (`env_step_*`, `env_reset_*`), the vector env's launch times and
        the device counters."""
        st = self._vec.get_performance_stats()
        prof = dict(st["profiler"])
        prof.update(self.profiler.get_stats())
        return {"profiler": prof, "optimizer": st["optimizer"], "solver": self.get_solver_info(), "health": st["health"]}

    def analyze_episode(self):
        if not self.episode_history:
            return {}
        h = self.episode_history
        total_energy = sum(x["energy"] for x in h)
        final_alignment = h[-1]["alignment"]
        switching_step = next((i + 1 for i, x in enumerate(h) if x["alignment"] >= self.success_threshold), None)
        return {"episode_length": len(h), "total_energy": total_energy, "final_alignment": final_alignment,
                "success": final_alignment >= self.success_threshold, "switching_step": switching_step,
                "average_reward": float(np.mean([x["reward"] for x in h])),
                "energy_efficiency": final_alignment / total_energy if total_energy > 0 else 0, "history": h.copy()}


def _parse_action_host(a: np.ndarray, max_current: float, max_duration: float):
    """Host restatement of the action clamp for the `info` dict only (monitoring.py:304-313,
    spin_torque_env.py:417-431); the values that drive the physics are computed in the kernel."""
    a = a.copy()
    if not np.isnan(a[0]):
        a[0] = np.clip(a[0], -1e8, 1e8)
    if not np.isnan(a[1]):
        a[1] = np.clip(a[1], 1e-12, 1e-6)
    if np.any(np.isnan(a)) or np.any(np.isinf(a)):
        a = np.array([0.0, 1e-12], dtype=a.dtype)
    J = float(np.clip(float(a[0]), -max_current, max_current))
    T = float(np.clip(float(a[1]), 1e-12, max_duration))
    return J, T


# What the reference has registered once `spin_torque_gym` and `spin_torque_gym.envs` are imported: both modules register the
# same ids, the second registration (envs/__init__.py:14-26) replaces the first (__init__.py:14-24).
REGISTRATIONS = {
    "SpinTorque-v0": dict(entry_point="spin_torque_gym_amd.envs:SpinTorqueEnv", max_episode_steps=100,
                          kwargs={"device_type": "stt_mram"}),
    "SpinTorqueArray-v0": dict(entry_point="spin_torque_gym_amd.array_env:SpinTorqueArrayEnv", max_episode_steps=200,
                               kwargs={"array_size": (4, 4), "device_type": "stt_mram"}),
}


def register_envs():
    """Registers 'SpinTorque-v0' and 'SpinTorqueArray-v0' with Gymnasium when it is installed, with the reference's final
    `max_episode_steps` and kwargs (reference: spin_torque_gym/__init__.py:14-24, envs/__init__.py:14-26), so that
    ``gym.make('SpinTorque-v0', **kwargs)`` builds the GPU-backed classes.  Called on ``import spin_torque_gym_amd``.
    ('SkyrmionRacetrack-v0' is a different physics and out of scope)"""
    if _gym is None:
        return False
    from gymnasium.envs.registration import register, registry
    for env_id, spec in REGISTRATIONS.items():
        if env_id not in registry:
            register(id=env_id, entry_point=spec["entry_point"], max_episode_steps=spec["max_episode_steps"],
                     kwargs=dict(spec["kwargs"]))
    return True

"""Solver level: the `spin_torque_gym.physics` classes that sit on the step path, backed by the HIP kernels.

  LLGSSolver ............ physics/llgs_solver.py:21-305   (SciPy RK45 semantics: rtol, atol, max_step)
  SimpleLLGSSolver ...... physics/simple_solver.py:21-399 (fixed-step 'rk4' / 'euler')
  RobustLLGSSolver ...... utils/robust_solver.py:22-345   (input/output gates, fallback result)
  ThermalFluctuations ... physics/thermal_model.py:12-137 (Brown field strength, white / OU field generator)

`solve()` keeps the reference signature and result dict ('t', 'm', 'success', and for LLGSSolver 'energy').  A Python
callable cannot run in a kernel, so `current_func` and `field_func` come in two forms the GPU integrates:

  * `PiecewiseLinear(times, values)` (below): a table of 2 ... 32 knots, for the current (scalar values) and / or the
    applied field (three components, A/m) -- rise and fall times, bipolar or pre-charge pulses, field-assisted
    switching, a bias field during relaxation.  The kernels evaluate the table per RHS call at that call's own time,
    with exactly the arithmetic of `PiecewiseLinear.__call__`, so the same object can be handed to the reference's
    solvers.
  * the rectangular pulse -- current_func(t) = J while t <= T, else 0, zero applied field -- the only form
    SpinTorqueEnv ever passes (spin_torque_env.py:442-447); `solve()` recognises it by probing the callable.

Any mixture works (table current with no field, rectangular callable with a table field, two tables with different
knots); any other callable raises NotImplementedError.  The batched entry `solve_batch()` takes arrays of (m0, J, T),
optionally `current_knots` / `field_knots`, and is what a vectorised caller should use.

SimpleLLGSSolver here always applies RobustLLGSSolver's gates, because that is the only way the reference env runs it;
the two classes differ only in their constructor signature.  The result cache of the reference (keyed
without J, stale hits) is deliberately not reproduced.
"""
import functools
import warnings
from typing import Any, Callable, Dict, Optional, Tuple

import numpy as np
import torch

from .backend import EnvConfig, HipBackend
from .devices import DeviceFactory, flatten_params

MU0 = 4 * np.pi * 1e-7


class _RawParams:
    """A bare device_params dict as the reference's solvers take it: they never build a device object, they read the dict
    with `.get(key, default)` (simple_solver.py:126-131; llgs_solver.py:79-82,192-205), so a partial dict is legal there."""
    device_type = "stt_mram"

    def __init__(self, device_params: Dict[str, Any]):
        self.device_params = device_params


def _flat_for(device_params: Dict[str, Any], device_type: str = "stt_mram", validate: bool = True):
    """The C-ABI parameter record of one solve.  validate: keep the outcome of the reference's `validate_parameters(params,
    'stt_mram')` gate (RobustLLGSSolver: an invalid dict ends in the fallback result, robust_solver.py:108-110,140-150); the plain solvers
    have no such gate."""
    if device_type == "stt_mram":
        p = flatten_params(_RawParams(device_params))
    else:
        p = flatten_params(DeviceFactory().create_device(device_type, device_params))
    if not validate:
        p.params_valid = 1
    return p


MAX_KNOTS = 32          # STG_MAX_KNOTS of include/spintorque_hip.h


class PiecewiseLinear:
    """A piecewise-linear waveform: K knots (2 <= K <= 32) at strictly increasing, finite `times`; `values` [K] (a current,
    A/m^2) or [K,3] (an applied field, A/m).  Calling it evaluates at time t, in plain Python floats:

        t <= times[0]   -> values[0]
        t >= times[-1]  -> values[-1]
        otherwise       -> k = the largest index with times[k] <= t,
                           values[k] + (t - times[k]) * ((values[k+1] - values[k]) / (times[k+1] - times[k]))

    -- the quotient is rounded first, then the product, then the sum, each field component by itself.  The kernels of
    stg_solve_wave use exactly this arithmetic, so the object gives the reference's solvers (as `current_func` /
    `field_func`) the same drive the GPU integrates.  A scalar table returns a float, a field table a new ndarray [3]."""

    def __init__(self, times, values):
        t = np.asarray(times, dtype=np.float64)
        v = np.asarray(values, dtype=np.float64)
        if t.ndim != 1 or not 2 <= t.shape[0] <= MAX_KNOTS:
            raise ValueError(f"a waveform has 2 ... {MAX_KNOTS} knots, got times of shape {t.shape}")
        if v.shape not in ((t.shape[0],), (t.shape[0], 3)):
            raise ValueError(f"values must have shape [K] or [K,3] with K = {t.shape[0]}, got {v.shape}")
        if not (np.isfinite(t).all() and np.isfinite(v).all()):
            raise ValueError("knot times and values must be finite")
        if not (np.diff(t) > 0).all():
            raise ValueError("knot times must be strictly increasing")
        self.times, self.values = t, v
        self.vector = v.ndim == 2
        self._t = [float(x) for x in t]
        self._v = [[float(x) for x in row] for row in (v if self.vector else v[:, None])]

    def __call__(self, t):
        t = float(t)
        tk, vk = self._t, self._v
        if t <= tk[0]:
            out = list(vk[0])
        elif t >= tk[-1]:
            out = list(vk[-1])
        else:
            k = 0
            while tk[k + 1] <= t:
                k += 1
            out = [a + (t - tk[k]) * ((b - a) / (tk[k + 1] - tk[k])) for a, b in zip(vk[k], vk[k + 1])]
        return np.array(out) if self.vector else out[0]

    def knots(self):
        """(times [K], values [K] or [K,3]) as `solve_batch` takes them."""
        return self.times, self.values


def _knot_tables(knots, n: int, width: int, what: str):
    """`(times, values)` of `solve_batch` -> (times [K,n], values [K,n] (width 1) or [K,3,n]) as the C-ABI lays them out.
    times [K] / values [K] or [K,3] are broadcast to all n problems; [K,n] / [K,n] or [K,n,3] are per problem.  Shapes and
    the knot count are checked here; the table CONTENTS (finite, strictly increasing) are checked per problem on the device."""
    if knots is None:
        return None
    try:
        times, values = knots
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a pair (times, values)") from None
    t = np.asarray(times, dtype=np.float64)
    v = np.asarray(values, dtype=np.float64)
    if t.ndim not in (1, 2) or (t.ndim == 2 and t.shape[1] != n):
        raise ValueError(f"{what}: times must have shape [K] or [K,{n}], got {t.shape}")
    k = t.shape[0]
    if not 2 <= k <= MAX_KNOTS:
        raise ValueError(f"{what}: a waveform has 2 ... {MAX_KNOTS} knots, got {k}")
    tail = () if width == 1 else (3,)
    if v.shape == (k,) + tail:
        v = np.broadcast_to(v[:, None] if width == 1 else v[:, None, :], (k, n) + tail)
    elif v.shape != (k, n) + tail:
        raise ValueError(f"{what}: values must have shape {(k,) + tail} or {(k, n) + tail}, got {v.shape}")
    if t.ndim == 1:
        t = np.broadcast_to(t[:, None], (k, n))
    if width == 3:
        v = np.transpose(v, (0, 2, 1))
    return np.array(t, order="C"), np.array(v, order="C")          # (copies: the broadcast views are read-only)


def _pulse_from_callable(current_func: Optional[Callable], t0: float, t1: float) -> float:
    """Recovers J from a rectangular-pulse current function; refuses anything else."""
    if current_func is None:
        return 0.0
    j0 = float(current_func(t0))
    span = t1 - t0
    probes = [t0 + f * span for f in (0.0, 0.25, 0.5, 0.75, 1.0)]
    if any(float(current_func(t)) != j0 for t in probes):
        raise NotImplementedError("the GPU solver integrates rectangular pulses (constant J over the time span) and "
                                  "physics.PiecewiseLinear waveforms; describe the current as a PiecewiseLinear table, or "
                                  "use the reference CPU solver for arbitrary current_func callables")
    return j0


def _check_zero_field(field_func: Optional[Callable], t0: float, t1: float) -> None:
    if field_func is None:
        return
    for t in (t0, 0.5 * (t0 + t1), t1):
        if np.any(np.asarray(field_func(t), dtype=float) != 0.0):
            raise NotImplementedError("an applied field must be given as a physics.PiecewiseLinear table with [K,3] values "
                                      "(a constant field is two knots); arbitrary field_func callables need the reference "
                                      "CPU solver")


# the device parameters that vary from device to device in a population (stg_switch_population), in the order of the library's sigma rows
VARIATION_KEYS = ("damping", "saturation_magnetization", "uniaxial_anisotropy", "volume", "polarization")


def _variation_sigma(variation, g: int, clip: float) -> np.ndarray:
    """variation {key: relative sigma, scalar or [G]} -> sigma float64 [5, G]; missing keys are 0.  Raises on unknown keys, on a sigma
    that is negative or not finite, on a clip that is not finite and positive, and on sigma * clip >= 1 (a parameter could come out
    non-positive)."""
    if not isinstance(variation, dict):
        raise TypeError("variation must be a dict {parameter name: relative sigma} or None")
    unknown = sorted(set(variation) - set(VARIATION_KEYS))
    if unknown:
        raise ValueError(f"variation: unknown keys {unknown}; the parameters that vary are {list(VARIATION_KEYS)}")
    clip = float(clip)
    if not (np.isfinite(clip) and clip > 0):
        raise ValueError("variation_clip must be finite and > 0")
    sigma = np.zeros((len(VARIATION_KEYS), g), dtype=np.float64)
    for k, name in enumerate(VARIATION_KEYS):
        if name in variation:
            s = np.asarray(variation[name], dtype=np.float64)
            if s.ndim > 1 or (s.ndim == 1 and s.shape[0] != g):
                raise ValueError(f"variation[{name!r}] must be a scalar or have shape [G] with G = {g}, got {s.shape}")
            sigma[k] = s
    if not np.isfinite(sigma).all() or (sigma < 0).any():
        raise ValueError("variation: every sigma must be finite and >= 0")
    if (sigma * clip >= 1.0).any():
        raise ValueError("variation: sigma * variation_clip must stay below 1 (a clipped draw could make a parameter non-positive)")
    return sigma


class _GpuSolverBase:
    _solver_name = "rk4"
    _validate_params = False        # (RobustLLGSSolver turns the parameter gate on)

    def __init__(self, rtol, atol, max_step, gamma=2.21e5, device_index=0, backend=None, seed=0, noise_model="white",
                 correlation_time=1e-12):
        self.rtol, self.atol, self.max_step, self.gamma = rtol, atol, max_step, gamma
        # thermal field of the fixed-step solvers (EnvConfig.noise_model): 'white', 'ou' (with correlation_time) or 'brown'
        self.noise_model, self.correlation_time = noise_model, correlation_time
        self.mu_0 = MU0
        self.device_index = device_index
        self._backend_factory = HipBackend if backend is None else backend
        self._seed = seed
        self.solve_count = 0

    def _backend(self, n, device_params, device_type, thermal_noise, temperature):
        cfg = EnvConfig(solver=self._solver_name, include_thermal_fluctuations=bool(thermal_noise),
                        temperature=float(temperature), gamma=self.gamma, max_step=self.max_step, rtol=self.rtol,
                        atol=self.atol, seed=self._seed, noise_model=self.noise_model, correlation_time=self.correlation_time)
        b = self._backend_factory(n, cfg, self.device_index, 0)
        b.set_params([_flat_for(device_params, device_type, self._validate_params)])
        return b

    def solve_batch(self, m_initial, current, duration, device_params: Dict[str, Any], thermal_noise: bool = False,
                    temperature: float = 300.0, device_type: str = "stt_mram", return_trajectory: int = 0,
                    env_step: int = 0, current_knots=None, field_knots=None) -> Dict[str, Any]:
        """N independent solves over (0, duration).  m_initial [N,3]; current, duration [N].
        Without knots: rectangular pulses `current` while t <= duration, zero applied field.
        current_knots = (tk, jk): piecewise-linear current_func(t) (`current` is then unused and may be None); field_knots =
        (tk, hk): piecewise-linear field_func(t) in A/m.  tk [K] with jk [K] / hk [K,3] is one table for all problems, tk [K,N]
        with jk [K,N] / hk [K,N,3] one per problem; 2 <= K <= 32, semantics as PiecewiseLinear.  A problem whose table is not
        finite or not strictly increasing fails (success False, m_final = m0).
        return_trajectory = K > 0 additionally returns the first K accepted points ('t' [K,N], 'm' [K,N,3])."""
        m0 = torch.as_tensor(np.asarray(m_initial, dtype=np.float64) if not torch.is_tensor(m_initial) else m_initial)
        n = m0.shape[0]
        wave = None
        if current_knots is not None or field_knots is not None:
            wave = {"current": _knot_tables(current_knots, n, 1, "current_knots"),
                    "field": _knot_tables(field_knots, n, 3, "field_knots")}
            wave = {k: None if v is None else tuple(torch.from_numpy(a) for a in v) for k, v in wave.items()}
        if current is None:
            if current_knots is None:
                raise ValueError("current is required without current_knots")
            current = np.zeros(n)
        b = self._backend(n, device_params, device_type, thermal_noise, temperature)
        try:
            out = b.solve(m0.t().contiguous(), torch.as_tensor(current, dtype=torch.float64),
                          torch.as_tensor(duration, dtype=torch.float64), env_step=env_step,
                          traj_cap=int(return_trajectory), want_energy=self._solver_name == "rk45",
                          **({} if wave is None else {"wave": wave}))      # (a backend without waveforms is never asked for them)
            res = {"m_final": out["m_final"].t().cpu().numpy(), "success": out["success"].cpu().numpy().astype(bool),
                   "n_points": out["n_points"].cpu().numpy()}
            if return_trajectory:
                res["t"] = out["t"].cpu().numpy()
                res["m"] = out["m"].permute(0, 2, 1).cpu().numpy()
                if out.get("energy") is not None:
                    res["energy"] = out["energy"].cpu().numpy()
                if out.get("torques") is not None:
                    res["torques"] = out["torques"].cpu().numpy()
        finally:
            b.close()
        self.solve_count += n
        return res

    def switching_statistics(self, m_initial, current, duration, device_params, n_trials: int, *, equilibrate=0.0, relax=0.0,
                             target=(0.0, 0.0, -1.0), threshold: float = 0.0, n_bins: int = 0, temperature: float = 300.0,
                             device_type="stt_mram", class_index=None, env_step: int = 0, trial_offset: int = 0, trial_stride=None,
                             max_trials_per_launch: int = 2 ** 22, current_knots=None, field_knots=None, time_bins: int = 0,
                             watch_phase: int = 0, variation=None, variation_clip: float = 4.0, variation_step: int = 2 ** 31,
                             trials_per_device: int = 1, per_device: bool = False) -> Dict[str, Any]:
        """Monte-Carlo switching statistics of G conditions with R = n_trials thermal trials each, with the trial loop and the
        reduction on the GPU (stg_switch_stats): no per-trial array exists, so R is bounded by time, not by memory.

        m_initial [G,3]; current, duration [G] (one pulse) or [P,G] (P phases run back to back, each from the previous one's final
        m, phase p on Philox counter word env_step + p; a phase of duration exactly 0 is skipped).  equilibrate > 0 (scalar or [G])
        prepends a phase at J = 0, relax > 0 appends one; at most 4 phases in all.  device_params: one dict, or a list of up to 64
        dicts with class_index [G] (device_type then a string or a list) for sweeps over device size.  A trial counts as switched
        when proj = m_final . target > threshold (target [3] or [G,3]); a trial one of whose solves fails ends there with that
        solve's m, is classified like any other and counted in n_failed.  n_bins > 0 also returns the histogram of proj over n_bins
        equal bins of [-1, 1] (outer bins open-ended).

        Trial r of condition g has the stream of problem g * trial_stride + trial_offset + r of solve_batch (trial_stride None:
        trial_offset + n_trials), so disjoint trial ranges -- later calls, other ranks -- are independent and their counts add up.
        The trials run in launches of at most max_trials_per_launch per condition, which keeps each kernel short on a shared
        device; the counts do not depend on it.  The thermal field is on (choose its model with the constructor's noise_model).

        current_knots = (tk, jk) and / or field_knots = (tk, hk) shape the pulse (stg_switch_stats_wave): piecewise-linear
        current_func(t) and field_func(t) as in switching_probability and solve_batch -- tk [K] with jk [K] / hk [K,3] is one table
        for all conditions, tk [K,G] with jk [K,G] / hk [K,G,3] one per condition; 2 <= K <= 32; t = 0 at the start of the pulse.
        current and duration then describe that single pulse ([G] or [1,G]; current may be None with current_knots, which replaces
        it); equilibrate and relax still add their rectangular J = 0 phases around it.  A condition whose table is not finite or not
        strictly increasing fails its pulse in every trial.  The tables are held once per condition, not per trial.

        Returns dict(p_switch [G] = n_switched / R, wer [G] = 1 - p_switch, n_switched [G], n_failed [G],
        stderr [G] = sqrt(p (1 - p) / R), hist [G,n_bins], bin_edges [n_bins + 1] (empty without bins)).

        time_bins > 0 (at most 1024) also answers WHEN the trials switched (stg_switch_times): during the pulse -- with current /
        duration given as [P,G], phase watch_phase of them -- a trial crosses at the first integrator point with m . target >
        threshold; its crossing time is the midpoint of that point and the one before it, binned into time_bins equal bins over the
        pulse's [0, duration].  The result gains n_crossed [G], n_returned [G] (crossed, yet not switched at the trial's end:
        back-hops, pulses cut short by a later phase), p_cross [G] = n_crossed / R, t_hist [G,time_bins], t_edges [G,time_bins + 1]
        (per condition: the durations differ), p_cross_by [G,time_bins] = cumsum(t_hist) / R -- the first-passage curve, i.e.
        p_cross for every pulse width up to the duration from one run -- and t_mean, t_std [G] over the crossed trials, formed
        from the bin centres (NaN where nobody crossed).  The moments are exact to one bin width; time_bins = n, the pulse's
        sub-step count, resolves every sub-step of a fixed-step solver.  With time_bins == 0 the call is exactly the one above: watch_phase is
        still checked against the number of phases, but has no meaning then.

        variation = {"damping": s, "saturation_magnetization": s, "uniaxial_anisotropy": s, "volume": s, "polarization": s} (each s a
        relative sigma, scalar or [G]; missing keys are 0) turns the R trials of a condition into trials of a POPULATION of devices
        around device_params (stg_switch_population): the statistics of a chip whose bits scatter, not of one device.  Trial r
        (counted from 0, trial_offset included) belongs to device r // trials_per_device; that device's five parameters are the
        nominal ones times 1 + s * clip(z, +- variation_clip), z standard normal from the stream of the device's first trial at
        counter word variation_step (which must differ from env_step + p of every phase), and the trial integrates with that device's
        own constants, thermal strength included.  A device depends on the seed, on its own index and on trial_stride alone, so
        launches, chunks and ranks see the same chip.  The result gains n_devices [G], the devices the trial range touches;
        per_device = True also returns dev_switched [G, n_dev], dev_trials [G, n_dev] (the first and the last device may be partial)
        and dev_p_switch = their ratio, for devices trial_offset // trials_per_device onwards (the count array held on the GPU is
        indexed from device 0).  `draw_devices` returns the devices themselves.  variation = None is exactly the call above."""
        m0 = np.asarray(m_initial.cpu() if torch.is_tensor(m_initial) else m_initial, dtype=np.float64).reshape(-1, 3)
        g, r = int(m0.shape[0]), int(n_trials)
        if r < 1:
            raise ValueError("n_trials must be >= 1")
        if int(max_trials_per_launch) < 1:
            raise ValueError("max_trials_per_launch must be >= 1")
        if not 0 <= int(n_bins) <= 64:
            raise ValueError("n_bins must be in 0 ... 64")
        if not 0 <= int(time_bins) <= 1024:
            raise ValueError("time_bins must be in 0 ... 1024")
        wave = None
        if current_knots is not None or field_knots is not None:
            wave = {"current": _knot_tables(current_knots, g, 1, "current_knots"), "field": _knot_tables(field_knots, g, 3, "field_knots")}
            wave = {k: None if v is None else tuple(torch.from_numpy(a) for a in v) for k, v in wave.items()}
        if current is None:
            if current_knots is None:
                raise ValueError("current is required without current_knots")
            current = np.zeros(np.shape(duration))
        J, T = (np.asarray(x, dtype=np.float64) for x in (current, duration))
        J, T = (np.broadcast_to(x, (g,))[None, :] if x.ndim <= 1 else x for x in (J, T))
        if wave is not None and (J.shape[0] != 1 or T.shape[0] != 1):
            raise ValueError("with current_knots / field_knots, current and duration describe the one shaped pulse: shape [G] or [1,G]")
        if J.shape != T.shape or J.ndim != 2 or J.shape[1] != g:
            raise ValueError(f"current and duration must both have shape [G] or [P,G] with G = {g}, got {J.shape} and {T.shape}")
        if not 0 <= int(watch_phase) < J.shape[0]:
            raise ValueError(f"watch_phase must be in 0 ... {J.shape[0] - 1}")
        phases = [(J, T)]
        wave_phase = 0                      # (the pulse's place in the chain: behind the equilibration, if there is one)
        for where, t in ((0, equilibrate), (1, relax)):
            t = np.broadcast_to(np.asarray(t, dtype=np.float64), (g,))
            if (t < 0).any():
                raise ValueError("equilibrate and relax must be >= 0")
            if (t > 0).any():
                ph = (np.zeros((1, g)), t[None, :])
                phases = [ph] + phases if where == 0 else phases + [ph]
                wave_phase += where == 0
        J, T = (np.ascontiguousarray(np.concatenate([ph[k] for ph in phases], axis=0)) for k in (0, 1))
        if J.shape[0] > 4:
            raise ValueError(f"a trial has at most 4 phases (equilibrate and relax included), got {J.shape[0]}")
        tgt = np.ascontiguousarray(np.broadcast_to(np.asarray(target, dtype=np.float64), (g, 3)).T)
        tables = device_params if isinstance(device_params, (list, tuple)) else [device_params]
        types = device_type if isinstance(device_type, (list, tuple)) else [device_type] * len(tables)
        if not 1 <= len(tables) <= 64 or len(types) != len(tables):
            raise ValueError("device_params is one dict or a list of 1 ... 64 dicts (with as many device types, or one)")
        cls = None
        if len(tables) > 1:
            if class_index is None:
                raise ValueError("class_index [G] is required with more than one device_params dict")
            cls = np.asarray(class_index).reshape(g)
            if cls.min() < 0 or cls.max() >= len(tables):
                raise ValueError("class_index out of range")
            cls = torch.from_numpy(cls.astype(np.uint8))
        stride = int(trial_offset) + r if trial_stride is None else int(trial_stride)
        if int(trial_offset) < 0 or stride < int(trial_offset) + r:
            raise ValueError("trial_offset must be >= 0 and trial_stride >= trial_offset + n_trials")
        sigma, q, dev_first, n_dev = None, int(trials_per_device), 0, 0
        if variation is not None:
            sigma = _variation_sigma(variation, g, variation_clip)
            if q < 1:
                raise ValueError("trials_per_device must be >= 1")
            if not 0 <= int(variation_step) < 2 ** 32 or (int(variation_step) - int(env_step)) % 2 ** 32 < J.shape[0]:
                raise ValueError("variation_step must be a 32-bit counter word other than env_step + p of the trial's phases")
            dev_first = int(trial_offset) // q
            n_dev = (int(trial_offset) + r - 1) // q - dev_first + 1
        cfg = EnvConfig(solver=self._solver_name, include_thermal_fluctuations=True, temperature=float(temperature), gamma=self.gamma,
                        max_step=self.max_step, rtol=self.rtol, atol=self.atol, seed=self._seed, noise_model=self.noise_model,
                        correlation_time=self.correlation_time)
        b = self._backend_factory(g, cfg, self.device_index, 0)
        dev_sw = None
        try:
            b.set_params([_flat_for(p, t, self._validate_params) for p, t in zip(tables, types)], cls)
            out, step = None, int(max_trials_per_launch)
            # (without knots: exactly the rectangular call; a backend without waveforms is never asked for them)
            if sigma is None:
                launch = b.switch_stats if wave is None else functools.partial(b.switch_stats_wave, wave=wave, wave_phase=int(wave_phase))
                if time_bins > 0:
                    launch = functools.partial(b.switch_times, watch_phase=int(wave_phase) + int(watch_phase), wave=wave, n_tbins=int(time_bins))
            else:
                # the chunks below keep absolute trial indices, so every launch sees the same devices and adds into the same counts
                if per_device:
                    dev_sw = torch.zeros((g, dev_first + n_dev), dtype=torch.int64, device=b.device)
                launch = functools.partial(b.switch_population, sigma=torch.from_numpy(sigma), watch_phase=int(wave_phase) + int(watch_phase),
                                           wave=wave, n_tbins=int(time_bins), passage=time_bins > 0, z_clip=float(variation_clip),
                                           var_step=int(variation_step), trials_per_device=q, dev_switched=dev_sw)
            for done in range(0, r, step):
                out = launch(torch.from_numpy(np.ascontiguousarray(m0.T)), torch.from_numpy(J), torch.from_numpy(T),
                             torch.from_numpy(tgt), min(step, r - done), trial0=int(trial_offset) + done, trial_stride=stride,
                             cond_cls=cls, env_step=env_step, threshold=float(threshold), n_bins=int(n_bins), out=out)
            n_sw, n_failed = (x.cpu().numpy().astype(np.int64) for x in out[:2])
            hist = out[2].cpu().numpy().astype(np.int64) if n_bins > 0 else np.zeros((g, 0), dtype=np.int64)
            if dev_sw is not None:
                dev_sw = dev_sw[:, dev_first:].cpu().numpy().astype(np.int64)
        finally:
            b.close()
        self.solve_count += g * r
        p = n_sw / r
        res = {"p_switch": p, "wer": 1.0 - p, "n_switched": n_sw, "n_failed": n_failed, "stderr": np.sqrt(p * (1.0 - p) / r),
               "hist": hist, "bin_edges": np.linspace(-1.0, 1.0, int(n_bins) + 1) if n_bins > 0 else np.zeros(0)}
        if time_bins > 0:
            n_cr, n_ret, t_hist = (x.cpu().numpy().astype(np.int64) for x in out[3:6])
            t_edges = np.linspace(0.0, 1.0, int(time_bins) + 1)[None, :] * T[int(wave_phase) + int(watch_phase)][:, None]
            centres = 0.5 * (t_edges[:, :-1] + t_edges[:, 1:])
            binned = t_hist.sum(axis=1).astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                t_mean = (t_hist * centres).sum(axis=1) / binned
                t_var = (t_hist * (centres - t_mean[:, None]) ** 2).sum(axis=1) / binned
            res.update({"n_crossed": n_cr, "n_returned": n_ret, "p_cross": n_cr / r, "t_hist": t_hist, "t_edges": t_edges,
                        "p_cross_by": np.cumsum(t_hist, axis=1) / r, "t_mean": t_mean, "t_std": np.sqrt(t_var)})
        if sigma is not None:
            res["n_devices"] = np.full(g, n_dev, dtype=np.int64)
            if per_device:
                # trials of each touched device inside [trial_offset, trial_offset + R): the first and the last may be partial
                lo = np.maximum((dev_first + np.arange(n_dev, dtype=np.int64)) * q, int(trial_offset))
                hi = np.minimum((dev_first + np.arange(n_dev, dtype=np.int64) + 1) * q, int(trial_offset) + r)
                dev_trials = np.broadcast_to(hi - lo, (g, n_dev)).copy()
                res.update({"dev_switched": dev_sw, "dev_trials": dev_trials, "dev_p_switch": dev_sw / dev_trials})
        return res

    def write_verify_statistics(self, m_initial, current, duration, device_params, n_trials: int, *, relax=0.0,
                                target=(0.0, 0.0, -1.0), threshold: float = 0.0, n_bins: int = 0, temperature: float = 300.0,
                                device_type="stt_mram", class_index=None, env_step: int = 0, trial_offset: int = 0, trial_stride=None,
                                max_trials_per_launch: int = 2 ** 22, variation=None, variation_clip: float = 4.0,
                                variation_step: int = 2 ** 31, trials_per_device: int = 1, per_device: bool = False) -> Dict[str, Any]:
        """Write - verify - write statistics of G conditions with R = n_trials thermal trials each, reduced on the GPU
        (stg_switch_verify): how an MRAM macro writes.  A trial is up to A attempts; after every attempt the bit is read -- the
        trial is classified as in switching_statistics, proj = m . target > threshold -- and only a trial that has not switched runs
        the next attempt, from the m the attempt before left behind.  A trial ends at attempt a when it is switched after it, when one
        of its solves failed (counted in n_failed, classified like any other) or when a = A - 1.  No per-trial array exists.

        m_initial [G,3]; current and duration are [A] (the same for all conditions), [A,G], or [A,P,G] (P phases per attempt, run
        back to back); at most 8 attempts.  relax > 0 (scalar or [G]) appends a J = 0 phase to every attempt; at most 4 phases per
        attempt in all; a phase of duration exactly 0 is skipped.  Phase p of attempt a runs on Philox counter word
        env_step + a * P + p.  device_params, device_type, class_index, target, threshold, n_bins, temperature, trial_offset,
        trial_stride and max_trials_per_launch are those of switching_statistics: trial r of condition g has the stream of problem
        g * trial_stride + trial_offset + r, disjoint trial ranges add up, and the counts do not depend on the chunking.

        Returns dict(n_switched_at [A,G], n_ended_at [A,G] (trials whose last attempt was a, and those of them that switched),
        n_failed [G], n_attempted [A,G] = R - sum_{b<a} n_ended_at[b], wer_after [A,G] = 1 - cumsum(n_switched_at) / R with
        stderr [A,G] = sqrt(wer (1 - wer) / R), p_switch [G] = 1 - wer_after[-1], mean_attempts [G] =
        sum_a (a + 1) n_ended_at[a] / R, hist [G,n_bins] of the final proj, bin_edges [n_bins + 1] (empty without bins)).

        variation, variation_clip, variation_step, trials_per_device and per_device are those of switching_statistics: with
        variation = {...} the R trials of a condition are trials of a POPULATION of devices around device_params
        (stg_switch_verify_population) -- trial r (trial_offset included) belongs to device r // trials_per_device, drawn exactly as
        there, so `draw_devices` returns these devices -- and every attempt of a trial runs on its own device: a weak bit stays weak
        over its retries, and the residual wer_after is set by the tail of the device distribution.  variation_step must differ from
        env_step + k of all A * P counter words of a trial.  The returned dict is the one above; per_device = True adds, for devices
        trial_offset // trials_per_device onwards, dev_switched_at [A,G,n_dev] (trials of the device that ended switched at attempt
        a), dev_trials [G,n_dev] (the first and the last device may be partial) and dev_wer_after [A,G,n_dev] =
        1 - cumsum(dev_switched_at) / dev_trials.  variation = None is exactly the call above."""
        m0 = np.asarray(m_initial.cpu() if torch.is_tensor(m_initial) else m_initial, dtype=np.float64).reshape(-1, 3)
        g, r = int(m0.shape[0]), int(n_trials)
        if r < 1:
            raise ValueError("n_trials must be >= 1")
        if int(max_trials_per_launch) < 1:
            raise ValueError("max_trials_per_launch must be >= 1")
        if not 0 <= int(n_bins) <= 64:
            raise ValueError("n_bins must be in 0 ... 64")
        J, T = (np.asarray(x, dtype=np.float64) for x in (current, duration))
        if not (1 <= J.ndim <= 3 and 1 <= T.ndim <= 3):
            raise ValueError("current and duration must have shape [A], [A,G] or [A,P,G]")
        # [A] -> [A,1,1], [A,G] -> [A,1,G]; then both to the common [A,P,G]
        J, T = (x[:, None, None] if x.ndim == 1 else x[:, None, :] if x.ndim == 2 else x for x in (J, T))
        if J.shape[0] != T.shape[0] or any(x.shape[2] not in (1, g) for x in (J, T)) or (J.shape[1] != T.shape[1] and 1 not in (J.shape[1], T.shape[1])):
            raise ValueError(f"current and duration must have shape [A], [A,G] or [A,P,G] with the same A (and P) and G = {g}, "
                             f"got {np.shape(current)} and {np.shape(duration)}")
        shape = (J.shape[0], max(J.shape[1], T.shape[1]), g)
        J, T = np.broadcast_to(J, shape), np.broadcast_to(T, shape)
        rl = np.broadcast_to(np.asarray(relax, dtype=np.float64), (g,))
        if (rl < 0).any():
            raise ValueError("relax must be >= 0")
        if (rl > 0).any():
            J = np.concatenate([J, np.zeros((shape[0], 1, g))], axis=1)
            T = np.concatenate([T, np.broadcast_to(rl, (shape[0], 1, g))], axis=1)
        J, T = np.array(J, order="C"), np.array(T, order="C")           # (copies: a broadcast view is read-only)
        n_att = J.shape[0]
        if not 1 <= n_att <= 8:
            raise ValueError(f"a trial has 1 ... 8 attempts, got {n_att}")
        if J.shape[1] > 4:
            raise ValueError(f"an attempt has at most 4 phases (relax included), got {J.shape[1]}")
        tgt = np.ascontiguousarray(np.broadcast_to(np.asarray(target, dtype=np.float64), (g, 3)).T)
        tables = device_params if isinstance(device_params, (list, tuple)) else [device_params]
        types = device_type if isinstance(device_type, (list, tuple)) else [device_type] * len(tables)
        if not 1 <= len(tables) <= 64 or len(types) != len(tables):
            raise ValueError("device_params is one dict or a list of 1 ... 64 dicts (with as many device types, or one)")
        cls = None
        if len(tables) > 1:
            if class_index is None:
                raise ValueError("class_index [G] is required with more than one device_params dict")
            cls = np.asarray(class_index).reshape(g)
            if cls.min() < 0 or cls.max() >= len(tables):
                raise ValueError("class_index out of range")
            cls = torch.from_numpy(cls.astype(np.uint8))
        stride = int(trial_offset) + r if trial_stride is None else int(trial_stride)
        if int(trial_offset) < 0 or stride < int(trial_offset) + r:
            raise ValueError("trial_offset must be >= 0 and trial_stride >= trial_offset + n_trials")
        sigma, q, dev_first, n_dev = None, int(trials_per_device), 0, 0
        if variation is not None:
            sigma = _variation_sigma(variation, g, variation_clip)
            if q < 1:
                raise ValueError("trials_per_device must be >= 1")
            if not 0 <= int(variation_step) < 2 ** 32 or (int(variation_step) - int(env_step)) % 2 ** 32 < n_att * J.shape[1]:
                raise ValueError("variation_step must be a 32-bit counter word other than env_step + a * P + p of the trial's phases")
            dev_first = int(trial_offset) // q
            n_dev = (int(trial_offset) + r - 1) // q - dev_first + 1
        cfg = EnvConfig(solver=self._solver_name, include_thermal_fluctuations=True, temperature=float(temperature), gamma=self.gamma,
                        max_step=self.max_step, rtol=self.rtol, atol=self.atol, seed=self._seed, noise_model=self.noise_model,
                        correlation_time=self.correlation_time)
        b = self._backend_factory(g, cfg, self.device_index, 0)
        dev_sw = None
        try:
            b.set_params([_flat_for(p, t, self._validate_params) for p, t in zip(tables, types)], cls)
            out, step = None, int(max_trials_per_launch)
            launch = b.switch_verify
            if sigma is not None:
                # the chunks below keep absolute trial indices, so every launch sees the same devices and adds into the same counts
                if per_device:
                    dev_sw = torch.zeros((n_att, g, dev_first + n_dev), dtype=torch.int64, device=b.device)
                launch = functools.partial(b.switch_verify_population, sigma=torch.from_numpy(sigma), z_clip=float(variation_clip),
                                           var_step=int(variation_step), trials_per_device=q, dev_switched_at=dev_sw)
            for done in range(0, r, step):
                out = launch(torch.from_numpy(np.ascontiguousarray(m0.T)), torch.from_numpy(J), torch.from_numpy(T),
                             torch.from_numpy(tgt), min(step, r - done), trial0=int(trial_offset) + done, trial_stride=stride,
                             cond_cls=cls, env_step=env_step, threshold=float(threshold), n_bins=int(n_bins), out=out)
            n_sw, n_end, n_failed = (x.cpu().numpy().astype(np.int64) for x in out[:3])
            hist = out[3].cpu().numpy().astype(np.int64) if n_bins > 0 else np.zeros((g, 0), dtype=np.int64)
            if dev_sw is not None:
                dev_sw = dev_sw[:, :, dev_first:].cpu().numpy().astype(np.int64)
        finally:
            b.close()
        self.solve_count += g * r
        wer = 1.0 - np.cumsum(n_sw, axis=0) / r
        res = {"n_switched_at": n_sw, "n_ended_at": n_end, "n_failed": n_failed,
               "n_attempted": r - (np.cumsum(n_end, axis=0) - n_end), "wer_after": wer, "stderr": np.sqrt(wer * (1.0 - wer) / r),
               "p_switch": 1.0 - wer[-1], "mean_attempts": ((np.arange(n_att, dtype=np.int64)[:, None] + 1) * n_end).sum(axis=0) / r,
               "hist": hist, "bin_edges": np.linspace(-1.0, 1.0, int(n_bins) + 1) if n_bins > 0 else np.zeros(0)}
        if dev_sw is not None:
            # trials of each touched device inside [trial_offset, trial_offset + R): the first and the last may be partial
            lo = np.maximum((dev_first + np.arange(n_dev, dtype=np.int64)) * q, int(trial_offset))
            hi = np.minimum((dev_first + np.arange(n_dev, dtype=np.int64) + 1) * q, int(trial_offset) + r)
            dev_trials = np.broadcast_to(hi - lo, (g, n_dev)).copy()
            res.update({"dev_switched_at": dev_sw, "dev_trials": dev_trials,
                        "dev_wer_after": 1.0 - np.cumsum(dev_sw, axis=0) / dev_trials[None]})
        return res

    def draw_devices(self, device_params, n_devices: int, variation, *, n_conditions: int = 1, variation_clip: float = 4.0,
                     variation_step: int = 2 ** 31, trials_per_device: int = 1, trial_stride=None, first_device: int = 0,
                     device_type="stt_mram", class_index=None, temperature: float = 300.0) -> Dict[str, Any]:
        """The devices `switching_statistics(variation=...)` draws for the same seed, variation, variation_clip, variation_step,
        trials_per_device and trial_stride (None: (first_device + n_devices) * trials_per_device, which is that method's default for
        a trial range ending with device first_device + n_devices - 1): devices first_device ... first_device + n_devices - 1 of each
        of n_conditions conditions, through the library's own draw (stg_switch_population_devices).  device_params, device_type and
        class_index as there.  Returns dict(device_params: per condition, a list of n_devices dicts -- the condition's nominal dict
        with the five varied entries replaced, fit to be handed back as device_params --, one float64 array [G, D] per varied key,
        and z [6, G, D], each device's six standard normals, the last of which is unused)."""
        g, d = int(n_conditions), int(n_devices)
        if g < 1 or d < 1:
            raise ValueError("n_conditions and n_devices must be >= 1")
        sigma = _variation_sigma(variation, g, variation_clip)
        tables = device_params if isinstance(device_params, (list, tuple)) else [device_params]
        types = device_type if isinstance(device_type, (list, tuple)) else [device_type] * len(tables)
        if not 1 <= len(tables) <= 64 or len(types) != len(tables):
            raise ValueError("device_params is one dict or a list of 1 ... 64 dicts (with as many device types, or one)")
        cls_np, cls = np.zeros(g, dtype=np.int64), None
        if len(tables) > 1:
            if class_index is None:
                raise ValueError("class_index [G] is required with more than one device_params dict")
            cls_np = np.asarray(class_index).reshape(g)
            if cls_np.min() < 0 or cls_np.max() >= len(tables):
                raise ValueError("class_index out of range")
            cls = torch.from_numpy(cls_np.astype(np.uint8))
        cfg = EnvConfig(solver=self._solver_name, include_thermal_fluctuations=True, temperature=float(temperature), gamma=self.gamma,
                        max_step=self.max_step, rtol=self.rtol, atol=self.atol, seed=self._seed, noise_model=self.noise_model,
                        correlation_time=self.correlation_time)
        b = self._backend_factory(g, cfg, self.device_index, 0)
        try:
            b.set_params([_flat_for(p, t, self._validate_params) for p, t in zip(tables, types)], cls)
            params, z = b.switch_population_devices(g, d, torch.from_numpy(sigma), dev0=int(first_device), trials_per_device=int(trials_per_device),
                                                    trial_stride=trial_stride, var_step=int(variation_step), z_clip=float(variation_clip),
                                                    cond_cls=cls, want_z=True)
            params, z = params.cpu().numpy(), z.cpu().numpy()
        finally:
            b.close()
        res = {name: params[k] for k, name in enumerate(VARIATION_KEYS)}
        res["z"] = z
        res["device_params"] = [[dict(tables[int(cls_np[i])], **{name: float(params[k, i, j]) for k, name in enumerate(VARIATION_KEYS)})
                                 for j in range(d)] for i in range(g)]
        return res

    def _solve_one(self, m_initial, t_span, device_params, current_func, field_func, thermal_noise, temperature,
                   traj_cap):
        t0, t1 = float(t_span[0]), float(t_span[1])
        if t0 != 0.0:
            raise NotImplementedError("time spans start at 0 on the step path (spin_torque_env.py:453)")
        J, current_knots, field_knots = 0.0, None, None
        if isinstance(current_func, PiecewiseLinear):
            if current_func.vector:
                raise ValueError("current_func must be a scalar PiecewiseLinear (values [K])")
            current_knots = current_func.knots()
        else:
            J = _pulse_from_callable(current_func, t0, t1)
        if isinstance(field_func, PiecewiseLinear):
            if not field_func.vector:
                raise ValueError("field_func must be a vector PiecewiseLinear (values [K,3])")
            field_knots = field_func.knots()
        else:
            _check_zero_field(field_func, t0, t1)
        r = self.solve_batch(np.asarray(m_initial, dtype=np.float64)[None, :], [J], [t1], device_params,
                             thermal_noise, temperature, return_trajectory=traj_cap, current_knots=current_knots,
                             field_knots=field_knots)
        k = int(r["n_points"][0]) + 1
        return r, k


class SimpleLLGSSolver(_GpuSolverBase):
    """simple_solver.py:21-399 ('euler' | 'rk4'), as RobustLLGSSolver runs it."""

    def __init__(self, method: str = "euler", rtol: float = 1e-3, atol: float = 1e-6, max_step: float = 1e-12,
                 timeout: float = 2.0, **kw):
        method = method.lower()
        if method not in ("euler", "rk4"):
            warnings.warn(f"Unknown method '{method}', using 'euler'")      # simple_solver.py:54-56
            method = "euler"
        super().__init__(rtol, atol, max_step, **kw)
        self.method = method
        self._solver_name = method
        self.timeout = timeout          # kept for API compatibility; kernels need no wall-clock guard

    def solve(self, m_initial, time_span: Tuple[float, float], device_params: Dict[str, Any],
              current_func: Optional[Callable] = None, field_func: Optional[Callable] = None,
              thermal_noise: bool = False, temperature: float = 300.0) -> Dict[str, Any]:
        cap = 5002                                                           # n <= 5000 for the env's 5 ns maximum
        r, k = self._solve_one(m_initial, time_span, device_params, current_func, field_func, thermal_noise,
                               temperature, cap)
        ok = bool(r["success"][0])
        if not ok:      # robust_solver.py:278-299 fallback result: the initial state repeated
            t1 = float(time_span[1])
            npts = max(2, int(t1 / self.max_step))
            return {"t": np.linspace(0.0, t1, npts), "m": np.tile(np.asarray(m_initial, dtype=float), (npts, 1)),
                    "success": False, "message": "Fallback result", "solve_time": 0.0, "is_fallback": True}
        k = min(k, cap)
        return {"t": r["t"][:k, 0], "m": r["m"][:k, 0, :], "success": True,
                "message": "Integration completed successfully", "solve_time": 0.0, "n_steps": k - 1}

    def switching_probability(self, m_initial, current, duration, device_params: Dict[str, Any], n_trials: int,
                              target=(0.0, 0.0, -1.0), threshold: float = 0.0, temperature: float = 300.0,
                              device_type: str = "stt_mram", env_step: int = 0, current_knots=None, field_knots=None) -> Dict[str, Any]:
        """Monte-Carlo switching probability of G conditions -- the rows of m_initial [G,3], current [G], duration [G] -- with
        R = n_trials thermal trials each, as ONE solve launch over the G R replicated problems: problem g R + r is trial r of
        condition g and has its own normal stream through its problem index.  A trial counts as switched when
        m_final . target > threshold (a failed solve hands back m_initial and is counted by that rule like any other; n_failed says
        how many there were).  The counts are reduced on the device; no per-trial array reaches the host.  Knots as in solve_batch,
        one table for all conditions ([K]) or one per condition ([K,G]).  Returns dict(p_switch [G] = n_switched / R, n_switched [G],
        n_failed [G], stderr [G] = sqrt(p (1 - p) / R)).  The thermal field is on; choose its model with the constructor's
        noise_model ('brown' is the one whose field can switch a device, see include/spintorque_hip.h)."""
        m0 = torch.as_tensor(np.asarray(m_initial, dtype=np.float64) if not torch.is_tensor(m_initial) else m_initial).reshape(-1, 3)
        g, r = int(m0.shape[0]), int(n_trials)
        if r < 1:
            raise ValueError("n_trials must be >= 1")
        wave = None
        if current_knots is not None or field_knots is not None:
            wave = {"current": _knot_tables(current_knots, g, 1, "current_knots"), "field": _knot_tables(field_knots, g, 3, "field_knots")}
            wave = {k: None if v is None else tuple(torch.from_numpy(a).repeat_interleave(r, dim=-1) for a in v) for k, v in wave.items()}
        if current is None:
            if current_knots is None:
                raise ValueError("current is required without current_knots")
            current = np.zeros(g)
        rep = lambda x: torch.as_tensor(x, dtype=torch.float64).reshape(g).repeat_interleave(r)          # noqa: E731
        b = self._backend(g * r, device_params, device_type, True, temperature)
        try:
            out = b.solve(m0.to(torch.float64).repeat_interleave(r, dim=0).t().contiguous(), rep(current), rep(duration),
                          env_step=env_step, **({} if wave is None else {"wave": wave}))
            mf = out["m_final"]                                          # [3, G R], on the backend's device
            tx, ty, tz = (float(x) for x in np.asarray(target, dtype=np.float64).reshape(3))
            proj = mf[0] * tx + mf[1] * ty + mf[2] * tz
            counts = torch.stack([(proj > float(threshold)).reshape(g, r).sum(1), (out["success"] == 0).reshape(g, r).sum(1)]).cpu().numpy()
        finally:
            b.close()
        self.solve_count += g * r
        n_sw, n_failed = counts[0].astype(np.int64), counts[1].astype(np.int64)
        p = n_sw / r
        return {"p_switch": p, "n_switched": n_sw, "n_failed": n_failed, "stderr": np.sqrt(p * (1.0 - p) / r)}

    def get_solver_info(self):
        return {"method": self.method, "solve_count": self.solve_count, "timeout_count": 0, "last_solve_time": 0.0,
                "timeout_rate": 0.0, "avg_solve_time": 0.0}


class RobustLLGSSolver(SimpleLLGSSolver):
    """utils/robust_solver.py:22-345: same kernels (the gates are always on), reference constructor signature."""
    _validate_params = True

    def __init__(self, method: str = "euler", rtol: float = 1e-3, atol: float = 1e-6, max_step: float = 1e-12,
                 timeout: float = 2.0, max_retries: int = 3, fallback_method: str = "euler",
                 enable_monitoring: bool = True, enable_validation: bool = True, **kw):
        super().__init__(method, rtol, atol, max_step, timeout, **kw)
        if not enable_validation:
            warnings.warn("enable_validation=False is not available on the GPU path; the gates stay on")
        self.max_retries, self.fallback_method = max_retries, fallback_method
        self.stats = {"total_solves": 0, "successful_solves": 0, "failed_solves": 0}

    def solve(self, m_initial, t_span, device_params, current_func=None, field_func=None, thermal_noise=False,
              temperature=300.0, **kwargs):
        res = super().solve(m_initial, t_span, device_params, current_func, field_func, thermal_noise, temperature)
        self.stats["total_solves"] += 1
        self.stats["successful_solves" if res["success"] else "failed_solves"] += 1
        return res

    def reset_statistics(self) -> None:
        """robust_solver.py:330-345 (the retry/fallback counters stay at zero here: the kernels have no retry path)."""
        self.stats = {"total_solves": 0, "successful_solves": 0, "failed_solves": 0}

    def get_statistics(self):
        st = dict(self.stats)
        tot = max(st["total_solves"], 1)
        st["success_rate"] = st["successful_solves"] / tot
        st["failure_rate"] = st["failed_solves"] / tot
        return st


class LLGSSolver(_GpuSolverBase):
    """physics/llgs_solver.py:21-305 with method='RK45' (the only method the step path configures, config.py:18-24)."""

    _solver_name = "rk45"

    def __init__(self, method: str = "RK45", rtol: float = 1e-6, atol: float = 1e-9, max_step: float = 1e-12,
                 gamma: float = 2.21e5, **kw):
        if method != "RK45":
            raise NotImplementedError(f"method '{method}': the GPU path implements SciPy's RK45 (Dormand-Prince 5(4))")
        if kw.get("noise_model", "white") != "white":
            raise ValueError("LLGSSolver (RK45) has the white thermal field only: 'ou' and 'brown' need a fixed dt (SimpleLLGSSolver)")
        super().__init__(rtol, atol, max_step, gamma, **kw)
        self.method = method
        self.k_b = 1.380649e-23

    def solve(self, m_initial, time_span, device_params, current_func, field_func=None, thermal_noise: bool = True,
              temperature: float = 300.0, max_points: int = 8192) -> Dict[str, Any]:
        r, k = self._solve_one(m_initial, time_span, device_params, current_func, field_func, thermal_noise,
                               temperature, max_points)
        if k > max_points:
            warnings.warn(f"trajectory truncated to max_points={max_points} of {k} accepted points")
            k = max_points
        t = r["t"][:k, 0]
        m = r["m"][:k, 0, :]
        # energy and |tau_stt| + |tau_fl| per accepted point are recorded by the kernel (llgs_solver.py:154-172)
        return {"t": t, "m": m, "energy": r["energy"][:k, 0], "torques": r["torques"][:k, 0], "success": bool(r["success"][0])}

    def find_stable_states(self, device_params: Dict[str, Any], n_trials: int = 100, threshold: float = 1e-6,
                           relax_time: float = 10e-9, seed: Optional[int] = None, initial_states=None,
                           applied_field=None) -> np.ndarray:
        """llgs_solver.py:264-305 as ONE batched relaxation of the n_trials random initial states (J = 0, no field, thermal
        off, 10 ns).  applied_field: a constant bias field [3] in A/m during the relaxation (a two-knot table; the reference
        method has no such argument).  The reference draws each trial's state from the GLOBAL legacy generator -- `np.random.normal(0, 1, 3)`
        per trial (llgs_solver.py:275-276) -- so does this method when `seed` is None: after `np.random.seed(s)` both give
        the same initial states, hence (within the solver tolerance) the same de-duplicated list, in the same order.
        `seed` draws from a private `RandomState(seed)` instead (same stream as `np.random.seed(seed)`, global state
        untouched); `initial_states` [n,3] bypasses the draws."""
        if initial_states is not None:
            m0 = np.asarray(initial_states, dtype=np.float64).reshape(-1, 3)
        else:
            gen = np.random if seed is None else np.random.RandomState(seed)
            m0 = np.array([gen.normal(0, 1, 3) for _ in range(n_trials)], dtype=np.float64).reshape(-1, 3)
        m0 = m0 / np.linalg.norm(m0, axis=1, keepdims=True)
        n = len(m0)
        field_knots = None
        if applied_field is not None:
            h = np.asarray(applied_field, dtype=np.float64).reshape(3)
            field_knots = (np.array([0.0, relax_time if relax_time > 0 else 1.0]), np.stack([h, h]))
        r = self.solve_batch(m0, np.zeros(n), np.full(n, relax_time), device_params, thermal_noise=False,
                             field_knots=field_knots)
        states = []
        for mf, ok in zip(r["m_final"], r["success"]):          # llgs_solver.py:290-300: first-come de-duplication
            if ok and all(np.linalg.norm(mf - s) >= threshold for s in states):
                states.append(mf)
        return np.array(states) if states else np.array([[0, 0, 1]])


class ThermalFluctuations:
    """physics/thermal_model.py:12-137.  Closed-form scalars and a host-side generator seeded like the reference's
    (``np.random.default_rng(seed)``), so the same seed gives the same field samples as the reference class.  It is API
    surface only: the env never samples this object (spin_torque_env.py:103-107 builds it, :303 only sets its
    temperature); the field the step path uses is drawn inside the kernels (csrc/stg_physics.hpp: NormalStream)."""

    def __init__(self, temperature: float = 300.0, correlation_time: float = 1e-12, seed: Optional[int] = None):
        self.temperature = temperature
        self.correlation_time = correlation_time
        self.k_b = 1.380649e-23
        self.mu_0 = MU0
        self.rng = np.random.default_rng(seed)
        self._previous_noise = np.zeros(3)

    def set_temperature(self, temperature: float) -> None:
        self.temperature = temperature

    def compute_noise_strength(self, damping, saturation_magnetization, volume, gamma: float = 2.21e5) -> float:
        if self.temperature <= 0:
            return 0.0
        return np.sqrt(2 * damping * self.k_b * self.temperature / (gamma * self.mu_0 * saturation_magnetization * volume))

    def generate_thermal_field(self, damping, saturation_magnetization, volume, dt, gamma: float = 2.21e5,
                               correlated: bool = True) -> np.ndarray:
        s = self.compute_noise_strength(damping, saturation_magnetization, volume, gamma)
        if s == 0:
            return np.zeros(3)
        white = self.rng.normal(0, 1, 3)
        if correlated and self.correlation_time > 0:      # Ornstein-Uhlenbeck update, thermal_model.py:113-137
            decay = np.exp(-dt / self.correlation_time)
            self._previous_noise = decay * self._previous_noise + np.sqrt(1 - decay ** 2) * white
            return s * self._previous_noise
        return s * white

    def compute_thermal_barrier(self, anisotropy_constant: float, volume: float) -> float:
        if self.temperature <= 0:
            return float("inf")
        return anisotropy_constant * volume / (self.k_b * self.temperature)

    def compute_switching_probability(self, energy_barrier, attempt_frequency: float = 1e9,
                                      measurement_time: float = 1e-9) -> float:
        if self.temperature <= 0:
            return 0.0
        rate = attempt_frequency * np.exp(-energy_barrier / (self.k_b * self.temperature))
        return min(1 - np.exp(-rate * measurement_time), 1.0)

    # -- Neel-Brown scalars (thermal_model.py:185-336): closed forms, host only ------------------------------------------
    _YEAR = 365.25 * 24 * 3600

    def _rate(self, energy_barrier, attempt_frequency):
        return attempt_frequency * np.exp(-energy_barrier / (self.k_b * self.temperature))

    def sample_switching_time(self, energy_barrier, attempt_frequency: float = 1e9) -> float:
        """thermal_model.py:185-207: exponential waiting time at the Arrhenius rate, from this object's generator."""
        if self.temperature <= 0:
            return float("inf")
        rate = self._rate(energy_barrier, attempt_frequency)
        return float("inf") if rate <= 0 else self.rng.exponential(1.0 / rate)

    def compute_retention_time(self, energy_barrier, failure_rate: float = 1e-9, attempt_frequency: float = 1e9) -> float:
        """thermal_model.py:209-232: -ln(failure_rate) / (f0 exp(-E_b / k_B T))."""
        if self.temperature <= 0 or failure_rate <= 0:
            return float("inf")
        return -np.log(failure_rate) / (attempt_frequency * np.exp(-(energy_barrier / (self.k_b * self.temperature))))

    def analyze_thermal_stability(self, device_params: dict, time_scale: float = 10.0) -> dict:
        """thermal_model.py:234-272 (time_scale in years)."""
        volume = device_params.get("volume", 1e-24)
        k_u = device_params.get("uniaxial_anisotropy", 1e6)
        e_b = k_u * volume
        delta = self.compute_thermal_barrier(k_u, volume)
        return {"thermal_stability_factor": delta, "energy_barrier_J": e_b,
                "energy_barrier_kT": e_b / (self.k_b * self.temperature),
                "switching_probability": self.compute_switching_probability(e_b, measurement_time=time_scale * self._YEAR),
                "retention_time_years": self.compute_retention_time(e_b) / self._YEAR,
                "is_thermally_stable": delta > 40, "temperature_K": self.temperature}

    def generate_temperature_sweep(self, temp_range: Tuple[float, float], device_params: dict, n_points: int = 100) -> dict:
        """thermal_model.py:274-336: stability factor, one-year switching probability, retention (years) and Brown field
        strength over a temperature grid; the object's temperature is restored afterwards."""
        temps = np.linspace(temp_range[0], temp_range[1], n_points)
        keep = self.temperature
        volume = device_params.get("volume", 1e-24)
        k_u = device_params.get("uniaxial_anisotropy", 1e6)
        damping = device_params.get("damping", 0.01)
        ms = device_params.get("saturation_magnetization", 800e3)
        cols = {"thermal_stability_factor": [], "switching_probability": [], "retention_time": [], "noise_strength": []}
        for t in temps:
            self.set_temperature(t)
            e_b = k_u * volume
            cols["thermal_stability_factor"].append(self.compute_thermal_barrier(k_u, volume))
            cols["switching_probability"].append(self.compute_switching_probability(e_b, measurement_time=self._YEAR))
            cols["retention_time"].append(self.compute_retention_time(e_b) / self._YEAR)
            cols["noise_strength"].append(self.compute_noise_strength(damping, ms, volume))
        self.set_temperature(keep)
        out = {"temperature": temps}
        out.update({k: np.array(v) for k, v in cols.items()})
        return out

"""HipBackend: one `stg_ctx` on one MI355X, driven through the C-ABI.

PyTorch-ROCm is used only as the device-memory container (tensors) and for the stream the kernels are
enqueued on; every computation happens in libspintorque_hip.so.  There is no CPU implementation here:
constructing a HipBackend without the built library or without a visible GPU raises.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib


@dataclass
class EnvConfig:
    """SpinTorqueEnv.__init__ keyword arguments that reach the step path (spin_torque_env.py:36-53) plus the
    solver constructor arguments (llgs_solver.py:24-31, simple_solver.py:24-31)."""
    solver: str = "rk4"                       # 'rk4' | 'euler' (SimpleLLGSSolver) | 'rk45' (LLGSSolver)
    include_thermal_fluctuations: bool = True
    temperature: float = 300.0
    gamma: float = 2.21e5
    max_step: float = 1e-12
    rtol: float = 1e-6
    atol: float = 1e-9
    max_steps: int = 100
    max_current: float = 2e6
    max_duration: float = 5e-9
    success_threshold: float = 0.9
    energy_penalty_weight: float = 0.1
    target_states: Sequence[Sequence[float]] = field(default_factory=lambda: [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]])
    seed: int = 0
    max_attempts: int = 200_000               # RK45 attempts per solve before giving up (a 5 ns pulse needs ~10 000)
    skip_done: bool = False
    torque_model: str = "reference"           # 'reference' (the env's type-agnostic RHS) | 'device' (opt-in)
    lane_sort: Optional[bool] = None          # duration-sorted lane schedule: None = automatic, True/False = force
    wave_spec: Optional[bool] = None          # producer/consumer wavefront pairs (thermal): None = automatic
    noise_model: str = "white"                # 'white' (reference solvers) | 'ou' (ThermalFluctuations) | 'brown' (the physical field:
                                              # standard deviation strength / sqrt(dt) per component); 'ou', 'brown': fixed-step only
    correlation_time: float = 1e-12           # ThermalFluctuations.correlation_time, for noise_model='ou'
    out_layout: str = "soa"                   # 'soa': obs [12,N] + reward/terminated/truncated arrays; 'records': one
                                              # [N,56]-byte record array (what the multi-GPU gather moves, copy-free)
    lane_refill: Optional[int] = None         # RK45 throughput launches: envs per lane (on average) of the lane-refill kernel; None =
                                              # automatic (the thresholds are in include/spintorque_hip.h, cfg.lane_refill),
                                              # False/0 = never, n >= 2 = force (results are bit-identical)
    diagnostics: bool = False                 # also write the step's fp64 reward, per-step energy and status bytes into separate
                                              # arrays (the C-ABI's optional outputs).  Off: those pointers are NULL, a step writes the
                                              # RL-facing outputs only (the status still rides in byte 54 of each record with
                                              # out_layout='records').  The terminal observations of same-step auto-reset are RL-facing
                                              # data, not a diagnostic: `final_obs` is written whenever auto-reset is on.

    def to_abi(self) -> "_lib.StgConfig":
        if self.solver not in _lib.SOLVERS:
            raise ValueError(f"Unknown solver '{self.solver}' (expected one of {list(_lib.SOLVERS)})")
        t = np.asarray(self.target_states, dtype=np.float64).reshape(-1, 3)
        if not 1 <= len(t) <= _lib.STG_MAX_TARGETS:
            raise ValueError(f"between 1 and {_lib.STG_MAX_TARGETS} target states are supported")
        c = _lib.StgConfig()
        c.solver = _lib.SOLVERS[self.solver]
        c.thermal = int(bool(self.include_thermal_fluctuations))
        c.temperature, c.gamma, c.max_step = float(self.temperature), float(self.gamma), float(self.max_step)
        c.rtol, c.atol = float(self.rtol), float(self.atol)
        c.max_steps, c.n_targets = int(self.max_steps), len(t)
        c.max_current, c.max_duration = float(self.max_current), float(self.max_duration)
        c.success_threshold, c.energy_penalty_weight = float(self.success_threshold), float(self.energy_penalty_weight)
        for i, row in enumerate(t):
            for j in range(3):
                c.targets[i][j] = float(row[j])
        c.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        c.max_attempts = int(self.max_attempts)
        c.skip_done = int(bool(self.skip_done))
        if self.torque_model not in ("reference", "device"):
            raise ValueError("torque_model must be 'reference' or 'device'")
        c.torque_model = int(self.torque_model == "device")
        c.lane_sort = 0 if self.lane_sort is None else (1 if self.lane_sort else -1)
        c.wave_spec = 0 if self.wave_spec is None else (1 if self.wave_spec else -1)
        if self.noise_model not in _lib.NOISE_MODELS:
            raise ValueError(f"noise_model must be one of {list(_lib.NOISE_MODELS)}")
        if self.noise_model == "brown" and self.solver == "rk45":
            raise ValueError("noise_model='brown' needs a fixed-step solver ('rk4' or 'euler'): an adaptive step has no fixed dt")
        c.noise_model = _lib.NOISE_MODELS[self.noise_model]
        c.noise_corr_time = float(self.correlation_time)
        if self.out_layout not in _lib.OUT_LAYOUTS:
            raise ValueError("out_layout must be 'soa' or 'records'")
        c.out_layout = _lib.OUT_LAYOUTS[self.out_layout]
        if self.lane_refill is None:
            c.lane_refill = 0
        elif not self.lane_refill:
            c.lane_refill = -1
        else:
            if int(self.lane_refill) < 2:
                raise ValueError("lane_refill must be None (automatic), False / 0 (never) or an integer >= 2 (envs per lane)")
            c.lane_refill = int(self.lane_refill)
        return c


PACKED_BYTES_PER_ENV = 54   # obs 12 x f32 + reward f32 + terminated u8 + truncated u8


def packed_step_buffer(n: int, device):
    """One contiguous uint8 buffer holding a step's RL-facing outputs, and typed views into it:
    [0, 48n) obs f32[12][n] | [48n, 52n) reward f32[n] | [52n, 53n) terminated u8[n] | [53n, 54n) truncated u8[n]."""
    buf = torch.zeros(PACKED_BYTES_PER_ENV * n, dtype=torch.uint8, device=device)
    return buf, unpack_step_buffer(buf, n)


def unpack_step_buffer(buf: torch.Tensor, n: int):
    obs = buf[: 48 * n].view(torch.float32).view(12, n)
    reward = buf[48 * n: 52 * n].view(torch.float32)
    return obs, reward, buf[52 * n: 53 * n], buf[53 * n: 54 * n]


RECORD_BYTES = _lib.RECORD_BYTES   # f32 obs[12] | f32 reward | u8 terminated | u8 truncated | u8 status | u8 0


def record_views(buf: torch.Tensor):
    """Typed views of a record array `buf` uint8[..., n, 56] (STG_OUT_RECORDS), no copies:
    obs f32[..., n, 12] (row stride 14 floats -- Gym's [N, 12] orientation), reward f32[..., n], terminated / truncated /
    status u8[..., n]."""
    f = buf.view(torch.float32)                       # [..., n, 14]
    return f[..., :12], f[..., 12], buf[..., 52], buf[..., 53], buf[..., 54]


def alloc_step_outputs(n: int, device, layout: str):
    """The RL-facing outputs of one step in the given layout: (container, obs [12,n] view, reward, terminated, truncated).
    'soa': the 54 B/env packed byte buffer (component-major obs); 'records': uint8 [n,56], obs = the transposed view."""
    if layout == "records":
        rec = torch.zeros((n, RECORD_BYTES), dtype=torch.uint8, device=device)
        obs, reward, term, trunc, _ = record_views(rec)
        return rec, obs.t(), reward, term, trunc
    buf, (obs, reward, term, trunc) = packed_step_buffer(n, device)
    return buf, obs, reward, term, trunc


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _pulse_knots(n: int, rows, field_knots):
    """What set_pulse_shape and set_pulse_knots marshal alike: `rows` ([n] each; not looked at with n = 0) and field_knots = (times [K],
    values [K,3]) or None, as contiguous float64 host arrays of exactly those shapes.  Returns (K, arrays, pointers) over rows + (times,
    values), None for what is absent; the arrays must outlive the call."""
    def host(x, shape_):
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
        if x.shape != shape_:
            raise ValueError(f"expected shape {shape_}, got {x.shape}")
        return x
    kh = 0 if field_knots is None else int(len(field_knots[0]))
    arrays = [host(r, (n,)) if n else None for r in rows]
    arrays += [host(field_knots[0], (kh,)), host(field_knots[1], (kh, 3))] if kh else [None, None]
    return kh, arrays, [None if x is None else C.c_void_p(x.ctypes.data) for x in arrays]


def alloc_final_obs(lead, m: int, device, layout: str):
    """Terminal-observation buffer of an auto-resetting step, shape `lead` + per-step: (what the kernel writes, its [.., 12, m] view).
    'records': env-major [.., m, 12] like the records (one 48-byte block per env) and the transposed view; else [.., 12, m] itself."""
    if layout == "records":
        buf = torch.zeros((*lead, m, 12), dtype=torch.float32, device=device)
        return buf, buf.transpose(-1, -2)
    buf = torch.zeros((*lead, 12, m), dtype=torch.float32, device=device)
    return buf, buf


class HipBackend:
    """Owns one stg_ctx.  All tensors are on ``cuda:<device_index>``; per-env arrays are component-major
    ([3,N], [12,N], [2,N]) as the C-ABI defines them."""

    def __init__(self, n_envs: int, cfg: EnvConfig, device_index: int = 0, env_id0: int = 0):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("HipBackend needs a visible MI355X (torch.cuda.is_available() is False); "
                               "there is no CPU fallback for the step path")
        self.n = int(n_envs)
        self.cfg = cfg
        self.device = torch.device("cuda", device_index)
        self.env_id0 = int(env_id0)
        self._ctx = C.c_void_p()
        abi = cfg.to_abi()
        _lib.check(self.lib.stg_create(C.byref(self._ctx), device_index, self.n, self.env_id0, C.byref(abi)))
        self._cls = None
        self.n_knots = 0               # P of set_pulse_knots (0: none set)
        n = self.n
        dev = self.device
        # (obs, reward, terminated, truncated) live in ONE buffer; the tensors below are views of it.  'soa': 54 B/env,
        # component-major obs [12,N]; 'records': [N,56] bytes, env-major -- a shard is one contiguous block, so the
        # multi-GPU path moves a step's results with a single all-gather straight into the global record array
        #  and `obs` is a strided [12,N] view (its .t() is Gym's [N,12]).
        self.records_layout = cfg.out_layout == "records"
        self.packed, self.obs, self.reward, self.terminated, self.truncated = alloc_step_outputs(n, dev, cfg.out_layout)
        self.diagnostics = bool(getattr(cfg, "diagnostics", False))
        if self.diagnostics:
            self.reward64 = torch.empty(n, dtype=torch.float64, device=dev)
            self.energy = torch.empty(n, dtype=torch.float64, device=dev)
            self.status = torch.empty(n, dtype=torch.uint8, device=dev)
        else:
            # the hot path writes nothing but the RL-facing outputs; in the records layout the status byte of each record
            # is still there (a view), in the SoA layout there is no status without diagnostics
            self.reward64 = self.energy = None
            self.status = record_views(self.packed)[4] if self.records_layout else None
        self.final_obs = None                 # [12,N] (a view of [N,12] in the records layout), allocated on the first auto-resetting step
        self._final_buf = None

    # -- plumbing -------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, t, dtype, shape=None):
        if t is None:
            return None
        t = torch.as_tensor(t)
        t = t.to(device=self.device, dtype=dtype).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def _out_ptrs(self, out, final, reward, reward64, energy, term, trunc, status):
        """The eight output-pointer arguments of stg_step_many / stg_step_ids in ABI order.  `out` is the record array or the obs
        array; in the records layout reward / terminated / truncated live in the records (NULL), and the status array is only
        written with diagnostics (without them `status` is at most a view of the records)."""
        rec = self.records_layout
        return (_ptr(out), _ptr(final), None if rec else _ptr(reward), _ptr(reward64), _ptr(energy), None if rec else _ptr(term),
                None if rec else _ptr(trunc), _ptr(status) if self.diagnostics else None)

    def close(self):
        if self._ctx:
            torch.cuda.synchronize(self.device)
            self.lib.stg_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- parameter surface ------------------------------------------------------------------------
    def set_params(self, table: List["_lib.StgDeviceParams"], cls=None):
        arr = (_lib.StgDeviceParams * len(table))(*table)
        self._cls = self._dev(cls, torch.uint8, (self.n,)) if len(table) > 1 else None
        if len(table) > 1 and self._cls is None:
            raise ValueError("a class index per env is required with more than one device class")
        if self._cls is not None and int(self._cls.max()) >= len(table):
            raise ValueError("class index out of range")
        _lib.check(self.lib.stg_set_params(self._ctx, arr, len(table), _ptr(self._cls)))
        self.n_classes = len(table)

    def set_params_per_env(self, block, dev_type, valid):
        """Per-env parameters: block float64 [STG_NPARAM, N] (rows = the double fields of stg_device_params in
        declaration order, see devices.PARAM_ROWS / per_env_param_block), dev_type uint8 [N], valid uint8 [N]."""
        block = self._dev(block, torch.float64, (_lib.STG_NPARAM, self.n))
        dev_type = self._dev(dev_type, torch.uint8, (self.n,))
        valid = self._dev(valid, torch.uint8, (self.n,))
        torch.cuda.synchronize(self.device)
        _lib.check(self.lib.stg_set_params_per_env(self._ctx, _ptr(block), _ptr(dev_type), _ptr(valid)))
        self._cls = None
        self.n_classes = 0

    def thermal_strength(self, cls=0) -> float:
        out = C.c_double()
        _lib.check(self.lib.stg_thermal_strength(self._ctx, cls, C.byref(out)))
        return out.value

    # -- env level ----------------------------------------------------------------------------------
    def reset(self, mask=None, init_m=None, target=None, seed=0):
        mask = self._dev(mask, torch.uint8, (self.n,))
        init_m = self._dev(init_m, torch.float64, (3, self.n))
        target = self._dev(target, torch.float64, (3, self.n))
        _lib.check(self.lib.stg_reset(self._ctx, _ptr(mask), _ptr(init_m), _ptr(target),
                                      int(seed) & 0xFFFFFFFFFFFFFFFF,
                                      _ptr(self.packed if self.records_layout else self.obs), self._stream()))
        self._keep = (mask, init_m, target)      # keep inputs alive until the stream has consumed them
        return self.obs

    def _one_step(self, launch, actions, autoreset, out):
        """What step() and step_wave() share: the actions on the device, the final_obs buffer, the destination (`out=`), the eight
        output pointers, and the views handed back.  launch(a, f64, out_ptrs): the library call, returns its code."""
        a = torch.as_tensor(actions)
        f64 = a.dtype == torch.float64
        a = self._dev(a, torch.float64 if f64 else torch.float32, (2, self.n))
        if autoreset and self.final_obs is None:
            self._final_buf, self.final_obs = alloc_final_obs((), self.n, self.device, self.cfg.out_layout)
        if out is not None and not self.records_layout:
            raise ValueError("out= needs out_layout='records'")
        dst = (self.packed if out is None else out) if self.records_layout else self.obs
        if self.records_layout and (dst.dtype != torch.uint8 or tuple(dst.shape) != (self.n, RECORD_BYTES) or not dst.is_contiguous()
                                    or dst.device != self.device):
            raise ValueError(f"out must be a contiguous uint8 [{self.n}, {RECORD_BYTES}] tensor on {self.device}")
        _lib.check(launch(a, int(f64), self._out_ptrs(dst, self._final_buf if autoreset else None, self.reward, self.reward64, self.energy,
                                                      self.terminated, self.truncated, self.status)))
        self._keep = (a,)
        if out is None:
            return self.obs, self.reward, self.reward64, self.terminated, self.truncated, self.status
        obs, reward, term, trunc, st = record_views(out)
        return obs.t(), reward, self.reward64, term, trunc, (self.status if self.diagnostics else st)

    def step(self, actions, autoreset=False, out: Optional[torch.Tensor] = None):
        """actions: [2,N] float32 or float64 tensor (row 0 current density, row 1 duration).  One kernel launch; the
        RL-facing outputs land in `self.packed`.  autoreset (same-step): an env whose episode ends ON THIS step reports
        this step's reward / terminated / truncated, is reset on the device inside the same launch, and its `obs` row
        already holds the new episode's first observation; the terminal observation goes to `self.final_obs` (always, with or
        without `diagnostics`: a learner that bootstraps at truncation needs it; rows of other envs keep their last content).
        out ('records' layout only): another uint8 [N,56] record array to write this step's outputs into instead of
        `self.packed` (callers that double-buffer, e.g. the pipelined multi-GPU gather); the returned views are of `out`."""
        return self._one_step(lambda a, f64, outs: self.lib.stg_step_many(self._ctx, 1, _ptr(a), f64, 1, int(bool(autoreset)), *outs,
                                                                          self._stream()), actions, autoreset, out)

    def _wave_tables(self, wave, n=None):
        """wave = dict(current=(tj [K,N], jk [K,N]) | None, field=(th [K,N], hk [K,3,N]) | None) -> (kj, tj, jk, kh, th, hk) on the
        device, as stg_solve_wave / stg_step_wave take them (a missing table: knot count 0, no pointers).  n: the number of columns
        (None: the context's envs; stg_switch_stats_wave has one column per condition)."""
        n = self.n if n is None else n
        tj = jk = th = hk = None
        kj = kh = 0
        if wave.get("current") is not None:
            tj, jk = wave["current"]
            kj = int(torch.as_tensor(tj).shape[0])
            tj, jk = self._dev(tj, torch.float64, (kj, n)), self._dev(jk, torch.float64, (kj, n))
        if wave.get("field") is not None:
            th, hk = wave["field"]
            kh = int(torch.as_tensor(th).shape[0])
            th, hk = self._dev(th, torch.float64, (kh, n)), self._dev(hk, torch.float64, (kh, 3, n))
        return kj, tj, jk, kh, th, hk

    def step_wave(self, actions, wave, autoreset=False, out: Optional[torch.Tensor] = None):
        """step() with piecewise-linear waveforms (stg_step_wave): wave = dict(current=(tj [K,N], jk [K,N]) | None,
        field=(th [K,N], hk [K,3,N]) | None) as solve(wave=) takes it -- times in seconds from the start of this pulse; a missing
        current table means the rectangular parsed J, a missing field table zero field.  The parsed duration is the integration
        span; with a current table the parsed J only fills the observation.  Everything else -- outputs, autoreset, out= -- as step()."""
        kj, tj, jk, kh, th, hk = self._wave_tables(wave)
        res = self._one_step(lambda a, f64, outs: self.lib.stg_step_wave(self._ctx, _ptr(a), f64, int(bool(autoreset)), kj, _ptr(tj), _ptr(jk),
                                                                         kh, _ptr(th), _ptr(hk), *outs, self._stream()),
                             actions, autoreset, out)
        self._keep = self._keep + (tj, jk, th, hk)
        return res

    def step_many(self, actions, out_every=True, autoreset=False):
        """actions: [K,2,N]; returns tensors with a leading K (out_every) or 1 dimension."""
        return self._many(self.lib.stg_step_many, actions, out_every, autoreset)

    def set_pulse_shape(self, shape, field_knots):
        """The env-level drive of step_shaped_many / step_shaped_ids (stg_set_pulse_shape): shape = a scalar physics.PiecewiseLinear
        over normalised time (times tau in [0, 1], values = factors on the action's current density) or None (the rectangular pulse);
        field_knots = (times [K] in seconds, values [K,3] in A/m) or None (zero field).  Both None clears the shape.  The library copies
        the knots; called once per context, not per step."""
        kj = 0 if shape is None else int(len(shape.times))
        kh, keep, (tau, scale, th, hk) = _pulse_knots(kj, (shape.times, shape.values) if kj else (None, None), field_knots)
        _lib.check(self.lib.stg_set_pulse_shape(self._ctx, kj, tau, scale, kh, th, hk))

    def step_shaped_many(self, actions, out_every=True, autoreset=False):
        """step_many under the shape of set_pulse_shape (stg_step_shaped): K env steps in one launch, the drive of each env at each step
        being the shape applied to that step's parsed action.  Arguments, buffers and return values are step_many's."""
        return self._many(self.lib.stg_step_shaped, actions, out_every, autoreset)

    def set_pulse_knots(self, tau, amplitude_limit, field_knots):
        """The knot times of step_knots_many / step_knots_ids (stg_set_pulse_knots): tau = [P] normalised knot times in [0, 1], strictly
        increasing; amplitude_limit = the clamp of an action's amplitudes; field_knots = (times [K] in seconds, values [K,3] in A/m) or
        None (zero field).  tau = None clears the knots.  The library copies them; called once per context, not per step."""
        p = 0 if tau is None else int(len(tau))
        kh, keep, (tau, th, hk) = _pulse_knots(p, (tau,), field_knots)
        _lib.check(self.lib.stg_set_pulse_knots(self._ctx, p, tau, float(amplitude_limit), kh, th, hk))
        self.n_knots = p

    def step_knots_many(self, actions, out_every=True, autoreset=False):
        """step_many with actions [K, 2+P, N] that carry the pulse's knot amplitudes (stg_step_knots; P knots set by set_pulse_knots):
        K env steps in one launch.  Buffers and return values are step_shaped_many's."""
        return self._many(self.lib.stg_step_knots, actions, out_every, autoreset, rows=2 + self.n_knots)

    def _many(self, entry, actions, out_every, autoreset, rows=2):
        """What step_many, step_shaped_many and step_knots_many share (their C-ABI entries have one signature): buffers, the call, the
        views.  rows: the rows of one step's action block."""
        a = torch.as_tensor(actions)
        f64 = a.dtype == torch.float64
        K = int(a.shape[0])
        a = self._dev(a, torch.float64 if f64 else torch.float32, (K, rows, self.n))
        ko = K if out_every else 1
        n, dev = self.n, self.device
        if self.records_layout:
            rec = torch.empty((ko, n, RECORD_BYTES), dtype=torch.uint8, device=dev)
            o, reward, term, trunc, _ = record_views(rec)
            obs, out_ptr = o.transpose(1, 2), rec             # [ko,12,n] view
        else:
            obs = torch.empty((ko, 12, n), dtype=torch.float32, device=dev)
            reward = torch.empty((ko, n), dtype=torch.float32, device=dev)
            term = torch.empty((ko, n), dtype=torch.uint8, device=dev)
            trunc = torch.empty((ko, n), dtype=torch.uint8, device=dev)
            out_ptr = obs
        diag = self.diagnostics
        reward64 = torch.empty((ko, n), dtype=torch.float64, device=dev) if diag else None
        status = torch.empty((ko, n), dtype=torch.uint8, device=dev) if diag else (record_views(rec)[4] if self.records_layout else None)
        self.energy_many = torch.empty((ko, n), dtype=torch.float64, device=dev) if diag else None
        fbuf, self.final_obs_many = alloc_final_obs((ko,), n, dev, self.cfg.out_layout) if autoreset else (None, None)
        _lib.check(entry(self._ctx, K, _ptr(a), int(f64), int(bool(out_every)), int(bool(autoreset)),
                         *self._out_ptrs(out_ptr, fbuf, reward, reward64, self.energy_many, term, trunc, status), self._stream()))
        self._keep = (a,)
        return obs, reward, reward64, term, trunc, status

    # -- subset stepping (stg_step_ids) and what the send/recv pool needs of a backend -----------------------------------
    def ids_workspace(self, m):
        """A workspace for stg_step_ids launches of up to m ids (uint8 device tensor, stg_step_ids_workspace_bytes)."""
        nb = int(self.lib.stg_step_ids_workspace_bytes(self._ctx, int(m)))
        if nb <= 0:
            raise ValueError("m must be >= 1")
        return torch.empty(nb, dtype=torch.uint8, device=self.device)

    def alloc_ids_outputs(self, m, autoreset=False):
        """Output arrays of one stg_step_ids launch of m ids, compact and in list order: dict(buf (what the kernel writes),
        obs [12,m] view, reward, terminated, truncated, status, reward64, energy, final_buf, final_obs [12,m] view)."""
        dev = self.device
        buf, obs, reward, term, trunc = alloc_step_outputs(m, dev, self.cfg.out_layout)
        out = dict(buf=buf, obs=obs, reward=reward, terminated=term, truncated=trunc, reward64=None, energy=None, final_buf=None,
                   final_obs=None, status=record_views(buf)[4] if self.records_layout else None)
        if self.diagnostics:
            out.update(reward64=torch.empty(m, dtype=torch.float64, device=dev), energy=torch.empty(m, dtype=torch.float64, device=dev),
                       status=torch.empty(m, dtype=torch.uint8, device=dev))
        if autoreset:
            out["final_buf"], out["final_obs"] = alloc_final_obs((), m, dev, self.cfg.out_layout)
        return out

    def step_ids(self, actions, env_ids, autoreset=False, workspace=None, out=None, stream=None):
        """stg_step_ids: one env step of the envs env_ids ([M] integers, host or device) only, with actions [2,M] in list order.
        Outputs are compact, in list order (output j belongs to env_ids[j]): the dict of alloc_ids_outputs (`out`, or new arrays).
        No range or duplicate checks here: an id >= N reports STATUS_BAD_ID (SpinTorqueVecEnv checks on the host).
        workspace: from ids_workspace(M' >= M), or None for a new one.  stream: a torch.cuda.Stream to launch on -- it first waits for
        the current stream (which produced the inputs) and the new arrays belong to it -- or None for the current stream.  Launches
        on different streams may overlap only under the header's concurrency contract (own workspace, pair-closed disjoint id sets)."""
        return self._ids(None, actions, env_ids, autoreset, workspace, out, stream)

    def step_shaped_ids(self, actions, env_ids, autoreset=False, out=None, stream=None):
        """step_ids under the shape of set_pulse_shape (stg_step_shaped_ids): one shaped env step of the envs env_ids only.  Arguments,
        outputs (alloc_ids_outputs) and the stream rules are step_ids's; there is no workspace (identity order: nothing is staged)."""
        return self._ids(self.lib.stg_step_shaped_ids, actions, env_ids, autoreset, None, out, stream)

    def step_knots_ids(self, actions, env_ids, autoreset=False, out=None, stream=None):
        """step_ids with actions [2+P, M] that carry the pulse's knot amplitudes (stg_step_knots_ids).  Arguments, outputs
        (alloc_ids_outputs) and the stream rules are step_shaped_ids's."""
        return self._ids(self.lib.stg_step_knots_ids, actions, env_ids, autoreset, None, out, stream, rows=2 + self.n_knots)

    def _ids(self, entry, actions, env_ids, autoreset, workspace, out, stream, rows=2):
        """What step_ids, step_shaped_ids and step_knots_ids share: inputs and outputs on the launch's stream, the call.  entry: a
        pulse-step entry, which takes no workspace (stg_step_shaped_ids' signature), or None for stg_step_ids; rows: the rows of an
        action block."""
        cur = torch.cuda.current_stream(self.device)
        s = cur if stream is None else stream
        if s is not cur:
            s.wait_stream(cur)
        with torch.cuda.stream(s):
            a = torch.as_tensor(actions)
            f64 = a.dtype == torch.float64
            m = int(a.shape[-1])
            a = self._dev(a, torch.float64 if f64 else torch.float32, (rows, m))
            ids = self._dev(env_ids, torch.int32, (m,))        # (the kernel reads uint32: same bits for ids < 2^31)
            if s is not cur:
                a.record_stream(s)
                ids.record_stream(s)
            ws = None if entry else (self.ids_workspace(m) if workspace is None else workspace)
            if out is None:
                out = self.alloc_ids_outputs(m, autoreset)
            outs = self._out_ptrs(out["buf"], out["final_buf"] if autoreset else None, out["reward"], out["reward64"], out["energy"],
                                  out["terminated"], out["truncated"], out["status"])
            head = (self._ctx, m, _ptr(ids), _ptr(a), int(f64), int(bool(autoreset)))
            if entry:
                _lib.check(entry(*head, *outs, C.c_void_p(s.cuda_stream)))
            else:
                _lib.check(self.lib.stg_step_ids(*head, _ptr(ws), *outs, C.c_void_p(s.cuda_stream)))
        out["_keep"] = (a, ids, ws)           # inputs stay alive while the launch may still read them
        return out

    def make_streams(self, k):
        return [torch.cuda.Stream(self.device) for _ in range(int(k))]

    def record_event(self, stream):
        ev = torch.cuda.Event()
        ev.record(stream)
        return ev

    def hand_over(self, out):
        """The arrays of a completed id launch are read on the current stream from now on (caching-allocator bookkeeping)."""
        cur = torch.cuda.current_stream(self.device)
        for k, t in out.items():
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(cur)

    def get_state(self):
        n, dev = self.n, self.device
        st = dict(m=torch.empty((3, n), dtype=torch.float64, device=dev),
                  target=torch.empty((3, n), dtype=torch.float64, device=dev),
                  total_energy=torch.empty(n, dtype=torch.float64, device=dev),
                  step_count=torch.empty(n, dtype=torch.int32, device=dev),
                  rng_step=torch.empty(n, dtype=torch.int32, device=dev),
                  done=torch.empty(n, dtype=torch.uint8, device=dev))
        _lib.check(self.lib.stg_get_state(self._ctx, _ptr(st["m"]), _ptr(st["target"]), _ptr(st["total_energy"]),
                                          _ptr(st["step_count"]), _ptr(st["rng_step"]), _ptr(st["done"]),
                                          self._stream()))
        return st

    def set_state(self, st):
        n = self.n
        m = self._dev(st.get("m"), torch.float64, (3, n))
        tg = self._dev(st.get("target"), torch.float64, (3, n))
        e = self._dev(st.get("total_energy"), torch.float64, (n,))
        sc = self._dev(st.get("step_count"), torch.int32, (n,))
        rs = self._dev(st.get("rng_step"), torch.int32, (n,))
        dn = self._dev(st.get("done"), torch.uint8, (n,))
        _lib.check(self.lib.stg_set_state(self._ctx, _ptr(m), _ptr(tg), _ptr(e), _ptr(sc), _ptr(rs), _ptr(dn),
                                          self._stream()))
        self._keep = (m, tg, e, sc, rs, dn)

    # -- solver level -------------------------------------------------------------------------------
    def solve(self, m0, J, T, env_step=0, traj_cap=0, want_energy=False, wave=None):
        """N solves over (0, T).  wave = None: rectangular pulses J while t <= T, zero field (stg_solve / stg_solve_traj).
        wave = dict(current=(tj [K,N], jk [K,N]) | None, field=(th [K,N], hk [K,3,N]) | None): piecewise-linear waveforms
        (stg_solve_wave; a missing current table means the rectangular J, a missing field table zero field; J may be None
        with a current table)."""
        n, dev = self.n, self.device
        m0 = self._dev(m0, torch.float64, (3, n))
        J = self._dev(J, torch.float64, (n,))
        T = self._dev(T, torch.float64, (n,))
        mf = torch.empty((3, n), dtype=torch.float64, device=dev)
        npts = torch.empty(n, dtype=torch.int32, device=dev)
        succ = torch.empty(n, dtype=torch.uint8, device=dev)
        out = dict(m_final=mf, n_points=npts, success=succ)
        t = m = e = tq = None
        if traj_cap > 0:
            t = torch.zeros((traj_cap, n), dtype=torch.float64, device=dev)
            m = torch.zeros((traj_cap, 3, n), dtype=torch.float64, device=dev)
            # energy and torques are LLGSSolver's by-products (llgs_solver.py:154-172), recorded together
            e = torch.zeros((traj_cap, n), dtype=torch.float64, device=dev) if want_energy else None
            tq = torch.zeros((traj_cap, n), dtype=torch.float64, device=dev) if want_energy else None
            out.update(t=t, m=m, energy=e, torques=tq)
        if wave is not None:
            kj, tj, jk, kh, th, hk = self._wave_tables(wave)
            _lib.check(self.lib.stg_solve_wave(self._ctx, _ptr(m0), _ptr(J), _ptr(T), kj, _ptr(tj), _ptr(jk), kh, _ptr(th), _ptr(hk),
                                               int(env_step), int(traj_cap), _ptr(t), _ptr(m), _ptr(e), _ptr(tq), _ptr(mf),
                                               _ptr(npts), _ptr(succ), self._stream()))
            self._keep = (m0, J, T, tj, jk, th, hk)
            return out
        if traj_cap > 0:
            _lib.check(self.lib.stg_solve_traj(self._ctx, _ptr(m0), _ptr(J), _ptr(T), int(env_step), int(traj_cap),
                                               _ptr(t), _ptr(m), _ptr(e), _ptr(tq), _ptr(mf), _ptr(npts), _ptr(succ),
                                               self._stream()))
        else:
            _lib.check(self.lib.stg_solve(self._ctx, _ptr(m0), _ptr(J), _ptr(T), int(env_step), _ptr(mf),
                                          _ptr(npts), _ptr(succ), self._stream()))
        self._keep = (m0, J, T)
        return out

    def _switch_args(self, m0, J, T, target, n_trials, trial0, trial_stride, cond_cls, bins, out):
        """What the three switching entries share: (G, R, trial0, stride, P) as ints, the condition arrays on the device in their
        shapes, and `out` -- the caller's, or zeros: two [G] counts and a [G,b] histogram (None for b = 0) for every b of `bins`.
        J may be None (a single tabled phase)."""
        m0 = self._dev(m0, torch.float64)
        g = int(m0.shape[-1])
        m0 = self._dev(m0, torch.float64, (3, g))
        T = self._dev(T, torch.float64)
        p = int(T.shape[0])
        J, T = self._dev(J, torch.float64, (p, g)), self._dev(T, torch.float64, (p, g))
        target = self._dev(target, torch.float64, (3, g))
        cond_cls = self._dev(cond_cls, torch.uint8, (g,))
        r, t0 = int(n_trials), int(trial0)
        stride = t0 + r if trial_stride is None else int(trial_stride)
        if out is None:
            zeros = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=self.device)      # noqa: E731
            out = tuple(x for b in bins for x in (zeros(g), zeros(g), zeros(g, int(b)) if b > 0 else None))
        self._keep = (m0, J, T, target, cond_cls)
        return (g, r, t0, stride, p), (m0, J, T, target, cond_cls), out

    def switch_stats(self, m0, J, T, target, n_trials, trial0=0, trial_stride=None, cond_cls=None, env_step=0, threshold=0.0,
                     n_bins=0, out=None):
        """Monte-Carlo switching counts reduced on the device (stg_switch_stats): trials trial0 ... trial0 + n_trials - 1 of the G
        conditions m0 [3,G], J, T [P,G], target [3,G]; cond_cls uint8 [G] picks each condition's class of set_params (None: class 0).
        Trial r of condition g is problem g * trial_stride + r of `solve` at env_step + p (trial_stride None: trial0 + n_trials).
        Returns (n_switched [G], n_failed [G], hist [G,n_bins] or None), int64 on the device; the call ADDS to them: `out` = the
        triple of an earlier call accumulates a chunked trial range, None starts from zero.  Enqueues only."""
        (g, r, t0, stride, p), (m0, J, T, target, cond_cls), out = self._switch_args(m0, J, T, target, n_trials, trial0, trial_stride,
                                                                                     cond_cls, (n_bins,), out)
        n_sw, n_failed, hist = out
        _lib.check(self.lib.stg_switch_stats(self._ctx, g, r, t0, stride, p, _ptr(m0), _ptr(J), _ptr(T), _ptr(cond_cls), int(env_step),
                                             _ptr(target), float(threshold), int(n_bins), _ptr(n_sw), _ptr(n_failed), _ptr(hist),
                                             self._stream()))
        return out

    def switch_verify(self, m0, J, T, target, n_trials, trial0=0, trial_stride=None, cond_cls=None, env_step=0, threshold=0.0,
                      n_bins=0, max_waves=0, out=None):
        """Write - verify - write counts reduced on the device (stg_switch_verify): a trial is up to A attempts of P rectangular phases,
        J, T [A,P,G] ([A,G]: one phase per attempt); after every attempt it is classified as in switch_stats, and it ends when it has
        switched, when a solve failed or after attempt A - 1; the next attempt starts from the m the one before left behind.  Phase p
        of attempt a of trial r of condition g is problem g * trial_stride + r of `solve` at env_step + a * P + p.  The other arguments
        are those of switch_stats; max_waves > 0 bounds the launch's wavefronts (>= G; the counts do not depend on it).  Returns
        (n_switched_at [A,G], n_ended_at [A,G], n_failed [G], hist [G,n_bins] or None), int64 on the device; the call ADDS to them:
        `out` = the tuple of an earlier call accumulates a chunked trial range, None starts from zero.  Enqueues only."""
        m0 = self._dev(m0, torch.float64)
        g = int(m0.shape[-1])
        m0 = self._dev(m0, torch.float64, (3, g))
        J, T = (x[:, None, :] if x.dim() == 2 else x for x in (self._dev(J, torch.float64), self._dev(T, torch.float64)))
        a, p = int(T.shape[0]), int(T.shape[1])
        J, T = self._dev(J, torch.float64, (a, p, g)), self._dev(T, torch.float64, (a, p, g))
        target = self._dev(target, torch.float64, (3, g))
        cond_cls = self._dev(cond_cls, torch.uint8, (g,))
        r, t0 = int(n_trials), int(trial0)
        stride = t0 + r if trial_stride is None else int(trial_stride)
        if out is None:
            zeros = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=self.device)      # noqa: E731
            out = (zeros(a, g), zeros(a, g), zeros(g), zeros(g, int(n_bins)) if n_bins > 0 else None)
        n_sw, n_end, n_failed, hist = out
        self._keep = (m0, J, T, target, cond_cls)
        _lib.check(self.lib.stg_switch_verify(self._ctx, g, r, t0, stride, a, p, _ptr(m0), _ptr(J), _ptr(T), _ptr(cond_cls), int(env_step),
                                              _ptr(target), float(threshold), int(n_bins), int(max_waves), _ptr(n_sw), _ptr(n_end),
                                              _ptr(n_failed), _ptr(hist), self._stream()))
        return out

    def switch_verify_population(self, m0, J, T, target, n_trials, sigma, z_clip=4.0, var_step=2 ** 31, trials_per_device=1,
                                 dev_switched_at=None, trial0=0, trial_stride=None, cond_cls=None, env_step=0, threshold=0.0, n_bins=0,
                                 max_waves=0, out=None):
        """switch_verify over a population of devices (stg_switch_verify_population): trial r (absolute) of condition g belongs to
        device r // trials_per_device, drawn as switch_population draws it (sigma float64 [5, G], z_clip, var_step -- which must differ
        from env_step + k of all A * P phases), and every attempt of the trial integrates with that device's own constants.
        dev_switched_at int64 [A, G, dev_stride] on the device, indexed by the absolute device id, gains one per trial of the device
        that ended switched at attempt a, when given.  Everything else, the returned tuple and `out` included, as switch_verify.
        Enqueues only."""
        m0 = self._dev(m0, torch.float64)
        g = int(m0.shape[-1])
        m0 = self._dev(m0, torch.float64, (3, g))
        J, T = (x[:, None, :] if x.dim() == 2 else x for x in (self._dev(J, torch.float64), self._dev(T, torch.float64)))
        a, p = int(T.shape[0]), int(T.shape[1])
        J, T = self._dev(J, torch.float64, (a, p, g)), self._dev(T, torch.float64, (a, p, g))
        target = self._dev(target, torch.float64, (3, g))
        cond_cls = self._dev(cond_cls, torch.uint8, (g,))
        sigma = self._dev(sigma, torch.float64, (_lib.STG_NVARY, g))
        r, t0 = int(n_trials), int(trial0)
        stride = t0 + r if trial_stride is None else int(trial_stride)
        if out is None:
            zeros = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=self.device)      # noqa: E731
            out = (zeros(a, g), zeros(a, g), zeros(g), zeros(g, int(n_bins)) if n_bins > 0 else None)
        n_sw, n_end, n_failed, hist = out
        dev_stride = 0
        if dev_switched_at is not None:
            if (not torch.is_tensor(dev_switched_at) or dev_switched_at.dtype != torch.int64 or dev_switched_at.dim() != 3
                    or tuple(dev_switched_at.shape[:2]) != (a, g) or not dev_switched_at.is_contiguous() or not dev_switched_at.is_cuda):
                raise ValueError(f"dev_switched_at must be a contiguous int64 tensor [A = {a}, G = {g}, dev_stride] on {self.device}")
            dev_stride = int(dev_switched_at.shape[2])
        self._keep = (m0, J, T, target, cond_cls, sigma)
        _lib.check(self.lib.stg_switch_verify_population(self._ctx, g, r, t0, stride, a, p, _ptr(m0), _ptr(J), _ptr(T), _ptr(cond_cls),
                                                         int(env_step), _ptr(target), float(threshold), int(n_bins), int(max_waves),
                                                         _ptr(n_sw), _ptr(n_end), _ptr(n_failed), _ptr(hist), _ptr(sigma), float(z_clip),
                                                         int(var_step), int(trials_per_device), _ptr(dev_switched_at), dev_stride,
                                                         self._stream()))
        return out

    def switch_stats_wave(self, m0, J, T, target, n_trials, wave, wave_phase=0, trial0=0, trial_stride=None, cond_cls=None, env_step=0,
                          threshold=0.0, n_bins=0, out=None):
        """switch_stats with phase `wave_phase` driven by piecewise-linear tables (stg_switch_stats_wave): wave = dict(current=(tj [K,G],
        jk [K,G]) | None, field=(th [K,G], hk [K,3,G]) | None) as solve(wave=) takes it, one column per CONDITION; times in seconds from
        the start of that phase.  A missing current table means the rectangular J[wave_phase], a missing field table zero field (not
        both).  The other phases are the rectangular J, T [P,G] of switch_stats; trial r of condition g is problem g * trial_stride + r
        of `solve(wave=)` at env_step + wave_phase and of `solve` at the other phases' env_step + p.  Returns and `out` as switch_stats."""
        (g, r, t0, stride, p), (m0, J, T, target, cond_cls), out = self._switch_args(m0, J, T, target, n_trials, trial0, trial_stride,
                                                                                     cond_cls, (n_bins,), out)
        kj, tj, jk, kh, th, hk = self._wave_tables(wave, g)
        n_sw, n_failed, hist = out
        _lib.check(self.lib.stg_switch_stats_wave(self._ctx, g, r, t0, stride, p, _ptr(m0), _ptr(J), _ptr(T), int(wave_phase), kj, _ptr(tj),
                                                  _ptr(jk), kh, _ptr(th), _ptr(hk), _ptr(cond_cls), int(env_step), _ptr(target),
                                                  float(threshold), int(n_bins), _ptr(n_sw), _ptr(n_failed), _ptr(hist), self._stream()))
        self._keep += (tj, jk, th, hk)
        return out

    def switch_times(self, m0, J, T, target, n_trials, watch_phase=0, wave=None, n_tbins=0, trial0=0, trial_stride=None, cond_cls=None,
                     env_step=0, threshold=0.0, n_bins=0, out=None):
        """switch_stats / switch_stats_wave plus the first passage of m . target over `threshold` during phase `watch_phase`
        (stg_switch_times).  wave = None: that phase is the rectangular J[watch_phase]; wave = dict(current=..., field=...) as
        switch_stats_wave takes it drives it.  A trial crosses at the first recorded point of the watched phase (the rows of
        `solve(traj_cap=)`) beyond the threshold; its crossing time is the midpoint of that point and the one before, binned into
        n_tbins equal bins over the phase's [0, T].  Returns (n_switched [G], n_failed [G], hist [G,n_bins] or None, n_crossed [G],
        n_returned [G], t_hist [G,n_tbins] or None), int64 on the device -- n_returned: crossed, yet not switched at the trial's end.
        The call ADDS to them: `out` = the tuple of an earlier call accumulates, None starts from zero.  Enqueues only."""
        (g, r, t0, stride, p), (m0, J, T, target, cond_cls), out = self._switch_args(m0, J, T, target, n_trials, trial0, trial_stride,
                                                                                     cond_cls, (n_bins, n_tbins), out)
        kj, tj, jk, kh, th, hk = self._wave_tables(wave, g) if wave is not None else (0, None, None, 0, None, None)
        n_sw, n_failed, hist, n_cr, n_ret, t_hist = out
        _lib.check(self.lib.stg_switch_times(self._ctx, g, r, t0, stride, p, _ptr(m0), _ptr(J), _ptr(T), int(watch_phase), kj, _ptr(tj),
                                             _ptr(jk), kh, _ptr(th), _ptr(hk), _ptr(cond_cls), int(env_step), _ptr(target),
                                             float(threshold), int(n_bins), _ptr(n_sw), _ptr(n_failed), _ptr(hist), int(n_tbins),
                                             _ptr(n_cr), _ptr(n_ret), _ptr(t_hist), self._stream()))
        self._keep += (tj, jk, th, hk)
        return out

    def switch_population(self, m0, J, T, target, n_trials, sigma, watch_phase=0, wave=None, n_tbins=0, passage=None, z_clip=4.0,
                          var_step=2 ** 31, trials_per_device=1, dev_switched=None, trial0=0, trial_stride=None, cond_cls=None, env_step=0,
                          threshold=0.0, n_bins=0, out=None):
        """switch_times over a population of devices (stg_switch_population): trial r (absolute) of condition g belongs to device
        r // trials_per_device, whose damping, Ms, K_u, volume and polarization are the condition's nominal ones (its class of
        set_params) times 1 + sigma[k, g] * clip(z_k, +- z_clip), z from the stream of the device's first trial at counter word
        var_step; the trial integrates with that device's own constants.  sigma float64 [5, G].  passage (None: n_tbins > 0) asks for
        the first-passage counts; without them the tuple is (n_switched, n_failed, hist) as switch_stats returns it, with them the six
        of switch_times.  dev_switched int64 [G, dev_stride] on the device, indexed by the absolute device id, is added to as well
        when given.  Everything else, `out` included, as switch_times.  Enqueues only."""
        passage = n_tbins > 0 if passage is None else bool(passage)
        (g, r, t0, stride, p), (m0, J, T, target, cond_cls), out = self._switch_args(
            m0, J, T, target, n_trials, trial0, trial_stride, cond_cls, (n_bins, n_tbins) if passage else (n_bins,), out)
        kj, tj, jk, kh, th, hk = self._wave_tables(wave, g) if wave is not None else (0, None, None, 0, None, None)
        sigma = self._dev(sigma, torch.float64, (_lib.STG_NVARY, g))
        n_sw, n_failed, hist, n_cr, n_ret, t_hist = tuple(out) + (() if passage else (None, None, None))
        dev_stride = 0
        if dev_switched is not None:
            if (not torch.is_tensor(dev_switched) or dev_switched.dtype != torch.int64 or dev_switched.dim() != 2 or dev_switched.shape[0] != g
                    or not dev_switched.is_contiguous() or not dev_switched.is_cuda):
                raise ValueError(f"dev_switched must be a contiguous int64 tensor [G = {g}, dev_stride] on {self.device}")
            dev_stride = int(dev_switched.shape[1])
        _lib.check(self.lib.stg_switch_population(self._ctx, g, r, t0, stride, p, _ptr(m0), _ptr(J), _ptr(T), int(watch_phase), kj, _ptr(tj),
                                                  _ptr(jk), kh, _ptr(th), _ptr(hk), _ptr(cond_cls), int(env_step), _ptr(target),
                                                  float(threshold), int(n_bins), _ptr(n_sw), _ptr(n_failed), _ptr(hist), int(n_tbins),
                                                  _ptr(n_cr), _ptr(n_ret), _ptr(t_hist), _ptr(sigma), float(z_clip), int(var_step),
                                                  int(trials_per_device), _ptr(dev_switched), dev_stride, self._stream()))
        self._keep += (tj, jk, th, hk, sigma)
        return out

    def switch_population_devices(self, n_cond, n_devices, sigma, dev0=0, trials_per_device=1, trial_stride=None, var_step=2 ** 31,
                                  z_clip=4.0, cond_cls=None, want_z=False):
        """The devices switch_population draws, made observable (stg_switch_population_devices): params float64 [5, G, D] -- damping,
        Ms, K_u, volume, polarization of devices dev0 ... dev0 + D - 1 of each of the G = n_cond conditions (NaN for a condition with
        a bad sigma column) -- and, with want_z, their six normals [6, G, D].  trial_stride None: (dev0 + D) * trials_per_device.
        Returns params, or (params, z).  Enqueues only."""
        g, d, q = int(n_cond), int(n_devices), int(trials_per_device)
        sigma = self._dev(sigma, torch.float64, (_lib.STG_NVARY, g))
        cond_cls = self._dev(cond_cls, torch.uint8, (g,))
        stride = (int(dev0) + d) * q if trial_stride is None else int(trial_stride)
        params = torch.empty((_lib.STG_NVARY, g, d), dtype=torch.float64, device=self.device)
        z = torch.empty((6, g, d), dtype=torch.float64, device=self.device) if want_z else None
        _lib.check(self.lib.stg_switch_population_devices(self._ctx, g, d, int(dev0), q, stride, int(var_step), float(z_clip), _ptr(sigma),
                                                          _ptr(cond_cls), _ptr(params), _ptr(z), self._stream()))
        self._keep = (sigma, cond_cls)
        return (params, z) if want_z else params

    def device_terms(self, m, J, volt):
        """Device-class formulas per env: (tau_dl [3,N], tau_fl [3,N], k_eff [N]) for m [3,N], J [N], volt [N]."""
        n, dev = self.n, self.device
        m = self._dev(m, torch.float64, (3, n))
        J = self._dev(J, torch.float64, (n,))
        volt = self._dev(volt, torch.float64, (n,))
        dl = torch.empty((3, n), dtype=torch.float64, device=dev)
        fl = torch.empty((3, n), dtype=torch.float64, device=dev)
        ke = torch.empty(n, dtype=torch.float64, device=dev)
        _lib.check(self.lib.stg_device_terms(self._ctx, _ptr(m), _ptr(J), _ptr(volt), _ptr(dl), _ptr(fl), _ptr(ke),
                                             self._stream()))
        self._keep = (m, J, volt)
        return dl, fl, ke

    def counters(self, reset=False):
        """On-device metrics: dict(env_steps, work_units, noop_steps).  Synchronises the device."""
        out = (C.c_uint64 * 4)()
        _lib.check(self.lib.stg_get_counters(self._ctx, out, int(bool(reset))))
        return {"env_steps": int(out[0]), "work_units": int(out[1]), "noop_steps": int(out[3])}

    PLACEMENT_CAP = 4096
    PLACEMENT_ENTRY = 4                   # STG_PLACEMENT_WORDS_PER_WAVE

    def placement(self, launches_back=0, raw=False):
        """Where the dispatcher put the wavefronts of a recent step launch and when each ran (stg_get_placement; 0 = the latest, up to
        31 back): dict(workgroups, waves_per_workgroup, waves_recorded, simds_used, integrating_per_simd (histogram {count: SIMDs}),
        simd_double_booked, span_us, simd_busy_frac, last_simd_alone_frac).
        `simd_double_booked` = SIMDs that held two or more INTEGRATING wavefronts of the launch -- for the launches scheduled for one
        integrating wavefront per SIMD (up to 65 536 envs; the wave-specialised pairs) it should be 0, and every such SIMD costs the
        launch the time of its two wavefronts back to back.  From the start / retire times: `span_us` = first start to last retire;
        `simd_busy_frac` = mean over the 1024 SIMDs of the share of that span during which the SIMD held at least one integrating
        wavefront; `last_simd_alone_frac` = share of the span left once 90 % of the SIMDs in use have retired their last integrating
        wavefront (the tail a makespan-bound launch ends with).  raw=True adds the arrays (`where`, `producer`, `t0_us`, `t1_us`, `work`, `slot` per recorded wavefront).
        Synchronises the device."""
        words = self.PLACEMENT_CAP * self.PLACEMENT_ENTRY
        out = (C.c_uint32 * words)()
        nwg, wpw = C.c_int32(), C.c_int32()
        n = self.lib.stg_get_placement(self._ctx, int(launches_back), out, words, C.byref(nwg), C.byref(wpw))
        if n < 0:
            _lib.check(n)
        e = np.frombuffer(out, dtype=np.uint32, count=n * self.PLACEMENT_ENTRY).reshape(n, self.PLACEMENT_ENTRY).copy()
        e = e[(e[:, 0] >> 31) == 1]
        w = e[:, 0]
        simd = (w & 0xFFFF) >> 4 & 3
        where = ((w >> 16 & 0xF).astype(np.int64) << 12) | ((w >> 8 & 0xFF).astype(np.int64) << 2) | simd      # (xcc, se/sh/cu, simd)
        prod = (w >> 20 & 1) == 1
        integ = where[~prod]
        _, cnt = np.unique(integ, return_counts=True)
        hist = {int(k): int(v) for k, v in zip(*np.unique(cnt, return_counts=True))}
        res = {"workgroups": int(nwg.value), "waves_per_workgroup": int(wpw.value), "waves_recorded": int(len(w)),
               "simds_used": int(len(np.unique(where))), "integrating_per_simd": hist,
               "simd_double_booked": int((cnt >= 2).sum())}
        # timeline (100 MHz ticks, 32-bit wrap-safe differences against the earliest start)
        ran = e[:, 2] != 0
        if ran.any():
            t0 = e[ran, 1].astype(np.int64)
            base = int(t0.min()) if (int(t0.max()) - int(t0.min())) < (1 << 31) else int(t0[0])
            s0 = ((e[:, 1].astype(np.int64) - base) & 0xFFFFFFFF).astype(np.float64) * 0.01
            s1 = ((e[:, 2].astype(np.int64) - base) & 0xFFFFFFFF).astype(np.float64) * 0.01
            s0, s1 = np.where(ran, s0, 0.0), np.where(ran, s1, 0.0)
            sel = ran & ~prod
            span = float(s1[sel].max() - s0[sel].min()) if sel.any() else 0.0
            busy = {}
            for k in np.unique(where[sel]):           # union of the integrating wavefronts' intervals per SIMD
                iv = sorted(zip(s0[sel & (where == k)], s1[sel & (where == k)]))
                tot, cur_a, cur_b = 0.0, iv[0][0], iv[0][1]
                for a_, b_ in iv[1:]:
                    if a_ > cur_b:
                        tot += cur_b - cur_a
                        cur_a, cur_b = a_, b_
                    else:
                        cur_b = max(cur_b, b_)
                busy[int(k)] = (tot + cur_b - cur_a, cur_b)
            n_simd = 1024
            ends = np.sort(np.array([v[1] for v in busy.values()]))
            res["span_us"] = round(span, 2)
            res["simd_busy_frac"] = round(sum(v[0] for v in busy.values()) / (n_simd * span), 4) if span > 0 else None
            # from the moment 90 % of the SIMDs in use have retired their last integrating wavefront the launch runs on a tenth of them
            t90 = float(ends[max(int(0.9 * len(ends)) - 1, 0)])
            res["last_simd_alone_frac"] = round(max(0.0, float(ends[-1]) - t90) / span, 4) if span > 0 else None
            if raw:
                res.update(where=where, producer=prod, t0_us=s0, t1_us=s1, work=e[:, 3].astype(np.int64), slot=(w & 0xF).astype(np.int64))
        return res

    def thermal_normals(self, env_step=0, call0=0, n_calls=1):
        z = torch.empty((n_calls, 3, self.n), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.stg_thermal_normals(self._ctx, int(env_step), int(call0), int(n_calls), _ptr(z),
                                                self._stream()))
        return z

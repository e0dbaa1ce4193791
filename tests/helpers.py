"""Test-only helpers.  `OracleBackend` offers HipBackend's interface on top of the CPU oracle so that

  * `-m gpu` parity tests can run the SAME host code (SpinTorqueVecEnv / SpinTorqueEnv) once over the HIP
    library and once over the oracle and compare the outputs, and
  * the world_size-2 gloo tests can exercise sharding and the (obs, reward, done) gather without a GPU.

It lives under tests/ because only tests may touch oracle/ (the product never does).
"""
import ctypes as C

import numpy as np
import torch

import oracle

RESET_KEY_XOR = 0x9E3779B97F4A7C15


def oracle_noise_model(name):
    """the env's noise_model name -> the oracle's value, through the library's own table; a name the table lacks raises"""
    from spin_torque_gym_amd._lib import NOISE_MODELS
    if name not in NOISE_MODELS:
        raise ValueError(f"noise_model {name!r}: the oracle knows {list(NOISE_MODELS)}")
    return NOISE_MODELS[name]


def oracle_config(cfg):
    """spin_torque_gym_amd.backend.EnvConfig -> oracle.Config"""
    return oracle.make_config(solver=cfg.solver, thermal=cfg.include_thermal_fluctuations, temperature=cfg.temperature,
                              gamma=cfg.gamma, max_step=cfg.max_step, rtol=cfg.rtol, atol=cfg.atol,
                              max_steps=cfg.max_steps, max_current=cfg.max_current, max_duration=cfg.max_duration,
                              success_threshold=cfg.success_threshold, energy_penalty_weight=cfg.energy_penalty_weight,
                              seed=cfg.seed, max_attempts=cfg.max_attempts,
                              torque_model=int(getattr(cfg, "torque_model", "reference") == "device"),
                              noise_model=oracle_noise_model(getattr(cfg, "noise_model", "white")),
                              noise_corr_time=getattr(cfg, "correlation_time", 1e-12))


def oracle_params(table):
    """list of _lib.StgDeviceParams -> (oracle.Params * k); the two records have the same field layout."""
    arr = (oracle.Params * len(table))()
    assert C.sizeof(oracle.Params) == C.sizeof(type(table[0]))
    for i, p in enumerate(table):
        C.memmove(C.byref(arr[i]), C.byref(p), C.sizeof(oracle.Params))
    return arr


def _philox(ctr, key):
    L = oracle.lib()
    L.stgo_philox4x32_10.argtypes = [C.POINTER(C.c_uint32)] * 3
    L.stgo_philox4x32_10.restype = None
    c = (C.c_uint32 * 4)(*ctr)
    k = (C.c_uint32 * 2)(*key)
    out = (C.c_uint32 * 4)()
    L.stgo_philox4x32_10(c, k, out)
    return [int(x) for x in out]


def device_reset_draw(seed, env_id, rng_step, targets):
    """The kernels' device-side reset draw (csrc/spintorque_hip.hip: device_reset_draw) through its oracle restatement."""
    L = oracle.lib()
    L.stgo_reset_draw.restype = None
    L.stgo_reset_draw.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    z = np.zeros(3)
    idx = C.c_int(0)
    L.stgo_reset_draw(seed & 0xFFFFFFFFFFFFFFFF, env_id, rng_step, len(targets), z.ctypes.data_as(C.POINTER(C.c_double)),
                      C.byref(idx))
    n = np.sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2])
    m = np.array([0.0, 0.0, 1.0]) if n < 1e-12 else z / n
    return m, np.array(targets[idx.value], dtype=np.float64)


class OracleBackend:
    """HipBackend's interface, computed by the CPU oracle.  Tensors are CPU torch tensors, component-major."""

    def __init__(self, n_envs, cfg, device_index=0, env_id0=0):
        self.n = int(n_envs)
        self.cfg = cfg
        self.ocfg = oracle_config(cfg)
        self.env_id0 = int(env_id0)
        self.device = torch.device("cpu")
        self.states = (oracle.EnvState * self.n)()
        self.done = np.zeros(self.n, dtype=np.uint8)
        self.params = None
        self.cls = None
        n = self.n
        from spin_torque_gym_amd.backend import alloc_step_outputs
        self.records_layout = getattr(cfg, "out_layout", "soa") == "records"
        self.packed, self.obs, self.reward, self.terminated, self.truncated = alloc_step_outputs(
            n, self.device, getattr(cfg, "out_layout", "soa"))
        self.reward64 = torch.zeros(n, dtype=torch.float64)
        self.energy = torch.zeros(n, dtype=torch.float64)
        self.status = torch.zeros(n, dtype=torch.uint8)
        self.final_obs = torch.zeros((12, n), dtype=torch.float32)
        self._counters = {"env_steps": 0, "work_units": 0, "noop_steps": 0}

    def close(self):
        pass

    def counters(self, reset=False):
        c = dict(self._counters)
        if reset:
            self._counters = {"env_steps": 0, "work_units": 0, "noop_steps": 0}
        return c

    def set_params(self, table, cls=None):
        self.params = oracle_params(table)
        self.n_classes = len(table)
        self.cls = None if (cls is None or len(table) == 1) else np.ascontiguousarray(torch.as_tensor(cls).cpu().numpy(), dtype=np.uint8)

    def _p(self, i):
        return self.params[int(self.cls[i]) if self.cls is not None else 0]

    def _obs_of(self, i, out):
        o = (C.c_float * 12)()
        oracle.lib().stgo_observation.restype = None
        oracle.lib().stgo_observation.argtypes = [C.POINTER(oracle.EnvState), C.POINTER(oracle.Params),
                                                  C.POINTER(oracle.Config), C.POINTER(C.c_float)]
        oracle.lib().stgo_observation(C.byref(self.states[i]), C.byref(self._p(i)), C.byref(self.ocfg), o)
        out[:, i] = torch.tensor(list(o), dtype=torch.float32)

    def reset(self, mask=None, init_m=None, target=None, seed=0):
        mask = None if mask is None else torch.as_tensor(mask).cpu().numpy().astype(bool)
        init_m = None if init_m is None else torch.as_tensor(init_m).cpu().numpy().astype(np.float64)
        target = None if target is None else torch.as_tensor(target).cpu().numpy().astype(np.float64)
        targets = np.asarray(self.cfg.target_states, dtype=np.float64).reshape(-1, 3)
        for i in range(self.n):
            s = self.states[i]
            if mask is not None and not mask[i]:
                s.last_action[:] = [0.0, 0.0]
                self._obs_of(i, self.obs)
                continue
            m, t = device_reset_draw(int(seed) & 0xFFFFFFFFFFFFFFFF, self.env_id0 + i, s.rng_step, targets)
            if init_m is not None:
                v = init_m[:, i]
                m = v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            if target is not None:
                v = target[:, i]
                t = v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            s.m[:] = list(m)
            s.target[:] = list(t)
            s.total_energy = 0.0
            s.step_count = 0
            s.last_action[:] = [0.0, 0.0]
            self.done[i] = 0
            self._obs_of(i, self.obs)
        return self.obs

    def _step_once(self, a, autoreset, outs, final=None):
        obs, reward, reward64, energy, term, trunc, status = outs
        final = self.final_obs if final is None else final
        a = np.ascontiguousarray(a.T)          # [N,2]
        f64 = a.dtype == np.float64
        targets = np.asarray(self.cfg.target_states, dtype=np.float64).reshape(-1, 3)
        # float64 actions: the safety clamp runs in float64 (monitoring.py:304-313 on a float64 array), the oracle's float64 entry
        step_batch = oracle.env_step_batch_f64 if f64 else oracle.env_step_batch
        outs_c = step_batch(self.states, a if f64 else a.astype(np.float32), self.params, self.cls, self.ocfg, env_id0=self.env_id0)
        for i in range(self.n):
            o = outs_c[i]
            obs[:, i] = torch.tensor(list(o.obs), dtype=torch.float32)
            reward[i] = float(np.float32(o.reward))
            reward64[i] = o.reward
            energy[i] = o.energy
            term[i] = o.terminated
            trunc[i] = o.truncated
            status[i] = o.status
            self._counters["env_steps"] += 1
            self._counters["work_units"] += int(o.n_sub)
            self._counters["noop_steps"] += int(o.status == 1)
            self.done[i] = 1 if (o.terminated or o.truncated) else 0
            if autoreset and self.done[i]:
                # same-step auto-reset (csrc/spintorque_hip.hip): terminal obs -> final_obs, redraw, obs of the new episode
                s = self.states[i]
                final[:, i] = obs[:, i]
                m, t = device_reset_draw(self.cfg.seed, self.env_id0 + i, s.rng_step, targets)
                s.m[:] = list(m)
                s.target[:] = list(t)
                s.total_energy = 0.0
                s.step_count = 0
                s.last_action[:] = [0.0, 0.0]
                self.done[i] = 0
                self._obs_of(i, obs)

    def step(self, actions, autoreset=False, out=None):
        a = torch.as_tensor(actions).cpu().numpy()
        obs, reward, term, trunc = self.obs, self.reward, self.terminated, self.truncated
        if out is not None:                      # 'records' layout: the caller's record array (double buffering)
            from spin_torque_gym_amd.backend import record_views
            assert self.records_layout and tuple(out.shape) == (self.n, 56)
            o, reward, term, trunc, st_b = record_views(out)
            obs = o.t()
        self._step_once(a, autoreset, (obs, reward, self.reward64, self.energy, term, trunc, self.status))
        if self.records_layout:                  # the record's status byte
            (out if out is not None else self.packed)[:, 54] = self.status
        return obs, reward, self.reward64, term, trunc, self.status

    def step_many(self, actions, out_every=True, autoreset=False):
        a = torch.as_tensor(actions).cpu().numpy()
        K, n = a.shape[0], self.n
        ko = K if out_every else 1
        obs = torch.zeros((ko, 12, n), dtype=torch.float32)
        reward = torch.zeros((ko, n), dtype=torch.float32)
        reward64 = torch.zeros((ko, n), dtype=torch.float64)
        self.energy_many = torch.zeros((ko, n), dtype=torch.float64)
        term = torch.zeros((ko, n), dtype=torch.uint8)
        trunc = torch.zeros((ko, n), dtype=torch.uint8)
        status = torch.zeros((ko, n), dtype=torch.uint8)
        self.final_obs_many = torch.zeros((ko, 12, n), dtype=torch.float32)
        for k in range(K):
            j = k if out_every else 0
            self._step_once(a[k], autoreset, (obs[j], reward[j], reward64[j], self.energy_many[j], term[j], trunc[j], status[j]),
                            final=self.final_obs_many[j])
        return obs, reward, reward64, term, trunc, status

    def get_state(self):
        n = self.n
        m = np.array([list(self.states[i].m) for i in range(n)]).T
        t = np.array([list(self.states[i].target) for i in range(n)]).T
        return dict(m=torch.from_numpy(np.ascontiguousarray(m)), target=torch.from_numpy(np.ascontiguousarray(t)),
                    total_energy=torch.tensor([self.states[i].total_energy for i in range(n)], dtype=torch.float64),
                    step_count=torch.tensor([self.states[i].step_count for i in range(n)], dtype=torch.int32),
                    rng_step=torch.tensor([self.states[i].rng_step for i in range(n)], dtype=torch.int64).to(torch.int32),
                    done=torch.from_numpy(self.done.copy()))

    def set_state(self, st):
        for i in range(self.n):
            s = self.states[i]
            if st.get("m") is not None:
                s.m[:] = [float(x) for x in st["m"][:, i]]
            if st.get("target") is not None:
                s.target[:] = [float(x) for x in st["target"][:, i]]
            if st.get("total_energy") is not None:
                s.total_energy = float(st["total_energy"][i])
            if st.get("step_count") is not None:
                s.step_count = int(st["step_count"][i])
            if st.get("rng_step") is not None:
                s.rng_step = int(st["rng_step"][i]) & 0xFFFFFFFF
            if st.get("done") is not None:
                self.done[i] = int(st["done"][i])

    def solve(self, m0, J, T, env_step=0, traj_cap=0, want_energy=False, wave=None):
        """wave: the dict HipBackend.solve takes -- current=(tj [K,N], jk [K,N]) | None, field=(th [K,N], hk [K,3,N]) | None --, for
        solver='rk45' only (oracle.llgs_solve_wave; J may be None with a current table).  Fixed-step waveforms stay with
        tests/waveform_ref.py: the C oracle does not integrate them."""
        m0 = torch.as_tensor(m0).cpu().numpy().astype(np.float64)
        J = np.zeros(self.n) if J is None else torch.as_tensor(J).cpu().numpy().astype(np.float64)
        cur = fld = None
        if wave is not None:
            if self.cfg.solver != "rk45":
                raise ValueError("OracleBackend.solve(wave=) is RK45 only; fixed-step waveforms: tests/waveform_ref.py")
            host = lambda a: torch.as_tensor(a).cpu().numpy().astype(np.float64)          # noqa: E731
            cur = None if wave.get("current") is None else tuple(host(a) for a in wave["current"])
            fld = None if wave.get("field") is None else tuple(host(a) for a in wave["field"])
        T = torch.as_tensor(T).cpu().numpy().astype(np.float64)
        n = self.n
        mf = np.zeros((3, n))
        npts = np.zeros(n, dtype=np.int32)
        succ = np.zeros(n, dtype=np.uint8)
        tt = np.zeros((max(traj_cap, 1), n))
        tm = np.zeros((max(traj_cap, 1), 3, n))
        te = np.zeros((max(traj_cap, 1), n))
        tq = np.zeros((max(traj_cap, 1), n))
        for i in range(n):
            p = self._p(i)
            if self.cfg.solver == "rk45":
                if wave is not None:
                    r = oracle.llgs_solve_wave(m0[:, i], T[i], p, self.ocfg, J[i], None if cur is None else (cur[0][:, i], cur[1][:, i]),
                                               None if fld is None else (fld[0][:, i], fld[1][:, :, i]), self.env_id0 + i, env_step,
                                               cap=max(traj_cap, 1))
                else:
                    r = oracle.llgs_solve(m0[:, i], T[i], p, self.ocfg, J[i], self.env_id0 + i, env_step, cap=max(traj_cap, 1))
                mf[:, i] = r["m_final"] if r["success"] else m0[:, i]
                npts[i] = max(r["n_points"] - 1, 0)           # (a bad table: no point at all)
                k = min(len(r["t"]), traj_cap)
                tt[:k, i], tm[:k, :, i], te[:k, i], tq[:k, i] = r["t"][:k], r["m"][:k], r["energy"][:k], r["torques"][:k]
            else:
                r = oracle.simple_solve(m0[:, i], T[i], p, self.ocfg, J[i], self.env_id0 + i, env_step, want_traj=traj_cap > 0)
                mf[:, i] = r["m_final"]
                npts[i] = r["n_steps"]
                if traj_cap > 0 and "m" in r:
                    k = min(len(r["m"]), traj_cap)
                    tm[:k, :, i] = r["m"][:k]
                    dt = T[i] / max(r["n_steps"], 1)
                    tt[:k, i] = np.arange(k) * dt
                    if k == r["n_steps"] + 1:
                        tt[k - 1, i] = T[i]
            succ[i] = r["success"]
        out = dict(m_final=torch.from_numpy(mf), n_points=torch.from_numpy(npts), success=torch.from_numpy(succ))
        if traj_cap > 0:
            out.update(t=torch.from_numpy(tt), m=torch.from_numpy(tm), energy=torch.from_numpy(te) if want_energy else None,
                       torques=torch.from_numpy(tq) if want_energy else None)
        return out


def make_states(n, m, target):
    st = (oracle.EnvState * n)()
    for i in range(n):
        st[i].m[:] = [float(x) for x in m[i]]
        st[i].target[:] = [float(x) for x in target[i]]
    return st


def unit_rows(rng, n):
    v = rng.normal(0, 1, (n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


class OracleArrayBackend:
    """HipArrayBackend's interface on the CPU oracle (test seam of SpinTorqueArrayVecEnv)."""

    def __init__(self, n_arrays, cfg, dev_params, coupling, device_index=0, env_id0=0):
        self.n, self.cfg = int(n_arrays), cfg
        self.n_dev = cfg.rows * cfg.cols
        self.obs_dim = self.n_dev * 6 + (4 if cfg.obs_mode == 1 else 0)
        self.device = torch.device("cpu")
        self.ocfg = oracle.ArrayConfig()
        C.memmove(C.byref(self.ocfg), C.byref(cfg), C.sizeof(oracle.ArrayConfig))
        self.p = oracle_params([dev_params])[0]
        self.coupling = np.zeros((self.n_dev, self.n_dev)) if coupling is None else np.ascontiguousarray(coupling, dtype=np.float64)
        self.states = [None] * self.n
        self.target = None
        self.env_id0 = int(env_id0)
        self.resets = np.zeros(self.n, dtype=np.uint32)      # per array: how many random resets it has had
        n = self.n
        self.obs = torch.zeros((self.obs_dim, n), dtype=torch.float32)
        self.reward = torch.zeros(n, dtype=torch.float32)
        self.reward64 = torch.zeros(n, dtype=torch.float64)
        self.energy = torch.zeros(n, dtype=torch.float64)
        self.terminated = torch.zeros(n, dtype=torch.uint8)
        self.truncated = torch.zeros(n, dtype=torch.uint8)

    def close(self):
        pass

    def reset(self, mask=None, init_pattern=None, target=None, seed=0):
        """stg_array_reset: selected arrays take `init_pattern` or, without one, the device-side random draw of
        (seed, env_id0 + i, this array's count of earlier random resets); `target`, else the target they have, else the
        checkerboard; energy and step count return to zero.  The observation of EVERY array is returned."""
        ip = None if init_pattern is None else torch.as_tensor(init_pattern).cpu().numpy()
        tg_in = None if target is None else torch.as_tensor(target).cpu().numpy()
        mask = None if mask is None else torch.as_tensor(mask).cpu().numpy().astype(bool)
        for i in range(self.n):
            if mask is None or mask[i]:
                if ip is not None:
                    pat = ip[:, i].reshape(-1, 3).copy()      # (a column of an N = 1 batch is contiguous: never alias the caller's array)
                else:
                    pat, _ = oracle.array_reset_draw(int(seed), self.env_id0 + i, int(self.resets[i]), self.n_dev)
                    self.resets[i] += 1
                if tg_in is not None:
                    tg = tg_in[:, i].reshape(-1, 3).copy()
                elif self.states[i] is not None:
                    tg = self.states[i].target
                else:                                  # checkerboard of +-z over (row, column)
                    r, c = np.divmod(np.arange(self.n_dev), self.cfg.cols)
                    tg = np.zeros((self.n_dev, 3))
                    tg[:, 2] = np.where((r + c) % 2 == 0, 1.0, -1.0)
                self.states[i] = oracle.ArrayEnvState(pat, tg)
            self.obs[:, i] = torch.from_numpy(oracle.array_observation(self.states[i], self.ocfg))
        return self.obs

    def step(self, actions):
        a = torch.as_tensor(actions).numpy().astype(np.float32)
        for i in range(self.n):
            obs, r, te, tr, en = oracle.array_step(self.states[i], a[:, i], self.p, self.ocfg, self.coupling)
            self.obs[:, i] = torch.from_numpy(obs)
            self.reward[i] = float(np.float32(r)); self.reward64[i] = r; self.energy[i] = en
            self.terminated[i] = int(te); self.truncated[i] = int(tr)
        return self.obs, self.reward, self.reward64, self.terminated, self.truncated

    def get_state(self):
        return dict(pattern=torch.from_numpy(np.stack([s.pattern.reshape(-1) for s in self.states], axis=1).copy()),
                    target=torch.from_numpy(np.stack([s.target.reshape(-1) for s in self.states], axis=1).copy()),
                    total_energy=torch.tensor([s.total_energy.value for s in self.states], dtype=torch.float64),
                    step_count=torch.tensor([s.step_count.value for s in self.states], dtype=torch.int32))


# ------------------------------------------------------------------------------------------------
# write-footprint guards (tests/test_gpu_write_footprint.py, tests/test_footprint_checker.py)
# ------------------------------------------------------------------------------------------------
# A caller-owned output array is handed to the C-ABI as the interior of a larger allocation that is filled with a sentinel bit
# pattern: a store outside the logical array lands in a guard (and fails an assertion instead of faulting), an element that is never
# written keeps the sentinel.  The patterns are quiet NaNs with a recognisable payload (no kernel computes them), 0xA5 bytes (flags are
# <= 1, status <= 4) and 0xA5A5A5A5 words; they are compared as integers, never with isnan.
GUARD_TILE = 4096                      # the sorted schedule's slot space is whole tiles of this many envs
GUARD_ALIGN = 256                      # bytes: the interior starts on this boundary, like an allocation of its own
_SENTINEL = {torch.float32: (torch.int32, 0x7FC5A5A5), torch.float64: (torch.int64, 0x7FF8A5A5A5A5A5A5),
             torch.uint8: (torch.uint8, 0xA5), torch.int32: (torch.int32, 0xA5A5A5A5 - (1 << 32))}


def sentinel_bits(dtype):
    """(integer dtype of the same width, the sentinel as a value of that dtype)"""
    return _SENTINEL[dtype]


class Guarded:
    """A sentinel-filled allocation around one logical array of `shape` whose axis `n_axis` is the env axis (length N, or M).

    `interior` is the contiguous view whose data_ptr() goes to the library.  Multi-row arrays are ONE flat block with the real row
    stride between a front and a back guard (a stride mix-up then shows as a wrong value or an unwritten element):
      back guard  >= the elements the array would have with N rounded up to the next multiple of 4096, plus one more row,
      front guard >= one row (the block along the env axis: N x the trailing dimensions), the interior 256-byte aligned.
    `min_back`: a larger back guard in elements (a capped array whose uncapped form must still fit inside the allocation)."""

    def __init__(self, name, shape, dtype, n_axis=-1, device="cuda", min_back=0):
        self.name, self.dtype = name, dtype
        self.bits_dtype, self.sentinel = sentinel_bits(dtype)
        shape = tuple(int(s) for s in shape)
        n_axis = n_axis % len(shape)
        n = shape[n_axis]
        numel = int(np.prod(shape))
        row = n * int(np.prod(shape[n_axis + 1:], dtype=np.int64))
        n_up = -(-n // GUARD_TILE) * GUARD_TILE
        item = torch.empty(0, dtype=dtype).element_size()
        per_line = GUARD_ALIGN // item
        self.back = max(numel // n * n_up + row, int(min_back))
        raw_numel = row + 2 * per_line + numel + self.back
        self.raw = torch.empty(raw_numel, dtype=self.bits_dtype, device=device)
        self.raw.fill_(self.sentinel)
        lo = row                       # first element at or behind one row whose address is a multiple of GUARD_ALIGN
        while (self.raw.data_ptr() + lo * item) % GUARD_ALIGN:
            lo += 1
        assert lo < row + 2 * per_line
        self.front, self.numel, self.shape = lo, numel, shape
        self.interior = self.raw[lo:lo + numel].view(dtype).view(shape)
        assert self.interior.is_contiguous() and self.interior.data_ptr() % GUARD_ALIGN == 0

    def bits(self):
        """the interior as integers (same shape)"""
        return self.raw[self.front:self.front + self.numel].view(self.shape)

    def untouched(self):
        """bool tensor of the interior's shape: the element still holds the sentinel"""
        return self.bits() == self.sentinel

    def check_guards(self):
        """Asserts that every guard element, in front of the interior and behind it, still holds the sentinel."""
        front, back = self.raw[:self.front], self.raw[self.front + self.numel:]
        for where, g in (("front", front), ("back", back)):
            bad = (g != self.sentinel).nonzero()
            assert bad.numel() == 0, f"{self.name}: {where} guard overwritten at {bad.reshape(-1)[:8].tolist()} ({bad.shape[0]} elements, guard of {g.numel()})"

    def check(self, written=True):
        """check_guards(), and the interior elements selected by `written` (True: all, False: none, or a bool tensor broadcastable to
        the interior's shape) do NOT hold the sentinel while every other interior element still does.  Returns the interior."""
        self.check_guards()
        un = self.untouched()
        want = torch.as_tensor(written, dtype=torch.bool, device=un.device).expand(un.shape) if not isinstance(written, bool) \
            else torch.full(un.shape, written, dtype=torch.bool, device=un.device)
        miss = (un & want).nonzero()
        assert miss.numel() == 0, f"{self.name}: {miss.shape[0]} elements were never written, first at {miss[:4].tolist()}"
        extra = (~un & ~want).nonzero()
        assert extra.numel() == 0, f"{self.name}: {extra.shape[0]} elements that must stay untouched were written, first at {extra[:4].tolist()}"
        return self.interior

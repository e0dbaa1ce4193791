#!/usr/bin/env python3
"""What shaped pulses cost on the env step path: the same non-thermal RK4 step of 65 536 envs with 1 ns pulses through stg_step
(rectangular pulse, sorted lane schedule: the yardstick -- its kernels are byte for byte the parent commit's,
profiles/step_wave_existing_kernels_unchanged.txt), through stg_step_wave with a 4-knot trapezoid current plus a 2-knot constant field, and
through stg_step_wave without tables (stg_step's integrator in the one-env-per-lane identity schedule).  Every repetition starts from the
same state (restored outside the timed region); the three forms are timed alternately in one process with device events around each
call, after a warm-up of all; the median, the spread and the ratios of the medians are printed, and one JSON line at the end.
usage (GPU box): python3 tools/step_wave_ab.py [reps=9] [uniform|mixed]     (mixed: durations U[0.1, 1] ns instead of 1 ns)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spin-torque-rl-gym_amd"))
import bench  # noqa: E402
import spin_torque_gym_amd as stg  # noqa: E402
from spin_torque_gym_amd.backend import EnvConfig, HipBackend  # noqa: E402
from spin_torque_gym_amd.envs import parse_actions_fp64, pulse_tables  # noqa: E402
from spin_torque_gym_amd.physics import PiecewiseLinear  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def ab(n, reps, mixed):
    solver = "rk4"
    b = HipBackend(n, EnvConfig(solver=solver, include_thermal_fluctuations=False))
    b.set_params([stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", bench.stt_params(bench.volume_for(solver))))])
    rng = np.random.default_rng(3)
    v = rng.normal(0, 1, (3, n))
    tgt = np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0)[None, :] * np.array([[0.0], [0.0], [1.0]])
    b.reset(init_m=torch.tensor(v / np.linalg.norm(v, axis=0, keepdims=True)), target=torch.tensor(tgt))
    torch.cuda.synchronize()
    start = {k: t.clone() for k, t in b.get_state().items()}
    dur = rng.uniform(1e-10, 1e-9, n) if mixed else np.full(n, 1e-9)
    act = torch.tensor(np.stack([rng.uniform(-2e6, 2e6, n), dur]), dtype=torch.float32, device=b.device)
    J, T = parse_actions_fp64(act, b.cfg.max_current, b.cfg.max_duration)
    # a trapezoid of the env's own amplitude and duration (rise over the first tenth, fall over the last fifth), a constant field
    cur = pulse_tables(PiecewiseLinear([0.0, 0.1, 0.8, 1.0], [0.0, 1.0, 1.0, 0.0]), J, T)
    th = torch.tensor([0.0, 5e-9], dtype=torch.float64, device=b.device)[:, None].expand(2, n).contiguous()
    hk = torch.tensor([2e4, 0.0, -1e4], dtype=torch.float64, device=b.device)[None, :, None].expand(2, 3, n).contiguous()
    forms = {"stg_step": lambda: b.step(act),
             "stg_step_wave": lambda: b.step_wave(act, {"current": cur, "field": (th, hk)}),
             "stg_step_wave_no_tables": lambda: b.step_wave(act, {"current": None, "field": None})}
    work = {}
    for name, fn in forms.items():           # warm-up: code objects loaded, allocator primed
        for _ in range(2):
            b.set_state(start)
            b.counters(reset=True)
            timed(fn)
        c = b.counters()
        assert c["noop_steps"] == 0, (name, c)
        work[name] = c["work_units"] / n
    ms = {name: [] for name in forms}
    for _ in range(reps):                    # alternate the forms
        for name, fn in forms.items():
            b.set_state(start)
            torch.cuda.synchronize()
            ms[name].append(timed(fn))
    b.close()
    res = {"solver": solver, "n": n, "reps": reps, "durations": "U[0.1, 1] ns" if mixed else "1 ns"}
    for name in forms:
        a = np.array(ms[name])
        res[name] = {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max()), "sub_steps_per_env": work[name],
                     "env_steps_per_s": n / (float(np.median(a)) * 1e-3)}
        print(f"{solver} n={n} {name:24s}: median {np.median(a):8.3f} ms (min {a.min():.3f}, max {a.max():.3f}), "
              f"{work[name]:.0f} sub-steps per env, {res[name]['env_steps_per_s']:.3e} env-steps/s", flush=True)
    for name in ("stg_step_wave", "stg_step_wave_no_tables"):
        res["ratio_" + name] = res[name]["median_ms"] / res["stg_step"]["median_ms"]
        print(f"{solver} n={n}: {name} / stg_step = {res['ratio_' + name]:.2f}", flush=True)
    return res


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    assert torch.cuda.is_available(), "needs the GPU"
    print(json.dumps(ab(65536, reps, len(sys.argv) > 2 and sys.argv[2] == "mixed")))

#!/usr/bin/env python3
"""What a piecewise-linear waveform costs on the solve path: the same non-thermal 1 ns problems through stg_solve (rectangular pulse:
the yardstick) and through stg_solve_wave with a 5-knot trapezoid current plus a 2-knot constant field, RK4 at 65 536 problems and
RK45 at 8 192.  The two forms are timed alternately in one process with device events around each solve (which is one kernel), after a
warm-up of both; the median, the spread and the ratio of the medians are printed, and one JSON line at the end.
usage (GPU box): python3 tools/waveform_ab.py [reps=7]"""
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


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def ab(solver, n, reps):
    vol = bench.volume_for(solver)
    b = HipBackend(n, EnvConfig(solver=solver, include_thermal_fluctuations=False))
    b.set_params([stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", bench.stt_params(vol)))])
    rng = np.random.default_rng(3)
    v = rng.normal(0, 1, (3, n))
    m0 = torch.tensor(v / np.linalg.norm(v, axis=0, keepdims=True), device=b.device)
    J = torch.tensor(rng.uniform(-2e6, 2e6, n), device=b.device)
    T = torch.full((n,), 1e-9, dtype=torch.float64, device=b.device)
    # per-problem tables: a trapezoid of the problem's own amplitude (0.1 ns rise, plateau, 0.2 ns fall, ending behind T), a constant field
    tj = torch.tensor([0.0, 1e-10, 7e-10, 9e-10, 1.2e-9], dtype=torch.float64, device=b.device)[:, None].expand(5, n).contiguous()
    jk = torch.stack([0 * J, J, J, -0.5 * J, 0 * J]).contiguous()
    th = torch.tensor([0.0, 1e-9], dtype=torch.float64, device=b.device)[:, None].expand(2, n).contiguous()
    hk = torch.tensor([2e4, 0.0, -1e4], dtype=torch.float64, device=b.device)[None, :, None].expand(2, 3, n).contiguous()
    wave = {"current": (tj, jk), "field": (th, hk)}
    forms = {"stg_solve": lambda: b.solve(m0, J, T), "stg_solve_wave": lambda: b.solve(m0, None, T, wave=wave)}
    work = {}
    for name, fn in forms.items():           # warm-up: code objects loaded, allocator primed
        for _ in range(2):
            _, out = timed(fn)
        assert bool(out["success"].all()), name
        work[name] = float(out["n_points"].double().mean())
    ms = {name: [] for name in forms}
    for _ in range(reps):                    # alternate the two forms
        for name, fn in forms.items():
            ms[name].append(timed(fn)[0])
    b.close()
    res = {"solver": solver, "n": n, "reps": reps}
    for name in forms:
        a = np.array(ms[name])
        res[name] = {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max()), "work_per_problem": work[name],
                     "solves_per_s": n / (float(np.median(a)) * 1e-3)}
        print(f"{solver} n={n} {name:15s}: median {np.median(a):8.3f} ms (min {a.min():.3f}, max {a.max():.3f}), "
              f"{work[name]:.0f} sub-steps / accepted points per problem, {res[name]['solves_per_s']:.3e} solves/s", flush=True)
    res["ratio"] = res["stg_solve_wave"]["median_ms"] / res["stg_solve"]["median_ms"]
    print(f"{solver} n={n}: stg_solve_wave / stg_solve = {res['ratio']:.2f}", flush=True)
    return res


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    assert torch.cuda.is_available(), "needs the GPU"
    out = [ab("rk4", 65536, reps), ab("rk45", 8192, reps)]
    print(json.dumps(out))

#!/usr/bin/env python3
"""What fusing buys under a shaped drive: K = 16 env steps of 65 536 envs (RK4, thermal field off, 1 ns pulses, a 4-knot trapezoid pulse
shape plus a 2-knot constant field) in these forms:

  (a) step x K ........... K calls of env.step(): stg_step_wave, per step the host builds the [K,N] current table with torch elementwise
                           kernels and the step kernel reads its tables back from HBM (the baseline: this path is the parent commit's,
                           profiles/step_shaped_existing_kernels_unchanged.txt);
  (b) step_many(K) ....... one stg_step_shaped launch of K steps: shape in LDS, state in registers between the steps;
  (c) step_many(1) x K ... K stg_step_shaped launches of one step: no tables, no fusing -- separates the table traffic from the fusing;
  (d) step_wave x K ...... K HipBackend.step_wave launches on tables built beforehand, outside the timed window: the kernel of (a) alone;
  (e), (f) ............... (b) and (c) through HipBackend.step_shaped_many, without the env's wrapper: the kernels of (b) and (c) alone.
  The wrapper of SpinTorqueVecEnv (the same in step, step_many and step_ids) converts the flag bytes to bool on the way out: two torch
  kernels over strided views per call, timed here by themselves ("flags_to_bool") because at this size they are not small.

All forms compute the same bits (checked here on the final state before anything is timed).  Every repetition starts from the same
state, restored outside the timed region; the forms are timed alternately in one process after a warm-up of all, each with a host clock
around work that ends in a device synchronise (the host work per step is part of what (a) costs) and with device events around the same
window; medians, spreads and ratios are printed, and one JSON line at the end.
usage (GPU box): python3 tools/step_shaped_ab.py [reps=7] [uniform|mixed] [n=65536] [K=16]     (mixed: durations U[0.1, 1] ns)"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spin-torque-rl-gym_amd"))
import bench  # noqa: E402
import spin_torque_gym_amd as stg  # noqa: E402
from spin_torque_gym_amd.physics import PiecewiseLinear  # noqa: E402


def timed(fn):
    """(host wall ms around fn + synchronise, device-event ms around fn)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def ab(n, K, reps, mixed):
    solver = "rk4"
    env = stg.SpinTorqueVecEnv(n, device_params=bench.stt_params(bench.volume_for(solver)), solver=solver, include_thermal_fluctuations=False,
                               seed=3, out_layout="records", pulse_shape=PiecewiseLinear([0.0, 0.1, 0.8, 1.0], [0.0, 1.0, 1.0, 0.0]),
                               applied_field=[2e4, 0.0, -1e4])
    env.reset(seed=3)
    b = env.backend
    torch.cuda.synchronize()
    start = {k: t.clone() for k, t in b.get_state().items()}
    rng = np.random.default_rng(3)
    dur = rng.uniform(1e-10, 1e-9, (K, n)) if mixed else np.full((K, n), 1e-9)
    act = torch.tensor(np.stack([rng.uniform(-2e6, 2e6, (K, n)), dur], axis=1), dtype=torch.float32, device=b.device)      # [K,2,N]

    def step_k():
        for k in range(K):
            env.step(act[k], actions_soa=True)

    def many_k():
        env.step_many(act, out_every=True, actions_soa=True)

    def many_1():
        for k in range(K):
            env.step_many(act[k:k + 1], out_every=True, actions_soa=True)
    waves = [env._wave_tables(act[k]) for k in range(K)]             # (d): the tables of every step, built once
    waves = [{"current": tuple(t.clone() for t in w["current"]), "field": w["field"]} for w in waves]

    def wave_k():
        for k in range(K):
            b.step_wave(act[k], waves[k], autoreset=False)

    def backend_k():
        b.step_shaped_many(act, out_every=True)

    def backend_1():
        for k in range(K):
            b.step_shaped_many(act[k:k + 1], out_every=True)

    def flags():
        for k in range(K):
            b.terminated.bool(), b.truncated.bool()
    forms = {"step_x_K": step_k, "step_many_K": many_k, "step_many_1_x_K": many_1, "step_wave_prebuilt_x_K": wave_k,
             "backend_shaped_K": backend_k, "backend_shaped_1_x_K": backend_1}
    work, final = {}, {}
    for name, fn in forms.items():           # warm-up: code objects loaded, allocator primed; and the forms agree
        for _ in range(2):
            b.set_state(start)
            b.counters(reset=True)
            timed(fn)
        c = b.counters()
        assert c["noop_steps"] == 0 and c["env_steps"] == K * n, (name, c)
        work[name] = c["work_units"] / (K * n)
        final[name] = {k: t.clone() for k, t in b.get_state().items()}
    for name in forms:
        for k, t in final[name].items():
            assert torch.equal(t, final["step_x_K"][k]), f"{name}: state field {k} differs from K calls of step()"
    ms = {name: ([], []) for name in forms}
    bool_ms = []
    for _ in range(reps):                    # alternate the forms
        for name, fn in forms.items():
            b.set_state(start)
            wall, dev = timed(fn)
            ms[name][0].append(wall)
            ms[name][1].append(dev)
        bool_ms.append(timed(flags)[0])
    env.close()
    res = {"solver": solver, "n": n, "K": K, "reps": reps, "durations": "U[0.1, 1] ns" if mixed else "1 ns", "same_bits": True}
    for name in forms:
        w, d = np.array(ms[name][0]), np.array(ms[name][1])
        res[name] = {"wall_median_ms": float(np.median(w)), "wall_min_ms": float(w.min()), "wall_max_ms": float(w.max()),
                     "events_median_ms": float(np.median(d)), "sub_steps_per_env_step": work[name],
                     "env_steps_per_s": K * n / (float(np.median(w)) * 1e-3)}
        print(f"{solver} n={n} K={K} {name:24s}: wall median {np.median(w):8.3f} ms (min {w.min():.3f}, max {w.max():.3f}), device events "
              f"{np.median(d):8.3f} ms, {work[name]:.0f} sub-steps per env-step, {res[name]['env_steps_per_s']:.3e} env-steps/s", flush=True)
    res["flags_to_bool_x_K_wall_median_ms"] = float(np.median(bool_ms))
    print(f"{solver} n={n} K={K} flags_to_bool x K (terminated.bool(), truncated.bool() of one step's [N] views): wall median {np.median(bool_ms):.3f} ms", flush=True)
    for name in ("step_many_K", "step_many_1_x_K", "step_wave_prebuilt_x_K", "backend_shaped_K", "backend_shaped_1_x_K"):
        res["ratio_" + name] = res[name]["wall_median_ms"] / res["step_x_K"]["wall_median_ms"]
        print(f"{solver} n={n} K={K}: {name} / step_x_K = {res['ratio_' + name]:.3f} (wall medians)", flush=True)
    return res


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    mixed = len(sys.argv) > 2 and sys.argv[2] == "mixed"
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
    K = int(sys.argv[4]) if len(sys.argv) > 4 else 16
    assert torch.cuda.is_available(), "needs the GPU"
    print(json.dumps(ab(n, K, reps, mixed)))

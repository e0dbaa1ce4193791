#!/usr/bin/env python3
"""What it costs to let the action carry the pulse's knot amplitudes: K = 16 env steps of 65 536 envs (RK4, thermal field off, 1 ns
pulses, a 2-knot constant field) under a P-knot pulse, P = 4 (a trapezoid) and P = 32 (the same trapezoid sampled at 32 knots), on ONE
context that holds both the fixed shape (stg_set_pulse_shape) and the knot times (stg_set_pulse_knots):

  (a) shaped_K ........... one stg_step_shaped launch of K steps, actions [K,2,N]: the fixed shape (tau_j, s_j) in LDS.  This kernel is
                           the parent commit's (profiles/step_knots_existing_kernels_unchanged.txt): the yardstick;
  (b) knots_K ............ one stg_step_knots launch of K steps, actions [K,2+P,N] whose amplitude rows hold the fixed shape's factors
                           s_j for every env and step: the same drive, read from the action;
  (c) step_wave x K ...... K stg_step_wave launches on per-env [P][N] tables built beforehand, outside the timed window: what an agent-
                           shaped pulse cost before, without the host-side table building.

All forms compute the same bits (checked here on the final state before anything is timed).  Every repetition starts from the same
state, restored outside the timed region; the forms are timed alternately in one process after a warm-up of all, with device events
around the launches (kernel against kernel) and a host clock around launches plus synchronise; medians, spreads and ratios are printed,
and one JSON line at the end.
usage (GPU box): python3 tools/step_knots_ab.py [reps=7] [uniform|mixed] [n=65536] [K=16]     (mixed: durations U[0.1, 1] ns)"""
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

TRAPEZOID = ([0.0, 0.1, 0.8, 1.0], [0.0, 1.0, 1.0, 0.0])


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


def ab(n, K, reps, mixed, P):
    solver = "rk4"
    if P == 4:
        tau, s = (np.array(x) for x in TRAPEZOID)
    else:
        tau = np.linspace(0.0, 1.0, P)
        s = np.interp(tau, *TRAPEZOID).astype(np.float32).astype(np.float64)       # (float32 values: the actions carry them exactly)
    env = stg.SpinTorqueVecEnv(n, device_params=bench.stt_params(bench.volume_for(solver)), solver=solver, include_thermal_fluctuations=False,
                               seed=3, out_layout="records", pulse_shape=PiecewiseLinear(tau, s), applied_field=[2e4, 0.0, -1e4])
    env.reset(seed=3)
    b = env.backend
    b.set_pulse_knots(tau, 1.0, env._field_knots)                    # the same context holds both: each entry reads its own
    torch.cuda.synchronize()
    start = {k: t.clone() for k, t in b.get_state().items()}
    rng = np.random.default_rng(3)
    dur = rng.uniform(1e-10, 1e-9, (K, n)) if mixed else np.full((K, n), 1e-9)
    jt = np.stack([rng.uniform(-2e6, 2e6, (K, n)), dur], axis=1)                                        # [K,2,N]
    act = torch.tensor(jt, dtype=torch.float32, device=b.device)
    act_p = torch.tensor(np.concatenate([jt, np.broadcast_to(s[None, :, None], (K, P, n))], axis=1), dtype=torch.float32, device=b.device)
    waves = [env._wave_tables(act[k]) for k in range(K)]             # (c): the tables of every step, built once
    waves = [{"current": tuple(t.clone() for t in w["current"]), "field": w["field"]} for w in waves]

    def shaped_k():
        b.step_shaped_many(act, out_every=True)

    def knots_k():
        b.step_knots_many(act_p, out_every=True)

    def wave_k():
        for k in range(K):
            b.step_wave(act[k], waves[k], autoreset=False)
    forms = {"shaped_K": shaped_k, "knots_K": knots_k, "step_wave_prebuilt_x_K": wave_k}
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
            assert torch.equal(t, final["shaped_K"][k]), f"{name}: state field {k} differs from stg_step_shaped"
    ms = {name: ([], []) for name in forms}
    for _ in range(reps):                    # alternate the forms
        for name, fn in forms.items():
            b.set_state(start)
            wall, dev = timed(fn)
            ms[name][0].append(wall)
            ms[name][1].append(dev)
    env.close()
    res = {"solver": solver, "n": n, "K": K, "P": P, "reps": reps, "durations": "U[0.1, 1] ns" if mixed else "1 ns", "same_bits": True}
    for name in forms:
        w, d = np.array(ms[name][0]), np.array(ms[name][1])
        res[name] = {"wall_median_ms": float(np.median(w)), "events_median_ms": float(np.median(d)), "events_min_ms": float(d.min()),
                     "events_max_ms": float(d.max()), "sub_steps_per_env_step": work[name]}
        print(f"{solver} n={n} K={K} P={P} {name:24s}: device events median {np.median(d):8.3f} ms (min {d.min():.3f}, max {d.max():.3f}), wall "
              f"median {np.median(w):8.3f} ms, {work[name]:.0f} sub-steps per env-step", flush=True)
    for name in ("knots_K", "step_wave_prebuilt_x_K"):
        res["ratio_" + name] = res[name]["events_median_ms"] / res["shaped_K"]["events_median_ms"]
        print(f"{solver} n={n} K={K} P={P}: {name} / shaped_K = {res['ratio_' + name]:.3f} (device-event medians)", flush=True)
    res["ratio_knots_K_vs_step_wave"] = res["knots_K"]["events_median_ms"] / res["step_wave_prebuilt_x_K"]["events_median_ms"]
    print(f"{solver} n={n} K={K} P={P}: knots_K / step_wave_prebuilt_x_K = {res['ratio_knots_K_vs_step_wave']:.3f}", flush=True)
    return res


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    mixed = len(sys.argv) > 2 and sys.argv[2] == "mixed"
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
    K = int(sys.argv[4]) if len(sys.argv) > 4 else 16
    assert torch.cuda.is_available(), "needs the GPU"
    print(json.dumps([ab(n, K, reps, mixed, P) for P in (4, 32)]))

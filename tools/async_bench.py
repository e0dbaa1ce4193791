#!/usr/bin/env python3
"""Asynchronous stepping on the headline configuration (65 536 thermal STT envs, RK45, J ~ U[-2e6, 2e6] A/m^2, pulses ~ U[0.1, 1] ns,
float32, volume 9.7e-6, autoreset): env-steps per second of
  * the synchronous step (HipBackend.step: one stg_step_many launch of all N envs),
  * stg_step_ids with M = N (the id path's overhead over the full launch),
  * the send/recv pool of SpinTorqueVecEnv at B = N/2, N/4, N/8 (4 streams), the policy replaced by a fixed device-side action bank,
plus the placement summary (stg_get_placement) of the last launch of each.  One JSON object per line.
usage: python tools/async_bench.py [--envs 65536] [--steps 60] [--warmup 10] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spin-torque-rl-gym_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=60, help="timed full-batch equivalents per row")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import spin_torque_gym_amd as stg
    n = args.envs
    p = stg.DeviceFactory().get_default_parameters("stt_mram")
    p["volume"] = 9.7e-6
    env = stg.SpinTorqueVecEnv(n, solver="rk45", device_params=p, include_thermal_fluctuations=True, autoreset=True, seed=0)
    env.reset(seed=0)
    g = torch.Generator(device="cpu").manual_seed(1)
    bank = 8                                                         # the fixed action generator: a bank of [2, N] action sets
    acts = torch.empty((bank, 2, n), dtype=torch.float32)
    acts[:, 0] = (torch.rand((bank, n), generator=g) * 2 - 1) * 2e6
    acts[:, 1] = 1e-10 + torch.rand((bank, n), generator=g) * 9e-10
    acts = acts.cuda()
    acts_g = acts.transpose(1, 2).contiguous()                       # Gym orientation [bank, N, 2] for send()
    b = env.backend
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    def placement_summary():
        try:
            pl = b.placement(0)
            return {k: pl.get(k) for k in ("workgroups", "waves_per_workgroup", "span_us", "simd_busy_frac", "last_simd_alone_frac")}
        except Exception as e:  # noqa: BLE001
            return {"error": str(e)}

    # synchronous step
    for k in range(args.warmup):
        b.step(acts[k % bank], autoreset=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        b.step(acts[k % bank], autoreset=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sync_rate = n * args.steps / dt
    emit({"row": "sync_step", "envs": n, "steps": args.steps, "ms_per_step": round(1e3 * dt / args.steps, 4),
          "env_steps_per_s": round(sync_rate), "placement": placement_summary()})

    # step_ids, M = N (identity list, own workspace, outputs preallocated)
    ids = torch.arange(n, dtype=torch.int32, device="cuda")
    ws = b.ids_workspace(n)
    out = b.alloc_ids_outputs(n, autoreset=True)
    for k in range(args.warmup):
        b.step_ids(acts[k % bank], ids, autoreset=True, workspace=ws, out=out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        b.step_ids(acts[k % bank], ids, autoreset=True, workspace=ws, out=out)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    emit({"row": "step_ids_M_eq_N", "envs": n, "steps": args.steps, "ms_per_step": round(1e3 * dt / args.steps, 4),
          "env_steps_per_s": round(n * args.steps / dt), "vs_sync": round(n * args.steps / dt / sync_rate, 4),
          "placement": placement_summary()})

    # the send/recv pool
    for div in (2, 4, 8):
        B = n // div
        env.async_reset(B, seed=0, num_streams=args.streams)
        rounds_w, rounds = args.warmup * div, args.steps * div
        sent = 0
        t0 = None
        for r in range(rounds_w + rounds):
            if r == rounds_w:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sent = 0
            _, _, _, _, info = env.recv()
            e_ids = info["env_id"]
            m = int(e_ids.shape[0])
            env.send(acts_g[r % bank, :m], e_ids)
            sent += m
        while env._pool.inflight:
            env.recv()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rate = sent / dt
        emit({"row": f"pool_B_N/{div}", "envs": n, "batch": B, "streams": args.streams, "rounds": rounds, "env_steps": sent,
              "env_steps_per_s": round(rate), "vs_sync": round(rate / sync_rate, 4), "placement_last_launch": placement_summary()})
        env.reset(seed=0)
    env.close()
    if args.out:
        with open(args.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

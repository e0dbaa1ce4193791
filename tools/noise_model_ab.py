"""Step time of the fixed-step thermal kernels per noise model -- 65 536 envs, RK4, 1 ns pulses (1000 sub-steps), ms per step.
Run once per library build (STG_HIP_LIBRARY=...), alternating the builds; a build without a model skips it.
A block is `steps` steps between two device events (200 steps = 0.1 s of kernel time); the first blocks still see the clocks settle, so
look at the median and at the last blocks.
usage: python tools/noise_model_ab.py [models=ou,brown,white] [blocks=7] [steps=200]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402

bench.cap_host_threads()
import spin_torque_gym_amd as stg  # noqa: E402

models = (sys.argv[1] if len(sys.argv) > 1 else "ou,brown,white").split(",")
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 7
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 200
tag = os.path.basename(os.environ.get("STG_HIP_LIBRARY", "in-tree"))
n = 65536
for model in models:
    try:
        env = stg.SpinTorqueVecEnv(n, device_params=bench.stt_params(bench.volume_for("rk4")), include_thermal_fluctuations=True,
                                   solver="rk4", seed=1234, autoreset=True, noise_model=model)
    except Exception as e:          # an older build refuses a model it does not have
        print(f"[{tag}] {model}: not in this build ({e})", flush=True)
        continue
    env.reset(seed=1234)
    a = bench.make_actions(steps, n, env.backend.device, 99)
    a[:, 1] = 1e-9
    for k in range(max(3, steps // 4)):
        env.backend.step(a[k], autoreset=True)
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for k in range(steps):
            env.backend.step(a[k], autoreset=True)
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / steps)
    print(f"[{tag}] rk4 thermal {model} n={n} T=1ns: median {statistics.median(ms):.4f} ms/step, blocks " +
          " ".join(f"{x:.4f}" for x in ms), flush=True)
    env.close()

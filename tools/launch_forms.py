#!/usr/bin/env python3
"""Which launch form each batch size gets: one step (full step and stg_step_ids with M = N) of a list of configurations -- the sizes
on either side of every schedule threshold of csrc/stg_launch_plan.hpp and those of tests/test_gpu_fullsize.py's odd-size sweep --
and, from HipBackend.placement(0, raw=True), the launch's workgroups, wavefronts per workgroup and producer wavefronts (among the
first 4096 recorded).  Results never depend on the form, so this table is what shows a threshold that moved: run it once per library
build (STG_HIP_LIBRARY=<path> selects one) and diff the outputs.
usage: python tools/launch_forms.py [--out FILE] [--max-envs N]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spin-torque-rl-gym_amd"))

import torch  # noqa: E402

THRESHOLDS = {
    ("rk45", True): (64, 4096, 65536, 65537, 70000, 98304, 98305, 131072, 131073, 200000, 524288, 524289),
    ("rk45", False): (64, 65536, 131072, 131073, 200000),
    ("rk4", True): (64, 4096, 65536, 65537, 80000, 90112, 90113, 200000),
    ("rk4", False): (64, 65535, 65536, 262144),
    ("euler", True): (4096, 80000),
}
SWEEP = {   # tests/test_gpu_fullsize.py::test_schedule_covers_every_env_once_at_odd_sizes
    ("rk4", False): (4097, 65600, 66000, 69632, 81920, 100000, 131136, 132000, 165000, 200001, 262145),
    ("rk4", True): (33000, 40960, 50000, 61440, 65535, 65537, 66000, 73729, 81920, 100000, 132000),
    ("rk45", True): (32832, 36864, 45000, 60000, 65472, 65537, 65600, 66000, 69633, 77777, 81920, 81921, 100000, 131136, 132000, 165000),
    ("rk45", False): (66000, 100000, 132000, 170000),
}
# (solver, thermal, n, constructor knobs, label): what the size alone does not select
KNOBS = [
    ("rk45", True, 200000, dict(wave_spec=True), "wave_spec=1"),
    ("rk45", True, 200000, dict(lane_refill=False), "lane_refill=-1"),
    ("rk45", True, 200000, dict(lane_refill=4), "lane_refill=4"),
    ("rk45", True, 70000, dict(lane_sort=False), "lane_sort=-1"),
    ("rk4", True, 4096, dict(temperature=0.0), "T=0K"),
    ("rk4", True, 80000, dict(torque_model="device"), "device-torque"),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--max-envs", type=int, default=1 << 20)
    args = ap.parse_args()
    import spin_torque_gym_amd as stg
    fac = stg.DeviceFactory()
    cases = []
    for key in THRESHOLDS:
        for n in sorted(set(THRESHOLDS[key]) | set(SWEEP.get(key, ()))):
            cases.append((key[0], key[1], n, {}, ""))
    cases += KNOBS
    lines = ["solver thermal n knobs | full: workgroups waves/wg producers | ids: workgroups waves/wg producers"]
    for solver, thermal, n, knobs, label in cases:
        if n > args.max_envs:
            continue
        p = fac.get_default_parameters("stt_mram")
        p["volume"] = 9.7e-6 if solver == "rk45" else 8.75e-11
        env = stg.SpinTorqueVecEnv(n, solver=solver, device_params=p, include_thermal_fluctuations=thermal, autoreset=True, seed=0, **knobs)
        env.reset(seed=0)
        b = env.backend
        g = torch.Generator(device="cpu").manual_seed(n)
        act = torch.empty((2, n), dtype=torch.float32)
        act[0] = (torch.rand(n, generator=g) * 2 - 1) * 2e6
        act[1] = 1e-10 + torch.rand(n, generator=g) * 2e-10         # short pulses: the form is what is looked at, not the time
        act = act.cuda()
        forms = []
        for ids in (False, True):
            if ids:
                b.step_ids(act, torch.arange(n, dtype=torch.int32, device=b.device), autoreset=True)
            else:
                b.step(act, autoreset=True)
            pl = b.placement(0, raw=True)
            forms.append(f"{pl['workgroups']} {pl['waves_per_workgroup']} {int(pl['producer'].sum()) if 'producer' in pl else 0}")
        lines.append(f"{solver} {int(thermal)} {n} {label or '-'} | {forms[0]} | {forms[1]}")
        print(lines[-1], flush=True)
        env.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What the per-lane row of stg_switch_population costs.  rk4 + noise_model='brown' (one RK45 row), the switching device of
tests/brown_ref.py from m0 = +z, 0.5 ns pulses (n = 500 sub-steps), target -z, threshold 0.

  ab     on the same arguments, alternating in one process, enqueue to device synchronise:
           (a) the unchanged stg_switch_stats and stg_switch_times (100 time bins)                                  -- the yardstick
           (b) stg_switch_population with every sigma 0, without and with the first-passage counts; its counts must equal (a)'s
           (c) all five sigma 0.05, Q = 1 and Q = 4096, without and with dev_switched
         The figure of interest is (b) / (a): the price of drawing a device per trial and integrating on a row of one's own.
  big    one population-scale run: G = 1, 2^log2 devices x 1024 trials each in launches of 2^22 trials, per-device counts kept.

Every step runs in a child process of its own under its own time limit; a step that fails or runs out of time ends the run (nothing is
tried again).

    python tools/switch_population_ab.py                    # ab at G = 8, R in {4096, 65536, 1048576} and rk45 at 4096; 7 rounds
    python tools/switch_population_ab.py --big 20           # also 2^20 devices x 1024 trials

Prints one JSON line per step."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWITCH = dict(volume=1.3856e-25, damping=0.02, J=1.2482e-9, T=5e-10)  # tests/brown_ref.py: thermally assisted switching
TBINS = 100
SIGMA = 0.05
BIG_Q = 1024


def _imports():
    sys.path.insert(0, os.path.join(ROOT, "spin-torque-rl-gym_amd"))
    import numpy as np
    import torch
    import spin_torque_gym_amd as stg
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    return np, torch, stg, EnvConfig, HipBackend


def make_backend(n, solver):
    _, _, stg, EnvConfig, HipBackend = _imports()
    p = stg.DeviceFactory().get_default_parameters("stt_mram")
    p.update(volume=SWITCH["volume"], damping=SWITCH["damping"], saturation_magnetization=8e5, uniaxial_anisotropy=1e6)
    b = HipBackend(n, EnvConfig(solver=solver, include_thermal_fluctuations=True, noise_model="brown" if solver != "rk45" else "white", seed=41))
    b.set_params([stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", p))])
    return b


def conditions(G, dev):
    _, torch, *_ = _imports()
    m0 = torch.tensor([[0.0], [0.0], [1.0]], dtype=torch.float64, device=dev).repeat(1, G)
    J = (SWITCH["J"] * torch.linspace(0.85, 1.15, G, dtype=torch.float64, device=dev))[None, :]
    T = torch.full((1, G), SWITCH["T"], dtype=torch.float64, device=dev)
    tgt = torch.tensor([[0.0], [0.0], [-1.0]], dtype=torch.float64, device=dev).repeat(1, G)
    return m0, J, T, tgt


def timed(fn):
    _, torch, *_ = _imports()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def step_ab(G, R, rounds, solver):
    np, torch, *_ = _imports()
    dev = torch.device("cuda", 0)
    m0, J, T, tgt = conditions(G, dev)
    b = make_backend(G, solver)
    zero = torch.zeros((5, G), dtype=torch.float64, device=dev)
    five = torch.full((5, G), SIGMA, dtype=torch.float64, device=dev)
    counts = {q: torch.zeros((G, -(-R // q)), dtype=torch.int64, device=dev) for q in (1, 4096)}

    def pop(sigma, **kw):
        return lambda: b.switch_population(m0, J, T, tgt, R, sigma, **kw)

    forms = {"stats": lambda: b.switch_stats(m0, J, T, tgt, R), "times": lambda: b.switch_times(m0, J, T, tgt, R, n_tbins=TBINS),
             "pop0": pop(zero), "pop0_times": pop(zero, n_tbins=TBINS),
             "pop_q1": pop(five, trials_per_device=1), "pop_q1_dev": pop(five, trials_per_device=1, dev_switched=counts[1]),
             "pop_q4096": pop(five, trials_per_device=4096), "pop_q4096_dev": pop(five, trials_per_device=4096, dev_switched=counts[4096])}
    ms, out, devs = {k: [] for k in forms}, {}, True
    for _ in range(rounds + 1):                                      # (the first round warms every form up and is dropped)
        for k, fn in forms.items():
            for c in counts.values():
                c.zero_()
            t, out[k] = timed(fn)
            ms[k].append(t)
            if k.endswith("_dev"):                                   # the per-device counts of this launch add up to its n_switched
                devs = devs and torch.equal(counts[int(k[5:-4])].sum(dim=1), out[k][0])
    same = all(torch.equal(out[a][i], out[c][i]) for a, c in (("pop0", "stats"), ("pop0_times", "times")) for i in (0, 1))
    same = same and all(torch.equal(out["pop0_times"][i], out["times"][i]) for i in (3, 4, 5))
    devs = devs and torch.equal(out["pop_q1"][0], out["pop_q1_dev"][0]) and torch.equal(out["pop_q4096"][0], out["pop_q4096_dev"][0])
    b.close()
    med = {k: float(np.median(v[1:])) for k, v in ms.items()}
    ratio = lambda a, c: round(med[a] / med[c], 4)                   # noqa: E731
    return dict(step="ab", solver=solver, G=G, R=R, rounds=rounds, **{k + "_ms": round(v, 4) for k, v in med.items()},
                pop0_over_stats=ratio("pop0", "stats"), pop0_times_over_times=ratio("pop0_times", "times"), pop_q1_over_stats=ratio("pop_q1", "stats"),
                pop_q4096_over_stats=ratio("pop_q4096", "stats"), dev_q1_over_without=ratio("pop_q1_dev", "pop_q1"),
                dev_q4096_over_without=ratio("pop_q4096_dev", "pop_q4096"), sigma0_equals_old=bool(same), device_counts_add_up=bool(devs),
                p_switch_nominal=[round(x, 4) for x in (out["stats"][0].cpu().numpy() / R).tolist()],
                p_switch_population=[round(x, 4) for x in (out["pop_q1"][0].cpu().numpy() / R).tolist()])


def step_big(log2_d, chunk):
    np, torch, *_ = _imports()
    dev = torch.device("cuda", 0)
    b = make_backend(1, "rk4")
    m0, J, T, tgt = conditions(1, dev)
    J = torch.full((1, 1), SWITCH["J"], dtype=torch.float64, device=dev)
    n_dev = 1 << log2_d
    total, done, out = n_dev * BIG_Q, 0, None
    sigma = torch.full((5, 1), SIGMA, dtype=torch.float64, device=dev)
    counts = torch.zeros((1, n_dev), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while done < total:
        r = min(chunk, total - done)
        out = b.switch_population(m0, J, T, tgt, r, sigma, trials_per_device=BIG_Q, dev_switched=counts, trial0=done, trial_stride=total, out=out)
        done += r
        if (done // chunk) % 8 == 0:
            torch.cuda.synchronize()                                 # (bounds the queue)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    n_sw, n_failed = int(out[0][0].item()), int(out[1][0].item())
    p = counts[0].cpu().numpy() / BIG_Q
    b.close()
    q = np.quantile(p, [0.001, 0.01, 0.1, 0.5, 0.9, 0.99, 0.999])
    return dict(step="big", G=1, devices=n_dev, trials_per_device=BIG_Q, trials=total, chunk=chunk, sigma=SIGMA, seconds=round(wall, 3),
                trials_per_second=round(total / wall), p_switch=n_sw / total, n_failed=n_failed, device_counts_add_up=bool(int(counts.sum().item()) == n_sw),
                device_p_switch_mean=float(p.mean()), device_p_switch_std=float(p.std()),
                device_p_switch_quantiles_0001_001_01_05_09_099_0999=[round(float(x), 4) for x in q],
                devices_that_never_switched=int((p == 0).sum()), devices_below_half=int((p < 0.5).sum()))


def child(spec):
    res = step_ab(spec["G"], spec["R"], spec["rounds"], spec["solver"]) if spec["step"] == "ab" else step_big(spec["log2"], spec["chunk"])
    print(json.dumps(res), flush=True)
    return 0 if res.get("sigma0_equals_old", True) and res.get("device_counts_add_up", True) else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--R", type=int, nargs="*", default=[4096, 65536, 1048576])
    ap.add_argument("--rk45-R", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--big", type=int, default=0, help="log2 of the device count of the population-scale run (0: none)")
    ap.add_argument("--chunk", type=int, default=1 << 22)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds each step may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(json.loads(a.child))
    steps = [dict(step="ab", G=a.G, R=r, rounds=a.rounds, solver="rk4") for r in a.R]
    if a.rk45_R:
        steps.append(dict(step="ab", G=a.G, R=a.rk45_R, rounds=a.rounds, solver="rk45"))
    if a.big:
        steps.append(dict(step="big", log2=a.big, chunk=a.chunk))
    for spec in steps:                                               # one child per step, each under its own limit; the first failure ends the run
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(spec)], timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(spec, error=f"no result within {a.limit} s")), flush=True)
            return 124
        if rc != 0:
            print(json.dumps(dict(spec, error=f"exit status {rc}")), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

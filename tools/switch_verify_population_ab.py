#!/usr/bin/env python
"""A/B of stg_switch_verify_population against the UNCHANGED stg_switch_verify, in one process, alternating: what the lane's own
device row, the draw and the per-device counts cost.  rk4 + noise_model='brown' (rk45 + 'white' at the smallest size), the switching
device of tests/brown_ref.py from m0 = +z, A = 2 attempts of one 0.5 ns pulse (the second 1.1 x the first), as
tools/switch_verify_ab.py.  Every path is timed from enqueue to a device synchronise with its inputs already on the device; round 0
warms every path up and is dropped.  Per size, the paths are

    verify      stg_switch_verify, the nominal device
    sigma0      the population entry with every sigma 0, one trial per device, no per-device counts: its counts must equal verify's
    pop_q1      all five sigmas 0.05, one trial per device (a draw per trial)
    pop_q4096   the same, 4096 trials per device (a lane keeps its row once Q >= 2 * 64 * W)
    pop_q1_dev / pop_q4096_dev   the same two with dev_switched_at: one 64-bit atomic per switched trial

    python tools/switch_verify_population_ab.py                       # G = 8, R in {4096, 65536, 1048576}, 7 rounds, rk45 at R = 4096
    python tools/switch_verify_population_ab.py --scale 20 --budget 240   # also G = 1, 2^20 devices x 1024 trials, A = 3, in launches of 2^22

Prints one JSON line per size: median milliseconds of each path, each path over verify in the same run, and the run-to-run spread of
the verify timing."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spin-torque-rl-gym_amd"))

import spin_torque_gym_amd as stg                                    # noqa: E402
from spin_torque_gym_amd.backend import EnvConfig, HipBackend        # noqa: E402

SWITCH = dict(volume=1.3856e-25, damping=0.02, J=1.2482e-9, T=5e-10)  # tests/brown_ref.py: thermally assisted switching, P ~ 0.39
SECOND = 1.1                                                          # the retry's current over the first pulse's
SIGMA = 0.05
RK45_J_SCALE = 1e-3                                                   # tests/switch_stats_ref.py: the unsaturated input of the LLGS solver


def make_backend(n, solver="rk4", noise="brown"):
    p = stg.DeviceFactory().get_default_parameters("stt_mram")
    p.update(volume=SWITCH["volume"], damping=SWITCH["damping"], saturation_magnetization=8e5, uniaxial_anisotropy=1e6)
    b = HipBackend(n, EnvConfig(solver=solver, include_thermal_fluctuations=True, noise_model=noise, seed=41))
    b.set_params([stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", p))])
    return b


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def ab(G, R, rounds, solver="rk4", noise="brown"):
    dev = torch.device("cuda", 0)
    scale = RK45_J_SCALE if solver == "rk45" else 1.0
    m0 = torch.tensor([[0.0], [0.0], [1.0]], dtype=torch.float64, device=dev).repeat(1, G)
    J1 = scale * SWITCH["J"] * torch.linspace(0.85, 1.15, G, dtype=torch.float64, device=dev)
    J = torch.stack([J1, SECOND * J1])[:, None, :].contiguous()                      # [A = 2, P = 1, G]
    T = torch.full((2, 1, G), SWITCH["T"], dtype=torch.float64, device=dev)
    tgt = torch.tensor([[0.0], [0.0], [-1.0]], dtype=torch.float64, device=dev).repeat(1, G)
    zero = torch.zeros((5, G), dtype=torch.float64, device=dev)
    sig = torch.full((5, G), SIGMA, dtype=torch.float64, device=dev)
    b = make_backend(G, solver, noise)
    counts = {q: torch.zeros((2, G, -(-R // q)), dtype=torch.int64, device=dev) for q in (1, 4096)}

    def pop(sigma, q, per_device):
        def run():
            d = counts[q] if per_device else None
            if d is not None:
                d.zero_()
            return b.switch_verify_population(m0, J, T, tgt, R, sigma, trials_per_device=q, dev_switched_at=d)[:2]
        return run

    paths = {"verify": lambda: b.switch_verify(m0, J, T, tgt, R)[:2], "sigma0": pop(zero, 1, False), "pop_q1": pop(sig, 1, False),
             "pop_q4096": pop(sig, 4096, False), "pop_q1_dev": pop(sig, 1, True), "pop_q4096_dev": pop(sig, 4096, True)}
    times, outs = {k: [] for k in paths}, {}
    for _ in range(rounds + 1):                                      # (the first round warms the paths up and is dropped)
        for k, fn in paths.items():
            t, outs[k] = timed(fn)
            times[k].append(t)
    same = all(bool(torch.equal(x, y)) for x, y in zip(outs["verify"], outs["sigma0"]))
    dev_sum = all(bool(torch.equal(counts[q].sum(dim=-1), outs[f"pop_q{q}_dev"][0])) and bool(torch.equal(outs[f"pop_q{q}_dev"][0], outs[f"pop_q{q}"][0]))
                  for q in (1, 4096))
    med = {k: float(np.median(t[1:])) for k, t in times.items()}
    p = {k: float(outs[k][0][0].sum().item()) / (G * R) for k in ("verify", "pop_q1", "pop_q4096")}
    b.close()
    res = dict(G=G, R=R, rounds=rounds, solver=solver, noise=noise, **{k + "_ms": round(v, 4) for k, v in med.items()})
    res.update({k + "_over_verify": round(v / med["verify"], 4) for k, v in med.items() if k != "verify"})
    res.update(dev_over_plain_q1=round(med["pop_q1_dev"] / med["pop_q1"], 4), dev_over_plain_q4096=round(med["pop_q4096_dev"] / med["pop_q4096"], 4),
               verify_spread=round((max(times["verify"][1:]) - min(times["verify"][1:])) / med["verify"], 4), sigma0_counts_equal_verify=same,
               dev_counts_sum_to_n_switched=dev_sum, p_first={k: round(v, 4) for k, v in p.items()})
    return res


def scale_run(log2_d, q, budget_s, chunk):
    """G = 1, 2^log2_d devices x q trials, A = 3 (the retries at 1.1 and 1.2 x the first pulse), all five sigmas 0.05, per-device counts
    on, through launches of `chunk` trials, stopping early once budget_s seconds have passed"""
    dev = torch.device("cuda", 0)
    b = make_backend(1)
    n_dev = 1 << log2_d
    total = n_dev * q
    m0 = torch.tensor([[0.0], [0.0], [1.0]], dtype=torch.float64, device=dev)
    J = (SWITCH["J"] * torch.tensor([1.0, 1.1, 1.2], dtype=torch.float64, device=dev))[:, None, None].contiguous()
    T = torch.full((3, 1, 1), SWITCH["T"], dtype=torch.float64, device=dev)
    tgt = torch.tensor([[0.0], [0.0], [-1.0]], dtype=torch.float64, device=dev)
    sig = torch.full((5, 1), SIGMA, dtype=torch.float64, device=dev)
    dsw = torch.zeros((3, 1, n_dev), dtype=torch.int64, device=dev)
    done, out = 0, None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while done < total and time.perf_counter() - t0 < budget_s:
        r = min(chunk, total - done)
        out = b.switch_verify_population(m0, J, T, tgt, r, sig, trials_per_device=q, dev_switched_at=dsw, trial0=done, trial_stride=total, out=out)
        done += r
        if (done // chunk) % 8 == 0:
            torch.cuda.synchronize()                                 # (bounds the queue, so that the budget is looked at in time)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    n_sw, n_end, n_failed = out[0][:, 0].cpu().numpy(), out[1][:, 0].cpu().numpy(), int(out[2].item())
    full = done // q                                                 # devices all of whose trials ran
    dev_wer = 1.0 - dsw[:, 0, :full].sum(dim=0).cpu().numpy() / q
    b.close()
    wer = 1.0 - np.cumsum(n_sw) / done
    quant = np.quantile(dev_wer, [0.001, 0.5, 0.999]).tolist() if full else None
    return dict(G=1, A=3, devices_asked=n_dev, trials_per_device=q, R_done=done, devices_done=full, chunk=chunk, wall_s=round(wall, 2),
                trials_per_s=round(done / wall), n_switched_at=n_sw.tolist(), n_ended_at=n_end.tolist(), n_failed=n_failed,
                wer_after=wer.tolist(), mean_attempts=float(((np.arange(3) + 1) * n_end).sum() / done),
                dev_wer_after_last_quantiles={"0.1%": quant[0], "50%": quant[1], "99.9%": quant[2]} if quant else None,
                dev_counts_sum_to_n_switched=bool(int(dsw.sum().item()) == int(n_sw.sum())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--R", type=int, nargs="+", default=[4096, 65536, 1048576])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-rk45", action="store_true", help="skip rk45 + white at the smallest size")
    ap.add_argument("--scale", type=int, default=0, help="also run G = 1, 2^SCALE devices x --q trials, A = 3, through chunked launches")
    ap.add_argument("--q", type=int, default=1024)
    ap.add_argument("--budget", type=float, default=240.0, help="seconds after which the --scale run stops early")
    ap.add_argument("--chunk", type=int, default=1 << 22)
    a = ap.parse_args()
    for R in a.R:
        print(json.dumps(ab(a.G, R, a.rounds)), flush=True)
    if a.R and not a.no_rk45:
        print(json.dumps(ab(a.G, min(a.R), a.rounds, "rk45", "white")), flush=True)
    if a.scale:
        print(json.dumps(scale_run(a.scale, a.q, a.budget, a.chunk)), flush=True)


if __name__ == "__main__":
    main()

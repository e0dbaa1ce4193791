#!/usr/bin/env python
"""A/B of the two ways to get write - verify - write statistics, in one process, alternating: the fused launch (stg_switch_verify:
attempts, verify and reduction on chip) against the chained route (one stg_solve launch per attempt over the G R replicated problems
with a torch mask between them), and against stg_switch_stats (A = 1: what one pulse alone costs).  rk4 + noise_model='brown', the
switching device of tests/brown_ref.py from m0 = +z, A = 2 attempts of one 0.5 ns pulse (the second 1.1 x the first).  Every path is
timed from enqueue to a device synchronise with its inputs already on the device; the counts of the fused and the chained route are
compared and must be equal.

    python tools/switch_verify_ab.py                       # G = 8, R in {4096, 65536, 1048576}, 7 rounds
    python tools/switch_verify_ab.py --big 30 --budget 60  # also G = 1, R = 2^30, A = 3 in chunks of 2^22, stopping after ~60 s

Prints one JSON line per size: median milliseconds of each path, time(A = 2) / time(A = 1) next to the work the counts imply,
1 + (1 - p) solves per trial with p the first attempt's success, and the run-to-run spread of the A = 1 timing."""
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


def make_backend(n):
    p = stg.DeviceFactory().get_default_parameters("stt_mram")
    p.update(volume=SWITCH["volume"], damping=SWITCH["damping"], saturation_magnetization=8e5, uniaxial_anisotropy=1e6)
    b = HipBackend(n, EnvConfig(solver="rk4", include_thermal_fluctuations=True, noise_model="brown", seed=41))
    b.set_params([stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", p))])
    return b


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def ab(G, R, rounds):
    dev = torch.device("cuda", 0)
    m0 = torch.tensor([[0.0], [0.0], [1.0]], dtype=torch.float64, device=dev).repeat(1, G)
    J1 = SWITCH["J"] * torch.linspace(0.85, 1.15, G, dtype=torch.float64, device=dev)
    J = torch.stack([J1, SECOND * J1])[:, None, :].contiguous()                      # [A = 2, P = 1, G]
    T = torch.full((2, 1, G), SWITCH["T"], dtype=torch.float64, device=dev)
    tgt = torch.tensor([[0.0], [0.0], [-1.0]], dtype=torch.float64, device=dev).repeat(1, G)
    fused_b, old_b = make_backend(G), make_backend(G * R)
    m0_rep, T_rep = m0.repeat_interleave(R, dim=1).contiguous(), T[0, 0].repeat_interleave(R)
    J_rep = [J[a, 0].repeat_interleave(R) for a in range(2)]

    def fused():
        return fused_b.switch_verify(m0, J, T, tgt, R)[:2]

    def one():
        return fused_b.switch_stats(m0, J[0], T[0], tgt, R)[0]

    def chained():
        """two solve launches; the mask between them picks the trials that take the second result"""
        mf = old_b.solve(m0_rep, J_rep[0], T_rep, env_step=0)["m_final"]
        sw0 = -mf[2] > 0.0
        mf2 = old_b.solve(mf, J_rep[1], T_rep, env_step=1)["m_final"]
        sw1 = ~sw0 & (-mf2[2] > 0.0)
        n_sw = torch.stack([sw0.reshape(G, R).sum(1), sw1.reshape(G, R).sum(1)])
        return n_sw, torch.stack([n_sw[0], R - n_sw[0]])

    t_f, t_1, t_c = [], [], []
    for _ in range(rounds + 1):                                      # (the first round warms the paths up and is dropped)
        a, n_f = timed(fused)
        b, n_1 = timed(one)
        c, n_c = timed(chained)
        t_f.append(a), t_1.append(b), t_c.append(c)
    same = all(bool(torch.equal(x.cpu(), y.cpu())) for x, y in zip(n_f, n_c)) and bool(torch.equal(n_1.cpu(), n_f[0][0].cpu()))
    fused_b.close(), old_b.close()
    f, o, c = (float(np.median(t[1:])) for t in (t_f, t_1, t_c))
    p = float(n_f[0][0].sum().item()) / (G * R)
    return dict(G=G, R=R, rounds=rounds, verify_ms=round(f, 4), stats_ms=round(o, 4), chained_ms=round(c, 4), chained_over_verify=round(c / f, 3),
                verify_over_stats=round(f / o, 3), solves_per_trial=round(2.0 - p, 3),
                stats_spread=round((max(t_1[1:]) - min(t_1[1:])) / o, 3), counts_equal=same, p_first=round(p, 4),
                chained_bytes_per_trial=69, verify_bytes_per_trial=0)


def big(log2_r, budget_s, chunk):
    """G = 1, R = 2^log2_r, A = 3 (the retries at 1.1 and 1.2 x the first pulse) through launches of `chunk` trials, stopping early
    once budget_s seconds have passed"""
    dev = torch.device("cuda", 0)
    b = make_backend(1)
    m0 = torch.tensor([[0.0], [0.0], [1.0]], dtype=torch.float64, device=dev)
    J = (SWITCH["J"] * torch.tensor([1.0, 1.1, 1.2], dtype=torch.float64, device=dev))[:, None, None].contiguous()
    T = torch.full((3, 1, 1), SWITCH["T"], dtype=torch.float64, device=dev)
    tgt = torch.tensor([[0.0], [0.0], [-1.0]], dtype=torch.float64, device=dev)
    total, done, out = 1 << log2_r, 0, None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while done < total and time.perf_counter() - t0 < budget_s:
        r = min(chunk, total - done)
        out = b.switch_verify(m0, J, T, tgt, r, trial0=done, trial_stride=total, out=out)
        done += r
        if (done // chunk) % 8 == 0:
            torch.cuda.synchronize()                                 # (bounds the queue, so that the budget is looked at in time)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    n_sw, n_end, n_failed = out[0][:, 0].cpu().numpy(), out[1][:, 0].cpu().numpy(), int(out[2].item())
    b.close()
    wer = 1.0 - np.cumsum(n_sw) / done
    return dict(G=1, A=3, R_asked=total, R_done=done, chunk=chunk, wall_s=round(wall, 2), trials_per_s=round(done / wall),
                n_switched_at=n_sw.tolist(), n_ended_at=n_end.tolist(), n_failed=n_failed, wer_after=wer.tolist(),
                stderr=np.sqrt(wer * (1.0 - wer) / done).tolist(), mean_attempts=float(((np.arange(3) + 1) * n_end).sum() / done))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--R", type=int, nargs="+", default=[4096, 65536, 1048576])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--big", type=int, default=0, help="also run G = 1, R = 2^BIG, A = 3 through chunked launches")
    ap.add_argument("--budget", type=float, default=60.0, help="seconds after which the --big run stops early")
    ap.add_argument("--chunk", type=int, default=1 << 22)
    a = ap.parse_args()
    for R in a.R:
        print(json.dumps(ab(a.G, R, a.rounds)), flush=True)
    if a.big:
        print(json.dumps(big(a.big, a.budget, a.chunk)), flush=True)


if __name__ == "__main__":
    main()

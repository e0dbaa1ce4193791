"""A/B of the array env's fused rollout against its single-step path, in one process, interleaved:

    python3 tools/array_rollout_ab.py [n] [blocks] [reps]       (262144 arrays of 4 x 4 STT cells, dipolar coupling; 5 blocks of 10 reps)

per action mode, for 8 array-steps:  (i) 8 x stg_array_step   (ii) stg_array_step_many(K=8, out_every=1)   (iii) K=8, out_every=0
(iv) (ii) and (iii) with autoreset=1.  One rep is 8 steps of every array; one block is `reps` reps between two device events; the variants
take turns block by block.  Reported: the device-event span per array-step over back-to-back launches issued from Python (not a kernel
time: it includes what the launches leave between them; median over blocks, min .. max = the block-to-block spread), the algorithmic
bytes per array-step and what that is in GB/s.  max_steps is the registered 200 and no array terminates (threshold 2.0); every env
starts with step counts spread uniformly over 0..199 (set_state), so in the auto-reset rows about one array in 200 restarts at every
step, scattered over the wavefronts -- the truncation-only rate of the registered env, not a learner's termination rate.  Writes one
JSON line per (mode, variant) after the table."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "spin-torque-rl-gym_amd"))
import spin_torque_gym_amd as stg  # noqa: E402

K = 8
SIZE = (4, 4)


def algorithmic_bytes(mode, variant):
    """Bytes one array-step has to move: (i) pattern + target + state + action in, addressed cells + observation + reward + flags + state
    out (bench.py's count); fused: pattern and state once per K steps, the target once per step, outputs per step or once per K."""
    ndev = SIZE[0] * SIZE[1]
    a_dim = 2 if mode == "global" else 3
    affected = {"individual": 1, "row": SIZE[1], "column": SIZE[0], "global": ndev}[mode]
    out = ndev * 24 + 4 + 8 + 8 + 2                  # observation (6 floats per cell), reward, reward_f64, energy, flags
    if variant == "step x8":
        return (ndev * 24 * 2 + 12 + 4 * a_dim) + (affected * 24 + out + 12)
    state = (2 * ndev * 24 + 2 * 12) / K
    return state + ndev * 24 + 4 * a_dim + (out if "every" in variant else out / K)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
    blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ndev = SIZE[0] * SIZE[1]
    rows = []
    for mode in ("individual", "row", "column", "global"):
        a_dim = 2 if mode == "global" else 3
        g = torch.Generator(device="cpu").manual_seed(5)
        acts = torch.empty((K, a_dim, n), dtype=torch.float32)
        if mode == "global":
            acts[:, 0] = (torch.rand((K, n), generator=g) * 2 - 1) * 2e6
            acts[:, 1] = (torch.rand((K, n), generator=g) * 2 - 1) * 2e6          # read as the current (reference quirk)
        else:
            acts[:, 0] = torch.rand((K, n), generator=g) * ndev
            acts[:, 1] = (torch.rand((K, n), generator=g) * 2 - 1) * 2e6
            acts[:, 2] = 1e-10 + torch.rand((K, n), generator=g) * 9e-10
        variants = {}
        for name, out_every, autoreset in (("step x8", None, 0), ("many every", 1, 0), ("many last", 0, 0), ("many every+reset", 1, 1),
                                           ("many last+reset", 0, 1)):
            env = stg.SpinTorqueArrayVecEnv(n, SIZE, action_mode=mode, seed=3, max_steps=200, success_threshold=2.0)
            env.reset(seed=1)
            b = env.backend
            b.set_state(step_count=torch.randint(0, 200, (n,), generator=torch.Generator().manual_seed(11), dtype=torch.int32))
            a = acts.to(b.device)
            if out_every is None:
                run = lambda b=b, a=a: [b.step(a[k]) for k in range(K)]
            else:
                out = b.many_outputs(K, out_every, autoreset)
                run = lambda b=b, a=a, oe=out_every, ar=autoreset, out=out: b.step_many(a, oe, ar, 7, out)
            for _ in range(3):
                run()
            variants[name] = (env, run, [])
        torch.cuda.synchronize()
        for _ in range(blocks):
            for name, (env, run, times) in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    run()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e6 / (reps * K * n))           # ns per array-step
        for name, (env, run, times) in variants.items():
            env.close()
            t = np.array(times)
            by = algorithmic_bytes(mode, name)
            rows.append(dict(mode=mode, variant=name, n=n, K=K, blocks=blocks, reps=reps, ns_per_array_step_median=float(np.median(t)),
                             ns_min=float(t.min()), ns_max=float(t.max()), bytes_per_array_step=round(by, 1),
                             gb_per_s=round(by / float(np.median(t)), 1)))
            r = rows[-1]
            print(f"{mode:10s} {name:17s} {r['ns_per_array_step_median']:.4f} ns/array-step (event span)  ({r['ns_min']:.4f} .. {r['ns_max']:.4f})  "
                  f"{r['bytes_per_array_step']:7.1f} B  {r['gb_per_s']:7.1f} GB/s", flush=True)
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()

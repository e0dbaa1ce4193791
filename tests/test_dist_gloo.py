"""N > 1 path on CPU: world_size-2 over gloo.  The sharding, the global-index Philox keying and the single
(obs, reward, done) all-gather are the product's code (spin_torque_gym_amd/distributed.py); the per-rank compute is
the oracle, injected through the backend test seam (there is no GPU here)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import stt_default_params


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n, steps, q):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (root, os.path.join(root, "spin-torque-rl-gym_amd"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from helpers import OracleBackend
    from spin_torque_gym_amd.distributed import ShardedSpinTorqueVecEnv
    m0, tgt, acts = _inputs(n, steps)
    kw = dict(device_params=stt_default_params(volume=8.75e-11), include_thermal_fluctuations=True, seed=77, backend=OracleBackend)
    env = ShardedSpinTorqueVecEnv(n, **kw)
    obs, _ = env.reset(options={"initial_state": m0, "target_state": tgt})
    rec = [obs.clone()]
    for k in range(steps):
        obs, r, te, tr, _ = env.step(torch.from_numpy(acts[k]))
        # what the learner gets are typed strided VIEWS of the global record array: Gym's [N,12] orientation, no copies
        assert tuple(obs.shape) == (n, 12) and obs.dtype == torch.float32 and tuple(obs.stride()) == (14, 1)
        assert tuple(r.shape) == (n,) and r.dtype == torch.float32 and te.dtype == torch.bool and tr.dtype == torch.bool
        glob = [g.untyped_storage().data_ptr() for g in env._glob]
        assert all(t.untyped_storage().data_ptr() in glob for t in (obs, r, te, tr))
        rec.append((obs.clone(), r.clone(), te.clone(), tr.clone()))
    assert (env.lo, env.hi) == (rank * n // world, (rank + 1) * n // world)
    # split form of the collective (gather_begin / gather_end; overlaps the next kernel on a GPU, synchronous over gloo),
    # pipelined over the two global arrays: step k's gather is collected after step k+1 was enqueued
    env2 = ShardedSpinTorqueVecEnv(n, **kw)
    env2.reset(options={"initial_state": m0, "target_state": tgt}, gather=False)
    piped = []
    for k in range(steps):
        env2.step(torch.from_numpy(acts[k]), gather=False)
        if k:
            piped.append(tuple(t.clone() for t in env2.gather_end()))
        env2.gather_begin()
    piped.append(tuple(t.clone() for t in env2.gather_end()))
    for a, b in zip(rec[1:], piped):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the one-shot point-to-point exchange gives the same global arrays as the all-gather
    env3 = ShardedSpinTorqueVecEnv(n, gather_algo="p2p", **kw)
    o3, _ = env3.reset(options={"initial_state": m0, "target_state": tgt})
    assert torch.equal(o3, rec[0])
    for k in range(steps):
        out3 = env3.step(torch.from_numpy(acts[k]))[:4]
        assert all(torch.equal(x, y) for x, y in zip(out3, rec[k + 1]))
    # a centralised learner: rank 0 scatters the global actions, every rank steps its shard with local actions
    env4 = ShardedSpinTorqueVecEnv(n, **kw)
    env4.reset(options={"initial_state": m0, "target_state": tgt})
    for k in range(steps):
        loc = env4.scatter_actions(torch.from_numpy(acts[k]) if rank == 0 else None, src=0)
        assert tuple(loc.shape) == (n // world, 2) and torch.equal(loc, torch.from_numpy(acts[k])[env4.lo:env4.hi])
        out4 = env4.step(loc, actions_are_local=True)[:4]
        assert all(torch.equal(x, y) for x, y in zip(out4, rec[k + 1]))
    st = env.get_performance_stats()["profiler"]
    assert st["gather_begin_count"] == steps + 1 and st["step_count"] == steps
    # ragged shards (num_envs not divisible by the ranks): the exchange switches to point-to-point, results unchanged
    nr = n - 1
    env5 = ShardedSpinTorqueVecEnv(nr, **kw)
    assert env5.gather_algo == "p2p" and (env5.hi - env5.lo) in (nr // world, nr // world + 1)
    o5, _ = env5.reset(options={"initial_state": m0[:nr], "target_state": tgt[:nr]})
    assert torch.equal(o5, rec[0][:nr])
    for k in range(steps):
        loc = env5.scatter_actions(torch.from_numpy(acts[k][:nr]) if rank == 0 else None, src=0)
        out5 = env5.step(loc, actions_are_local=True)[:4]
        assert all(torch.equal(x, y[:nr]) for x, y in zip(out5, rec[k + 1]))
    if rank == 0:
        q.put(_to_numpy(rec))
    dist.barrier()
    dist.destroy_process_group()


def _to_numpy(rec):
    """By value through the queue: a torch tensor travels as a shared-memory handle that the receiver can only open while the
    sending process is alive -- the worker may have exited by then (seen once as FileNotFoundError in the parent)."""
    return [x.numpy().copy() if torch.is_tensor(x) else tuple(t.numpy().copy() for t in x) for x in rec]


def _from_numpy(rec):
    return [torch.from_numpy(x) if isinstance(x, np.ndarray) else tuple(torch.from_numpy(t) for t in x) for x in rec]


def _inputs(n, steps):
    rng = np.random.default_rng(5)
    v = rng.normal(0, 1, (n, 3))
    m0 = v / np.linalg.norm(v, axis=1, keepdims=True)
    tgt = np.where(rng.integers(0, 2, (n, 1)) == 0, 1.0, -1.0) * np.array([[0.0, 0.0, 1.0]])
    acts = np.empty((steps, n, 2), dtype=np.float32)
    acts[..., 0] = rng.uniform(-2e6, 2e6, (steps, n))
    acts[..., 1] = rng.uniform(1e-10, 3e-10, (steps, n))
    return m0, tgt, acts


@pytest.mark.timeout(300)
def test_two_rank_sharded_env_equals_single_process(oracle_mod):
    import spin_torque_gym_amd as stg
    from helpers import OracleBackend
    n, steps, world = 48, 2, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, steps, q)) for r in range(world)]
    for p in procs:
        p.start()
    rec = _from_numpy(q.get(timeout=240))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # single-process run over all n envs
    m0, tgt, acts = _inputs(n, steps)
    env = stg.SpinTorqueVecEnv(n, diagnostics=True, device_params=stt_default_params(volume=8.75e-11), include_thermal_fluctuations=True,
                               seed=77, backend=OracleBackend)
    obs, _ = env.reset(options={"initial_state": m0, "target_state": tgt})
    assert torch.equal(rec[0], obs)
    for k in range(steps):
        obs, r, te, tr, _ = env.step(torch.from_numpy(acts[k]))
        o2, r2, te2, tr2 = rec[k + 1]
        # bit-identical: the thermal stream is keyed by the global env index, not by the rank-local one
        assert torch.equal(o2, obs) and torch.equal(r2, r) and torch.equal(te2, te) and torch.equal(tr2, tr)


def _subgroup_worker(rank, world, port, n, steps, q):
    """world_size 3, the env lives on the sub-group [1, 2] (group rank != global rank; global rank 0 idles): every
    point-to-point operation has to address its peer by GLOBAL rank (torch.distributed.P2POp)."""
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (root, os.path.join(root, "spin-torque-rl-gym_amd"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    members = [1, 2]
    grp = dist.new_group(members)                     # (every rank of the world calls new_group)
    if rank in members:
        from helpers import OracleBackend
        from spin_torque_gym_amd.distributed import ShardedSpinTorqueVecEnv
        m0, tgt, acts = _inputs(n, steps)
        kw = dict(device_params=stt_default_params(volume=8.75e-11), include_thermal_fluctuations=True, seed=77, backend=OracleBackend)
        outs = {}
        for name, nn, algo in (("all_gather", n, "all_gather"), ("p2p", n, "p2p"), ("ragged", n - 1, "all_gather")):
            env = ShardedSpinTorqueVecEnv(nn, group=grp, gather_algo=algo, **kw)
            assert env.world == 2 and env.rank == members.index(rank) and env._global == members
            o, _ = env.reset(options={"initial_state": m0[:nn], "target_state": tgt[:nn]})
            rec = [o.clone()]
            for k in range(steps):
                # a centralised learner on GROUP rank 1 (= global rank 2) scatters the actions
                loc = env.scatter_actions(torch.from_numpy(acts[k][:nn]) if env.rank == 1 else None, src=1)
                assert torch.equal(loc, torch.from_numpy(acts[k][:nn])[env.lo:env.hi])
                rec.append(tuple(t.clone() for t in env.step(loc, actions_are_local=True)[:4]))
            outs[name] = rec
        for k in range(1, steps + 1):
            assert all(torch.equal(x, y) for x, y in zip(outs["all_gather"][k], outs["p2p"][k]))
            assert all(torch.equal(x[:n - 1], y) for x, y in zip(outs["all_gather"][k], outs["ragged"][k]))
        if rank == members[0]:
            q.put(_to_numpy(outs["p2p"]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_env_on_a_subgroup_addresses_peers_by_global_rank(oracle_mod):
    """ADVICE r2 / VERDICT r2 item 8: group != world."""
    import spin_torque_gym_amd as stg
    from helpers import OracleBackend
    n, steps, world = 32, 2, 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_subgroup_worker, args=(r, world, port, n, steps, q)) for r in range(world)]
    for p in procs:
        p.start()
    rec = _from_numpy(q.get(timeout=240))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    m0, tgt, acts = _inputs(n, steps)
    env = stg.SpinTorqueVecEnv(n, device_params=stt_default_params(volume=8.75e-11), include_thermal_fluctuations=True,
                               seed=77, backend=OracleBackend)
    obs, _ = env.reset(options={"initial_state": m0, "target_state": tgt})
    assert torch.equal(rec[0], obs)
    for k in range(steps):
        obs, r, te, tr, _ = env.step(torch.from_numpy(acts[k]))
        o2, r2, te2, tr2 = rec[k + 1]
        assert torch.equal(o2, obs) and torch.equal(r2, r) and torch.equal(te2, te) and torch.equal(tr2, tr)


# ------------------------------------------------------------------------------------------------
# noise_model='brown' on the oracle: the shards' streams are keyed by the global env index under this model too
# ------------------------------------------------------------------------------------------------
BROWN_VOLUME = 1e-26          # (tests/wave_config_cases.py: VOL_THERMAL; currents scaled by the volume ratio)


def _brown_kw():
    from helpers import OracleBackend
    return dict(device_params=stt_default_params(volume=BROWN_VOLUME), include_thermal_fluctuations=True, seed=77, solver="rk4",
                noise_model="brown", temperature=450.0, max_current=2e6 * BROWN_VOLUME / 8.75e-11, backend=OracleBackend)


def _brown_inputs(n, steps):
    m0, tgt, acts = _inputs(n, steps)
    acts[..., 0] *= np.float32(BROWN_VOLUME / 8.75e-11)
    return m0, tgt, acts


def _brown_worker(rank, world, port, n, steps, q):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (root, os.path.join(root, "spin-torque-rl-gym_amd"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from spin_torque_gym_amd.distributed import ShardedSpinTorqueVecEnv
    m0, tgt, acts = _brown_inputs(n, steps)
    env = ShardedSpinTorqueVecEnv(n, **_brown_kw())
    assert env.local.backend.ocfg.noise_model == 2 and env.local.env_id0 == rank * n // world
    obs, _ = env.reset(options={"initial_state": m0, "target_state": tgt})
    rec = [obs.clone()]
    for k in range(steps):
        rec.append(tuple(t.clone() for t in env.step(torch.from_numpy(acts[k]))[:4]))
    if rank == 0:
        q.put(_to_numpy(rec))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_sharded_env_under_the_brown_field_equals_single_process(oracle_mod):
    """2 ranks, 2 steps, noise_model='brown' on the oracle: the gathered records equal the one-process OracleBackend env's bit for bit,
    and the Brown field is what ran (the same env under 'white' gives other observations)"""
    import spin_torque_gym_amd as stg
    n, steps, world = 16, 2, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_brown_worker, args=(r, world, port, n, steps, q)) for r in range(world)]
    for p in procs:
        p.start()
    rec = _from_numpy(q.get(timeout=240))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    m0, tgt, acts = _brown_inputs(n, steps)
    last = {}
    for noise in ("brown", "white"):
        env = stg.SpinTorqueVecEnv(n, **dict(_brown_kw(), noise_model=noise))
        obs, _ = env.reset(options={"initial_state": m0, "target_state": tgt})
        assert torch.equal(rec[0], obs)
        for k in range(steps):
            obs, r, te, tr, _ = env.step(torch.from_numpy(acts[k]))
            if noise == "brown":
                o2, r2, te2, tr2 = rec[k + 1]
                assert torch.equal(o2, obs) and torch.equal(r2, r) and torch.equal(te2, te) and torch.equal(tr2, tr)
        last[noise] = obs.clone()
        env.close()
    assert float((last["brown"][:, :3] - last["white"][:, :3]).abs().max()) > 1e-2


def test_shard_range_partitions():
    from spin_torque_gym_amd.distributed import shard_range
    for n, w in ((1048576, 8), (10, 3), (7, 8)):
        spans = [shard_range(n, w, r) for r in range(w)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        sizes = [b - a for a, b in spans]
        assert max(sizes) - min(sizes) <= 1

"""Sharded rollouts and checkpoints on the GPU (`pytest -m gpu`): ShardedSpinTorqueVecEnv.step_many / state_dict / load_state_dict over the
HIP backend with two live ranks.

As in tests/test_gpu_multirank.py the two ranks share cuda:0 and exchange over gloo (one GPU here, and RCCL refuses two ranks on one GPU);
everything else is the product's path: ONE stg_step_many launch per rank in the records layout, the blocks of step k gathered into
out[k, lo_r:hi_r] of the [K, N_global, 56] record array, typed views, and -- with overlap=True -- the exchange on the side stream.
tests/test_dist_checkpoint.py covers the same host logic on CPU with the oracle as the backend, at 2 and 3 ranks.

N_GLOBAL = 193 = 3 wavefronts + 1 lane; the shards are 97 + 96 envs (ragged, so the exchange is the point-to-point one), and the boundary
at env 97 splits a 128-byte pair of state records.  max_steps = 3: every env is reset on the device inside the K = 4 launch and again in
the K = 2 continuation after the checkpoint.

Processes: the pytest process plus the two ranks, later plus one fresh child -- three with the GPU open at most.  Every child is a new
interpreter (spawn), waited for under a time limit of its own and killed and joined when that runs out; once a child has failed -- fault,
abort, time limit or a plain exception -- nothing else in this file starts on the GPU (`_TROUBLE`).
"""
import functools
import os
import queue as _queue
import socket
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import stt_default_params

pytestmark = pytest.mark.gpu

N_GLOBAL, K, K2, SLICE, SENTINEL = 193, 4, 2, 32, -7.5
KW = dict(include_thermal_fluctuations=True, temperature=300.0, solver="rk45", seed=1234, autoreset=True, max_steps=3)
STATE_KEYS = ("m", "target", "total_energy", "step_count", "rng_step", "done")
CHILD_TIMEOUT = 180                      # s per child: interpreter + HIP start-up dominate; the launches themselves take milliseconds
_TROUBLE = []                            # why nothing more may start on the GPU from this file


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _kw():
    return dict(KW, device_params=stt_default_params(volume=9.7e-6))


def _inputs():
    rng = np.random.default_rng(2025)
    v = rng.normal(0, 1, (N_GLOBAL, 3))
    m0 = v / np.linalg.norm(v, axis=1, keepdims=True)
    tgt = np.where(rng.integers(0, 2, (N_GLOBAL, 1)) == 0, 1.0, -1.0) * np.array([[0.0, 0.0, 1.0]])
    acts = np.empty((K + K2, N_GLOBAL, 2), dtype=np.float32)
    acts[..., 0] = rng.uniform(-2e6, 2e6, (K + K2, N_GLOBAL))
    acts[..., 1] = rng.uniform(1e-10, 6e-10, (K + K2, N_GLOBAL))
    return m0, tgt, torch.from_numpy(acts)


def _np(x):
    if torch.is_tensor(x):
        return x.cpu().numpy().copy()
    if isinstance(x, dict):
        return {k: _np(v) for k, v in x.items()}
    return x


def _child_paths():
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (root, os.path.join(root, "spin-torque-rl-gym_amd"), here):
        if p not in sys.path:
            sys.path.insert(0, p)


# -- the children ----------------------------------------------------------------------------------------------------------------------
def _rank_job(rank, world):
    from spin_torque_gym_amd.backend import HipBackend
    from spin_torque_gym_amd.distributed import ShardedSpinTorqueVecEnv
    m0, tgt, acts = _inputs()
    opts = {"initial_state": m0, "target_state": tgt}
    dev_acts = acts.cuda()
    runs = {}
    for name, overlap in (("plain", None), ("overlap", True)):
        env = ShardedSpinTorqueVecEnv(N_GLOBAL, overlap=overlap, **_kw())
        assert isinstance(env.local.backend, HipBackend) and env.device.type == "cuda" and env._overlap is bool(overlap)
        assert (env.lo, env.hi) == ((0, 97), (97, 193))[rank] and env.gather_algo == "p2p"
        env.reset(options=opts)
        before = env.local.backend.counters()["env_steps"]
        obs, r, te, tr, info = env.step_many(dev_acts[:K] if overlap else acts[:K])
        torch.cuda.synchronize()
        steps = env.local.backend.counters()["env_steps"] - before
        rec = info["records"]
        assert rec.is_cuda and tuple(rec.shape) == (K, N_GLOBAL, 56) and rec.is_contiguous()
        assert tuple(obs.shape) == (K, N_GLOBAL, 12) and tuple(obs.stride()) == (14 * N_GLOBAL, 14, 1)
        assert all(t.untyped_storage().data_ptr() == rec.untyped_storage().data_ptr() for t in (obs, r, te, tr, info["status"]))
        assert te.dtype == torch.bool and tuple(info["final_obs"].shape) == (K, N_GLOBAL, 12)
        runs[name] = (env, rec, info["final_obs"], steps)
    (env, rec, fin, steps), (env_o, rec_o, fin_o, steps_o) = runs["plain"], runs["overlap"]
    assert torch.equal(rec, rec_o) and torch.equal(fin, fin_o) and steps == steps_o
    # K calls of the sharded step: the same records
    by_step = ShardedSpinTorqueVecEnv(N_GLOBAL, **_kw())
    by_step.reset(options=opts)
    for k in range(K):
        by_step.step(acts[k])
        assert torch.equal(by_step._glob[by_step._last], rec[k]), ("step_many vs step", k)
    # local actions, and a final_obs array of the caller's: rows of envs that did not end at a step keep the sentinel
    pre = ShardedSpinTorqueVecEnv(N_GLOBAL, **_kw())
    pre.reset(options=opts)
    buf = torch.full((K, N_GLOBAL, 12), SENTINEL, dtype=torch.float32, device="cuda")
    pinfo = pre.step_many(acts[:K, pre.lo:pre.hi].clone(), actions_are_local=True, final_obs_out=buf)[4]
    ended = te | tr
    assert torch.equal(pinfo["records"], rec) and pinfo["final_obs"] is buf and bool(ended[2].any()) and not bool(ended[0].all())
    assert bool((buf[~ended] == SENTINEL).all()) and torch.equal(buf[ended], fin[ended]) and bool((fin[~ended] == 0).all())
    # the checkpoint of this rank, and the gathered one
    st = env.state_dict()
    assert all(st[k].is_cuda for k in STATE_KEYS) and (st["lo"], st["hi"], st["n_global"], st["world"], st["rank"]) == (env.lo, env.hi, N_GLOBAL, 2, rank)
    full = env.state_dict(gather_to=0)
    # resume in place from the own dict while a gather is in flight on the side stream, then the K2 continuation
    env_o.step(dev_acts[K], gather=False)
    env_o.gather_begin()
    env_o.load_state_dict(st)
    assert not env_o.gather_in_flight and env_o._filled is None and env_o._done == [None, None]
    cont = env_o.step_many(dev_acts[K:])[4]
    torch.cuda.synchronize()
    out = dict(env_steps=steps, shard_state=_np(st), cont_records=_np(cont["records"]), cont_final=_np(cont["final_obs"]))
    if rank == 0:
        out.update(records=_np(rec), final_obs=_np(fin), full_state=_np(full))
    for e in (env, env_o, by_step, pre):
        e.close()
    return out


def _rank_worker(rank, world, port, q):
    _child_paths()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        q.put((rank, True, _rank_job(rank, world)))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        q.put((rank, False, traceback.format_exc()))
        raise


def _resume_worker(rank, world, shards, q):
    """A fresh process: a one-process SpinTorqueVecEnv of all 193 envs resumes from the two per-rank dicts and runs the K2 continuation."""
    _child_paths()
    try:
        import spin_torque_gym_amd as stg
        from spin_torque_gym_amd.distributed import _records_behind
        _, _, acts = _inputs()
        env = stg.SpinTorqueVecEnv(N_GLOBAL, **_kw())
        env.load_state_dict(shards)
        before = env.backend.counters()["env_steps"]
        obs, r, te, tr, info = env.step_many(acts[K:])
        rec = _records_behind(obs, r, te, tr, info["status"])
        out = dict(records=_np(rec), final_obs=_np(info["final_obs"]), state=_np(env.state_dict()),
                   env_steps=env.backend.counters()["env_steps"] - before)
        env.close()
        q.put((rank, True, out))
    except BaseException:
        q.put((rank, False, traceback.format_exc()))
        raise


def _run_children(target, world, args):
    """`world` fresh processes of `target(rank, world, *args, q)`; their results by rank.  Each child has CHILD_TIMEOUT seconds to report;
    after a failure or a timeout every child still alive is killed and joined, and `_TROUBLE` keeps this file off the GPU from then on."""
    if _TROUBLE:
        pytest.fail("not started: an earlier child of this file failed (" + _TROUBLE[0].splitlines()[0] + ")")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, *args, q)) for r in range(world)]
    for p in procs:
        p.start()
    got, failure = {}, None
    try:
        while len(got) < world and failure is None:
            try:
                rank, ok, res = q.get(timeout=CHILD_TIMEOUT)
            except _queue.Empty:
                failure = f"no result from ranks {sorted(set(range(world)) - set(got))} within {CHILD_TIMEOUT} s"
                break
            if ok:
                got[rank] = res
            else:
                failure = f"rank {rank} failed:\n{res}"
        if failure is None:
            for p in procs:
                p.join(timeout=60)
    finally:
        for p in procs:
            if p.is_alive():
                failure = failure or f"a child did not exit within 60 s of reporting (pid {p.pid})"
                p.kill()
            p.join()
    codes = [p.exitcode for p in procs]
    if failure is None and codes != [0] * world:
        failure = f"children exited with {codes}"
    if failure is not None:
        _TROUBLE.append(failure)
        pytest.fail(failure)
    return got


@functools.lru_cache(maxsize=None)
def _two_ranks():
    return _run_children(_rank_worker, 2, (_free_port(),))


@functools.lru_cache(maxsize=None)
def _one_process():
    """The uninterrupted one-process run: K steps in one launch, then K2 more.  Only after the ranks came back clean."""
    import spin_torque_gym_amd as stg
    from spin_torque_gym_amd.distributed import _records_behind
    _two_ranks()
    m0, tgt, acts = _inputs()
    env = stg.SpinTorqueVecEnv(N_GLOBAL, **_kw())
    env.reset(options={"initial_state": m0, "target_state": tgt})
    out = {}
    for name, a in (("first", acts[:K]), ("cont", acts[K:])):
        obs, r, te, tr, info = env.step_many(a)
        out[name] = dict(records=_np(_records_behind(obs, r, te, tr, info["status"])), final_obs=_np(info["final_obs"]),
                         state=_np(env.state_dict()))
    assert env.backend.counters()["env_steps"] == (K + K2) * N_GLOBAL
    env.close()
    return out


# -- the tests -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_sharded_rollout_equals_one_process_and_oracle():
    """Two HIP ranks, 193 envs (97 + 96), rk45 + thermal field + autoreset, K = 4 in one launch per rank: the gathered [K, N_global] record
    array and final_obs equal the one-process SpinTorqueVecEnv.step_many byte for byte; one oracle slice per shard agrees within the
    tolerances of tests/test_gpu_multirank.py (its oracle loop: obs rtol 3e-7 / atol 1e-7, reward rtol 1e-6 / atol 1e-7, terminal rows of
    ended envs atol 2e-6 -- taken from there unchanged); the ranks' env_steps counters advanced by K * N_global together."""
    import spin_torque_gym_amd as stg
    from helpers import OracleBackend
    from spin_torque_gym_amd.backend import record_views
    assert torch.cuda.is_available()
    ranks = _two_ranks()
    one = _one_process()
    rec, want = torch.from_numpy(ranks[0]["records"]), torch.from_numpy(one["first"]["records"])
    assert rec.dtype == torch.uint8 and tuple(rec.shape) == (K, N_GLOBAL, 56)
    assert torch.equal(rec, want), ("two ranks vs one process", int((rec != want).sum()))
    assert torch.equal(torch.from_numpy(ranks[0]["final_obs"]), torch.from_numpy(one["first"]["final_obs"]))
    assert ranks[0]["env_steps"] + ranks[1]["env_steps"] == K * N_GLOBAL and ranks[0]["env_steps"] == K * 97
    ended_any = (rec[..., 52] | rec[..., 53]).bool()
    assert bool(ended_any.any(dim=0).all())                      # max_steps = 3: every env was reset on the device inside the launch
    # the gathered checkpoint is the one-process one, and the per-rank dicts are its slices
    for k in STATE_KEYS:
        assert np.array_equal(ranks[0]["full_state"][k], one["first"]["state"][k]), k
        for r, (lo, hi) in enumerate(((0, 97), (97, 193))):
            assert np.array_equal(ranks[r]["shard_state"][k], one["first"]["state"][k][..., lo:hi]), (r, k)
    # the oracle on one slice per shard, keyed by env_id0 (the second one ends at the last, odd env)
    m0, tgt, acts = _inputs()
    worst = 0.0
    for s0 in (60, N_GLOBAL - SLICE):
        sl = slice(s0, s0 + SLICE)
        ora = stg.SpinTorqueVecEnv(SLICE, diagnostics=True, env_id0=s0, backend=OracleBackend, **_kw())
        ora.reset(options={"initial_state": m0[sl], "target_state": tgt[sl]})
        redrawn = np.zeros(SLICE, dtype=bool)
        for k in range(K):
            o, r, te, tr, info = ora.step(acts[k][sl])
            ho, hr, hte, htr, hst = (t.numpy() for t in record_views(rec[k][sl]))
            clean = ~redrawn
            assert np.array_equal(hte[clean].astype(bool), te.numpy()[clean]) and np.array_equal(htr[clean].astype(bool), tr.numpy()[clean]), (s0, k)
            assert np.array_equal(hst[clean], info["status"].numpy()[clean]), (s0, k)
            ended = (te.numpy() | tr.numpy()) & clean
            keep = clean & ~ended            # (an env that ended holds a state redrawn from fp32 device normals: 1e-7 from libm's)
            d = np.abs(ho[keep] - o.numpy()[keep])
            worst = max(worst, float(d[:, :3].max(initial=0.0)))
            assert np.allclose(ho[keep], o.numpy()[keep], rtol=3e-7, atol=1e-7), (s0, k, d.max())
            assert np.allclose(hr[clean], r.numpy()[clean], rtol=1e-6, atol=1e-7), (s0, k)
            assert np.allclose(ho[ended], o.numpy()[ended], rtol=0, atol=2e-6), (s0, k)
            redrawn |= ended
        assert redrawn.all()
        ora.close()
    print("sharded step_many, two HIP ranks, 193 envs rk45 + thermal: worst |obs m - oracle| on slices =", worst)


@pytest.mark.timeout(600)
def test_checkpoint_resumes_in_another_process_bit_for_bit():
    """The two per-rank dicts saved after the rollout, loaded into a one-process SpinTorqueVecEnv(193) in a fresh child, K = 2 more steps: the
    records, final_obs and the final state equal the uninterrupted one-process run's -- and so does the sharded env's own continuation,
    resumed in place from its dicts while a gather was in flight on the side stream."""
    ranks = _two_ranks()
    one = _one_process()
    want = one["cont"]
    cont = torch.from_numpy(ranks[0]["cont_records"])
    assert torch.equal(cont, torch.from_numpy(want["records"])), ("sharded resume", int((cont != torch.from_numpy(want["records"])).sum()))
    assert np.array_equal(ranks[1]["cont_records"], want["records"]) and np.array_equal(ranks[0]["cont_final"], want["final_obs"])
    got = _run_children(_resume_worker, 1, ([ranks[1]["shard_state"], ranks[0]["shard_state"]],))[0]
    rec = torch.from_numpy(got["records"])
    assert rec.dtype == torch.uint8 and tuple(rec.shape) == (K2, N_GLOBAL, 56)
    assert torch.equal(rec, torch.from_numpy(want["records"])), ("2 ranks -> 1 process", int((rec != torch.from_numpy(want["records"])).sum()))
    assert np.array_equal(got["final_obs"], want["final_obs"]) and got["env_steps"] == K2 * N_GLOBAL
    for k in STATE_KEYS:
        assert np.array_equal(got["state"][k], want["state"][k]), k
    assert bool((rec[..., 52] | rec[..., 53]).any())                     # envs ended -- and were redrawn on the device -- after the resume too

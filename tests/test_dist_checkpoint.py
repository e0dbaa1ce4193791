"""ShardedSpinTorqueVecEnv: checkpoint, resume at another world size, K fused steps per launch -- on CPU, gloo ranks over the oracle backend
(started the way tests/test_dist_gloo.py starts its ranks; tests/test_gpu_multirank_rollout.py runs the HIP backend through the same code).

Everything compared here is two runs of the same backend doing the same per-env arithmetic under different partitions of the envs, so every
comparison is `array_equal`: an env's Philox streams are keyed by (seed, GLOBAL env id, rng_step), all of which a checkpoint carries.
N_GLOBAL = 37 is odd on purpose: the shards are ragged at 2 ranks (19 + 18) and at 3 (13 + 12 + 12), no boundary of one partition is a
boundary of the other, and 19 and 13 are odd, so a boundary falls inside a 128-byte pair of state records.  max_steps = 3 ends every episode
after three steps at the latest, so every env is reset on the device at least twice in the 8 steps, on both sides of the checkpoint.
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

N_GLOBAL, STEPS, HALF, K_MANY = 37, 8, 4, 3
SEED, RESET_SEED, SENTINEL = 77, 11, -7.5
STATE_KEYS = ("m", "target", "total_energy", "step_count", "rng_step", "done")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _kw(autoreset=True, **over):
    from helpers import OracleBackend
    kw = dict(device_params=stt_default_params(volume=8.75e-11), include_thermal_fluctuations=True, solver="rk4", seed=SEED, max_steps=3,
              autoreset=autoreset, backend=OracleBackend)
    kw.update(over)
    return kw


def _actions():
    rng = np.random.default_rng(9)
    a = np.empty((STEPS, N_GLOBAL, 2), dtype=np.float32)
    a[..., 0] = rng.uniform(-2e6, 2e6, (STEPS, N_GLOBAL))
    a[..., 1] = rng.uniform(1e-10, 3e-10, (STEPS, N_GLOBAL))
    return torch.from_numpy(a)


def _np(x):
    """By value through the queue (a torch tensor would travel as a shared-memory handle of a process that may be gone by then)."""
    if torch.is_tensor(x):
        return x.cpu().numpy().copy()
    if isinstance(x, dict):
        return {k: _np(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_np(v) for v in x]
    return x


def _rollout(env, acts):
    """step_many(acts) -> dict of numpy arrays with a leading K: what the learner sees."""
    obs, r, te, tr, info = env.step_many(acts)
    out = dict(obs=obs, reward=r, terminated=te, truncated=tr)
    if "final_obs" in info:
        out["final_obs"] = info["final_obs"]
    return _np(out)


def _cat(rolls):
    return {k: np.concatenate([r[k] for r in rolls], axis=0) for k in rolls[0]}


def _same(a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (what, k)


def _state_same(a, b, what, keys=STATE_KEYS):
    for k in keys:
        x, y = np.asarray(_np(a[k])), np.asarray(_np(b[k]))
        assert x.dtype == y.dtype and np.array_equal(x, y), (what, k)


# -- the uninterrupted one-process runs: computed once, never modified ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference():
    import spin_torque_gym_amd as stg
    acts = _actions()
    env = stg.SpinTorqueVecEnv(N_GLOBAL, **_kw())
    env.reset(seed=RESET_SEED)
    steps, state = [], {}
    for k in range(STEPS):
        steps.append(_rollout(env, acts[k:k + 1]))
        if k + 1 in (HALF, 6, STEPS):
            state[k + 1] = _np(env.state_dict())
    ended = np.stack([s["terminated"][0] | s["truncated"][0] for s in steps])
    assert ended.sum(axis=0).min() >= 2                          # max_steps = 3: every env was reset on the device at least twice
    ref = dict(steps=steps, state=state, many={})
    for auto in (True, False):
        for out_every in (True, False):
            e = stg.SpinTorqueVecEnv(N_GLOBAL, **_kw(autoreset=auto))
            e.reset(seed=RESET_SEED)
            obs, r, te, tr, info = e.step_many(acts[:K_MANY], out_every=out_every)
            d = dict(obs=obs, reward=r, terminated=te, truncated=tr)
            if auto:
                d["final_obs"] = info["final_obs"]
            ref["many"][(auto, out_every)] = _np(d)
    return ref


# -- what the ranks run ----------------------------------------------------------------------------------------------------------------
def _check_step_many(rank, world):
    """Sharded step_many against K calls of sharded step, with local actions, and with a prefilled final_obs array; returns the views."""
    from spin_torque_gym_amd.distributed import ShardedSpinTorqueVecEnv
    acts = _actions()[:K_MANY]
    got = {}
    for auto in (True, False):
        by_step = ShardedSpinTorqueVecEnv(N_GLOBAL, **_kw(autoreset=auto))
        by_step.reset(seed=RESET_SEED)
        single = [tuple(t.clone() for t in by_step.step(acts[k])[:4]) for k in range(K_MANY)]
        for out_every in (True, False):
            env = ShardedSpinTorqueVecEnv(N_GLOBAL, **_kw(autoreset=auto))
            env.reset(seed=RESET_SEED)
            obs, r, te, tr, info = env.step_many(acts, out_every=out_every, autoreset=auto)
            ko = K_MANY if out_every else 1
            # typed strided views of ONE [ko, N_global, 56] record array
            rec = info["records"]
            assert tuple(rec.shape) == (ko, N_GLOBAL, 56) and rec.dtype == torch.uint8 and rec.is_contiguous()
            assert tuple(obs.shape) == (ko, N_GLOBAL, 12) and obs.dtype == torch.float32 and tuple(obs.stride()) == (14 * N_GLOBAL, 14, 1)
            assert tuple(r.shape) == (ko, N_GLOBAL) and r.dtype == torch.float32 and te.dtype == torch.bool and tr.dtype == torch.bool
            base = rec.untyped_storage().data_ptr()
            assert all(t.untyped_storage().data_ptr() == base for t in (obs, r, te, tr, info["status"]))
            assert ("final_obs" in info) == auto
            for j, k in enumerate(range(K_MANY) if out_every else [K_MANY - 1]):
                assert all(torch.equal(x[j], y) for x, y in zip((obs, r, te, tr), single[k])), ("step_many vs step", auto, out_every, k)
            # local actions: the same result
            loc = ShardedSpinTorqueVecEnv(N_GLOBAL, **_kw(autoreset=auto))
            loc.reset(seed=RESET_SEED)
            res = loc.step_many(acts[:, loc.lo:loc.hi].clone(), out_every=out_every, actions_are_local=True)
            assert torch.equal(res[4]["records"], rec), ("actions_are_local", auto, out_every)
            if auto:
                assert torch.equal(res[4]["final_obs"], info["final_obs"])
            # gather=False: this rank's envs only, nothing exchanged
            own = ShardedSpinTorqueVecEnv(N_GLOBAL, **_kw(autoreset=auto))
            own.reset(seed=RESET_SEED)
            lo_, lr, lte, ltr, linfo = own.step_many(acts, out_every=out_every, gather=False)
            assert all(torch.equal(x, y[:, own.lo:own.hi]) for x, y in zip((lo_, lr, lte, ltr), (obs, r, te, tr)))
            if auto:
                assert torch.equal(linfo["final_obs"], info["final_obs"][:, own.lo:own.hi])
            if auto and out_every:
                # rows of envs that did not end at a step stay untouched in an array of the caller's
                pre = ShardedSpinTorqueVecEnv(N_GLOBAL, **_kw(autoreset=auto))
                pre.reset(seed=RESET_SEED)
                buf = torch.full((K_MANY, N_GLOBAL, 12), SENTINEL, dtype=torch.float32)
                pinfo = pre.step_many(acts, final_obs_out=buf)[4]
                ended = te | tr
                assert pinfo["final_obs"] is buf and bool(ended.any()) and not bool(ended.all())
                assert bool((buf[~ended] == SENTINEL).all()) and torch.equal(buf[ended], info["final_obs"][ended])
                assert bool((info["final_obs"][~ended] == 0).all())
            with pytest.raises(ValueError, match="autoreset"):
                env.step_many(acts, autoreset=not auto)
            d = dict(obs=obs, reward=r, terminated=te, truncated=tr)
            if auto:
                d["final_obs"] = info["final_obs"]
            got[(auto, out_every)] = _np(d)
    # equal shards (36 envs divide by 2 and by 3) take the other form of the exchange: one all-gather per step slice
    n_even = 36
    by_step = ShardedSpinTorqueVecEnv(n_even, **_kw())
    assert by_step.gather_algo == "all_gather" and by_step.n_local * world == n_even
    by_step.reset(seed=RESET_SEED)
    single = [by_step.step(acts[k, :n_even], gather=True) and by_step._glob[by_step._last].clone() for k in range(K_MANY)]
    for out_every in (True, False):
        env = ShardedSpinTorqueVecEnv(n_even, **_kw())
        env.reset(seed=RESET_SEED)
        info = env.step_many(acts[:, :n_even], out_every=out_every)[4]
        assert torch.equal(info["records"], torch.stack(single if out_every else single[-1:])), ("all-gather form", out_every)
        assert tuple(info["final_obs"].shape) == (K_MANY if out_every else 1, n_even, 12)
    return got


def _job_two_ranks(rank, world, payload):
    from spin_torque_gym_amd.distributed import ShardedSpinTorqueVecEnv
    acts = _actions()
    out = {}
    env = ShardedSpinTorqueVecEnv(N_GLOBAL, **_kw())
    assert (env.lo, env.hi) == ((0, 19), (19, 37))[rank]
    env.reset(seed=RESET_SEED)
    for k in range(HALF):
        env.step(acts[k])
    st = env.state_dict()
    assert (st["n_global"], st["world"], st["rank"], st["lo"], st["hi"], st["env_id0"], st["cfg_seed"]) == (N_GLOBAL, 2, rank, env.lo, env.hi, env.lo, SEED)
    assert st["config"]["solver"] == "rk4" and st["config"]["max_steps"] == 3 and st["config"]["autoreset"] is True
    assert st["config"]["include_thermal_fluctuations"] is True and st["config"]["noise_model"] == "white"
    assert tuple(st["m"].shape) == (3, env.n_local) and tuple(st["rng_step"].shape) == (env.n_local,)
    out["shard_state"] = _np(st)
    full = env.state_dict(gather_to=0)
    if rank == 0:
        assert (full["lo"], full["hi"], full["env_id0"], full["n_global"]) == (0, N_GLOBAL, 0, N_GLOBAL)
        out["full_state"] = _np(full)
    else:
        assert (full["lo"], full["hi"]) == (env.lo, env.hi)
    # a load ends a gather in flight and leaves the slot ring as new; (a) the per-rank dict of the same world size and rank
    env.step(acts[HALF], gather=False)
    env.gather_begin()
    assert env.gather_in_flight
    env.load_state_dict(st)
    assert not env.gather_in_flight and env._filled is None and env._last is None and env._slot == 0 and env._done == [None, None]
    with pytest.raises(RuntimeError):
        env.gather_begin()
    out["same_world"] = _rollout(env, acts[HALF:])
    # (b) full dicts: a one-process SpinTorqueVecEnv's, and gather_to's (rank 0 has it; the others take theirs from the payload's twin)
    for name, src in (("from_single", payload["single_state"]), ("from_full", payload["single_state"] if rank else full)):
        e = ShardedSpinTorqueVecEnv(N_GLOBAL, **_kw())
        e.load_state_dict(src)
        out[name] = _rollout(e, acts[HALF:])
        end = e.state_dict(gather_to=0)
        if rank == 0:
            out[name + "_state"] = _np(end)
    # rejections: every one a ValueError that names the field
    from spin_torque_gym_amd.envs import assemble_state
    shards = [None] * world
    dist.all_gather_object(shards, out["shard_state"])
    with pytest.raises(ValueError, match="n_global"):
        ShardedSpinTorqueVecEnv(N_GLOBAL + 1, **_kw()).load_state_dict(shards)
    with pytest.raises(ValueError, match="n_global"):
        ShardedSpinTorqueVecEnv(N_GLOBAL + 1, **_kw()).load_state_dict(payload["single_state"])
    with pytest.raises(ValueError, match="solver"):
        ShardedSpinTorqueVecEnv(N_GLOBAL, **_kw(solver="euler")).load_state_dict(shards)
    with pytest.raises(ValueError, match="max_steps"):
        ShardedSpinTorqueVecEnv(N_GLOBAL, **_kw(max_steps=4)).load_state_dict(shards[rank])
    with pytest.raises(ValueError, match="autoreset"):
        ShardedSpinTorqueVecEnv(N_GLOBAL, **_kw(autoreset=False)).load_state_dict(shards)
    fresh = ShardedSpinTorqueVecEnv(N_GLOBAL, **_kw())
    meta = {k: shards[1][k] for k in ("n_global", "cfg_seed", "config", "host_rng")}
    late = dict(assemble_state(shards, 21, N_GLOBAL), lo=21, hi=N_GLOBAL, **meta)            # envs 19 and 20 in nobody's dict
    early = dict(assemble_state(shards, 15, N_GLOBAL), lo=15, hi=N_GLOBAL, **meta)           # envs 15..18 in two dicts
    with pytest.raises(ValueError, match=r"hole.*\[19, 21\)"):
        fresh.load_state_dict([shards[0], late])
    with pytest.raises(ValueError, match=r"hole.*\[19, 37\)"):
        fresh.load_state_dict([shards[0]])
    with pytest.raises(ValueError, match=r"overlap.*\[15, 19\)"):
        fresh.load_state_dict([early, shards[0]])
    with pytest.raises(ValueError, match="overlap"):
        fresh.load_state_dict([shards[0], shards[1], shards[1]])
    with pytest.raises(ValueError, match="cfg_seed"):
        fresh.load_state_dict([shards[0], dict(shards[1], cfg_seed=SEED + 1)])
    with pytest.raises(ValueError, match="lo, hi"):
        fresh.load_state_dict(shards[1 - rank])                  # one dict of ANOTHER rank: it does not hold this rank's envs
    with pytest.raises(RuntimeError):
        fresh.step(acts[0])                                      # ... and none of the refused loads left the env resumed
    out["many"] = _check_step_many(rank, world)
    return out


def _job_three_ranks(rank, world, payload):
    from spin_torque_gym_amd.distributed import ShardedSpinTorqueVecEnv
    acts = _actions()
    out = {}
    env = ShardedSpinTorqueVecEnv(N_GLOBAL, **_kw())
    assert (env.lo, env.hi) == ((0, 13), (13, 25), (25, 37))[rank]
    env.load_state_dict(payload["shards"])                       # (c) the two dicts of the 2-rank run, into 3 ranks
    rolls = [_rollout(env, acts[HALF:6])]
    out["shard_state"] = _np(env.state_dict())
    rolls += [_rollout(env, acts[6:7]), _rollout(env, acts[7:8])]
    out["resumed"] = _cat(rolls)
    end = env.state_dict(gather_to=0)
    if rank == 0:
        out["resumed_state"] = _np(end)
    out["many"] = _check_step_many(rank, world)
    return out


_JOBS = {2: _job_two_ranks, 3: _job_three_ranks}


def _worker(rank, world, port, payload, q):
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (root, os.path.join(root, "spin-torque-rl-gym_amd"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        q.put((rank, True, _JOBS[world](rank, world, payload)))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:
        q.put((rank, False, traceback.format_exc()))
        raise


def _run_ranks(world, payload, timeout=240):
    """Starts `world` gloo ranks, returns their results by rank.  A rank that failed is reported with its traceback; whatever is still
    alive then, or after the timeout, is killed: no rank is left waiting in a collective."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, payload, q)) for r in range(world)]
    for p in procs:
        p.start()
    got, failure = {}, None
    try:
        while len(got) < world and failure is None:
            try:
                rank, ok, res = q.get(timeout=timeout)
            except _queue.Empty:
                failure = f"no result from ranks {sorted(set(range(world)) - set(got))} within {timeout} s"
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
                p.kill()
            p.join()
    if failure is not None:
        raise RuntimeError(failure)
    assert [p.exitcode for p in procs] == [0] * world
    return got


@functools.lru_cache(maxsize=None)
def _two_ranks():
    return _run_ranks(2, {"single_state": _reference()["state"][HALF]})


@functools.lru_cache(maxsize=None)
def _three_ranks():
    two = _two_ranks()
    return _run_ranks(3, {"shards": [two[0]["shard_state"], two[1]["shard_state"]]})


# -- the tests -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_resume_at_another_world_size(oracle_mod):
    """4 steps at 2 ranks, the two per-rank dicts loaded at 3 ranks, 4 more steps: steps 5..8 and the final state equal the uninterrupted
    one-process run of 8 steps bit for bit (device-side auto-resets at steps 3 and 6, thermal field on)."""
    ref, three = _reference(), _three_ranks()
    want = _cat(ref["steps"][HALF:])
    for rank in range(3):
        _same(three[rank]["resumed"], want, ("2 -> 3 ranks", rank))
    _state_same(three[0]["resumed_state"], ref["state"][STEPS], "2 -> 3 ranks, final state")
    # ... as does a resume at the SAME world size from each rank's own dict, loaded while a gather was in flight
    two = _two_ranks()
    for rank in range(2):
        _same(two[rank]["same_world"], want, ("2 -> 2 ranks", rank))


@pytest.mark.timeout(600)
def test_resume_three_ranks_to_one_process_and_one_process_to_two_ranks(oracle_mod):
    import spin_torque_gym_amd as stg
    ref, acts = _reference(), _actions()
    # the 3-rank dicts after step 6 (themselves resumed from 2 ranks) -> a plain SpinTorqueVecEnv
    three = _three_ranks()
    env = stg.SpinTorqueVecEnv(N_GLOBAL, **_kw())
    env.load_state_dict([three[r]["shard_state"] for r in (2, 0, 1)])           # (any order)
    _same(_rollout(env, acts[6:]), _cat(ref["steps"][6:]), "3 ranks -> 1 process")
    _state_same(env.state_dict(), ref["state"][STEPS], "3 ranks -> 1 process, final state")
    with pytest.raises(ValueError, match="solver"):
        stg.SpinTorqueVecEnv(N_GLOBAL, **_kw(solver="euler")).load_state_dict([three[r]["shard_state"] for r in range(3)])
    with pytest.raises(ValueError, match="hole"):
        stg.SpinTorqueVecEnv(N_GLOBAL, **_kw()).load_state_dict([three[r]["shard_state"] for r in (0, 2)])
    # a plain SpinTorqueVecEnv.state_dict() after step 4 -> 2 ranks, each slicing its own [lo, hi)
    two = _two_ranks()
    want = _cat(ref["steps"][HALF:])
    for rank in range(2):
        _same(two[rank]["from_single"], want, ("1 process -> 2 ranks", rank))
        _same(two[rank]["from_full"], want, ("gather_to dict -> 2 ranks", rank))
    _state_same(two[0]["from_single_state"], ref["state"][STEPS], "1 process -> 2 ranks, final state")


def test_gather_to_dict_equals_the_one_process_dict(oracle_mod):
    ref, two = _reference(), _two_ranks()
    full, single = two[0]["full_state"], ref["state"][HALF]
    assert set(single) <= set(full)
    _state_same(full, single, "gather_to=0")
    assert full["cfg_seed"] == single["cfg_seed"] and full["env_id0"] == single["env_id0"] == 0
    assert full["host_rng"] == single["host_rng"]
    # ... and the per-rank dicts are its slices
    for rank, (lo, hi) in enumerate(((0, 19), (19, 37))):
        for k in STATE_KEYS:
            assert np.array_equal(two[rank]["shard_state"][k], single[k][..., lo:hi]), (rank, k)


def test_rejections_name_the_field(oracle_mod):
    """The ValueErrors themselves are raised -- and checked with pytest.raises -- inside the ranks (_job_two_ranks): wrong n_global, changed
    solver / max_steps / autoreset, a hole, an overlap, another cfg_seed, another rank's dict.  Here: the same checks need no process group."""
    from spin_torque_gym_amd.envs import assemble_state, check_state_config
    two = _two_ranks()
    shards = [two[0]["shard_state"], two[1]["shard_state"]]
    with pytest.raises(ValueError, match=r"hole.*\[19, 37\)"):
        assemble_state(shards[:1], 0, 19)
    with pytest.raises(ValueError, match=r"hole.*\[0, 19\)"):
        assemble_state(shards[1:], 19, 37)
    with pytest.raises(ValueError, match="overlap"):
        assemble_state([shards[0], shards[0], shards[1]], 0, 37)
    with pytest.raises(ValueError, match="n_global"):
        assemble_state([shards[0], dict(shards[1], n_global=38)], 0, 37)
    with pytest.raises(ValueError, match="holds 18 envs"):
        assemble_state([shards[0], dict(shards[1], lo=20)], 0, 37)
    with pytest.raises(ValueError, match="noise_model"):
        check_state_config(shards[0], dict(shards[0]["config"], noise_model="ou"))
    got = assemble_state(shards, 13, 25)                     # rank 1 of 3: the overlap with each of the two
    assert got["env_id0"] == 13 and tuple(got["m"].shape) == (3, 12) and got["cfg_seed"] == SEED


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_step_many_equals_one_process(oracle_mod, world):
    """K = 3 at 2 and at 3 ranks, out_every on / off, autoreset on / off: the [K, N_global] views equal the one-process step_many (and, in
    the ranks, K calls of the sharded step, the actions_are_local form and gather=False; a prefilled final_obs keeps its sentinel)."""
    ref = _reference()
    ranks = _two_ranks() if world == 2 else _three_ranks()
    for rank in range(world):
        assert set(ranks[rank]["many"]) == set(ref["many"])
        for key, want in ref["many"].items():
            _same(ranks[rank]["many"][key], want, (world, rank, key))

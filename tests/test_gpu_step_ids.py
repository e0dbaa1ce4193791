"""stg_step_ids and the send/recv pool on the MI355X: a subset step is the full step restricted to those envs, bit for bit, and leaves
every other env alone; asynchronous rounds replay to the synchronous trajectories; id launches are graph-capturable; bad ids are
reported and never dereferenced."""
import functools
import zlib

import numpy as np
import pytest
import torch

from conftest import sot_default_params, stt_default_params, vcma_default_params

pytestmark = pytest.mark.gpu

VOL_RK4, VOL_RK45 = 8.75e-11, 9.7e-6          # the regimes in which the current drives switching (bench.py: volume_for)
STATE_KEYS = ("m", "target", "total_energy", "step_count", "rng_step", "done")


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as stg
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return stg


def _unit_rows(rng, n):
    v = rng.normal(0, 1, (n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _actions(rng, n, t_max, f64=False):
    a = np.empty((2, n), dtype=np.float64 if f64 else np.float32)
    a[0] = rng.uniform(-2e6, 2e6, n)
    a[1] = rng.uniform(1e-11, t_max, n)
    return torch.tensor(a, device="cuda")


def f_actions(ids, k, t_lo=1e-11, t_hi=3e-10):
    """The action of env `ids` at its own step `k`: a fixed function of both (Gym orientation [M, 2], float32)."""
    ids = np.asarray(ids, dtype=np.uint64)
    k = np.asarray(k, dtype=np.uint64)
    h = (ids * np.uint64(0x9E3779B1) + (k + np.uint64(1)) * np.uint64(0x85EBCA77)) & np.uint64(0xFFFFFFFF)
    h2 = (h * np.uint64(0xC2B2AE3D) + np.uint64(0x27D4EB2F)) & np.uint64(0xFFFFFFFF)
    u1, u2 = h.astype(np.float64) / 2**32, h2.astype(np.float64) / 2**32
    return np.stack([(2 * u1 - 1) * 2e6, t_lo + u2 * (t_hi - t_lo)], axis=1).astype(np.float32)


def _state(env):
    return {k: v.clone() for k, v in env.get_state().items()}


def _cols(t, idx):
    return t[..., idx]


def _mixed_kw(solver):
    fac_vol = VOL_RK45 if solver == "rk45" else VOL_RK4
    return dict(device_type=["stt_mram", "sot_mram", "vcma_mram"],
                device_params=[stt_default_params(volume=fac_vol), sot_default_params(volume=fac_vol, polarization=0.7),
                               vcma_default_params(volume=fac_vol, polarization=0.7)])


N1 = 5000
CASES = {
    "rk4-thermal-records-f32-autoreset": (dict(solver="rk4", out_layout="records", autoreset=True, max_steps=1), False),
    "rk4-T0-soa-f64": (dict(solver="rk4", include_thermal_fluctuations=False, out_layout="soa"), True),
    "euler-thermal-soa-f32-autoreset": (dict(solver="euler", out_layout="soa", autoreset=True, max_steps=1), False),
    "rk45-thermal-records-f64": (dict(solver="rk45", out_layout="records"), True),
    "rk45-T0-soa-f32-refill": (dict(solver="rk45", include_thermal_fluctuations=False, out_layout="soa", lane_refill=2), False),
    "rk45-thermal-mixed-classes-records": ("mixed-rk45", False),
    "rk4-devphys-mixed-classes-records-autoreset": ("mixed-devphys", False),
    "rk4-thermal-per-env-soa": ("per-env", False),
    "rk4-thermal-skip-done-records": (dict(solver="rk4", out_layout="records", skip_done=True, max_steps=3), False),
    "rk4-thermal-identity-schedule-soa": (dict(solver="rk4", out_layout="soa", lane_sort=False, wave_spec=False), False),
}


def _case_env(stg, name, n, seed=11):
    spec, f64 = CASES[name]
    rng = np.random.default_rng(5)
    if spec == "mixed-rk45":
        kw = dict(_mixed_kw("rk45"), solver="rk45", out_layout="records", class_index=(np.arange(n) % 3).astype(np.uint8))
    elif spec == "mixed-devphys":
        kw = dict(_mixed_kw("rk4"), solver="rk4", out_layout="records", torque_model="device", autoreset=True, max_steps=1,
                  class_index=rng.integers(0, 3, n).astype(np.uint8))
    elif spec == "per-env":
        kw = dict(solver="rk4", out_layout="soa", device_params=stt_default_params(volume=VOL_RK4),
                  per_env_params={"damping": rng.uniform(0.005, 0.03, n), "polarization": rng.uniform(0.5, 0.8, n)})
    else:
        kw = dict(spec)
        kw.setdefault("device_params", stt_default_params(volume=VOL_RK45 if kw["solver"] == "rk45" else VOL_RK4))
    return stg.SpinTorqueVecEnv(n, diagnostics=True, seed=seed, **kw), f64


@pytest.mark.parametrize("name", list(CASES))
def test_subset_equals_full_step_on_those_envs(stg, name):
    """Case 1: stg_step_ids on a random unsorted subset == stg_step with the same actions for those envs (outputs and states, bit for
    bit); every other env's state is unchanged.  M in {1, 63, 65, 4097, N}."""
    n = N1
    ea, f64 = _case_env(stg, name, n)
    eb, _ = _case_env(stg, name, n)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    m0, tgt = _unit_rows(rng, n), np.where(rng.integers(0, 2, (n, 1)) == 0, 1.0, -1.0) * np.array([[0.0, 0.0, 1.0]])
    ar = ea.autoreset
    for M in (1, 63, 65, 4097, n):
        for e in (ea, eb):
            e.reset(options={"initial_state": m0, "target_state": tgt})
        ea.backend.set_state(eb.get_state())  # (a reset keeps each env's stream position, which the previous M advanced unequally)
        if ea.backend.cfg.skip_done:          # finished envs in the batch: a full step first (some episodes end at it)
            a0 = _actions(rng, n, 3e-10, f64)
            for e in (ea, eb):
                e.backend.step(a0, autoreset=False)
                e.backend.step(a0, autoreset=False)
        ids = rng.permutation(n)[:M]
        a_full = _actions(rng, n, 3e-10, f64)
        a_sub = a_full[:, torch.as_tensor(ids, device="cuda")].contiguous()
        pre = _state(ea)
        out = ea.backend.step_ids(a_sub, torch.as_tensor(ids, device="cuda"), autoreset=ar)
        eb.backend.step(a_full, autoreset=ar)
        torch.cuda.synchronize()
        b = eb.backend
        idx = torch.as_tensor(ids, device="cuda")
        pairs = [("obs", out["obs"], b.obs), ("reward", out["reward"], b.reward), ("terminated", out["terminated"], b.terminated),
                 ("truncated", out["truncated"], b.truncated), ("status", out["status"], b.status), ("reward64", out["reward64"], b.reward64),
                 ("energy", out["energy"], b.energy)]
        if ar:
            pairs.append(("final_obs", out["final_obs"], b.final_obs))
        for what, x, y in pairs:
            assert torch.equal(x, _cols(y, idx)), (name, M, what)
        sa, sb = ea.get_state(), eb.get_state()
        rest = torch.ones(n, dtype=torch.bool, device="cuda")
        rest[idx] = False
        for k in STATE_KEYS:
            assert torch.equal(_cols(sa[k], idx), _cols(sb[k], idx)), (name, M, k)
            assert torch.equal(_cols(sa[k], rest), _cols(pre[k], rest)), (name, M, k, "untouched env changed")
    ea.close(); eb.close()


R2, N2, S3 = 20, 2000, 256


@functools.lru_cache(maxsize=None)
def _replay_case(seed=21):
    """Case 2 set-up: 20 rounds of random subsets with autoreset on one context, per-env actions f(env_id, own step index); the
    synchronous full-step replay of the same per-env sequences on another."""
    import spin_torque_gym_amd as stg
    kw = dict(solver="rk4", out_layout="records", autoreset=True, max_steps=4, device_params=stt_default_params(volume=VOL_RK4), seed=seed)
    rng = np.random.default_rng(seed)
    m0, tgt = _unit_rows(rng, N2), np.where(rng.integers(0, 2, (N2, 1)) == 0, 1.0, -1.0) * np.array([[0.0, 0.0, 1.0]])
    ref = stg.SpinTorqueVecEnv(N2, diagnostics=True, **kw)
    ref.reset(options={"initial_state": m0, "target_state": tgt})
    states = [_state(ref)]
    rows = []                                           # round r: (obs, reward, terminated, truncated, final_obs, reward_f64)
    for r in range(R2):
        obs, rew, te, tr, info = ref.step(f_actions(np.arange(N2), np.full(N2, r)))
        rows.append((obs.clone(), rew.clone(), te.clone(), tr.clone(), info["final_obs"].clone(), info["reward_f64"].clone()))
        states.append(_state(ref))
    env = stg.SpinTorqueVecEnv(N2, diagnostics=True, **kw)
    env.reset(options={"initial_state": m0, "target_state": tgt})
    env.backend.counters(reset=True)
    k = np.zeros(N2, dtype=np.int64)
    got = []                                            # (ids, step index, outputs)
    sum_m = 0
    for r in range(R2):
        M = int(rng.integers(1, N2 + 1))
        ids = rng.permutation(N2)[:M]
        obs, rew, te, tr, info = env.step_ids(f_actions(ids, k[ids]), torch.as_tensor(ids))
        assert torch.equal(info["env_id"].cpu(), torch.as_tensor(ids))
        got.append((ids, k[ids].copy(), (obs.clone(), rew.clone(), te.clone(), tr.clone(), info["final_obs"].clone(),
                                         info["reward_f64"].clone())))
        k[ids] += 1
        sum_m += M
    counters = env.backend.counters()
    final = _state(env)
    env.close(); ref.close()
    return dict(rows=rows, states=states, got=got, k=k, final=final, counters=counters, sum_m=sum_m, m0=m0, tgt=tgt, seed=seed)


def test_per_env_replay_of_random_subsets(stg):
    """Case 2: every env's trajectory under 20 rounds of random subsets (autoreset) equals the synchronous replay of its own action
    sequence; the on-device env-step counter grows by sum(M)."""
    c = _replay_case()
    rows, states = c["rows"], c["states"]
    for ids, ks, outs in c["got"]:
        idx = torch.as_tensor(ids, device="cuda")
        for q in range(len(outs)):
            want = torch.empty_like(outs[q])
            for kk in np.unique(ks):
                sel = np.nonzero(ks == kk)[0]
                want[torch.as_tensor(sel, device="cuda")] = rows[int(kk)][q][idx[torch.as_tensor(sel, device="cuda")]]
            if q == 4:                                  # (final_obs rows are defined where the episode ended)
                ended = outs[2] | outs[3]
                assert torch.equal(outs[q][ended], want[ended]), q
            else:
                assert torch.equal(outs[q], want), q
    k = c["k"]
    for key in STATE_KEYS:
        want = torch.empty_like(c["final"][key])
        for kk in np.unique(k):
            sel = torch.as_tensor(np.nonzero(k == kk)[0], device="cuda")
            want[..., sel] = states[int(kk)][key][..., sel]
        assert torch.equal(c["final"][key], want), key
    assert c["counters"]["env_steps"] == c["sum_m"]


def test_oracle_slices_of_the_replay(stg):
    """Case 3: the first 256 envs of case 2 against the CPU oracle stepping the same per-env action sequences."""
    from helpers import OracleBackend
    c = _replay_case()
    kw = dict(solver="rk4", out_layout="records", autoreset=True, max_steps=4, device_params=stt_default_params(volume=VOL_RK4),
              seed=c["seed"])
    # the same host generator draws (the reset's device seed) as the HIP contexts of case 2
    orc = stg.SpinTorqueVecEnv(S3, diagnostics=True, backend=OracleBackend, **kw)
    orc.reset(options={"initial_state": c["m0"][:S3], "target_state": c["tgt"][:S3]})
    o_rows = []
    for r in range(R2):
        obs, rew, te, tr, info = orc.step(f_actions(np.arange(S3), np.full(S3, r)))
        o_rows.append((obs.clone(), te.clone(), tr.clone(), info["reward_f64"].clone(), info["final_obs"].clone()))
    # an auto-reset redraws the state from fp32 device normals (1e-7 from the oracle's libm draws, tests/test_gpu_fullsize.py:
    # _cmp_slice): each env is compared up to and including the step its first episode ends at, where the terminal observation is
    first_end = np.full(S3, R2, dtype=np.int64)
    for r in range(R2 - 1, -1, -1):
        ended = (o_rows[r][1] | o_rows[r][2]).numpy()
        first_end[ended] = r
    n_cmp = 0
    for ids, ks, outs in c["got"]:
        obs, _, te, tr, fin, r64 = (t.cpu() for t in outs)
        for j in np.nonzero(ids < S3)[0]:
            e, kk = int(ids[j]), int(ks[j])
            if kk > first_end[e]:
                continue
            oo, ot, otr, or64, ofin = o_rows[kk]
            assert bool(te[j]) == bool(ot[e]) and bool(tr[j]) == bool(otr[e]), (e, kk)
            assert np.allclose(r64[j].numpy(), or64[e].numpy(), rtol=1e-9, atol=1e-8), (e, kk)
            if kk == first_end[e]:
                assert np.allclose(fin[j].numpy(), ofin[e].numpy(), rtol=3e-7, atol=1e-7), (e, kk)
            else:
                assert np.allclose(obs[j].numpy(), oo[e].numpy(), rtol=3e-7, atol=1e-7), (e, kk)
            n_cmp += 1
    assert n_cmp > 300
    orc.close()


@pytest.mark.parametrize("solver", ["rk45", "rk4"])
def test_step_ids_graph_capture(stg, solver):
    """Case 4: stg_step_ids captured in a graph (RK45 with the lane-refill launch and its workspace cursors; RK4 with the thermal field)
    and replayed three times == three eager calls, bit for bit."""
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    from spin_torque_gym_amd.devices import flatten_params
    n, M = 8192, 6000
    p = stt_default_params(volume=VOL_RK45 if solver == "rk45" else VOL_RK4)
    table = [flatten_params(stg.DeviceFactory().create_device("stt_mram", p))]
    cfg = EnvConfig(solver=solver, include_thermal_fluctuations=True, seed=3, out_layout="soa", diagnostics=True,
                    lane_refill=4 if solver == "rk45" else None, max_steps=2)
    rng = np.random.default_rng(1)
    ids = torch.as_tensor(rng.permutation(n)[:M].astype(np.int32), device="cuda")
    acts = [_actions(rng, M, 3e-10) for _ in range(3)]
    res = []
    for use_graph in (False, True):
        b = HipBackend(n, cfg)
        b.set_params(table)
        b.reset(None, None, None, 5)
        a_static = acts[0].clone()
        ws = b.ids_workspace(M)
        out = b.alloc_ids_outputs(M, autoreset=True)
        seen = []
        if use_graph:
            st0 = {k: v.clone() for k, v in b.get_state().items()}
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                b.step_ids(a_static, ids, autoreset=True, workspace=ws, out=out)      # warm-up (loads the code objects)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    b.step_ids(a_static, ids, autoreset=True, workspace=ws, out=out)
            b.set_state(st0)
            torch.cuda.synchronize()
            for r in range(3):
                a_static.copy_(acts[r])
                g.replay()
                torch.cuda.synchronize()
                seen.append([out[k].clone() for k in ("buf", "final_buf", "reward64", "energy", "status")])
        else:
            for r in range(3):
                a_static.copy_(acts[r])
                b.step_ids(a_static, ids, autoreset=True, workspace=ws, out=out)
                torch.cuda.synchronize()
                seen.append([out[k].clone() for k in ("buf", "final_buf", "reward64", "energy", "status")])
        res.append((seen, {k: v.clone() for k, v in b.get_state().items()}))
        b.close()
    (e_seen, e_st), (g_seen, g_st) = res
    for r in range(3):
        for x, y in zip(e_seen[r], g_seen[r]):
            assert torch.equal(x, y), r
    for k in STATE_KEYS:
        assert torch.equal(e_st[k], g_st[k]), k


@pytest.mark.parametrize("layout", ["soa", "records"])
def test_bad_ids_report_status_4_and_change_nothing(stg, layout):
    """Case 5: ids >= N are never dereferenced: status 4, zero outputs; the good ids of the same list step as in a full step."""
    n = 3000
    kw = dict(solver="rk4", out_layout=layout, device_params=stt_default_params(volume=VOL_RK4))
    ea = stg.SpinTorqueVecEnv(n, diagnostics=True, seed=4, **kw)
    eb = stg.SpinTorqueVecEnv(n, diagnostics=True, seed=4, **kw)
    for e in (ea, eb):
        e.reset()
    rng = np.random.default_rng(2)
    good = rng.permutation(n)[:200]
    ids = np.concatenate([good[:100], [n, n + 1, 2**31 - 1, 10 * n], good[100:], [n + 7]]).astype(np.int64)
    bad = ids >= n
    a_full = _actions(rng, n, 3e-10)
    a_sub = torch.zeros((2, ids.size), dtype=torch.float32, device="cuda")
    a_sub[:, torch.as_tensor(np.nonzero(~bad)[0], device="cuda")] = a_full[:, torch.as_tensor(ids[~bad], device="cuda")]
    a_sub[:, torch.as_tensor(np.nonzero(bad)[0], device="cuda")] = 1.0
    pre = _state(ea)
    out = ea.backend.step_ids(a_sub, torch.as_tensor(ids.astype(np.int32), device="cuda"))
    eb.backend.step(a_full)
    torch.cuda.synchronize()
    jb = torch.as_tensor(np.nonzero(bad)[0], device="cuda")
    jg = torch.as_tensor(np.nonzero(~bad)[0], device="cuda")
    g = torch.as_tensor(ids[~bad], device="cuda")
    assert (out["status"][jb] == 4).all()
    for k in ("obs", "reward", "terminated", "truncated", "reward64", "energy"):
        assert (_cols(out[k], jb) == 0).all(), k
    b = eb.backend
    for what, x, y in (("obs", out["obs"], b.obs), ("reward64", out["reward64"], b.reward64), ("status", out["status"], b.status)):
        assert torch.equal(_cols(x, jg), _cols(y, g)), what
    sa, sb = ea.get_state(), eb.get_state()
    rest = torch.ones(n, dtype=torch.bool, device="cuda")
    rest[g] = False
    for k in STATE_KEYS:
        assert torch.equal(_cols(sa[k], g), _cols(sb[k], g)), k
        assert torch.equal(_cols(sa[k], rest), _cols(pre[k], rest)), k
    # the env layer rejects such ids on the host
    with pytest.raises(ValueError):
        ea.step_ids(np.zeros((1, 2), np.float32), [n])
    ea.close(); eb.close()


def test_pool_at_scale_replays_bit_for_bit(stg):
    """Case 6: 65 536 envs, RK45 + thermal, B = 16 384, 4 streams in flight, 30 recv/send rounds with merged and split sends: every
    env's trajectory equals the synchronous replay of its own action sequence, and no env is in two in-flight sets at once."""
    n, B, rounds = 65536, 16384, 30
    kw = dict(solver="rk45", out_layout="records", autoreset=True, max_steps=6, device_params=stt_default_params(volume=VOL_RK45))
    env = stg.SpinTorqueVecEnv(n, seed=8, **kw)
    ref = stg.SpinTorqueVecEnv(n, seed=8, **kw)
    f = functools.partial(f_actions, t_lo=1e-10, t_hi=1e-9)           # the bench's U[0.1, 1] ns pulses
    env.async_reset(B, seed=1)
    ref.reset(seed=1)
    init = _state(ref)
    k = np.zeros(n, dtype=np.int64)
    got = []
    held = []
    rng = np.random.default_rng(3)
    in_flight = np.zeros(n, dtype=bool)
    sent_in_round = []
    for r in range(rounds):
        obs, rew, te, tr, info = env.recv()
        ids = info["env_id"].cpu().numpy()
        assert in_flight[ids].all() or r < n // B
        in_flight[ids] = False
        if k[ids].min() > 0:
            got.append((ids, k[ids] - 1, (obs.clone(), rew.clone(), te.clone(), tr.clone(), info["final_obs"].clone())))
        held.append(ids)
        if r % 3 == 0 and len(held) >= 2:                               # merge two received batches
            send = np.concatenate([held.pop(0), held.pop(0)])
        elif r % 3 == 1:                                                # split one along pairs, the rest waits
            x = np.sort(held.pop(0))
            h = (x.size // 2) & ~1
            send, rest = x[:h], x[h:]
            if rest.size:
                held.insert(0, rest)
            if send.size == 0:
                send = held.pop(0)
        else:
            send = held.pop(0)
        pr = send.reshape(-1, 2) if send.size % 2 == 0 and (send.reshape(-1, 2)[:, 0] ^ 1 == send.reshape(-1, 2)[:, 1]).all() else None
        if pr is not None:                                              # unsorted list order, pairs kept together
            send = pr[rng.permutation(pr.shape[0])].reshape(-1)
        assert not in_flight[send].any() and np.unique(send).size == send.size
        env.send(f(send, k[send]), send)
        in_flight[send] = True
        k[send] += 1
        sent_in_round.append(send.size)
    while env._pool.inflight:                                           # the rest of what is in flight
        obs, rew, te, tr, info = env.recv()
        ids = info["env_id"].cpu().numpy()
        got.append((ids, k[ids] - 1, (obs.clone(), rew.clone(), te.clone(), tr.clone(), info["final_obs"].clone())))
        held.append(ids)
    final = _state(env)
    R = int(k.max())
    rows, states = [], [init]
    for r in range(R):
        obs, rew, te, tr, info = ref.step(f(np.arange(n), np.full(n, r)))
        rows.append((obs.clone(), rew.clone(), te.clone(), tr.clone(), info["final_obs"].clone()))
        states.append(_state(ref))
    for ids, ks, outs in got:
        idx = torch.as_tensor(ids, device="cuda")
        for q in range(len(outs)):
            want = torch.empty_like(outs[q])
            for kk in np.unique(ks):
                sel = torch.as_tensor(np.nonzero(ks == kk)[0], device="cuda")
                want[sel] = rows[int(kk)][q][idx[sel]]
            if q == 4:                                  # (final_obs rows are defined where the episode ended)
                ended = outs[2] | outs[3]
                assert torch.equal(outs[q][ended], want[ended]), q
            else:
                assert torch.equal(outs[q], want), q
    for key in STATE_KEYS:
        want = torch.empty_like(final[key])
        for kk in np.unique(k):
            sel = torch.as_tensor(np.nonzero(k == kk)[0], device="cuda")
            want[..., sel] = states[int(kk)][key][..., sel]
        assert torch.equal(final[key], want), key
    assert sum(sent_in_round) == int(k.sum()) and k.max() <= rounds
    env.reset()
    env.close(); ref.close()

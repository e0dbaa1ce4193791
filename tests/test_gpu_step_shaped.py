"""Shaped pulses and an applied field in fused K-step rollouts, subset stepping and the send/recv pool (stg_set_pulse_shape,
stg_step_shaped, stg_step_shaped_ids), on the GPU: `pytest -m gpu`.

The oracle for "bit for bit" is the unchanged stg_step_wave on a second context with the same seed and start state, fed the tables
envs.pulse_tables builds from the parsed actions plus the field table expanded to every env.

  1. fused equals K single steps (K = 1, 2, 5): every output of every step, final_obs, state, counters -- solvers x thermal fields, sizes,
     drive cases, knot counts, action dtypes, out_every, layouts, class tables;
  2. auto-reset inside a launch (max_steps = 2, K = 5), and skip_done without it;
  3. actions that hit the parse edges inside a launch, and a lane whose scaled knot times tie;
  4. stg_step_shaped_ids: listed envs get the bits of a full shaped step, unlisted envs are untouched, a bad id reports itself;
  5. the golden episodes of G23 as single step_many launches through SpinTorqueVecEnv;
  6. the env's step_many / step_ids / send-recv against step() on a twin env;
  7. the write footprint of both entries;  8. graph capture;  9. checked errors launch nothing;  10. thermal partition invariance.
Sizes are N = 1, 64, 65 and 130 (two full wavefronts plus two lanes)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import stt_default_params
from helpers import Guarded
import wave_step_ref
from wave_step_ref import check_step_against_g23, g23_action, g23_params, g23_shape_and_field

pytestmark = pytest.mark.gpu

F32, F64, U8, I32 = torch.float32, torch.float64, torch.uint8, torch.int32
VOL = {"rk4": (8.75e-11, 2e-11), "euler": (8.75e-11, 2e-11), "rk45": (9.7e-6, 2e-6)}
STATE_KEYS = ("m", "target", "total_energy", "step_count", "rng_step", "done")
OUT_KEYS = ("obs", "reward", "reward_f64", "terminated", "truncated", "status", "energy")
# (the thermal cases use the factory's own volume, where the Brown field shows; the spin torque goes with J / volume, so currents are
# scaled down with it: tests/test_gpu_step_wave.py)
THERMAL_J = 1e-13
TOL_CHAINED = 10 * 1e-13         # tests/test_wave_step_host.py: 10 * TOL_M for the steps of an episode, which chain
STATUS_NOOP, STATUS_BAD_ID = 1, 4


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _flat(stg, d):
    return stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", d))


def _backend(stg, n, plist, cls=None, env_id0=0, **cfg):
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    b = HipBackend(n, EnvConfig(**{"diagnostics": True, **cfg}), 0, env_id0)
    b.set_params([_flat(stg, p) for p in plist], cls)
    return b


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _bits(t):
    t = t.contiguous()
    return t.view({F32: torch.int32, F64: torch.int64}.get(t.dtype, t.dtype))


def _same(x, y, what):
    """bit for bit (floats compared as integers)"""
    assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape, x.dtype, y.dtype)
    bad = (_bits(x) != _bits(y)).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements differ, first at {bad[:4].tolist()}"


def _state(b):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in b.get_state().items()}


def _same_state(a, b, what):
    for k in STATE_KEYS:
        _same(a[k], b[k], (what, "state", k))


def _shape(kj, seed=0):
    """a pulse shape of kj knots over [0, 1]: both ends or an inner span, with exact zeros among the factors"""
    from spin_torque_gym_amd.physics import PiecewiseLinear
    rng = np.random.default_rng(100 + kj + seed)
    tau = np.sort(rng.uniform(0.02, 0.98, kj))
    if kj % 2 == 0:
        tau[0], tau[-1] = 0.0, 1.0
    assert (np.diff(tau) > 0).all()
    s = rng.uniform(-1.0, 1.2, kj)
    s[rng.random(kj) < 0.2] = 0.0
    return PiecewiseLinear(tau, s)


def _field(kh, span, seed=0):
    """field knots (times [kh] over about `span` seconds, starting a little before t = 0 for odd kh; values [kh,3] in A/m)"""
    rng = np.random.default_rng(200 + kh + seed)
    t = np.sort(rng.uniform(0.0, 1.0, kh)) * span
    if kh % 2:
        t = t - 0.1 * span
    assert (np.diff(t) > 0).all()
    return t, rng.uniform(-1e5, 1e5, (kh, 3))


def _problem(n, solver, seed, K, f64=False, thermal=False):
    """unit rows, +-z targets, K action sets [K,N,2] with mixed J (zeros and both signs)"""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (n, 3))
    m0 = v / np.linalg.norm(v, axis=1, keepdims=True)
    tgt = np.where(rng.integers(0, 2, (n, 1)) == 0, 1.0, -1.0) * np.array([[0.0, 0.0, 1.0]])
    T = rng.uniform(1e-11, 3e-11, (K, n)) if solver == "rk45" else rng.uniform(2e-11, 1.2e-10, (K, n))
    J = rng.uniform(-2e6, 2e6, (K, n))
    J[:, ::5] = 0.0
    if thermal:
        J *= THERMAL_J
    return m0, tgt, np.stack([J, T], axis=2).astype(np.float64 if f64 else np.float32)


def _start(b, m0, tgt):
    b.reset(init_m=_dev(m0.T), target=_dev(tgt.T))


def _tables(stg, b, a, shape, fk):
    """the `wave` of HipBackend.step_wave for actions a [2,N] on the device, built as SpinTorqueVecEnv.step builds it"""
    from spin_torque_gym_amd import envs
    wave = {"current": None, "field": None}
    if shape is not None:
        J, T = envs.parse_actions_fp64(a, b.cfg.max_current, b.cfg.max_duration)
        wave["current"] = envs.pulse_tables(shape, J, T)
    if fk is not None:
        th, hk = _dev(fk[0]), _dev(fk[1])
        wave["field"] = (th[:, None].expand(-1, b.n).contiguous(), hk[:, :, None].expand(-1, -1, b.n).contiguous())
    return wave


def _oracle(stg, b, acts, shape, fk, autoreset=False):
    """K calls of stg_step_wave on b: (per step dict of OUT_KEYS + final [12,N] + done [N], state, counters)"""
    steps = []
    for k in range(acts.shape[0]):
        a = _dev(acts[k].T)
        res = b.step_wave(a, _tables(stg, b, a, shape, fk), autoreset=autoreset)
        torch.cuda.synchronize()
        d = {key: v.clone() for key, v in zip(OUT_KEYS, res)}
        d["energy"] = b.energy.clone()
        d["done"] = (d["terminated"] | d["truncated"]) != 0
        if autoreset:
            d["final"] = b.final_obs.clone()
        steps.append(d)
    return steps, _state(b), b.counters()


def _fused(b, acts, out_every=True, autoreset=False):
    """one stg_step_shaped launch of acts [K,N,2] on b: dict of OUT_KEYS with a leading [K or 1] (+ final [K or 1,12,N])"""
    res = b.step_shaped_many(_dev(np.ascontiguousarray(acts.transpose(0, 2, 1))), out_every=out_every, autoreset=autoreset)
    torch.cuda.synchronize()
    d = {key: v.clone() for key, v in zip(OUT_KEYS, res)}
    d["energy"] = b.energy_many.clone()
    if autoreset:
        d["final"] = b.final_obs_many.clone()
    return d


def _same_step(f, j, ref, what, autoreset=False):
    """slot j of a fused launch's outputs against one oracle step"""
    for key in OUT_KEYS:
        _same(f[key][j], ref[key], (what, key))
    if autoreset:
        done = ref["done"]
        _same(f["final"][j][:, done], ref["final"][:, done], (what, "final_obs of the envs that ended"))
        assert bool((f["final"][j][:, ~done] == 0).all()), (what, "final_obs of the other envs is untouched (allocated as zeros)")


# ------------------------------------------------------------------------------------------------
# 1. fused equals K single steps
# ------------------------------------------------------------------------------------------------
def _case(solver="rk4", noise=None, n=130, kj=4, kh=3, f64=False, out_every=True, layout="soa", **cfg):
    return dict(solver=solver, noise=noise, n=n, kj=kj, kh=kh, f64=f64, out_every=out_every, layout=layout, cfg=cfg)


FIELDS = [(s, f) for s in ("rk4", "euler", "rk45") for f in (None, "white")] + [("rk4", "ou"), ("euler", "ou")]
CASES = ([_case(s, f) for s, f in FIELDS] +                                                    # solvers x thermal fields, shape + field
         [_case(n=n) for n in (1, 64, 65)] +                                                    # sizes
         [_case(kj=2, kh=0), _case(kj=0, kh=2), _case(kj=17, kh=32), _case(kj=32, kh=17),      # shape only, field only, knot counts
          _case("rk45", kj=17, kh=0), _case("euler", "white", kj=0, kh=17)] +
         [_case(f64=True), _case("rk45", f64=True, layout="records")] +                        # float64 actions
         [_case(out_every=False), _case("euler", "white", out_every=False, layout="records"), _case("rk45", out_every=False)] +
         [_case(layout="records"), _case("rk4", "ou", layout="records", kj=2, kh=2)])


def _case_id(c):
    return "-".join(str(c[k]) for k in ("solver", "noise", "n", "kj", "kh")) + ("-f64" if c["f64"] else "") + \
        ("" if c["out_every"] else "-last") + ("-records" if c["layout"] == "records" else "")


def _setup(stg, c, K, seed, key=77, **extra):
    """(plist, cls, m0, tgt, acts, shape, field knots, backend factory) of a case; two device classes through cls whenever n > 1;
    key: the contexts' stream key (cfg.seed)"""
    thermal = c["noise"] is not None
    solver, n = c["solver"], c["n"]
    plist = [stt_default_params(volume=v) for v in VOL[solver]] if not thermal else [stt_default_params(), stt_default_params(damping=0.02)]
    cls = torch.tensor((np.arange(n) % 2).astype(np.uint8)) if n > 1 else None
    if n == 1:
        plist = plist[:1]
    m0, tgt, acts = _problem(n, solver, seed, K, c["f64"], thermal)
    shape = _shape(c["kj"]) if c["kj"] else None
    fk = _field(c["kh"], 2.5e-11 if solver == "rk45" else 1e-10) if c["kh"] else None
    kw = dict(solver=solver, include_thermal_fluctuations=thermal, seed=key, out_layout=c["layout"], **c["cfg"], **extra)
    if c["noise"] == "ou":
        kw["noise_model"] = "ou"

    def make(env_id0=0, sl=slice(None)):
        b = _backend(stg, len(range(n)[sl]), plist, None if cls is None else cls[sl], env_id0=env_id0, **kw)
        _start(b, m0[sl], tgt[sl])
        return b
    return plist, cls, m0, tgt, acts, shape, fk, make


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_fused_equals_k_single_steps(stg, c):
    K = 5
    plist, cls, m0, tgt, acts, shape, fk, make = _setup(stg, c, K, 31)
    ref = make()
    steps, st_ref, cnt_ref = _oracle(stg, ref, acts, shape, fk)
    ref.close()
    assert all(bool((s["status"] == 0).all()) for s in steps) and cnt_ref["work_units"] > K * c["n"]
    every = c["out_every"]
    # one launch of K = 5
    b = make()
    b.set_pulse_shape(shape, fk)
    f = _fused(b, acts, out_every=every)
    assert f["obs"].shape[0] == (K if every else 1)
    for k in (range(K) if every else [K - 1]):
        _same_step(f, k if every else 0, steps[k], (_case_id(c), "K=5, step", k))
    _same_state(_state(b), st_ref, (_case_id(c), "K=5"))
    assert b.counters() == cnt_ref, (b.counters(), cnt_ref)
    b.close()
    # K = 1, then K = 2: steps 0, 1-2
    b = make()
    b.set_pulse_shape(shape, fk)
    f1 = _fused(b, acts[:1], out_every=every)
    _same_step(f1, 0, steps[0], (_case_id(c), "K=1"))
    f2 = _fused(b, acts[1:3], out_every=every)
    for k in ((1, 2) if every else (2,)):
        _same_step(f2, k - 1 if every else 0, steps[k], (_case_id(c), "K=2, step", k))
    ref = make()
    _, st3, cnt3 = _oracle(stg, ref, acts[:3], shape, fk)
    _same_state(_state(b), st3, (_case_id(c), "K=1 + K=2"))
    assert b.counters() == cnt3
    ref.close()
    b.close()


# ------------------------------------------------------------------------------------------------
# 2. auto-reset inside a launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("autoreset", "skip_done"))
@pytest.mark.parametrize("layout", ("soa", "records"))
def test_episodes_end_inside_a_launch(stg, mode, layout):
    """max_steps = 2 and K = 5: every env is truncated at steps 2 and 4 (some succeed earlier: threshold 0).  With autoreset the kernel
    redraws them inside the launch, step by step as the single-step entry does; without it and with skip_done they stop stepping."""
    K = 5
    auto = mode == "autoreset"
    c = _case(layout=layout, max_steps=2, success_threshold=0.0, skip_done=not auto)
    plist, cls, m0, tgt, acts, shape, fk, make = _setup(stg, c, K, 41)
    ref = make()
    steps, st_ref, cnt_ref = _oracle(stg, ref, acts, shape, fk, autoreset=auto)
    ref.close()
    ended = sum(int(s["done"].sum()) for s in steps)
    assert ended > 2 * c["n"] and not all(bool(s["done"].all()) for s in steps)
    if not auto:
        assert bool((steps[-1]["status"] == 3).all()) and cnt_ref["env_steps"] < 3 * c["n"]
    for every in (True, False):
        b = make()
        b.set_pulse_shape(shape, fk)
        f = _fused(b, acts, out_every=every, autoreset=auto)
        for k in (range(K) if every else [K - 1]):
            _same_step(f, k if every else 0, steps[k], (mode, layout, every, "step", k), autoreset=auto)
        _same_state(_state(b), st_ref, (mode, layout, every))
        assert b.counters() == cnt_ref
        b.close()


# ------------------------------------------------------------------------------------------------
# 3. parse edges and tied knot times inside a launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knots", ("plain", "tied"))
def test_parse_edges_and_tied_knots_inside_a_launch(stg, knots):
    """NaN / Inf actions, J = 0 and durations at the 1e-12 clip inside a K = 3 launch, under an ordinary shape and under one whose last
    two knots are one ulp apart: there tau * T ties for some T -- which T is worked out here on the CPU -- and exactly those lanes
    report a no-op for exactly those steps."""
    from spin_torque_gym_amd.physics import PiecewiseLinear
    K, n = 3, 130
    # two adjacent knots just below 1: tau * T is T - x ulp(T) with x = 1.f and 1.f / 2 for T = 1.f 2^e, so the two products round to
    # the same double when 1.f < 1.5 and to different ones when 1.f > 1.5
    ta, tb = 1.0 - 2.0 ** -52, 1.0 - 2.0 ** -53
    assert np.nextafter(ta, 2.0) == tb and tb < 1.0
    tau = np.array([0.0, 0.3, ta, tb]) if knots == "tied" else np.array([0.0, 0.3, 0.8, 1.0])
    shape = PiecewiseLinear(tau, [0.0, 1.0, 1.0, 0.4])
    fk = _field(3, 1e-10)
    T_tie, T_ok = float(np.float32(1.25 * 2.0 ** -34)), float(np.float32(1.75 * 2.0 ** -34))
    assert ta * T_tie == tb * T_tie and ta * T_ok < tb * T_ok and 5e-11 < T_tie < T_ok < 1.5e-10
    c = _case(kj=4, kh=3)
    plist, cls, m0, tgt, acts, _, _, make = _setup(stg, c, K, 51)
    acts[:, :, 1] = np.float32(T_ok)
    tie_lane, tie_step = 66, 1
    acts[tie_step, tie_lane, 1] = np.float32(T_tie)
    edge = {3: (np.nan, 1e-10), 5: (1e6, np.nan), 64: (np.inf, 1e-10), 65: (-np.inf, 1e-10), 70: (1e6, np.inf), 100: (0.0, 1e-10),
            101: (-0.0, 8e-11), 129: (1.5e6, 1e-12), 128: (1.5e6, 1e-13), 7: (1.5e6, -1.0), 8: (9e9, 1e-3)}
    for lane, (j, t) in edge.items():
        acts[1, lane] = (j, t)
    acts[2, 3] = (np.nan, np.nan)
    # which (step, lane) have a scaled table that is not strictly increasing
    noop = np.zeros((K, n), dtype=bool)
    for k in range(K):
        _, T = wave_step_ref.parse_actions(acts[k], 2e6, 5e-9)
        noop[k] = ~(np.diff(tau[:, None] * T[None, :], axis=0) > 0).all(axis=0)
    assert noop[tie_step, tie_lane] == (knots == "tied") and not noop[tie_step, tie_lane - 1] and not noop[tie_step, tie_lane + 1]
    assert not noop[0].any() and noop.any() == (knots == "tied")
    ref = make()
    steps, st_ref, cnt_ref = _oracle(stg, ref, acts, shape, fk)
    ref.close()
    b = make()
    b.set_pulse_shape(shape, fk)
    f = _fused(b, acts)
    for k in range(K):
        _same_step(f, k, steps[k], ("edges", knots, "step", k))
    _same_state(_state(b), st_ref, ("edges", knots))
    assert b.counters() == cnt_ref and cnt_ref["noop_steps"] == int(noop.sum())
    # a tied lane reports a no-op for that step only, with no energy; its neighbours and its other steps are ordinary steps
    st = f["status"].cpu().numpy()
    assert np.array_equal(st, np.where(noop, STATUS_NOOP, 0)), np.argwhere(st != np.where(noop, STATUS_NOOP, 0))[:8]
    e = f["energy"].cpu().numpy()
    assert (e[noop] == 0.0).all() and e[tie_step, tie_lane + 1] > 0.0 and e[0, tie_lane] > 0.0
    # the parsed actions show in the observation: NaN -> (0, 1e-12); Inf meets the safety clamp first, then the clips; durations
    # below 1e-12 are clipped up to it
    o = f["obs"][1].cpu().numpy()
    t_min = np.float32(1e-12 * (1.0 / 5e-9))
    for lane in (3, 5):
        assert o[10, lane] == 0.0 and o[11, lane] == t_min, lane
    assert o[10, 64] == 1.0 and o[10, 65] == -1.0 and o[10, 70] == 0.5 and o[11, 70] == 1.0
    for lane in (129, 128, 7):
        assert o[11, lane] == t_min and o[10, lane] == 0.75, lane
    assert o[10, 8] == 1.0 and o[11, 8] == 1.0
    b.close()


# ------------------------------------------------------------------------------------------------
# 4. stg_step_shaped_ids
# ------------------------------------------------------------------------------------------------
def _id_list(n, m, seed):
    """m env ids out of n: whole pairs (2k, 2k+1), plus one env of another pair when m is odd, in a random order"""
    rng = np.random.default_rng(seed)
    pairs = rng.permutation(n // 2)
    ids = [x for p in pairs[: m // 2] for x in (2 * p, 2 * p + 1)]
    if m % 2:
        ids.append(2 * pairs[m // 2] + 1)
    ids = np.array(ids, dtype=np.int64)
    assert len(ids) == m and len(set(ids.tolist())) == m
    return rng.permutation(ids)


@pytest.mark.parametrize("m", (1, 2, 65, 130))
@pytest.mark.parametrize("solver,noise,layout,auto", [("rk4", None, "soa", False), ("rk4", "white", "records", True), ("rk45", None, "soa", True)])
def test_step_shaped_ids(stg, m, solver, noise, layout, auto):
    n = 130
    c = _case(solver, noise, layout=layout, max_steps=2, success_threshold=0.0)
    plist, cls, m0, tgt, acts, shape, fk, make = _setup(stg, c, 2, 61)
    ids = _id_list(n, m, m)
    full, sub = make(), make()
    for b in (full, sub):
        b.set_pulse_shape(shape, fk)
        _fused(b, acts[:1])                      # one step first: stream position 1, some episodes about to end
    before = _state(sub)
    f = _fused(full, acts[1:2], autoreset=auto)
    a_list = np.ascontiguousarray(acts[1][ids].T)
    out = sub.step_shaped_ids(_dev(a_list), _dev(ids), autoreset=auto)
    torch.cuda.synchronize()
    idt = _dev(ids)
    for key, name in (("obs", "obs"), ("reward", "reward"), ("reward_f64", "reward64"), ("terminated", "terminated"), ("truncated", "truncated"),
                      ("status", "status"), ("energy", "energy")):
        _same(out[name].contiguous(), f[key][0][..., idt].contiguous(), ("ids", m, key))
    if auto:
        done = ((out["terminated"] | out["truncated"]) != 0)
        assert int(done.sum()) > 0 or m < 3
        _same(out["final_obs"][:, done].contiguous(), f["final"][0][:, idt][:, done].contiguous(), ("ids", m, "final_obs"))
        assert bool((out["final_obs"][:, ~done] == 0).all())
    after, st_full = _state(sub), _state(full)
    listed = torch.zeros(n, dtype=torch.bool, device="cuda")
    listed[idt] = True
    for k in STATE_KEYS:
        _same(after[k][..., listed], st_full[k][..., listed], ("ids", m, "state of the listed envs", k))
        _same(after[k][..., ~listed], before[k][..., ~listed], ("ids", m, "state of the unlisted envs", k))
    assert sub.counters()["env_steps"] == n + m
    full.close()
    sub.close()


@pytest.mark.parametrize("layout", ("soa", "records"))
def test_step_shaped_ids_bad_id(stg, layout):
    n = 130
    c = _case(layout=layout)
    plist, cls, m0, tgt, acts, shape, fk, make = _setup(stg, c, 1, 62)
    ids = np.array([5, 4, 130, 129, 128, 0xFFFFFFF0, 64, 65], dtype=np.int64)
    good = np.array([0, 1, 3, 4, 6, 7])
    a_list = np.ascontiguousarray(acts[0][:len(ids)].T)
    clean, b = make(), make()
    for x in (clean, b):
        x.set_pulse_shape(shape, fk)
    want = clean.step_shaped_ids(_dev(a_list[:, good]), _dev(ids[good]))
    before = _state(b)
    idt = torch.as_tensor(ids.astype(np.uint32).view(np.int32), device="cuda")
    out = b.step_shaped_ids(_dev(a_list), idt)
    torch.cuda.synchronize()
    for name in ("obs", "reward", "reward64", "terminated", "truncated", "status", "energy"):
        _same(out[name][..., _dev(good)].contiguous(), want[name].contiguous(), ("bad id: the other entries", name))
        assert bool((out[name][..., [2, 5]] == (STATUS_BAD_ID if name == "status" else 0)).all()), name
    _same_state(_state(b), _state(clean), "bad id")
    assert b.counters()["env_steps"] == len(good)
    assert _state(b)["rng_step"].sum() == len(good) and before["rng_step"].sum() == 0
    clean.close()
    b.close()


# ------------------------------------------------------------------------------------------------
# 5. golden episodes as single launches
# ------------------------------------------------------------------------------------------------
def test_golden_episodes_as_single_step_many_launches(stg, golden):
    """Each G23 episode through SpinTorqueVecEnv.step_many.  A launch hands back the fp64 magnetisation of its last step only, so step k
    of an episode is checked on the launch of the episode's first k + 1 steps from its start state (the last of these launches is the
    whole episode)."""
    g = golden("G23_wave_step")
    worst = 0.0
    for e in np.unique(g["episode"]):
        ks = np.nonzero(g["episode"] == e)[0]
        shape, field = g23_shape_and_field(g, ks[0])
        env = stg.SpinTorqueVecEnv(2, diagnostics=True, out_layout="records" if e % 2 else "soa", device_params=g23_params(g),
                                   include_thermal_fluctuations=False, solver=("rk4", "euler")[int(g["solver"][ks[0]])],
                                   pulse_shape=shape, applied_field=field)
        # one launch takes one action dtype.  An episode that mixes them goes in as float64: the float32 actions widened, which parse
        # to the same (J, T) as long as none of them sits at a bound of the safety clamp (whose bounds are rounded to the action's
        # dtype) -- checked against the (J, T) the file records
        acts = np.stack([np.repeat(g23_action(g, k), 2, axis=0) for k in ks]) if not g["act_f64"][ks].any() else \
            np.stack([np.repeat(g23_action(g, k).astype(np.float64), 2, axis=0) for k in ks])   # [L,2,2]
        J, T = wave_step_ref.parse_actions(acts[:, 0], 2e6, float(g["max_duration"]))
        assert np.array_equal(J, g["J"][ks]) and np.array_equal(T, g["T"][ks])
        for j, k in enumerate(ks):
            env.reset(options={"initial_state": g["m_before"][ks[0]], "target_state": g["target"][ks[0]]})
            obs, rew, term, trunc, info = env.step_many(torch.from_numpy(acts[:j + 1]), out_every=False)
            torch.cuda.synchronize()
            m = env.get_state()["m"].cpu().numpy()
            for i in range(2):
                got = dict(m=m[:, i], obs=obs[0, i].cpu().numpy(), reward=float(info["reward_f64"][0, i]), terminated=bool(term[0, i]),
                           truncated=bool(trunc[0, i]), energy=float(info["energy"][0, i]))
                err = check_step_against_g23(g, k, got, TOL_CHAINED, f"episode {e}, launch of {j + 1} steps")
                worst = max(worst, err)
            print(f"G23 episode {e} step {j} (kj={g['kj'][k]}, kh={g['kh'][k]}): |m - m_ref| = {err:.2e}")
        env.close()
    print(f"G23 as step_many launches: worst |m - m_ref| = {worst:.2e} (bound {TOL_CHAINED:.0e})")


# ------------------------------------------------------------------------------------------------
# 6. env level
# ------------------------------------------------------------------------------------------------
def _envs(stg, n, **kw):
    p = [stt_default_params(volume=v) for v in VOL["rk4"]]
    args = dict(device_type=["stt_mram", "stt_mram"], device_params=p, class_index=(np.arange(n) % 2).astype(np.uint8),
                include_thermal_fluctuations=False, seed=9, diagnostics=True, pulse_shape=_shape(4), applied_field=[2e4, 0.0, -5e4],
                max_duration=2e-10, **kw)
    return stg.SpinTorqueVecEnv(n, **args), stg.SpinTorqueVecEnv(n, **args)


def _env_actions(n, K, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-2e6, 2e6, (K, n)), rng.uniform(2e-11, 1.2e-10, (K, n))], axis=2).astype(np.float32)


@pytest.mark.parametrize("layout,auto", [("records", False), ("soa", True)])
def test_env_step_many_and_step_ids_equal_step_on_a_twin(stg, layout, auto):
    n, K = 130, 3
    env, twin = _envs(stg, n, out_layout=layout, autoreset=auto, max_steps=2)
    acts = _env_actions(n, K + 1, 71)
    for e in (env, twin):
        e.reset(seed=4)
    obs, rew, term, trunc, info = env.step_many(torch.from_numpy(acts[:K]))
    for k in range(K):
        o, r, te, tr, inf = twin.step(torch.from_numpy(acts[k]))
        torch.cuda.synchronize()
        for x, y, what in ((obs[k], o, "obs"), (rew[k], r, "reward"), (term[k], te, "terminated"), (trunc[k], tr, "truncated"),
                           (info["status"][k], inf["status"], "status"), (info["reward_f64"][k], inf["reward_f64"], "reward_f64"),
                           (info["energy"][k], inf["energy"], "energy")):
            _same(x.contiguous(), y.contiguous(), ("step_many vs step()", k, what))
        if auto:
            done = te | tr
            _same(info["final_obs"][k][done].contiguous(), inf["final_obs"][done].contiguous(), ("step_many vs step()", k, "final_obs"))
    _same_state(_state(env.backend), _state(twin.backend), "step_many vs step()")
    # step_ids of a subset against a full step() of the twin
    ids = _id_list(n, 65, 5)
    o, r, te, tr, inf = env.step_ids(torch.from_numpy(acts[K][ids]), ids)
    before = _state(twin.backend)
    O, R_, TE, TR, INF = twin.step(torch.from_numpy(acts[K]))
    torch.cuda.synchronize()
    idt = _dev(ids)
    assert inf["env_id"].tolist() == ids.tolist()
    for x, y, what in ((o, O, "obs"), (r, R_, "reward"), (te, TE, "terminated"), (tr, TR, "truncated"), (inf["status"], INF["status"], "status"),
                       (inf["energy"], INF["energy"], "energy")):
        _same(x.contiguous(), y[idt].contiguous(), ("step_ids vs step()", what))
    listed = torch.zeros(n, dtype=torch.bool, device="cuda")
    listed[idt] = True
    st, st_twin = _state(env.backend), _state(twin.backend)
    for k in STATE_KEYS:
        _same(st[k][..., listed], st_twin[k][..., listed], ("step_ids vs step(), listed", k))
        _same(st[k][..., ~listed], before[k][..., ~listed], ("step_ids, unlisted", k))
    env.close()
    twin.close()


def test_env_send_recv_round_equals_step_on_a_twin(stg):
    n, B = 8, 4
    env, twin = _envs(stg, n)
    acts = _env_actions(n, 1, 72)[0]
    env.async_reset(B, seed=6, num_streams=2)
    reset_obs, _ = twin.reset(seed=6)
    got = {}
    for _ in range(n // B):
        obs, rew, term, trunc, info = env.recv()
        ids = info["env_id"]
        _same(obs.contiguous(), reset_obs[ids].contiguous(), "reset batches")
        order = torch.flip(ids, dims=(0,))                                   # a permuted, pair-closed list
        env.send(torch.from_numpy(acts)[order.cpu()], order)
    for _ in range(n // B):
        obs, rew, term, trunc, info = env.recv()
        torch.cuda.synchronize()
        for j, i in enumerate(info["env_id"].tolist()):
            got[i] = (obs[j].clone(), rew[j].clone(), term[j].clone(), trunc[j].clone(), info["status"][j].clone(), info["energy"][j].clone())
    O, R_, TE, TR, INF = twin.step(torch.from_numpy(acts))
    torch.cuda.synchronize()
    assert sorted(got) == list(range(n))
    for i in range(n):
        for x, y, what in zip(got[i], (O[i], R_[i], TE[i], TR[i], INF["status"][i], INF["energy"][i]), ("obs", "reward", "terminated", "truncated", "status", "energy")):
            _same(x.contiguous(), y.contiguous(), ("send/recv vs step(), env", i, what))
    env.reset(seed=6)                                                            # ends async mode; the pool had no workspaces to free
    env.close()
    twin.close()


# ------------------------------------------------------------------------------------------------
# 7. write footprint
# ------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _guards(lead, n, layout, final):
    """every caller-owned output of a launch with `lead` leading slots over n envs (or list entries), between sentinels"""
    g = {}
    if layout == "records":
        g["records"] = Guarded("records", (lead, n, 14), I32, n_axis=1)        # 56-byte records as 14 words
        if final:
            g["final_obs"] = Guarded("final_obs", (lead, n, 12), F32, n_axis=1)
    else:
        g["obs"] = Guarded("obs", (lead, 12, n), F32)
        g["reward"], g["terminated"], g["truncated"] = Guarded("reward", (lead, n), F32), Guarded("terminated", (lead, n), U8), Guarded("truncated", (lead, n), U8)
        if final:
            g["final_obs"] = Guarded("final_obs", (lead, 12, n), F32)
    for name, dt in (("reward_f64", F64), ("energy", F64), ("status", U8)):
        g[name] = Guarded(name, (lead, n), dt)
    return g


def _gargs(g):
    p = lambda k: _ptr(g[k].interior) if k in g else None               # noqa: E731
    return (p("records") if "records" in g else p("obs"), p("final_obs"), p("reward"), p("reward_f64"), p("energy"), p("terminated"),
            p("truncated"), p("status"))


def _check_guards(g, layout, want, slots, what):
    """the slots `slots` of every array are written and equal `want` (dict of OUT_KEYS + final with a leading dimension), every other
    slot and every guard is untouched; final_obs is written exactly where an episode ended"""
    lead = next(iter(g.values())).shape[0]
    sel = torch.zeros(lead, dtype=torch.bool, device="cuda")
    sel[list(slots)] = True

    def mask(ndim):
        return sel.view(-1, *([1] * (ndim - 1)))
    if layout == "records":
        rec = g["records"].check(written=mask(3)).view(U8)                # [lead, n, 56]
        from spin_torque_gym_amd.backend import record_views
        obs, reward, term, trunc, status = record_views(rec)
        got = dict(obs=obs.transpose(1, 2), reward=reward, terminated=term, truncated=trunc)
    else:
        got = {k: g[k].check(written=mask(g[k].interior.dim())) for k in ("obs", "reward", "terminated", "truncated")}
    for k in ("reward_f64", "energy", "status"):
        got[k] = g[k].check(written=mask(2))
    for j, s in enumerate(slots):
        for k in OUT_KEYS:
            _same(got[k][s].contiguous(), want[k][j].contiguous(), (what, "slot", s, k))
    if "final_obs" in g:
        done = torch.zeros((lead, want["terminated"].shape[-1]), dtype=torch.bool, device="cuda")
        for j, s in enumerate(slots):
            done[s] = (want["terminated"][j] | want["truncated"][j]) != 0
        assert 0 < int(done.sum()) < done[sel].numel(), what
        fo = g["final_obs"].check(written=done[:, :, None] if layout == "records" else done[:, None, :])
        fo = fo.transpose(1, 2) if layout == "records" else fo
        for j, s in enumerate(slots):
            _same(fo[s][:, done[s]].contiguous(), want["final"][j][:, done[s]].contiguous(), (what, "final_obs", s))


@pytest.mark.parametrize("layout", ("soa", "records"))
@pytest.mark.parametrize("n", (65, 130))
def test_write_footprint_of_both_entries(stg, n, layout):
    K = 3
    c = _case(n=n, layout=layout, max_steps=2, success_threshold=0.0)
    plist, cls, m0, tgt, acts, shape, fk, make = _setup(stg, c, K + 1, 81)
    a_dev = _dev(np.ascontiguousarray(acts[:K].transpose(0, 2, 1)))
    for every in (1, 0):
        plain = make()
        plain.set_pulse_shape(shape, fk)
        want = _fused(plain, acts[:K], out_every=bool(every), autoreset=True)
        b = make()
        b.set_pulse_shape(shape, fk)
        g = _guards(K, n, layout, True)                                   # K slots allocated either way: out_every = 0 writes slot 0 only
        rc = b.lib.stg_step_shaped(b._ctx, K, _ptr(a_dev), 0, every, 1, *_gargs(g), b._stream())
        assert rc == 0, b.lib.stg_last_error()
        torch.cuda.synchronize()
        _check_guards(g, layout, want, range(K) if every else [0], ("stg_step_shaped", n, layout, every))
        _same_state(_state(b), _state(plain), ("footprint", every))
        # the id entry on the next step: M < N
        m = n - 31
        ids = _id_list(n, m, 9)
        a_ids = _dev(np.ascontiguousarray(acts[K][ids].T))
        w = plain.step_shaped_ids(a_ids, _dev(ids), autoreset=True)
        torch.cuda.synchronize()
        want_ids = {k: w[name][None] for k, name in (("obs", "obs"), ("reward", "reward"), ("reward_f64", "reward64"), ("terminated", "terminated"),
                                                     ("truncated", "truncated"), ("status", "status"), ("energy", "energy"), ("final", "final_obs"))}
        gi = _guards(1, m, layout, True)
        idt = _dev(ids.astype(np.int32))
        rc = b.lib.stg_step_shaped_ids(b._ctx, m, _ptr(idt), _ptr(a_ids), 0, 1, *_gargs(gi), b._stream())
        assert rc == 0, b.lib.stg_last_error()
        torch.cuda.synchronize()
        _check_guards(gi, layout, want_ids, [0], ("stg_step_shaped_ids", n, layout))
        _same_state(_state(b), _state(plain), ("footprint, ids", every))
        plain.close()
        b.close()


# ------------------------------------------------------------------------------------------------
# 8. graph capture
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise", [("rk4", "white"), ("rk45", None)])
def test_graph_capture_replays_between_eager_calls(stg, solver, noise):
    """stg_step_shaped with K = 2 captured once; launches 1 and 3 of five are replays, 0, 2 and 4 eager calls: every launch gives the bits
    of the all-eager run."""
    K, R, n = 2, 5, 130
    c = _case(solver, noise)
    plist, cls, m0, tgt, acts, shape, fk, make = _setup(stg, c, K * R, 91, max_steps=3)
    ref = make()
    ref.set_pulse_shape(shape, fk)
    eager = [_fused(ref, acts[K * r:K * r + K], autoreset=True) for r in range(R)]
    st_ref, cnt_ref = _state(ref), ref.counters()
    ref.close()
    b = make()
    b.set_pulse_shape(shape, fk)
    abuf = torch.empty((K, 2, n), dtype=F32, device="cuda")
    out = dict(obs=torch.zeros((K, 12, n), dtype=F32, device="cuda"), final=torch.zeros((K, 12, n), dtype=F32, device="cuda"),
               reward=torch.zeros((K, n), dtype=F32, device="cuda"), reward_f64=torch.zeros((K, n), dtype=F64, device="cuda"),
               energy=torch.zeros((K, n), dtype=F64, device="cuda"), terminated=torch.zeros((K, n), dtype=U8, device="cuda"),
               truncated=torch.zeros((K, n), dtype=U8, device="cuda"), status=torch.zeros((K, n), dtype=U8, device="cuda"))

    def launch():
        rc = b.lib.stg_step_shaped(b._ctx, K, _ptr(abuf), 0, 1, 1, _ptr(out["obs"]), _ptr(out["final"]), _ptr(out["reward"]), _ptr(out["reward_f64"]),
                                   _ptr(out["energy"]), _ptr(out["terminated"]), _ptr(out["truncated"]), _ptr(out["status"]), b._stream())
        assert rc == 0, b.lib.stg_last_error()

    def load(r):
        abuf.copy_(_dev(np.ascontiguousarray(acts[K * r:K * r + K].transpose(0, 2, 1))))
        out["final"].zero_()

    def check(r, how):
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            _same(out[k], eager[r][k], (how, "launch", r, k))
        done = (eager[r]["terminated"] | eager[r]["truncated"]) != 0
        _same(out["final"].transpose(0, 1)[:, done].contiguous(), eager[r]["final"].transpose(0, 1)[:, done].contiguous(), (how, "launch", r, "final_obs"))

    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        load(0)
        launch()
        check(0, "eager")
        with torch.cuda.graph(graph, stream=s):
            launch()
        for r in range(1, R):
            load(r)
            if r % 2:
                graph.replay()
            else:
                launch()
            check(r, "replay" if r % 2 else "eager")
    torch.cuda.synchronize()
    _same_state(_state(b), st_ref, "graph")
    assert b.counters() == cnt_ref
    b.close()


# ------------------------------------------------------------------------------------------------
# 9. checked errors launch nothing
# ------------------------------------------------------------------------------------------------
def test_checked_errors_launch_nothing(stg):
    from spin_torque_gym_amd import _lib
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    from spin_torque_gym_amd.devices import per_env_param_block_multi
    n, K, m = 66, 2, 4
    c = _case(n=n)
    plist, cls, m0, tgt, acts, shape, fk, make = _setup(stg, c, K, 95)
    a = _dev(np.ascontiguousarray(acts.transpose(0, 2, 1)))
    ids = _dev(np.array([1, 0, 64, 65], dtype=np.int32))
    a_ids = _dev(np.ascontiguousarray(acts[0][:m].T))

    def many(b, g, K_=K, a_=a, obs=True):
        args = list(_gargs(g))
        if not obs:
            args[0] = None
        return b.lib.stg_step_shaped(b._ctx, K_, _ptr(a_), 0, 1, 0, *args, b._stream())

    def by_id(b, g, m_=m, ids_=ids, a_=a_ids):
        return b.lib.stg_step_shaped_ids(b._ctx, m_, _ptr(ids_), _ptr(a_), 0, 0, *_gargs(g), b._stream())

    def untouched(b, gs, before):
        torch.cuda.synchronize()
        for g in gs:
            for k in g:
                g[k].check(written=False)
        _same_state(_state(b), before, "state after a refused call")
        assert b.counters()["env_steps"] == 0

    # (a) no shape set; then bad arguments with one
    b = make()
    before = _state(b)
    g, gi = _guards(K, n, "soa", False), _guards(1, m, "soa", False)
    assert many(b, g) == _lib.STG_E_STATE and b"stg_set_pulse_shape" in b.lib.stg_last_error()
    assert by_id(b, gi) == _lib.STG_E_STATE and b"stg_set_pulse_shape" in b.lib.stg_last_error()
    b.set_pulse_shape(shape, fk)
    b.set_pulse_shape(None, None)                                          # cleared again
    assert many(b, g) == _lib.STG_E_STATE and by_id(b, gi) == _lib.STG_E_STATE
    b.set_pulse_shape(shape, fk)
    bad_tau = np.array([0.0, 0.5, 0.5])
    rc = b.lib.stg_set_pulse_shape(b._ctx, 3, C.c_void_p(bad_tau.ctypes.data), C.c_void_p(bad_tau.ctypes.data), 0, None, None)
    assert rc == _lib.STG_E_INVALID                                        # refused: the shape set before stays in force (used below)
    for kw in (dict(K_=0), dict(K_=-1), dict(a_=None), dict(obs=False)):
        assert many(b, g, **kw) == _lib.STG_E_INVALID, kw
    for kw in (dict(m_=-1), dict(ids_=None), dict(a_=None)):
        assert by_id(b, gi, **kw) == _lib.STG_E_INVALID, kw
    assert by_id(b, gi, m_=0) == 0                                         # an empty list: fine, nothing to do
    untouched(b, (g, gi), before)
    ref = make()
    ref.set_pulse_shape(shape, fk)
    want = _fused(ref, acts)
    assert many(b, g) == 0
    torch.cuda.synchronize()
    _same(g["obs"].check(), want["obs"], "the shape that stayed in force")
    ref.close()
    b.close()
    # (b) the device-physics torque model
    c2 = _case(n=n, torque_model="device")
    _, _, _, _, _, _, _, make2 = _setup(stg, c2, K, 95)
    b = make2()
    b.set_pulse_shape(shape, fk)
    before = _state(b)
    g, gi = _guards(K, n, "soa", False), _guards(1, m, "soa", False)
    assert many(b, g) == _lib.STG_E_INVALID and b"torque" in b.lib.stg_last_error()
    assert by_id(b, gi) == _lib.STG_E_INVALID and b"torque" in b.lib.stg_last_error()
    untouched(b, (g, gi), before)
    with pytest.raises(_lib.StgError):
        b.step_shaped_many(a)
    b.close()
    # (c) per-env parameter records
    b = HipBackend(n, EnvConfig(solver="rk4", include_thermal_fluctuations=False, diagnostics=True))
    b.set_params_per_env(*per_env_param_block_multi([_flat(stg, plist[0])], None, n, {"volume": np.full(n, VOL["rk4"][0])}))
    _start(b, m0, tgt)
    b.set_pulse_shape(shape, fk)
    before = _state(b)
    g, gi = _guards(K, n, "soa", False), _guards(1, m, "soa", False)
    assert many(b, g) == _lib.STG_E_STATE and b"per-env" in b.lib.stg_last_error()
    assert by_id(b, gi) == _lib.STG_E_STATE and b"per-env" in b.lib.stg_last_error()
    untouched(b, (g, gi), before)
    b.close()


# ------------------------------------------------------------------------------------------------
# 10. thermal partition invariance
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise", [("rk4", "white"), ("euler", "ou"), ("rk45", "white")])
def test_thermal_partition_invariance(stg, solver, noise):
    """envs [0, 130) in one context and as [0, 65) + [65, 130) in two (env_id0): the same bits for a launch of K = 3"""
    K, n = 3, 130
    c = _case(solver, noise)
    plist, cls, m0, tgt, acts, shape, fk, make = _setup(stg, c, K, 97)
    whole = make()
    whole.set_pulse_shape(shape, fk)
    f = _fused(whole, acts)
    st = _state(whole)
    whole.close()
    assert bool((f["status"] == 0).all())
    for lo, hi in ((0, 65), (65, 130)):
        part = make(env_id0=lo, sl=slice(lo, hi))
        part.set_pulse_shape(shape, fk)
        fp = _fused(part, acts[:, lo:hi])
        for k in OUT_KEYS:
            _same(fp[k], f[k][..., lo:hi].contiguous(), (solver, noise, "partition", lo, k))
        sp = _state(part)
        for k in STATE_KEYS:
            _same(sp[k], st[k][..., lo:hi].contiguous(), (solver, noise, "partition state", lo, k))
        part.close()
    # the field is on: another seed ends elsewhere by far more than rounding
    _, _, _, _, _, _, _, make_other = _setup(stg, c, K, 97, key=78)
    other = make_other()
    other.set_pulse_shape(shape, fk)
    _fused(other, acts)
    assert float((_state(other)["m"] - st["m"]).abs().max()) > 1e-10
    other.close()

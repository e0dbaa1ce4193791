"""Actions that carry the pulse's knot amplitudes, [J, T, s_0 ... s_{P-1}] (stg_set_pulse_knots, stg_step_knots, stg_step_knots_ids), on
the GPU: `pytest -m gpu`.

The yardstick for "bit for bit" is the unchanged stg_step_wave on a twin context with the same seed and start state, fed tables this
file builds in NumPy from the parse rule of the header (tests/knots_ref.py): tj = tau_j * T, jk = J * s_j, the field table replicated.

  1. fused equals K single stg_step_wave steps -- solvers x thermal fields, sizes, knot counts, action dtypes, out_every, layouts, class
     tables; every env of the yardstick's own run reports STG_STATUS_OK;
  2. episodes that end inside a launch: autoreset with final_obs, and skip_done;
  3. parse edges inside one launch, and a lane whose scaled knot times tie;
  4. stg_step_knots_ids: permuted lists, untouched envs, a bad id;
  5. one check that does not go through this library: the NumPy restatement of the step (rk4), the CPU oracle (rk45);
  6. the write footprint of both entries;  7. graph capture;  8. checked errors launch nothing;  9. the envs on a twin.
Sizes are N = 1, 65 and 130 (one lane; one and two block boundaries), K = 1 and 3, P = 2, 5 and 32."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import stt_default_params
from helpers import Guarded, OracleBackend                                                        # noqa: F401
import wave_step_ref
from knots_ref import edge_actions, knot_tables_np, parse_np, wave_rows
from test_gpu_step_shaped import (OUT_KEYS, STATE_KEYS, THERMAL_J, VOL, _backend, _check_guards, _dev, _field, _flat, _gargs, _guards, _id_list,
                                  _ptr, _same, _same_state, _same_step, _start, _state)

pytestmark = pytest.mark.gpu

F32, F64, U8 = torch.float32, torch.float64, torch.uint8
TOL_RK4 = 1e-10                  # tests/test_gpu_step_wave.py
TOL_RK45 = 1e-8
STATUS_NOOP, STATUS_BAD_ID = 1, 4
LIMIT = 1.0
MAXC, MAXD = 2e6, 5e-9           # EnvConfig's max_current / max_duration


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _tau(P, seed=0):
    """P normalised knot times: both ends of [0, 1] for even P, an inner span for odd P"""
    rng = np.random.default_rng(300 + P + seed)
    tau = np.sort(rng.uniform(0.02, 0.98, P))
    if P % 2 == 0:
        tau[0], tau[-1] = 0.0, 1.0
    assert (np.diff(tau) > 0).all()
    return tau


def _problem(n, solver, seed, K, P, f64=False, thermal=False):
    """unit rows, +-z targets, K action sets [K,N,2+P]: mixed J (zeros and both signs), amplitudes in +-1.3 -- some beyond the limit of
    1, which clamps them -- with exact zeros among them"""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (n, 3))
    m0 = v / np.linalg.norm(v, axis=1, keepdims=True)
    tgt = np.where(rng.integers(0, 2, (n, 1)) == 0, 1.0, -1.0) * np.array([[0.0, 0.0, 1.0]])
    T = rng.uniform(1e-11, 3e-11, (K, n)) if solver == "rk45" else rng.uniform(2e-11, 1.2e-10, (K, n))
    J = rng.uniform(-2e6, 2e6, (K, n))
    J[:, ::5] = 0.0
    if thermal:
        J *= THERMAL_J
    s = rng.uniform(-1.3, 1.3, (K, n, P))
    s[rng.random((K, n, P)) < 0.2] = 0.0
    return m0, tgt, np.concatenate([J[:, :, None], T[:, :, None], s], axis=2).astype(np.float64 if f64 else np.float32)


def _wave_np(b, a, tau, fk, limit=LIMIT):
    """the `wave` of HipBackend.step_wave for actions a [N,2+P] (NumPy), built here from the parse rule: the yardstick's tables"""
    J, T, s = parse_np(a, b.cfg.max_current, b.cfg.max_duration, limit)
    tj, jk = knot_tables_np(tau, J, T, s)
    wave = {"current": (_dev(tj.T), _dev(jk.T)), "field": None}
    if fk is not None:
        th, hk = _dev(fk[0]), _dev(fk[1])
        wave["field"] = (th[:, None].expand(-1, b.n).contiguous(), hk[:, :, None].expand(-1, -1, b.n).contiguous())
    return wave


def _yardstick(b, acts, tau, fk, autoreset=False, limit=LIMIT):
    """K calls of stg_step_wave on b: (per step dict of OUT_KEYS + final [12,N] + done [N], state, counters)"""
    steps = []
    for k in range(acts.shape[0]):
        res = b.step_wave(_dev(wave_rows(acts[k]).T), _wave_np(b, acts[k], tau, fk, limit), autoreset=autoreset)
        torch.cuda.synchronize()
        d = {key: v.clone() for key, v in zip(OUT_KEYS, res)}
        d["energy"] = b.energy.clone()
        d["done"] = (d["terminated"] | d["truncated"]) != 0
        if autoreset:
            d["final"] = b.final_obs.clone()
        steps.append(d)
    return steps, _state(b), b.counters()


def _fused(b, acts, out_every=True, autoreset=False):
    """one stg_step_knots launch of acts [K,N,2+P] on b: dict of OUT_KEYS with a leading [K or 1] (+ final [K or 1,12,N])"""
    res = b.step_knots_many(_dev(np.ascontiguousarray(acts.transpose(0, 2, 1))), out_every=out_every, autoreset=autoreset)
    torch.cuda.synchronize()
    d = {key: v.clone() for key, v in zip(OUT_KEYS, res)}
    d["energy"] = b.energy_many.clone()
    if autoreset:
        d["final"] = b.final_obs_many.clone()
    return d


def _case(solver="rk4", noise=None, n=130, P=5, kh=3, f64=False, out_every=True, layout="soa", **cfg):
    return dict(solver=solver, noise=noise, n=n, P=P, kh=kh, f64=f64, out_every=out_every, layout=layout, cfg=cfg)


def _case_id(c):
    return "-".join(str(c[k]) for k in ("solver", "noise", "n", "P", "kh")) + ("-f64" if c["f64"] else "") + \
        ("" if c["out_every"] else "-last") + ("-records" if c["layout"] == "records" else "")


def _setup(stg, c, K, seed, key=77, tau=None, **extra):
    """(m0, tgt, acts, tau, field knots, make) of a case; two device classes through cls whenever n > 1; make(knots=True): a context at
    the start state, with the knots set or (the yardstick) without"""
    thermal = c["noise"] is not None
    solver, n = c["solver"], c["n"]
    plist = [stt_default_params(volume=v) for v in VOL[solver]] if not thermal else [stt_default_params(), stt_default_params(damping=0.02)]
    cls = torch.tensor((np.arange(n) % 2).astype(np.uint8)) if n > 1 else None
    if n == 1:
        plist = plist[:1]
    m0, tgt, acts = _problem(n, solver, seed, K, c["P"], c["f64"], thermal)
    tau = _tau(c["P"]) if tau is None else tau
    fk = _field(c["kh"], 2.5e-11 if solver == "rk45" else 1e-10) if c["kh"] else None
    kw = dict(solver=solver, include_thermal_fluctuations=thermal, seed=key, out_layout=c["layout"], **c["cfg"], **extra)
    if c["noise"] == "ou":
        kw["noise_model"] = "ou"

    def make(knots=True):
        b = _backend(stg, n, plist, cls, **kw)
        _start(b, m0, tgt)
        if knots:
            b.set_pulse_knots(tau, LIMIT, fk)
        return b
    return m0, tgt, acts, tau, fk, make


# ------------------------------------------------------------------------------------------------
# 1. fused equals K single stg_step_wave steps
# ------------------------------------------------------------------------------------------------
FIELDS = [(s, f) for s in ("rk4", "euler", "rk45") for f in (None, "white")] + [("rk4", "ou"), ("euler", "ou")]
CASES = ([_case(s, f) for s, f in FIELDS] +                                                    # solvers x thermal fields
         [_case(n=1), _case(n=65), _case("rk45", n=65)] +                                       # sizes
         [_case(P=2, kh=0), _case(P=32, kh=17), _case("rk45", P=32, kh=0), _case("euler", "white", P=2, kh=32)] +      # knot counts
         [_case(f64=True), _case("rk45", f64=True, layout="records")] +                        # float64 actions
         [_case(out_every=False), _case("euler", "white", out_every=False, layout="records"), _case("rk45", out_every=False)] +
         [_case(layout="records"), _case("rk4", "ou", layout="records", P=2, kh=2)])


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_fused_equals_k_single_step_wave_steps(stg, c):
    K = 3
    m0, tgt, acts, tau, fk, make = _setup(stg, c, K, 31)
    ref = make(knots=False)
    steps, st_ref, cnt_ref = _yardstick(ref, acts, tau, fk)
    ref.close()
    # a comparison of no-ops proves nothing: the yardstick's own run solved every env at every step
    assert all(bool((s["status"] == 0).all()) for s in steps) and cnt_ref["work_units"] > K * c["n"] and cnt_ref["noop_steps"] == 0
    every = c["out_every"]
    b = make()
    f = _fused(b, acts, out_every=every)
    assert f["obs"].shape[0] == (K if every else 1)
    for k in (range(K) if every else [K - 1]):
        _same_step(f, k if every else 0, steps[k], (_case_id(c), "K=3, step", k))
    _same_state(_state(b), st_ref, (_case_id(c), "K=3"))
    assert b.counters() == cnt_ref, (b.counters(), cnt_ref)
    b.close()
    # K = 1 three times
    b = make()
    for k in range(K):
        _same_step(_fused(b, acts[k:k + 1], out_every=every), 0, steps[k], (_case_id(c), "K=1, step", k))
    _same_state(_state(b), st_ref, (_case_id(c), "3 x K=1"))
    assert b.counters() == cnt_ref
    b.close()


# ------------------------------------------------------------------------------------------------
# 2. episodes that end inside a launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("autoreset", "skip_done"))
@pytest.mark.parametrize("layout", ("soa", "records"))
def test_episodes_end_inside_a_launch(stg, mode, layout):
    """max_steps = 2 and K = 3: every env is truncated at step 2 (some succeed earlier: threshold 0).  With autoreset the kernel redraws
    them inside the launch, step by step as the single-step entry does; without it and with skip_done they stop stepping."""
    K = 3
    auto = mode == "autoreset"
    c = _case(layout=layout, max_steps=2, success_threshold=0.0, skip_done=not auto)
    m0, tgt, acts, tau, fk, make = _setup(stg, c, K, 41)
    ref = make(knots=False)
    steps, st_ref, cnt_ref = _yardstick(ref, acts, tau, fk, autoreset=auto)
    ref.close()
    ended = sum(int(s["done"].sum()) for s in steps)
    assert ended > c["n"] and not all(bool(s["done"].all()) for s in steps)
    if not auto:
        assert bool((steps[-1]["status"] == 3).all()) and cnt_ref["env_steps"] < 3 * c["n"]
    for every in (True, False):
        b = make()
        f = _fused(b, acts, out_every=every, autoreset=auto)
        for k in (range(K) if every else [K - 1]):
            _same_step(f, k if every else 0, steps[k], (mode, layout, every, "step", k), autoreset=auto)
        _same_state(_state(b), st_ref, (mode, layout, every))
        assert b.counters() == cnt_ref
        b.close()


# ------------------------------------------------------------------------------------------------
# 3. parse edges and tied knot times inside one launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knots", ("plain", "tied"))
@pytest.mark.parametrize("f64", (False, True), ids=("f32", "f64"))
def test_parse_edges_and_tied_knots_inside_a_launch(stg, knots, f64):
    """The rows of knots_ref.edge_actions at step 1 of a K = 3 launch -- amplitudes beyond +-limit, +-Inf, a NaN amplitude, NaN J with
    finite amplitudes, all-zero amplitudes --, under ordinary knot times and under a tau whose last two knots are one ulp apart: there
    tau * T ties for some T -- which, is worked out here on the CPU -- and exactly those lanes report a no-op for exactly those steps."""
    K, n, P = 3, 130, 4
    ta, tb = 1.0 - 2.0 ** -52, 1.0 - 2.0 ** -53                              # tests/test_gpu_step_shaped.py: ties iff T = 1.f 2^e with 1.f < 1.5
    assert np.nextafter(ta, 2.0) == tb and tb < 1.0
    tau = np.array([0.0, 0.3, ta, tb]) if knots == "tied" else np.array([0.0, 0.3, 0.8, 1.0])
    T_tie, T_ok = float(np.float32(1.25 * 2.0 ** -34)), float(np.float32(1.75 * 2.0 ** -34))
    assert ta * T_tie == tb * T_tie and ta * T_ok < tb * T_ok and 5e-11 < T_tie < T_ok < 1.5e-10
    c = _case(P=P, kh=3, f64=f64)
    m0, tgt, acts, _, fk, make = _setup(stg, c, K, 51, tau=tau)
    acts[:, :, 1] = T_ok
    tie_lane, tie_step = 66, 1
    acts[tie_step, tie_lane, 1] = T_tie
    edges = edge_actions(acts.dtype, P, LIMIT)
    edges[[0, 1, 2, 8, 9, 12], 1] = T_ok                                     # (the rows with an ordinary duration: this test's, which does not tie)
    lanes = np.array([3, 5, 62, 63, 64, 70, 71, 100, 101, 102, 127, 128, 129])
    assert len(lanes) == len(edges) and tie_lane not in lanes and tie_lane - 1 not in lanes and tie_lane + 1 not in lanes
    acts[1, lanes] = edges
    acts[2, 3, 2:] = np.nan                                                  # and a void action at another step of the same lane
    # which (step, lane) have a scaled table that is not strictly increasing, and what every lane parses to
    noop = np.zeros((K, n), dtype=bool)
    parsed = []
    for k in range(K):
        J, T, s = parse_np(acts[k], MAXC, MAXD, LIMIT)
        parsed.append((J, T, s))
        noop[k] = ~wave_step_ref.tables_valid(*knot_tables_np(tau, J, T, s))
    assert noop[tie_step, tie_lane] == (knots == "tied") and not noop[tie_step, tie_lane - 1] and not noop[tie_step, tie_lane + 1]
    assert not noop[0].any() and noop.any() == (knots == "tied")
    ref = make(knots=False)
    steps, st_ref, cnt_ref = _yardstick(ref, acts, tau, fk)
    ref.close()
    b = make()
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
    # the parsed actions show in the observation and in the energy
    o = f["obs"][1].cpu().numpy()
    t_min = np.float32(1e-12 * (1.0 / MAXD))
    row = dict(zip(range(len(lanes)), lanes))
    for r in (3, 4):                                                         # a NaN amplitude: the whole action is void
        assert o[10, row[r]] == 0.0 and o[11, row[r]] == t_min and e[1, row[r]] == 0.0, r
    assert f["obs"][2].cpu().numpy()[10, 3] == 0.0 and f["obs"][2].cpu().numpy()[11, 3] == t_min and e[2, 3] == 0.0
    for r in (5, 6):                                                         # NaN in (J, T) alone: stg_step's rule, J = 0 -> a zero table
        assert o[10, row[r]] == 0.0 and o[11, row[r]] == t_min and e[1, row[r]] == 0.0, r
    assert o[10, row[7]] == 1.0 and e[1, row[7]] > 0.0                       # Inf J meets the safety clamp, then the clip
    for r in (8, 9, 12):                                                     # all-zero amplitudes, J = 0: a pulse of no current
        assert e[1, row[r]] == 0.0 and st[1, row[r]] == 0, r
    assert o[10, row[8]] == 0.75 and o[10, row[12]] == 0.0
    # clamped and infinite amplitudes: the energy is that of the table at +-limit, which the yardstick was fed (compared above); here
    # that it is the energy of amplitudes exactly at the limit
    J, T, s = parsed[1]
    assert s[row[1]].tolist() == [LIMIT, -LIMIT, LIMIT, -LIMIT] and s[row[2]].tolist() == [LIMIT, -LIMIT, 0.5, 0.5]
    assert e[1, row[0]] > 0.0 and e[1, row[1]] > 0.0 and e[1, row[2]] > 0.0
    b.close()


# ------------------------------------------------------------------------------------------------
# 4. stg_step_knots_ids
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (1, 2, 65, 130))
@pytest.mark.parametrize("solver,noise,layout,auto", [("rk4", None, "soa", False), ("rk4", "white", "records", True), ("rk45", None, "soa", True)])
def test_step_knots_ids(stg, m, solver, noise, layout, auto):
    """the listed envs, in a permuted order, get the bits of the yardstick's full step; every other env stays as it was"""
    n = 130
    c = _case(solver, noise, layout=layout, max_steps=2, success_threshold=0.0)
    m0, tgt, acts, tau, fk, make = _setup(stg, c, 2, 61)
    ids = _id_list(n, m, m)
    full, sub = make(knots=False), make()
    _yardstick(full, acts[:1], tau, fk)            # one step first: stream position 1, some episodes about to end
    _fused(sub, acts[:1])
    before = _state(sub)
    _same_state(before, _state(full), "after the first step")
    steps, st_full, _ = _yardstick(full, acts[1:2], tau, fk, autoreset=auto)
    want = steps[0]
    assert bool((want["status"] == 0).all())
    out = sub.step_knots_ids(_dev(np.ascontiguousarray(acts[1][ids].T)), _dev(ids), autoreset=auto)
    torch.cuda.synchronize()
    idt = _dev(ids)
    for key, name in (("obs", "obs"), ("reward", "reward"), ("reward_f64", "reward64"), ("terminated", "terminated"), ("truncated", "truncated"),
                      ("status", "status"), ("energy", "energy")):
        _same(out[name].contiguous(), want[key][..., idt].contiguous(), ("ids", m, key))
    if auto:
        done = ((out["terminated"] | out["truncated"]) != 0)
        assert int(done.sum()) > 0 or m < 3
        _same(out["final_obs"][:, done].contiguous(), want["final"][:, idt][:, done].contiguous(), ("ids", m, "final_obs"))
        assert bool((out["final_obs"][:, ~done] == 0).all())
    after = _state(sub)
    listed = torch.zeros(n, dtype=torch.bool, device="cuda")
    listed[idt] = True
    for k in STATE_KEYS:
        _same(after[k][..., listed], st_full[k][..., listed], ("ids", m, "state of the listed envs", k))
        _same(after[k][..., ~listed], before[k][..., ~listed], ("ids", m, "state of the unlisted envs", k))
    assert sub.counters()["env_steps"] == n + m
    full.close()
    sub.close()


@pytest.mark.parametrize("layout", ("soa", "records"))
def test_step_knots_ids_bad_id(stg, layout):
    """ids >= n_envs report STG_STATUS_BAD_ID with zero outputs; nothing is read or written for them: the other entries and the whole
    state are those of the same list without them"""
    n = 130
    c = _case(layout=layout)
    m0, tgt, acts, tau, fk, make = _setup(stg, c, 1, 62)
    ids = np.array([5, 4, 130, 129, 128, 0xFFFFFFF0, 64, 65], dtype=np.int64)
    good = np.array([0, 1, 3, 4, 6, 7])
    a_list = np.ascontiguousarray(acts[0][:len(ids)].T)
    clean, b = make(), make()
    want = clean.step_knots_ids(_dev(np.ascontiguousarray(a_list[:, good])), _dev(ids[good]))
    before = _state(b)
    idt = torch.as_tensor(ids.astype(np.uint32).view(np.int32), device="cuda")
    out = b.step_knots_ids(_dev(a_list), idt)
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
# 5. one check that does not go through this library
# ------------------------------------------------------------------------------------------------
def test_rk4_against_the_numpy_restatement(stg):
    """A K = 2 launch against wave_step_ref.step called twice on tables built here (the second call from the first call's state)."""
    n, K, P = 65, 2, 5
    plist = [stt_default_params(volume=v) for v in VOL["rk4"]]
    cls = (np.arange(n) % 2).astype(np.uint8)
    tau = _tau(P)
    fk = _field(3, 1e-10)
    for seed in range(500, 520):              # drawn again until no flag of the reference rests on rounding
        m0, tgt, acts = _problem(n, "rk4", seed, K, P)
        state = dict(m=m0, target=tgt, total_energy=np.zeros(n), step_count=np.zeros(n, dtype=np.int64))
        refs = []
        for k in range(K):
            J, T, s = parse_np(acts[k], MAXC, MAXD, LIMIT)
            fld = (np.broadcast_to(fk[0], (n, 3)), np.broadcast_to(fk[1], (n, 3, 3)))
            refs.append(wave_step_ref.step(state, wave_rows(acts[k]), plist, "rk4", current=knot_tables_np(tau, J, T, s), field=fld, cls=cls))
            state = dict(m=refs[-1]["m"], target=tgt, total_energy=refs[-1]["total_energy"], step_count=refs[-1]["step_count"])
        if all((np.abs(r["alignment"] - 0.9) > 1e-6).all() for r in refs):
            break
    assert all((np.abs(r["alignment"] - 0.9) > 1e-6).all() and (r["status"] == 0).all() for r in refs)
    b = _backend(stg, n, plist, torch.tensor(cls), solver="rk4", include_thermal_fluctuations=False)
    _start(b, m0, tgt)
    b.set_pulse_knots(tau, LIMIT, fk)
    f = _fused(b, acts)
    m = _state(b)["m"].cpu().numpy().T
    err = float(np.abs(m - refs[-1]["m"]).max())
    print(f"stg_step_knots rk4 vs the NumPy restatement, K = {K}: worst |m - m_ref| = {err:.2e} (bound {TOL_RK4:.0e})")
    assert err <= TOL_RK4
    for k, ref in enumerate(refs):
        e, e_ref = f["energy"][k].cpu().numpy(), ref["energy"]
        assert np.all(np.abs(e - e_ref) <= 1e-13 * np.abs(e_ref)), k                # tests/test_gpu_step_wave.py: a few ulp
        assert np.array_equal(f["terminated"][k].cpu().numpy().astype(bool), ref["terminated"])
        assert np.array_equal(f["truncated"][k].cpu().numpy().astype(bool), ref["truncated"])
        assert np.array_equal(f["status"][k].cpu().numpy(), ref["status"])
        ob, ob_ref = f["obs"][k].cpu().numpy().T, ref["obs"]
        print(f"  step {k}: worst observation difference {float(np.abs(ob - ob_ref).max()):.2e}")
        assert np.all(np.abs(ob - ob_ref) <= wave_step_ref.F32_ULP * np.abs(ob_ref) + 2 * TOL_RK4), k    # the bound of tests/test_gpu_step_wave.py
        assert np.all(np.abs(f["reward_f64"][k].cpu().numpy() - ref["reward"]) <= 1e-9), k
    assert b.counters() == {"env_steps": K * n, "work_units": int(sum(r["n_sub"].sum() for r in refs)), "noop_steps": 0}
    b.close()


def test_rk45_against_the_cpu_oracle(stg):
    """The NumPy restatement has no RK45.  The independent integrator for it is the CPU oracle's, which knows the rectangular pulse only:
    amplitudes at and beyond the limit of 1 -- all clamped to exactly 1 -- make the table the constant J over (0, T), the same drive.
    m against the oracle's step; the energy against the closed form of the table in NumPy, and against the oracle's J^2 T form.
    (Amplitudes that are NOT flat, against the oracle's waveform solve: tests/test_gpu_wave_rk45_oracle.py.)"""
    from spin_torque_gym_amd.backend import EnvConfig
    n, P = 65, 5
    p = stt_default_params(volume=VOL["rk45"][0])
    tau = _tau(P)
    m0, tgt, acts = _problem(n, "rk45", 77, 1, P)
    acts[0, :, 2:] = np.random.default_rng(5).uniform(1.0, 3.0, (n, P)).astype(np.float32)
    acts[0, 3, 2:] = np.inf
    J, T, s = parse_np(acts[0], MAXC, MAXD, LIMIT)
    assert (s == 1.0).all()
    cfg = dict(solver="rk45", include_thermal_fluctuations=False, diagnostics=True)
    o = OracleBackend(n, EnvConfig(**cfg))
    o.set_params([_flat(stg, p)])
    o.reset(init_m=torch.from_numpy(m0.T.copy()), target=torch.from_numpy(tgt.T.copy()))
    o_obs, _, o_rew, o_term, o_trunc, o_status = o.step(torch.from_numpy(np.ascontiguousarray(acts[0][:, :2].T)))
    assert bool((o_status == 0).all())
    m_ref = o.get_state()["m"].numpy().T
    align = (m_ref * tgt).sum(axis=1)
    assert (np.abs(align - 0.9) > 1e-6).all()                                    # no flag rests on rounding
    b = _backend(stg, n, [p], **{k: v for k, v in cfg.items() if k != "diagnostics"})
    _start(b, m0, tgt)
    b.set_pulse_knots(tau, LIMIT, None)
    f = _fused(b, acts)
    m = _state(b)["m"].cpu().numpy().T
    err = float(np.abs(m - m_ref).max())
    print(f"stg_step_knots rk45 vs the CPU oracle under a flat pulse: worst |m - m_ref| = {err:.2e} (bound {TOL_RK45:.0e})")
    assert err <= TOL_RK45 and bool((f["status"] == 0).all())
    r = wave_step_ref.resistance(m0, p)
    ra = r * p["area"]
    e_ref = (ra * ra) / r * wave_step_ref.pulse_sq_integral(*knot_tables_np(tau, J, T, s), T)
    e = f["energy"][0].cpu().numpy()
    assert np.all(np.abs(e - e_ref) <= 1e-13 * np.abs(e_ref))
    assert np.all(np.abs(e - o.energy.numpy()) <= 1e-12 * np.abs(e))             # (J R A)^2 / R * T in another order of operations
    assert np.array_equal(f["terminated"][0].cpu().numpy(), o_term.numpy()) and np.array_equal(f["truncated"][0].cpu().numpy(), o_trunc.numpy())
    ob, ob_ref = f["obs"][0].cpu().numpy().T, o_obs.numpy().T
    # fp32 observations: one float32 ulp, plus what TOL_RK45 on m allows in the components that follow m; obs[9] follows the energy
    idx = [i for i in range(12) if i != 9]
    assert np.all(np.abs(ob[:, idx] - ob_ref[:, idx]) <= wave_step_ref.F32_ULP * np.abs(ob_ref[:, idx]) + 2 * TOL_RK45)
    assert np.all(np.abs(ob[:, 9] - ob_ref[:, 9]) <= 2 * wave_step_ref.F32_ULP * np.abs(ob_ref[:, 9]))
    b.close()


# ------------------------------------------------------------------------------------------------
# 6. write footprint
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("soa", "records"))
@pytest.mark.parametrize("n", (65, 130))
def test_write_footprint_of_both_entries(stg, n, layout):
    K = 3
    c = _case(n=n, layout=layout, max_steps=2, success_threshold=0.0)
    m0, tgt, acts, tau, fk, make = _setup(stg, c, K + 1, 81)
    a_dev = _dev(np.ascontiguousarray(acts[:K].transpose(0, 2, 1)))
    for every in (1, 0):
        plain = make()
        want = _fused(plain, acts[:K], out_every=bool(every), autoreset=True)
        b = make()
        g = _guards(K, n, layout, True)                                   # K slots allocated either way: out_every = 0 writes slot 0 only
        rc = b.lib.stg_step_knots(b._ctx, K, _ptr(a_dev), 0, every, 1, *_gargs(g), b._stream())
        assert rc == 0, b.lib.stg_last_error()
        torch.cuda.synchronize()
        _check_guards(g, layout, want, range(K) if every else [0], ("stg_step_knots", n, layout, every))
        _same_state(_state(b), _state(plain), ("footprint", every))
        # the id entry on the next step: M < N
        m = n - 31
        ids = _id_list(n, m, 9)
        a_ids = _dev(np.ascontiguousarray(acts[K][ids].T))
        w = plain.step_knots_ids(a_ids, _dev(ids), autoreset=True)
        torch.cuda.synchronize()
        want_ids = {k: w[name][None] for k, name in (("obs", "obs"), ("reward", "reward"), ("reward_f64", "reward64"), ("terminated", "terminated"),
                                                     ("truncated", "truncated"), ("status", "status"), ("energy", "energy"), ("final", "final_obs"))}
        gi = _guards(1, m, layout, True)
        idt = _dev(ids.astype(np.int32))
        rc = b.lib.stg_step_knots_ids(b._ctx, m, _ptr(idt), _ptr(a_ids), 0, 1, *_gargs(gi), b._stream())
        assert rc == 0, b.lib.stg_last_error()
        torch.cuda.synchronize()
        _check_guards(gi, layout, want_ids, [0], ("stg_step_knots_ids", n, layout))
        _same_state(_state(b), _state(plain), ("footprint, ids", every))
        plain.close()
        b.close()


# ------------------------------------------------------------------------------------------------
# 7. graph capture
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise", [("rk4", "white"), ("rk45", None)])
def test_graph_capture_replays_between_eager_calls(stg, solver, noise):
    """stg_step_knots with K = 3 captured once; of seven launches 0, 2, 4 and 6 are eager calls and 1, 3 and 5 replays: every launch gives
    the bits of the all-eager run."""
    K, R, n = 3, 7, 130
    c = _case(solver, noise)
    m0, tgt, acts, tau, fk, make = _setup(stg, c, K * R, 91, max_steps=4)
    P = c["P"]
    ref = make()
    eager = [_fused(ref, acts[K * r:K * r + K], autoreset=True) for r in range(R)]
    st_ref, cnt_ref = _state(ref), ref.counters()
    ref.close()
    b = make()
    abuf = torch.empty((K, 2 + P, n), dtype=F32, device="cuda")
    out = dict(obs=torch.zeros((K, 12, n), dtype=F32, device="cuda"), final=torch.zeros((K, 12, n), dtype=F32, device="cuda"),
               reward=torch.zeros((K, n), dtype=F32, device="cuda"), reward_f64=torch.zeros((K, n), dtype=F64, device="cuda"),
               energy=torch.zeros((K, n), dtype=F64, device="cuda"), terminated=torch.zeros((K, n), dtype=U8, device="cuda"),
               truncated=torch.zeros((K, n), dtype=U8, device="cuda"), status=torch.zeros((K, n), dtype=U8, device="cuda"))

    def launch():
        rc = b.lib.stg_step_knots(b._ctx, K, _ptr(abuf), 0, 1, 1, _ptr(out["obs"]), _ptr(out["final"]), _ptr(out["reward"]), _ptr(out["reward_f64"]),
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
# 8. checked errors launch nothing
# ------------------------------------------------------------------------------------------------
def test_checked_errors_launch_nothing(stg):
    from spin_torque_gym_amd import _lib
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    from spin_torque_gym_amd.devices import per_env_param_block_multi
    from spin_torque_gym_amd.physics import PiecewiseLinear
    n, K, m = 66, 2, 4
    c = _case(n=n)
    m0, tgt, acts, tau, fk, make = _setup(stg, c, K, 95)
    P = c["P"]
    a = _dev(np.ascontiguousarray(acts.transpose(0, 2, 1)))
    ids = _dev(np.array([1, 0, 64, 65], dtype=np.int32))
    a_ids = _dev(np.ascontiguousarray(acts[0][:m].T))

    def many(b, g, K_=K, a_=a, obs=True):
        args = list(_gargs(g))
        if not obs:
            args[0] = None
        return b.lib.stg_step_knots(b._ctx, K_, _ptr(a_), 0, 1, 0, *args, b._stream())

    def by_id(b, g, m_=m, ids_=ids, a_=a_ids):
        return b.lib.stg_step_knots_ids(b._ctx, m_, _ptr(ids_), _ptr(a_), 0, 0, *_gargs(g), b._stream())

    def untouched(b, gs, before):
        torch.cuda.synchronize()
        for g in gs:
            for k in g:
                g[k].check(written=False)
        _same_state(_state(b), before, "state after a refused call")
        assert b.counters()["env_steps"] == 0

    def set_knots(b, tau_, limit):
        t = np.ascontiguousarray(tau_, dtype=np.float64)
        return b.lib.stg_set_pulse_knots(b._ctx, len(t), C.c_void_p(t.ctypes.data), float(limit), 0, None, None)

    # (a) no knots set -- a pulse shape does not count, the two are independent --; then bad arguments with knots
    b = make(knots=False)
    before = _state(b)
    g, gi = _guards(K, n, "soa", False), _guards(1, m, "soa", False)
    assert many(b, g) == _lib.STG_E_STATE and b"stg_set_pulse_knots" in b.lib.stg_last_error()
    assert by_id(b, gi) == _lib.STG_E_STATE and b"stg_set_pulse_knots" in b.lib.stg_last_error()
    b.set_pulse_shape(PiecewiseLinear([0.0, 1.0], [1.0, 0.5]), None)
    assert many(b, g) == _lib.STG_E_STATE and by_id(b, gi) == _lib.STG_E_STATE
    b.set_pulse_knots(tau, LIMIT, fk)
    b.set_pulse_knots(None, LIMIT, None)                                   # cleared again
    assert many(b, g) == _lib.STG_E_STATE and by_id(b, gi) == _lib.STG_E_STATE
    b.set_pulse_knots(tau, LIMIT, fk)
    # refused settings: what was set before stays in force (the launch below proves it)
    for bad_tau in ([0.0, 0.5, 0.5], [0.0, 1.5], [0.0, np.nan, 1.0], [0.5]):
        assert set_knots(b, bad_tau, LIMIT) == _lib.STG_E_INVALID, bad_tau
    for bad_limit in (0.0, -1.0, np.inf, np.nan):
        assert set_knots(b, [0.0, 1.0], bad_limit) == _lib.STG_E_INVALID, bad_limit
    for kw in (dict(K_=0), dict(K_=-1), dict(a_=None), dict(obs=False)):
        assert many(b, g, **kw) == _lib.STG_E_INVALID, kw
    for kw in (dict(m_=-1), dict(ids_=None), dict(a_=None)):
        assert by_id(b, gi, **kw) == _lib.STG_E_INVALID, kw
    assert by_id(b, gi, m_=0) == 0                                         # an empty list: fine, nothing to do
    untouched(b, (g, gi), before)
    ref = make()
    want = _fused(ref, acts)
    assert many(b, g) == 0
    torch.cuda.synchronize()
    for k in ("obs", "reward", "reward_f64", "energy", "status"):
        _same(g[k].check(), want[k], ("the knots that stayed in force", k))
    _same_state(_state(b), _state(ref), "the knots that stayed in force")
    ref.close()
    b.close()
    # (b) the device-physics torque model
    c2 = _case(n=n, torque_model="device")
    make2 = _setup(stg, c2, K, 95)[-1]
    b = make2()
    before = _state(b)
    g, gi = _guards(K, n, "soa", False), _guards(1, m, "soa", False)
    assert many(b, g) == _lib.STG_E_INVALID and b"torque" in b.lib.stg_last_error()
    assert by_id(b, gi) == _lib.STG_E_INVALID and b"torque" in b.lib.stg_last_error()
    untouched(b, (g, gi), before)
    with pytest.raises(_lib.StgError):
        b.step_knots_many(a)
    b.close()
    # (c) per-env parameter records
    plist0 = stt_default_params(volume=VOL["rk4"][0])
    b = HipBackend(n, EnvConfig(solver="rk4", include_thermal_fluctuations=False, diagnostics=True))
    b.set_params_per_env(*per_env_param_block_multi([_flat(stg, plist0)], None, n, {"volume": np.full(n, VOL["rk4"][0])}))
    _start(b, m0, tgt)
    b.set_pulse_knots(tau, LIMIT, fk)
    before = _state(b)
    g, gi = _guards(K, n, "soa", False), _guards(1, m, "soa", False)
    assert many(b, g) == _lib.STG_E_STATE and b"per-env" in b.lib.stg_last_error()
    assert by_id(b, gi) == _lib.STG_E_STATE and b"per-env" in b.lib.stg_last_error()
    untouched(b, (g, gi), before)
    b.close()


# ------------------------------------------------------------------------------------------------
# 9. env level
# ------------------------------------------------------------------------------------------------
ENV_TAU = [0.0, 0.15, 0.6, 1.0]
ENV_FIELD = [2e4, 0.0, -5e4]


def _envs(stg, n, **kw):
    p = [stt_default_params(volume=v) for v in VOL["rk4"]]
    args = dict(device_type=["stt_mram", "stt_mram"], device_params=p, class_index=(np.arange(n) % 2).astype(np.uint8),
                include_thermal_fluctuations=False, seed=9, diagnostics=True, pulse_knots=ENV_TAU, amplitude_limit=1.2, applied_field=ENV_FIELD,
                max_duration=2e-10, **kw)
    return stg.SpinTorqueVecEnv(n, **args), stg.SpinTorqueVecEnv(n, **args)


def _env_actions(n, K, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-2e6, 2e6, (K, n, 1)), rng.uniform(2e-11, 1.2e-10, (K, n, 1)), rng.uniform(-1.5, 1.5, (K, n, 4))],
                          axis=2).astype(np.float32)


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


def test_env_step_equals_backend_step_wave_on_test_built_tables(stg):
    """SpinTorqueVecEnv(pulse_knots=).step() on the knot entry against HipBackend.step_wave on a bare context, fed the tables this file
    builds in NumPy -- edge rows of the parse among the actions"""
    n = 130
    env, spare = _envs(stg, n, out_layout="soa")
    spare.close()
    acts = _env_actions(n, 2, 73)
    edges = edge_actions(np.float32, 4, 1.2)
    acts[1, 20:20 + len(edges)] = edges
    env.reset(seed=4)
    start = _state(env.backend)
    cfg = env.backend.cfg
    b = _backend(stg, n, [stt_default_params(volume=v) for v in VOL["rk4"]], torch.tensor((np.arange(n) % 2).astype(np.uint8)),
                 solver="rk4", include_thermal_fluctuations=False, seed=cfg.seed, max_duration=2e-10, out_layout="soa")
    b.set_state({k: start[k] for k in STATE_KEYS})
    fk = (np.array([0.0, 2e-10]), np.array([ENV_FIELD, ENV_FIELD]))
    for k in range(2):
        o, r, te, tr, inf = env.step(torch.from_numpy(acts[k]))
        J, T, s = parse_np(acts[k], 2e6, 2e-10, 1.2)
        tj, jk = knot_tables_np(ENV_TAU, J, T, s)
        th, hk = _dev(fk[0]), _dev(fk[1])
        wave = {"current": (_dev(tj.T), _dev(jk.T)), "field": (th[:, None].expand(-1, n).contiguous(), hk[:, :, None].expand(-1, -1, n).contiguous())}
        O, R_, R64, TE, TR, ST = b.step_wave(_dev(wave_rows(acts[k]).T), wave)
        torch.cuda.synchronize()
        for x, y, what in ((o, O.t(), "obs"), (r, R_, "reward"), (te, TE.bool(), "terminated"), (tr, TR.bool(), "truncated"), (inf["status"], ST, "status"),
                           (inf["reward_f64"], R64, "reward_f64"), (inf["energy"], b.energy, "energy")):
            _same(x.contiguous(), y.contiguous(), ("step() vs step_wave", k, what))
    _same_state(_state(env.backend), _state(b), "step() vs step_wave")
    env.close()
    b.close()


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
    env.reset(seed=6)
    env.close()
    twin.close()


def test_single_env_episode_equals_env_0_of_the_vector_env(stg):
    """five steps of SpinTorqueEnv(pulse_knots=) against env 0 of a one-env SpinTorqueVecEnv from the same start state"""
    p = stt_default_params(volume=VOL["rk4"][0])
    kw = dict(device_params=p, include_thermal_fluctuations=False, pulse_knots=ENV_TAU, amplitude_limit=1.2, applied_field=ENV_FIELD,
              max_duration=2e-10, seed=3)
    one = stg.SpinTorqueEnv(**kw)
    vec = stg.SpinTorqueVecEnv(1, diagnostics=True, **kw)
    assert one.action_space.shape == (6,)
    m0, tgt = np.array([0.6, 0.0, 0.8]), np.array([0.0, 0.0, -1.0])
    one.reset(options={"initial_state": m0, "target_state": tgt})
    vec.reset(options={"initial_state": m0[None], "target_state": tgt[None]})
    acts = _env_actions(1, 5, 74)[:, 0]
    acts[3, 4] = np.nan                                                      # a void action inside the episode
    for k in range(5):
        o, r, te, tr, info = one.step(acts[k])
        O, R_, TE, TR, INF = vec.step(torch.from_numpy(acts[k][None]))
        torch.cuda.synchronize()
        assert "error" not in info, info
        assert np.array_equal(o.view(np.int32), O[0].cpu().numpy().view(np.int32)), k
        assert r == float(INF["reward_f64"][0]) and te == bool(TE[0]) and tr == bool(TR[0]) and info["energy_consumed"] == float(INF["energy"][0])
        J, T, _ = parse_np(acts[k][None], 2e6, 2e-10, 1.2)
        assert (info["current_density"], info["pulse_duration"]) == (float(J[0]), float(T[0])), k
    assert np.array_equal(one.current_magnetization, vec.get_state()["m"][:, 0].cpu().numpy())
    assert one.get_device_info()["pulse_knots"] == ENV_TAU
    one.close()
    vec.close()

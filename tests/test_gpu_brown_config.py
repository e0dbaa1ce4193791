"""noise_model='brown' off its defaults, on the GPU: `pytest -m gpu`.  tests/test_gpu_brown.py runs the Brown field at the default
configuration only, where one branch of dt = min(max_step, T / 100) is ever taken and 1 / sqrt(dt) is within 1 % of 1e6.  Here, on the
cases of tests/brown_config_cases.py (max_step 2.5e-12 / 3e-13 / 1e-10 x gamma, 77 and 450 K, both methods, EPISODE's fields, the
five-target list, the class table STT / SOT / VCMA, float32 and float64 actions alternating, the stream key (SEED, ENV_ID0 = 37),
N = 130 and one case with n = 1, two chained steps), every fixed-step entry point is held to two references that are FED THE DEVICE'S
OWN NORMALS (stg_thermal_normals at each env's own rng_step):

  tests/brown_ref.py                 the NumPy restatement (rectangular pulses and the waveform tables);
  the C oracle's fed-normals step    oracle/stg_oracle.c: stgo_simple_solve_fed / stgo_env_step_fed (rectangular pulses, and the device
                                     torque model on EVERY lane: STT, SOT and VCMA under J != 0).

  stg_solve, stg_solve_traj          final m, sub-step counts, the trajectories of six lanes (both lanes of the tail among them);
  step()                             two chained steps;
  step_many                          K = 3, out_every, autoreset with max_steps = 3: resets fall inside the launch; a redrawn env takes
                                     the device's own redraw in the references too (held to the restated draw at 2e-6, its target exactly);
  step_ids                           a permuted subset that includes the tail, twice; the other envs stay bit for bit;
  stg_solve_wave, stg_step_wave, stg_step_shaped(_ids), stg_step_knots(_ids)     against the restatement under tables (the oracle has
                                     no waveforms);
  the stream key                     two envs of 65 with env_id0 = 0 and 65 against one of 130, bit for bit;
  the gates                          temperature <= 0 and include_thermal_fluctuations=False: 'brown' is 'white' bit for bit.

Tolerances are the project's: TOL_RK4 = 1e-10 on m with exact status bytes, sub-step counts and flags (no thermal factor: the
references take the device's normals); observations one float32 ulp + 2 tol, the fp64 reward 1e-9 + 2 tol, the energy 1e-13 relative
in a first step.  tests/test_brown_config_conditioning.py shows on the CPU that every case moves by less than 1e-12 per ulp of the start
rows and of the normals.  Every test prints its worst |m - m_ref|; profiles/NOTEBOOK.md has the table of a run.

Measured on an MI355X, worst |m - m_ref| over the 13 cases (bound 1e-10): stg_solve / stg_solve_traj 4.7e-14, step() 7.6e-14, the K = 3
launch with autoreset 1.3e-13, step_ids 7.6e-14, stg_solve_wave 2.6e-14, stg_step_wave 1.2e-13, stg_step_shaped 6.7e-13 (_ids 1.1e-13),
stg_step_knots 1.4e-13 (_ids 6.2e-14); the device torque model on all 130 lanes 7.9e-14."""
import numpy as np
import pytest
import torch

import brown_config_cases as bcc
import brown_ref as br
import wave_step_ref as wsr
from env_config_cases import backend_factory, unit_targets

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
OUT_NAMES = ("obs", "reward", "reward_f64", "terminated", "truncated", "status")
STATE_KEYS = ("m", "target", "total_energy", "step_count", "rng_step", "done")
CASES, DEVICE_CASES = bcc.cases(), bcc.device_cases()
NAMES = [c["name"] for c in CASES]
TOL = bcc.TOL
TRAJ_LANES = (0, 63, 64, 127, 128, 129)
_WORST = {}


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _backend(stg, c, p, noise="brown", thermal=True, start=True, **extra):
    """a context on the case's configuration (every field off its default), class table and start state"""
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    cfg = dict(dict(diagnostics=True, solver=c["method"], seed=bcc.SEED, include_thermal_fluctuations=thermal, noise_model=noise), **p["cfg"])
    cfg.update(extra)
    cfg["target_states"] = unit_targets(cfg["target_states"]).tolist()       # (stg_config.targets are unit vectors: the env normalises its list)
    b = HipBackend(c["n"], EnvConfig(**cfg), 0, bcc.ENV_ID0)
    flat = [stg.flatten_params(stg.DeviceFactory().create_device(t, d)) for d, t in zip(p["plist"], bcc.DEV_TYPES)]
    b.set_params(flat, torch.as_tensor(p["cls"]))
    if start:
        st = p["state"]
        b.reset(init_m=_dev(st["m"].T), target=_dev(st["target"].T))
        b.set_state(dict(total_energy=st["total_energy"], step_count=st["step_count"].astype(np.int32)))
    return b


def _normals_of(b):
    """the device's own draws of every env at stream position rng_step -> [N, count, 3]"""
    return lambda rng_step, count: b.thermal_normals(int(rng_step), 0, int(count)).permute(2, 0, 1).cpu().numpy()


def _state(b):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in b.get_state().items()}


def _np(t):
    return t.cpu().numpy()


def _got(out, st=None, k=None, energy=None):
    """a launch's outputs (and the state after it) env-major, as brown_config_cases.compare_step takes them; k: the step of a fused launch"""
    pick = (lambda t: t) if k is None else (lambda t: t[k])
    g = {name: _np(pick(out[name])) for name in OUT_NAMES if name != "reward"}
    g["obs"] = g["obs"].T
    g["energy"] = _np(pick(energy if energy is not None else out["energy"]))
    if st is not None:
        g.update(m=_np(st["m"]).T, step_count=_np(st["step_count"]), total_energy=_np(st["total_energy"]))
    return g


def _outs(b, res):
    torch.cuda.synchronize()
    d = {k: v.clone() for k, v in zip(OUT_NAMES, res)}
    d["energy"] = b.energy.clone()
    return d


def _many_outs(b, res):
    torch.cuda.synchronize()
    d = {k: v.clone() for k, v in zip(OUT_NAMES, res)}
    d["energy"] = b.energy_many.clone()
    return d


def _ids_outs(out):
    torch.cuda.synchronize()
    return dict(obs=out["obs"], reward_f64=out["reward64"], terminated=out["terminated"], truncated=out["truncated"], status=out["status"],
                energy=out["energy"])


def _bits(t):
    t = t.contiguous()
    return t.view({F32: torch.int32, F64: torch.int64, torch.bool: torch.uint8}.get(t.dtype, t.dtype))


def _same(x, y, what):
    assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape, x.dtype, y.dtype)
    bad = (_bits(x) != _bits(y)).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements differ, first at {bad[:4].tolist()}"


def _clear_of_the_threshold(refs, p, tag):
    """no flag of the comparison rests on rounding: the references' alignments (at the device's normals) stay 1e-8 off the threshold"""
    near = min(float(np.abs(r["alignment"] - p["cfg"]["success_threshold"]).min()) for r in refs)
    assert near > 1e-8, (tag, near)


def _record(test, name, err):
    _WORST[(test, name)] = max(_WORST.get((test, name), 0.0), err)


def _ids(c):
    """a permuted subset that holds the 2-lane tail (66 of 130 ids); the one env of the one-lane case"""
    n = c["n"]
    if n == 1:
        return np.array([0])
    rng = np.random.default_rng(9)
    ids = rng.permutation(np.concatenate([rng.permutation(n - 2)[:64], [n - 2, n - 1]]))
    assert len(np.unique(ids)) == 66 and n - 1 in ids and n - 2 in ids and not np.array_equal(ids, np.sort(ids))
    return ids


def _wave(cur=None, fld=None):
    """per-env knots env-major -- cur = (tj [N,K], jk [N,K]), fld = (th [N,K], hk [N,K,3]) -- as HipBackend takes them"""
    w = {"current": None, "field": None}
    if cur is not None:
        w["current"] = (_dev(np.asarray(cur[0]).T), _dev(np.asarray(cur[1]).T))
    if fld is not None:
        w["field"] = (_dev(np.asarray(fld[0]).T), _dev(np.transpose(np.asarray(fld[1]), (1, 2, 0))))
    return w


def _soa(acts):
    """[K,N,W] -> [K,W,N]"""
    return _dev(np.ascontiguousarray(np.asarray(acts).transpose(0, 2, 1)))


# ------------------------------------------------------------------------------------------------
# stg_solve, stg_solve_traj
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_solve_and_trajectory_vs_both_references(stg, oracle_mod, name):
    c = bcc.case(CASES, name)
    p = bcc.problem(c)
    n, cfg, cls = c["n"], p["cfg"], p["cls"]
    m0 = p["state"]["m"]
    J, T = wsr.parse_actions(p["acts"][0], cfg["max_current"], cfg["max_duration"])
    ns, _ = br.substeps(T, cfg["max_step"])
    b = _backend(stg, c, p, start=False)
    z = _normals_of(b)(bcc.ENV_STEP, int(ns.max()))
    s = bcc.strengths(oracle_mod, c, p)
    for ci in range(3):
        assert abs(b.thermal_strength(ci) - s[ci]) <= 1e-14 * s[ci]                      # dt-free, at this gamma and temperature
    ref_m, ora_m = np.zeros((n, 3)), np.zeros((n, 3))
    ocfg = bcc.oracle_config(oracle_mod, c, p)
    po = [oracle_mod.make_params(d, t) for d, t in zip(p["plist"], bcc.DEV_TYPES)]
    lanes = [j for j in TRAJ_LANES if j < n]
    ora_traj = {}
    for ci, d in enumerate(p["plist"]):
        sel = np.nonzero(cls == ci)[0]
        if len(sel):
            r = br.solve(m0[sel], T[sel], d, s[ci], z[sel], c["method"], J=J[sel], max_step=cfg["max_step"], temperature=cfg["temperature"], gamma=cfg["gamma"])
            assert r["success"].all() and np.array_equal(r["n_steps"], ns[sel])
            ref_m[sel] = r["m_final"]
    for i in range(n):
        o = oracle_mod.simple_solve(m0[i], T[i], po[int(cls[i])], ocfg, J[i], normals=z[i], want_traj=i in lanes)
        assert o["success"] and o["n_steps"] == ns[i]
        ora_m[i] = o["m_final"]
        if i in lanes:
            ora_traj[i] = o["m"]
    cap = int(ns.max()) + 1
    for traj_cap in (0, cap):
        out = b.solve(_dev(m0.T), _dev(J), _dev(T), env_step=bcc.ENV_STEP, traj_cap=traj_cap)
        torch.cuda.synchronize()
        mf = _np(out["m_final"]).T
        e_r, e_o = float(np.abs(mf - ref_m).max()), float(np.abs(mf - ora_m).max())
        print(f"solve {name} traj_cap={traj_cap}: |m - m_ref| = {e_r:.2e} (restatement), {e_o:.2e} (oracle); sub-steps {int(ns.min())} ... {int(ns.max())}")
        _record("solve", name, max(e_r, e_o))
        assert e_r <= TOL and e_o <= TOL, (name, traj_cap, e_r, e_o)
        assert np.array_equal(_np(out["n_points"]), ns) and bool((out["success"] == 1).all())
    assert float(np.abs(mf - m0).max()) > 1e-3
    t, m = _np(out["t"]), _np(out["m"])
    for j in lanes:
        d = p["plist"][int(cls[j])]
        rj = br.solve(m0[j:j + 1], T[j:j + 1], d, s[int(cls[j])], z[j:j + 1], c["method"], J=J[j:j + 1], max_step=cfg["max_step"],
                      temperature=cfg["temperature"], gamma=cfg["gamma"], trajectory=True)
        k = int(ns[j]) + 1
        assert np.array_equal(t[:k, j], rj["t"]), (name, j)
        e_r, e_o = float(np.abs(m[:k, :, j] - rj["m"]).max()), float(np.abs(m[:k, :, j] - ora_traj[j]).max())
        _record("solve", name, max(e_r, e_o))
        assert e_r <= TOL and e_o <= TOL, (name, "trajectory of lane", j, e_r, e_o)
        assert not t[k:, j].any() and not m[k:, :, j].any()
    b.close()


# ------------------------------------------------------------------------------------------------
# step(), step_many with autoreset, step_ids: both references
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_two_chained_steps_vs_both_references(stg, oracle_mod, name):
    c = bcc.case(CASES, name)
    p = bcc.problem(c)
    n = c["n"]
    b = _backend(stg, c, p)
    refs = {e: bcc.run_chain(c, p, oracle_mod, _normals_of(b), engine=e) for e in ("restatement", "oracle")}
    _clear_of_the_threshold(refs["restatement"], p, name)
    for k in range(bcc.STEPS):
        a = p["acts"][k]
        assert a.dtype == (np.float64 if c["f64"] else np.float32)
        o = _outs(b, b.step(_dev(a.T)))
        st = _state(b)
        for e, r in refs.items():
            err = bcc.compare_step(_got(o, st), r[k], TOL, (name, "step", k, e), first=k == 0)
            print(f"step {name} step {k} against the {e}: |m - m_ref| = {err:.2e}")
            _record("step", name, err)
        assert bool((st["rng_step"] == k + 1).all())
    work = int(sum(r["n_sub"].sum() for r in refs["restatement"]))
    assert b.counters() == {"env_steps": bcc.STEPS * n, "work_units": work, "noop_steps": 0}
    if n > 1:
        assert any(r["terminated"].any() for r in refs["restatement"]) and not all(r["terminated"].all() for r in refs["restatement"])
    b.close()


@pytest.mark.parametrize("name", NAMES)
def test_fused_launch_with_autoreset_vs_both_references(stg, oracle_mod, name):
    """step_many, K = 3, out_every, autoreset.  A fused launch hands back the fp64 state of its last step only, so the state after step k
    comes from a launch of the first k + 1 steps on a twin context; an env that is redrawn inside the launch takes the device's own
    redraw in the references too."""
    from helpers import device_reset_draw
    c = bcc.case(CASES, name)
    p = bcc.problem(c)
    n, K = c["n"], bcc.K_MANY
    states, out, final = [], None, None
    for j in range(1, K + 1):
        b = _backend(stg, c, p)
        res = b.step_many(_soa(p["acts"][:j]), out_every=True, autoreset=True)
        states.append({key: _np(v) for key, v in _state(b).items()})
        if j == K:
            out, final = _many_outs(b, res), b.final_obs_many.clone()
            normals_of = _normals_of(b)
            refs = {e: bcc.run_chain(c, p, oracle_mod, normals_of, engine=e, K=K, autoreset=True,
                                     reset_of=lambda k, ids, rng_step: (states[k]["m"][:, ids].T, states[k]["target"][:, ids].T))
                    for e in ("restatement", "oracle")}
            cnt = b.counters()
        b.close()
    _clear_of_the_threshold(refs["restatement"], p, name)
    targets = unit_targets(p["cfg"]["target_states"])
    resets = []
    for k in range(K):
        base = refs["restatement"][k]
        done = base["done"]
        resets.append(int(done.sum()))
        g = _got(out, k=k)
        new_obs = g["obs"].copy()
        g["obs"] = np.where(done[:, None], _np(final[k]).T, g["obs"])                       # the terminal observation of a redrawn env
        live = ~done
        for e, chain in refs.items():
            r = chain[k]
            assert np.array_equal(r["done"], done)
            bcc.compare_step(g, dict(r, obs=r["final_obs"]), TOL, (name, "step_many", k, e), first=k == 0)
            err = float(np.abs(states[k]["m"].T[live] - r["m"][live]).max()) if live.any() else 0.0
            print(f"step_many {name} step {k} against the {e}: |m - m_ref| = {err:.2e} over {int(live.sum())} envs, {int(done.sum())} redrawn")
            _record("step_many", name, err)
            assert err <= TOL, (name, k, e, err)
            after = r["state_after"]
            assert np.array_equal(states[k]["step_count"], after["step_count"])
            assert np.all(np.abs(states[k]["total_energy"] - after["total_energy"]) <= 10 * TOL * np.abs(after["total_energy"]))
            # the first observation of the new episode, from the device's own redraw
            ob_ref = r["obs"][done]
            assert np.all(np.abs(new_obs[done] - ob_ref) <= wsr.F32_ULP * np.abs(ob_ref) + 2 * TOL), (name, k, e, "obs of the new episode")
        # the redraw itself: the restated draw at the env's stream position (fp32 device normals: 2e-6), its target a table row, exactly
        for i in np.nonzero(done)[0]:
            m_d, t_d = device_reset_draw(bcc.SEED, bcc.ENV_ID0 + int(i), k + 1, targets)
            assert np.abs(states[k]["m"][:, i] - m_d).max() < 2e-6 and np.abs(states[k]["target"][:, i] - t_d).max() <= 5e-16, (name, k, i)
        assert (states[k]["rng_step"] == k + 1).all()
    print(f"step_many {name}: redrawn per step {resets}")
    if n > 1:
        assert resets[0] > 0 and resets[1] > 0 and max(resets) < n                         # resets inside the launch, not everywhere
    assert cnt["env_steps"] == K * n and cnt["noop_steps"] == 0 and cnt["work_units"] == int(sum(r["n_sub"].sum() for r in refs["restatement"]))


@pytest.mark.parametrize("name", NAMES)
def test_step_ids_on_a_permuted_subset_vs_both_references(stg, oracle_mod, name):
    c = bcc.case(CASES, name)
    p = bcc.problem(c)
    n, ids = c["n"], _ids(c)
    others = np.setdiff1d(np.arange(n), ids)
    b = _backend(stg, c, p)
    start = _state(b)
    refs = {e: bcc.run_chain(c, p, oracle_mod, _normals_of(b), engine=e, sel=ids) for e in ("restatement", "oracle")}
    _clear_of_the_threshold(refs["restatement"], p, name)
    for k in range(bcc.STEPS):
        o = _ids_outs(b.step_ids(_dev(p["acts"][k][ids].T), _dev(ids)))
        st = _state(b)
        sub = {key: v[..., _dev(ids)] for key, v in st.items()}
        for e, r in refs.items():
            err = bcc.compare_step(_got(o, sub), r[k], TOL, (name, "step_ids", k, e), first=k == 0)
            print(f"step_ids {name} step {k} against the {e}: |m - m_ref| = {err:.2e} over {len(ids)} envs")
            _record("step_ids", name, err)
        if len(others):
            rest = _dev(others)
            for key in STATE_KEYS:
                _same(st[key][..., rest], start[key][..., rest], (name, "step_ids: unlisted envs", k, key))
        assert bool((sub["rng_step"] == k + 1).all())
    b.close()


# ------------------------------------------------------------------------------------------------
# the waveform entry points against the restatement under tables
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_solve_wave_vs_restatement(stg, oracle_mod, name):
    c = bcc.case(CASES, name)
    p = bcc.problem(c)
    n, cfg, cls = c["n"], p["cfg"], p["cls"]
    m0 = p["state"]["m"]
    _, T = wsr.parse_actions(p["acts"][0], cfg["max_current"], cfg["max_duration"])
    ns, _ = br.substeps(T, cfg["max_step"])
    (tj, jk), (th, hk) = bcc.wave_tables(p, 0)
    b = _backend(stg, c, p, start=False)
    z = _normals_of(b)(bcc.ENV_STEP, int(ns.max()))
    s = bcc.strengths(oracle_mod, c, p)
    ref_m = np.zeros((n, 3))
    for ci, d in enumerate(p["plist"]):
        sel = np.nonzero(cls == ci)[0]
        if len(sel):
            r = br.solve(m0[sel], T[sel], d, s[ci], z[sel], c["method"], current=(tj[sel], jk[sel]), field=(th[sel], hk[sel]), max_step=cfg["max_step"],
                         temperature=cfg["temperature"], gamma=cfg["gamma"])
            assert r["success"].all()
            ref_m[sel] = r["m_final"]
    out = b.solve(_dev(m0.T), None, _dev(T), env_step=bcc.ENV_STEP, wave=_wave((tj, jk), (th, hk)))
    torch.cuda.synchronize()
    err = float(np.abs(_np(out["m_final"]).T - ref_m).max())
    print(f"solve_wave {name}: |m - m_ref| = {err:.2e}")
    _record("solve_wave", name, err)
    assert err <= TOL and np.array_equal(_np(out["n_points"]), ns) and bool((out["success"] == 1).all())
    b.close()


@pytest.mark.parametrize("name", NAMES)
def test_step_wave_two_chained_steps_vs_restatement(stg, oracle_mod, name):
    c = bcc.case(CASES, name)
    p = bcc.problem(c)
    b = _backend(stg, c, p)
    refs = bcc.run_chain(c, p, oracle_mod, _normals_of(b), drive="wave")
    _clear_of_the_threshold(refs, p, name)
    for k in range(bcc.STEPS):
        o = _outs(b, b.step_wave(_dev(p["acts"][k].T), _wave(*bcc.wave_tables(p, k))))
        err = bcc.compare_step(_got(o, _state(b)), refs[k], TOL, (name, "step_wave", k), first=k == 0)
        print(f"step_wave {name} step {k}: |m - m_ref| = {err:.2e}")
        _record("step_wave", name, err)
    assert b.counters()["work_units"] == int(sum(r["n_sub"].sum() for r in refs))
    b.close()


@pytest.mark.parametrize("drive", ("shaped", "knots"))
@pytest.mark.parametrize("name", NAMES)
def test_shaped_and_knot_entries_vs_restatement(stg, oracle_mod, name, drive):
    """stg_step_shaped / stg_step_knots: launches of one and of two steps (a launch hands back the fp64 state of its last step), then
    stg_step_shaped_ids / stg_step_knots_ids: the second step on the permuted subset after a full first step"""
    c = bcc.case(CASES, name)
    p = bcc.problem(c)
    n, ids = c["n"], _ids(c)
    acts = p["kacts"] if drive == "knots" else p["acts"]

    def make():
        b = _backend(stg, c, p)
        if drive == "knots":
            b.set_pulse_knots(p["tau"], p["limit"], p["fk"])
        else:
            b.set_pulse_shape(p["shape"], p["fk"])
        return b
    many = (lambda b, a, **kw: b.step_knots_many(a, **kw)) if drive == "knots" else (lambda b, a, **kw: b.step_shaped_many(a, **kw))
    refs = None
    for j in range(1, bcc.STEPS + 1):
        b = make()
        if refs is None:
            refs = bcc.run_chain(c, p, oracle_mod, _normals_of(b), drive=drive)
            _clear_of_the_threshold(refs, p, (name, drive))
        o = _many_outs(b, many(b, _soa(acts[:j]), out_every=False))
        err = bcc.compare_step(_got(o, _state(b), k=0), refs[j - 1], TOL, (name, drive, "launch of", j), first=j == 1)
        print(f"{drive} {name} launch of {j}: |m - m_ref| = {err:.2e}")
        _record(drive, name, err)
        assert b.counters()["work_units"] == int(sum(r["n_sub"].sum() for r in refs[:j]))
        b.close()
    b = make()
    many(b, _soa(acts[:1]), out_every=False)
    before = _state(b)
    entry = b.step_knots_ids if drive == "knots" else b.step_shaped_ids
    o = _ids_outs(entry(_dev(acts[1][ids].T), _dev(ids)))
    st = _state(b)
    idt = _dev(ids)
    sub = {key: v[..., idt] for key, v in st.items()}
    ref = {key: (v[ids] if isinstance(v, np.ndarray) and len(v) == n else v) for key, v in refs[1].items()}
    err = bcc.compare_step(_got(o, sub), ref, TOL, (name, drive, "ids"), first=False)
    print(f"{drive}_ids {name}: |m - m_ref| = {err:.2e} over {len(ids)} envs")
    _record(drive + "_ids", name, err)
    others = np.setdiff1d(np.arange(n), ids)
    if len(others):
        for key in STATE_KEYS:
            _same(st[key][..., _dev(others)], before[key][..., _dev(others)], (name, drive, "ids: unlisted envs", key))
    b.close()


# ------------------------------------------------------------------------------------------------
# the device torque model: every lane against the fed-normals oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in DEVICE_CASES])
def test_device_torque_model_every_lane_vs_the_fed_oracle(stg, oracle_mod, name):
    """torque_model='device', STT + SOT + VCMA, J != 0 in every lane: the SOT and VCMA lanes' own torque by value (the NumPy
    restatement knows the reference torque model only; tests/test_gpu_brown.py asserts them finite and unit)"""
    c = bcc.case(DEVICE_CASES, name)
    p = bcc.problem(c)
    n, cls = c["n"], p["cls"]
    b = _backend(stg, c, p, torque_model="device")
    refs = bcc.run_chain(c, p, oracle_mod, _normals_of(b), engine="oracle", torque_model=1)
    other = bcc.run_chain(c, p, oracle_mod, _normals_of(b), engine="oracle", torque_model=0)
    _clear_of_the_threshold(refs, p, name)
    J, _ = wsr.parse_actions(p["acts"][0], p["cfg"]["max_current"], p["cfg"]["max_duration"])
    assert (np.abs(J) > 1e-12).all() and set(cls.tolist()) == {0, 1, 2}
    for k in range(bcc.STEPS):
        o = _outs(b, b.step(_dev(p["acts"][k].T)))
        st = _state(b)
        err = bcc.compare_step(_got(o, st), refs[k], TOL, (name, k), first=k == 0)                       # all 130 lanes
        m = _np(st["m"]).T
        per = [float(np.abs(m[cls == ci] - refs[k]["m"][cls == ci]).max()) for ci in range(3)]
        print(f"{name} step {k}: |m - m_oracle| STT {per[0]:.2e}, SOT {per[1]:.2e}, VCMA {per[2]:.2e}")
        _record("device torque", name, err)
    # the comparison is of each class's own torque: the reference torque model is far from it on the SOT and VCMA lanes
    d = np.abs(refs[0]["m"] - other[0]["m"]).max(axis=1)
    assert (d[cls == 1] > 1e-8).all() and (d[cls == 2] > 1e-8).all()
    assert b.counters() == {"env_steps": bcc.STEPS * n, "work_units": int(sum(r["n_sub"].sum() for r in refs)), "noop_steps": 0}
    b.close()


# ------------------------------------------------------------------------------------------------
# the stream key and the configuration gates
# ------------------------------------------------------------------------------------------------
def _vec_env(stg, c, p, n, lo, noise="brown", **over):
    cfg = dict(p["cfg"])
    solver_consts = dict(max_step=cfg.pop("max_step"), gamma=cfg.pop("gamma"))
    kw = dict(diagnostics=True, device_type=list(bcc.DEV_TYPES), device_params=p["plist"], class_index=p["cls"][lo:lo + n], solver=c["method"],
              seed=bcc.SEED, include_thermal_fluctuations=True, noise_model=noise, env_id0=lo, backend=backend_factory(None, **solver_consts))
    kw.update(cfg)
    kw.update(over)
    env = stg.SpinTorqueVecEnv(n, **kw)
    st = p["state"]
    env.reset(options={"initial_state": st["m"][lo:lo + n], "target_state": st["target"][lo:lo + n]})
    return env


def _env_step(env, a):
    obs, r, te, tr, info = env.step(torch.from_numpy(a))
    torch.cuda.synchronize()
    st = env.get_state()
    return dict(obs=obs.clone(), reward=r.clone(), terminated=te.clone(), truncated=tr.clone(), reward_f64=info["reward_f64"].clone(),
                energy=info["energy"].clone(), status=info["status"].clone(), **{"state_" + k: v.clone() for k, v in st.items()})


@pytest.mark.parametrize("name", [NAMES[3], NAMES[8]])
def test_stream_key_two_envs_of_65_equal_one_of_130(stg, name):
    """env_id0 = 0 and env_id0 = 65 against one env of 130, two steps under 'brown': state and outputs bit for bit (the field of env i is
    keyed by its global index, whichever context holds it)"""
    c = bcc.case(CASES, name)
    p = bcc.problem(c)
    half = 65
    whole, lo_env, hi_env = _vec_env(stg, c, p, 2 * half, 0), _vec_env(stg, c, p, half, 0), _vec_env(stg, c, p, half, half)
    for k in range(bcc.STEPS):
        a = p["acts"][k]
        w, lo, hi = _env_step(whole, a), _env_step(lo_env, a[:half]), _env_step(hi_env, a[half:])
        for key in w:
            env_axis = 0 if key in ("obs",) or w[key].dim() == 1 else 1
            joined = torch.cat([lo[key], hi[key]], dim=env_axis)
            _same(joined, w[key], (name, "stream key", k, key))
        assert bool((w["status"] == 0).all())
    # ... and the key matters: the second half stepped as if it were the first is another stream
    again = _vec_env(stg, c, p, half, half, env_id0=0)
    x = _env_step(again, p["acts"][0][half:])
    assert float((x["state_m"] - _env_step(_vec_env(stg, c, p, half, half), p["acts"][0][half:])["state_m"]).abs().max()) > 1e-3
    for e in (whole, lo_env, hi_env, again):
        e.close()


@pytest.mark.parametrize("gate", ("temperature 0", "temperature -3", "thermal off"))
@pytest.mark.parametrize("name", [NAMES[0], NAMES[9]])
def test_gated_off_brown_is_white_bit_for_bit(stg, name, gate):
    """temperature <= 0 (the fixed-step solve is rejected: a no-op step) and include_thermal_fluctuations=False (the solve without a
    field): no field is drawn, the model name decides nothing, and rng_step still advances"""
    c = bcc.case(CASES, name)
    p = bcc.problem(c)
    over = dict(thermal=False) if gate == "thermal off" else dict(temperature=float(gate.split()[1]))
    runs = {}
    for noise in ("brown", "white"):
        b = _backend(stg, c, p, noise=noise, **over)
        rec = []
        for k in range(bcc.STEPS):
            o = _outs(b, b.step(_dev(p["acts"][k].T)))
            rec.append((o, _state(b)))
        runs[noise] = rec
        b.close()
    for k in range(bcc.STEPS):
        (ob, sb), (ow, sw) = runs["brown"][k], runs["white"][k]
        for key in ob:
            _same(ob[key], ow[key], (name, gate, k, key))
        for key in STATE_KEYS:
            _same(sb[key], sw[key], (name, gate, k, "state", key))
        assert bool((sb["rng_step"] == k + 1).all())
        assert bool((ob["status"] == (0 if gate == "thermal off" else 1)).all()), (gate, ob["status"][:8])
    if gate == "thermal off":
        assert float((runs["brown"][0][1]["m"] - _dev(p["state"]["m"].T)).abs().max()) > 1e-3


def test_zz_worst_differences_table():
    """prints what the tests above measured (profiles/NOTEBOOK.md holds the table of a run)"""
    tests = sorted({t for t, _ in _WORST})
    for t in tests:
        rows = {n: v for (tt, n), v in _WORST.items() if tt == t}
        print(f"{t}: worst |m - m_ref| = {max(rows.values()):.2e} over {len(rows)} cases")
        for n, v in rows.items():
            print(f"    {n}: {v:.2e}")

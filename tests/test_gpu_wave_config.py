"""The waveform entry points (stg_solve_wave, stg_step_wave, stg_step_shaped, stg_step_shaped_ids) off their defaults, on the GPU:
`pytest -m gpu`.  Solver constants (rtol, atol, max_step, gamma, max_attempts), temperatures, the thermal field with non-zero tables,
the episode fields, the five-target list and a class table STT / SOT / VCMA -- none of which the tests these kernels came with vary.

  stg_solve_wave   the rows the reference computed under those settings (tests/golden/G24_wave_config.npz), thermal off and on through
                   the oracle's normal stream, with the trajectory and by-products of one row; a random fixed-step sweep against the
                   NumPy restatement (max_step x gamma x noise, 77 / 450 K) with exact sub-step counts; thermal on at temperature 0
                   (fixed step: every problem rejected; RK45: the solve without the field);
  stg_step_wave    the env steps of G24 through the C-ABI and through SpinTorqueVecEnv(pulse_shape=, applied_field=); the sweep under
                   the non-default episode configuration with three device classes, float32 and float64 actions (a reduced
                   cross of max_step and gamma: wave_config_cases.step_cases);
  stg_step_shaped  (K = 3, out_every 0 and 1) and stg_step_shaped_ids (100 of 130, permuted): bit for bit K calls of stg_step_wave with
                   pulse_tables under the same configuration, per solver, noise model and layout; and once directly against the
                   restatement;
  max_attempts     an RK45 budget below the attempts G24 records: a failed solve, a no-op step that is charged its energy.

Tolerances are the project's: TOL_RK4 = 1e-10, TOL_RK45 = 1e-8, x 50 under the thermal field (the device normals carry fp32
transcendentals); energy 1e-13 relative; observations one float32 ulp plus 2 tol.  tests/test_wave_config_conditioning.py shows on the
CPU that every restatement case moves by less than tolerance / 100 per ulp of the start rows, the generator of G24 shows the same for its
rows.  N = 130 throughout (two full wavefronts and a two-lane tail), one case each at N = 1.

Measured on an MI355X, worst |m - m_ref| (each test prints its own): G24 solve rows rk4 1.2e-14, euler 4.7e-14, rk45 1.1e-13, under
the thermal field 4.1e-13, 8.7e-13 and 2.3e-9 (bound 5e-7); G24 env steps 1.8e-15, thermal 6.1e-13, through the envs 7.5e-13; solve
sweep 8.2e-13, thermal 8.4e-11; step sweep 1.2e-12, thermal 1.6e-9 (bound 5e-9: the second of two chained steps); the last of three
steps of a shaped launch under the thermal field 2.8e-11; energies at most 6e-16 relative in every step, a later step's from the
kernels' own start rows (in a fused launch: from a launch of the steps before it on a twin context)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import stt_default_params
from env_config_cases import backend_factory, tol_for
from helpers import Guarded
import wave_config_cases as wcc
import wave_step_ref

pytestmark = pytest.mark.gpu

F32, F64, U8, I32 = torch.float32, torch.float64, torch.uint8, torch.int32
OUT_NAMES = ("obs", "reward", "reward_f64", "terminated", "truncated", "status")
OUT_KEYS = OUT_NAMES + ("energy",)
STATE_KEYS = ("m", "target", "total_energy", "step_count", "rng_step", "done")
STATUS_NOOP = 1


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _flat(stg, d, device_type="stt_mram"):
    return stg.flatten_params(stg.DeviceFactory().create_device(device_type, d))


def _backend(stg, n, plist, dev_types=None, cls=None, env_id0=0, **cfg):
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    b = HipBackend(n, EnvConfig(**{"diagnostics": True, **cfg}), 0, env_id0)
    dev_types = dev_types or ["stt_mram"] * len(plist)
    b.set_params([_flat(stg, p, t) for p, t in zip(plist, dev_types)], None if cls is None else torch.as_tensor(cls))
    return b


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _wave(cur=None, fld=None):
    """per-problem knots in the tests' layout -- cur = (tj [N,K], jk [N,K]), fld = (th [N,K], hk [N,K,3]) -- as HipBackend takes them"""
    w = {"current": None, "field": None}
    if cur is not None:
        w["current"] = (_dev(np.asarray(cur[0]).T), _dev(np.asarray(cur[1]).T))
    if fld is not None:
        w["field"] = (_dev(np.asarray(fld[0]).T), _dev(np.transpose(np.asarray(fld[1]), (1, 2, 0))))
    return w


def _bits(t):
    t = t.contiguous()
    return t.view({F32: torch.int32, F64: torch.int64}.get(t.dtype, t.dtype))


def _same(x, y, what):
    """bit for bit (floats compared as integers)"""
    assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape, x.dtype, y.dtype)
    bad = (_bits(x) != _bits(y)).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements differ, first at {bad[:4].tolist()}"


def _outs(b, res):
    torch.cuda.synchronize()
    d = {k: v.clone() for k, v in zip(OUT_NAMES, res)}
    d["energy"] = b.energy.clone()
    return d


def _state(b):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in b.get_state().items()}


def _noise_cfg(noise):
    kw = dict(include_thermal_fluctuations=noise is not None)
    if noise == "ou":
        kw.update(noise_model="ou", correlation_time=wcc.CORR_TIME)
    return kw


# ------------------------------------------------------------------------------------------------
# stg_solve_wave
# ------------------------------------------------------------------------------------------------
def test_solve_rows_of_g24(stg, golden):
    g = golden("G24_wave_config")
    traj_case = int(g["sv_traj_case"])
    worst = {}
    for k in range(len(g["sv_T"])):
        solver, thermal = wcc.g24_solver(g, k), bool(g["sv_thermal"][k])
        b = _backend(stg, 1, [stt_default_params(volume=float(g["sv_volume"][k]))], env_id0=int(g["sv_env_id"][k]), solver=solver,
                     include_thermal_fluctuations=thermal, seed=int(g["sv_seed"][k]), temperature=float(g["sv_temperature"][k]),
                     rtol=float(g["sv_rtol"][k]), atol=float(g["sv_atol"][k]), max_step=float(g["sv_max_step"][k]), gamma=float(g["sv_gamma"][k]))
        cur, fld = wcc.g24_solve_knots(g, k)
        T, npts = float(g["sv_T"][k]), int(g["sv_n_points"][k])
        cap = npts + 9 if k == traj_case else 0
        out = b.solve(_dev(g["sv_m0"][k][:, None]), None if cur is not None else torch.zeros(1, dtype=F64), torch.tensor([T], dtype=F64),
                      env_step=int(g["sv_env_step"][k]), traj_cap=cap, want_energy=cap > 0, wave=_wave(cur, fld))
        res = {key: (None if v is None else v.cpu().numpy()) for key, v in out.items()}
        b.close()
        tol = tol_for(solver, thermal)
        err = float(np.abs(res["m_final"][:, 0] - g["sv_m_final"][k]).max())
        worst[(solver, thermal)] = max(worst.get((solver, thermal), 0.0), err)
        print(f"G24 solve {k} ({solver}, thermal={thermal}, {g['sv_temperature'][k]:g} K, max_step={g['sv_max_step'][k]:g}, gamma={g['sv_gamma'][k]:g}): "
              f"n_points {int(res['n_points'][0])} (ref {npts}, {int(g['sv_attempts'][k])} attempts), |m - m_ref| = {err:.2e} (bound {tol:.0e})")
        assert bool(res["success"][0]) == bool(g["sv_success"][k]), k
        if not (thermal and solver == "rk45"):                 # (RK45 under the thermal field: printed, the device normals carry fp32 transcendentals)
            assert int(res["n_points"][0]) == npts, (k, int(res["n_points"][0]), npts)
        assert err <= tol, (k, err)
        if cap:
            rt, rm, re, rq = (g[f"sv_traj_{name}"] for name in ("t", "m", "energy", "torques"))
            kk = len(rt)
            errs = (np.abs(res["t"][:kk, 0] - rt).max(), np.abs(res["m"][:kk, :, 0] - rm).max(), np.abs(res["energy"][:kk, 0] - re).max(),
                    np.abs(res["torques"][:kk, 0] - rq).max())
            print(f"G24 solve {k} trajectory: t {errs[0]:.2e} (T {T:g}), m {errs[1]:.2e}, energy {errs[2]:.2e} (max {np.abs(re).max():.2e}), "
                  f"torques {errs[3]:.2e} (max {np.abs(rq).max():.2e})")
            assert errs[0] <= 1e-9 * rt[-1] and errs[1] <= tol and errs[2] <= 1e-8 * np.abs(re).max() and errs[3] <= 1e-8 * np.abs(rq).max()
    print("G24 solve rows, worst |m - m_ref|: " + ", ".join(f"{s}{' thermal' if t else ''} {v:.2e}" for (s, t), v in sorted(worst.items())))


SOLVE_CASES = wcc.solve_cases()


@pytest.mark.parametrize("name", [c["name"] for c in SOLVE_CASES])
def test_solve_sweep_vs_restatement(stg, oracle_mod, name):
    c = wcc.case(SOLVE_CASES, name)
    p, ref = wcc.solve_ref(c, oracle_mod)
    n, thermal = c["n"], c["noise"] is not None
    b = _backend(stg, n, [p["params"]], env_id0=wcc.ENV_ID0, solver=c["method"], seed=wcc.SEED, temperature=c["temperature"], max_step=c["max_step"],
                 gamma=c["gamma"], **_noise_cfg(c["noise"]))
    out = b.solve(_dev(p["m0"].T), None, _dev(p["T"]), env_step=wcc.ENV_STEP, wave=_wave(p["cur"], p["fld"]))
    ok = out["success"].cpu().numpy().astype(bool)
    mf = out["m_final"].cpu().numpy().T
    b.close()
    err, tol = float(np.abs(mf - ref["m_final"]).max()), tol_for(c["method"], thermal)
    print(f"solve sweep {name}: worst |m - m_ref| = {err:.2e} (bound {tol:.0e}), sub-steps {int(ref['n_steps'].min())} ... {int(ref['n_steps'].max())}")
    assert ref["success"].all() and np.array_equal(ok, ref["success"])
    assert np.array_equal(out["n_points"].cpu().numpy(), ref["n_steps"])                 # max_step decides them (wave_config_cases.py)
    assert err <= tol


@pytest.mark.parametrize("method", ("rk4", "euler"))
def test_thermal_on_at_temperature_zero_rejects_every_problem(stg, method):
    c = next(x for x in SOLVE_CASES if x["method"] == method and x["noise"] == "white" and x["n"] == wcc.N)
    p = wcc.solve_problem(c)
    n, cap = c["n"], 4
    b = _backend(stg, n, [p["params"]], solver=method, seed=wcc.SEED, temperature=0.0, **_noise_cfg("white"))
    m0, T = _dev(p["m0"].T), _dev(p["T"])
    kj, tj, jk, kh, th, hk = b._wave_tables(_wave(p["cur"], p["fld"]))
    # the trajectory arrays between sentinels: no row of a rejected problem is written
    g = {k: Guarded(k, s, d) for k, s, d in (("t", (cap, n), F64), ("m", (cap, 3, n), F64), ("m_final", (3, n), F64), ("n_points", (n,), I32),
                                             ("success", (n,), U8))}
    ptr = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    rc = b.lib.stg_solve_wave(b._ctx, ptr(m0), None, ptr(T), kj, ptr(tj), ptr(jk), kh, ptr(th), ptr(hk), 0, cap, ptr(g["t"].interior),
                              ptr(g["m"].interior), None, None, ptr(g["m_final"].interior), ptr(g["n_points"].interior), ptr(g["success"].interior),
                              b._stream())
    assert rc == 0, b.lib.stg_last_error()
    torch.cuda.synchronize()
    g["t"].check(written=False)
    g["m"].check(written=False)
    assert not bool(g["success"].check().any()) and bool((g["n_points"].check() == 0).all())
    _same(g["m_final"].check(), m0, "m_final of a rejected problem")
    b.close()


def test_rk45_thermal_on_at_temperature_zero_is_the_solve_without_the_field(stg, golden):
    """RK45 has no temperature gate (oracle/stg_oracle.c, stgo_llgs_solve; llgs_solver.py:85-90): at temperature 0 the thermal strength
    is sqrt(0) = 0, the draws are multiplied by it, and the solve is the one without the field -- here a thermal-off RK45 row of G24."""
    g = golden("G24_wave_config")
    k = next(i for i in range(len(g["sv_T"])) if wcc.g24_solver(g, i) == "rk45" and not g["sv_thermal"][i] and g["sv_kj"][i] == 0)
    b = _backend(stg, 1, [stt_default_params(volume=float(g["sv_volume"][k]))], solver="rk45", include_thermal_fluctuations=True, seed=9,
                 temperature=0.0, rtol=float(g["sv_rtol"][k]), atol=float(g["sv_atol"][k]), max_step=float(g["sv_max_step"][k]),
                 gamma=float(g["sv_gamma"][k]))
    cur, fld = wcc.g24_solve_knots(g, k)
    out = b.solve(_dev(g["sv_m0"][k][:, None]), torch.zeros(1, dtype=F64), torch.tensor([float(g["sv_T"][k])], dtype=F64), env_step=3,
                  wave=_wave(cur, fld))
    torch.cuda.synchronize()
    err = float(np.abs(out["m_final"][:, 0].cpu().numpy() - g["sv_m_final"][k]).max())
    print(f"rk45, thermal on at 0 K, against G24 solve {k}: n_points {int(out['n_points'][0])} (ref {int(g['sv_n_points'][k])}), |m - m_ref| = {err:.2e}")
    assert bool(out["success"][0]) and int(out["n_points"][0]) == int(g["sv_n_points"][k])
    assert err <= tol_for("rk45", False)
    b.close()


# ------------------------------------------------------------------------------------------------
# stg_step_wave
# ------------------------------------------------------------------------------------------------
def _g24_env_backend_cfg(g, k):
    cfg = wcc.g24_env_cfg(g, k)
    return dict(cfg, solver=("rk4", "euler")[int(g["ev_solver"][k])], include_thermal_fluctuations=bool(g["ev_thermal"][k]), seed=int(g["ev_seed"]))


def test_env_steps_of_g24_through_the_c_abi(stg, golden):
    g = golden("G24_wave_config")
    worst = {False: 0.0, True: 0.0}
    for k in range(len(g["ev_T"])):
        thermal = bool(g["ev_thermal"][k])
        b = _backend(stg, 1, [stt_default_params(volume=float(g["ev_volume"][k]))], env_id0=int(g["ev_env_id"]), **_g24_env_backend_cfg(g, k))
        b.reset(init_m=_dev(g["ev_m_before"][k][:, None]), target=_dev(g["ev_target"][k][:, None]))
        b.set_state(dict(m=g["ev_m_before"][k][:, None], target=g["ev_target"][k][:, None], total_energy=np.array([g["ev_etot_before"][k]]),
                         step_count=np.array([g["ev_step_before"][k]], dtype=np.int32), rng_step=np.array([g["ev_step_before"][k]], dtype=np.int32),
                         done=np.zeros(1, dtype=np.uint8)))
        cur, fld = wcc.g24_env_tables(g, k)
        o = _outs(b, b.step_wave(_dev(wcc.g24_env_action(g, k).T), _wave(cur, fld)))
        m = _state(b)["m"][:, 0].cpu().numpy()
        b.close()
        got = dict(m=m, obs=o["obs"][:, 0].cpu().numpy(), reward=float(o["reward_f64"][0]), terminated=int(o["terminated"][0]),
                   truncated=int(o["truncated"][0]), energy=float(o["energy"][0]))
        err = wcc.check_step_against_g24(g, k, got, tol_for("rk4", thermal), "C-ABI")
        worst[thermal] = max(worst[thermal], err)
        print(f"G24 env step {k} (episode {g['ev_episode'][k]}, thermal={thermal}, kj={g['ev_kj'][k]}, kh={g['ev_kh'][k]}, T={g['ev_T'][k]:g}): "
              f"|m - m_ref| = {err:.2e}")
        assert int(o["status"][0]) == 0
    print(f"G24 env steps through the C-ABI: worst |m - m_ref| thermal off {worst[False]:.2e}, thermal on {worst[True]:.2e}")


@pytest.mark.parametrize("how", ("step", "step_many"))
def test_episodes_of_g24_through_the_vec_env(stg, golden, how):
    """The envs build the tables themselves: step() calls stg_step_wave with pulse_tables, step_many() is one stg_step_shaped launch.  A
    launch hands back the fp64 magnetisation of its last step only, so step j of an episode is checked on the launch of its first j + 1
    steps.  Lane 1 is the env whose stream the thermal episodes were recorded on; without the thermal field both lanes are checked."""
    from spin_torque_gym_amd.physics import PiecewiseLinear
    g = golden("G24_wave_config")
    worst = 0.0
    for e in np.unique(g["ev_episode"]):
        ks = np.nonzero(g["ev_episode"] == e)[0]
        k0 = ks[0]
        thermal = bool(g["ev_thermal"][k0])
        shape, fk = wcc.g24_shape_and_field(g, k0)
        cfg = wcc.g24_env_cfg(g, k0)
        max_step = cfg.pop("max_step")
        lanes = [int(g["ev_env_id"])] if thermal else [0, 1]

        def make():
            env = stg.SpinTorqueVecEnv(2, diagnostics=True, out_layout="records" if e % 2 else "soa", device_params=stt_default_params(volume=float(g["ev_volume"][k0])),
                                       include_thermal_fluctuations=thermal, solver=("rk4", "euler")[int(g["ev_solver"][k0])], seed=int(g["ev_seed"]),
                                       pulse_shape=shape, applied_field=None if fk is None else PiecewiseLinear(*fk),
                                       backend=backend_factory(None, max_step=max_step), **cfg)
            env.reset(options={"initial_state": g["ev_m_before"][k0], "target_state": g["ev_target"][k0]})
            return env
        tol = tol_for("rk4", thermal)
        if how == "step":
            env = make()
            for k in ks:
                obs, rew, term, trunc, info = env.step(torch.from_numpy(np.repeat(wcc.g24_env_action(g, k), 2, axis=0)))
                torch.cuda.synchronize()
                m = env.get_state()["m"].cpu().numpy()
                for i in lanes:
                    got = dict(m=m[:, i], obs=obs[i].cpu().numpy(), reward=float(info["reward_f64"][i]), terminated=bool(term[i]),
                               truncated=bool(trunc[i]), energy=float(info["energy"][i]))
                    worst = max(worst, wcc.check_step_against_g24(g, k, got, tol, f"episode {e}"))
            env.close()
            continue
        # one launch takes one action dtype: the float32 actions widened parse to the same (J, T) (checked against the file)
        acts = np.stack([np.repeat(wcc.g24_env_action(g, k).astype(np.float64), 2, axis=0) for k in ks])
        J, T = wave_step_ref.parse_actions(acts[:, 0], cfg["max_current"], cfg["max_duration"])
        assert np.array_equal(J, g["ev_J"][ks]) and np.array_equal(T, g["ev_T"][ks])
        for j, k in enumerate(ks):
            env = make()
            obs, rew, term, trunc, info = env.step_many(torch.from_numpy(acts[:j + 1]), out_every=False)
            torch.cuda.synchronize()
            m = env.get_state()["m"].cpu().numpy()
            for i in lanes:
                got = dict(m=m[:, i], obs=obs[0, i].cpu().numpy(), reward=float(info["reward_f64"][0, i]), terminated=bool(term[0, i]),
                           truncated=bool(trunc[0, i]), energy=float(info["energy"][0, i]))
                worst = max(worst, wcc.check_step_against_g24(g, k, got, tol, f"episode {e}, launch of {j + 1} steps"))
            env.close()
    print(f"G24 episodes through SpinTorqueVecEnv.{how}: worst |m - m_ref| = {worst:.2e}")


def _compare_step(o, st, ref, n, tol, tag, e_ref=None, etot_ref=None):
    """one step's outputs and state against the restatement, as tests/test_gpu_step_wave.py: test_random_sweep_vs_restatement.
    The energy goes with the resistance of the state BEFORE the step.  In a first step that state is the given one and the energy is
    held to 1e-13; in a later step it is the kernels' own state, which follows the restatement's to `tol` only, so the caller hands in
    the closed form evaluated at the kernels' own start rows (e_ref, etot_ref), still at 1e-13."""
    m = st["m"].cpu().numpy().T
    err = float(np.abs(m - ref["m"]).max())
    e = o["energy"].cpu().numpy()
    e_ref = ref["energy"] if e_ref is None else e_ref
    etot_ref = ref["total_energy"] if etot_ref is None else etot_ref
    e_err = float(np.max(np.abs(e - e_ref) / np.maximum(np.abs(e_ref), 1e-300)))
    print(f"{tag}: worst |m - m_ref| = {err:.2e} (bound {tol:.0e}), worst relative energy difference {e_err:.1e}")
    assert err <= tol, tag
    assert np.all(np.abs(e - e_ref) <= 1e-13 * np.abs(e_ref)), (tag, e_err)
    assert np.array_equal(o["terminated"].cpu().numpy().astype(bool), ref["terminated"]), tag
    assert np.array_equal(o["truncated"].cpu().numpy().astype(bool), ref["truncated"]), tag
    assert np.array_equal(o["status"].cpu().numpy(), ref["status"]), tag
    ob, ob_ref = o["obs"].cpu().numpy().T, ref["obs"]
    assert np.all(np.abs(ob - ob_ref) <= wave_step_ref.F32_ULP * np.abs(ob_ref) + 2 * tol), (tag, np.argwhere(np.abs(ob - ob_ref) > wave_step_ref.F32_ULP * np.abs(ob_ref) + 2 * tol)[:4])
    assert np.all(np.abs(o["reward_f64"].cpu().numpy() - ref["reward"]) <= 1e-9 + 2 * tol), tag
    assert np.array_equal(st["step_count"].cpu().numpy(), ref["step_count"]), tag
    assert np.all(np.abs(st["total_energy"].cpu().numpy() - etot_ref) <= 1e-13 * np.abs(etot_ref)), tag
    return err


STEP_CASES = wcc.step_cases()


def _step_backend(stg, c, p, **extra):
    cfg = dict(p["cfg"])
    b = _backend(stg, c["n"], p["plist"], wcc.DEV_TYPES, p["cls"], env_id0=wcc.ENV_ID0, solver=c["method"], seed=wcc.SEED, **_noise_cfg(c["noise"]),
                 **cfg, **extra)
    st = p["state"]
    b.reset(init_m=_dev(st["m"].T), target=_dev(st["target"].T))
    b.set_state(dict(total_energy=st["total_energy"], step_count=st["step_count"].astype(np.int32)))
    return b


@pytest.mark.parametrize("name", [c["name"] for c in STEP_CASES])
def test_step_sweep_vs_restatement(stg, oracle_mod, name):
    c = wcc.case(STEP_CASES, name)
    p, refs = wcc.step_ref(c, oracle_mod)
    n, thermal = c["n"], c["noise"] is not None
    for r in refs:
        assert (np.abs(r["alignment"] - p["cfg"]["success_threshold"]) > 1e-6).all() and (r["status"] == 0).all()     # every env is compared
    assert n < 3 or (len(set(p["cls"])) == 3 and any(r["terminated"].any() for r in refs) and refs[-1]["truncated"].any()
                     and (np.abs(refs[0]["J"]) == p["cfg"]["max_current"]).any())
    b = _step_backend(stg, c, p)
    tol = tol_for(c["method"], thermal)
    for k, ref in enumerate(refs):
        before = _state(b)
        o = _outs(b, b.step_wave(_dev(p["acts"][k].T), _wave(p["cur"][k], p["fld"][k])))
        e_ref = wcc.pulse_energy(p, k, before["m"].cpu().numpy().T)
        if k == 0:
            assert np.all(np.abs(e_ref - ref["energy"]) <= 1e-14 * np.abs(ref["energy"]))       # (the reset normalises the given rows once more)
        _compare_step(o, _state(b), ref, n, tol, f"step sweep {name}, step {k}", e_ref=e_ref, etot_ref=before["total_energy"].cpu().numpy() + e_ref)
    assert b.counters() == {"env_steps": wcc.STEPS * n, "work_units": int(sum(r["n_sub"].sum() for r in refs)), "noop_steps": 0}
    b.close()


# ------------------------------------------------------------------------------------------------
# stg_step_shaped, stg_step_shaped_ids
# ------------------------------------------------------------------------------------------------
K_SHAPED = wcc.K_SHAPED
_shaped_setup = wcc.shaped_problem


def _wave_tables(b, a, shape, fk):
    """the `wave` of HipBackend.step_wave for actions a [2,N] on the device, built as SpinTorqueVecEnv.step builds it"""
    from spin_torque_gym_amd import envs
    J, T = envs.parse_actions_fp64(a, b.cfg.max_current, b.cfg.max_duration)
    th, hk = _dev(fk[0]), _dev(fk[1])
    return {"current": envs.pulse_tables(shape, J, T), "field": (th[:, None].expand(-1, b.n).contiguous(), hk[:, :, None].expand(-1, -1, b.n).contiguous())}


SHAPED = [(s, f, lay) for s, f in [(s, f) for s in ("rk4", "euler", "rk45") for f in (None, "white")] + [("rk4", "ou"), ("euler", "ou")]
          for lay in ("soa", "records")]


@pytest.mark.parametrize("solver,noise,layout", SHAPED)
def test_shaped_entries_are_k_calls_of_step_wave_bit_for_bit(stg, solver, noise, layout):
    n, K = wcc.N, K_SHAPED
    s = _shaped_setup(solver, noise, f64=layout == "records", seed=7000 + len(solver) + len(noise or ""))
    c = dict(method=solver, noise=noise, n=n)
    extra = dict(out_layout=layout)
    # the oracle of "bit for bit": K calls of stg_step_wave with the tables pulse_tables builds
    ref = _step_backend(stg, c, s, **extra)
    steps, states = [], []
    for k in range(K):
        a = _dev(s["acts"][k].T)
        steps.append(_outs(ref, ref.step_wave(a, _wave_tables(ref, a, s["shape"], s["fk"]))))
        states.append(_state(ref))
    cnt_ref = ref.counters()
    ref.close()
    assert all(bool((x["status"] == 0).all()) for x in steps) and cnt_ref["work_units"] > K * n
    # obs[6] is each class's own resistance form at the kernels' own rows
    m_after, o6 = states[0]["m"].cpu().numpy().T, steps[0]["obs"][6].cpu().numpy()
    for ci, (d, t) in enumerate(zip(s["plist"], wcc.DEV_TYPES)):
        sel = s["cls"] == ci
        want = (wave_step_ref.resistance(m_after[sel], d, t) / d["resistance_parallel"]).astype(np.float32)
        assert np.all(np.abs(o6[sel] - want) <= wave_step_ref.F32_ULP * np.abs(want)), (t, np.abs(o6[sel] - want).max())
    acts = _dev(np.ascontiguousarray(s["acts"].transpose(0, 2, 1)))
    for every in (True, False):
        b = _step_backend(stg, c, s, **extra)
        b.set_pulse_shape(s["shape"], s["fk"])
        res = b.step_shaped_many(acts, out_every=every)
        torch.cuda.synchronize()
        f = {key: v.clone() for key, v in zip(OUT_NAMES, res)}
        f["energy"] = b.energy_many.clone()
        assert f["obs"].shape[0] == (K if every else 1)
        for k in (range(K) if every else [K - 1]):
            for key in OUT_KEYS:
                _same(f[key][k if every else 0], steps[k][key], (solver, noise, layout, "out_every", every, "step", k, key))
        st = _state(b)
        for key in STATE_KEYS:
            _same(st[key], states[-1][key], (solver, noise, layout, "state", key))
        assert b.counters() == cnt_ref
        b.close()
    # stg_step_shaped_ids: 100 of the 130 envs in a permuted order take step 1 after a full step 0
    ids = np.random.default_rng(3).permutation(n)[:100]
    b = _step_backend(stg, c, s, **extra)
    b.set_pulse_shape(s["shape"], s["fk"])
    b.step_shaped_many(acts[:1])
    before = _state(b)
    out = b.step_shaped_ids(_dev(np.ascontiguousarray(s["acts"][1][ids].T)), _dev(ids))
    torch.cuda.synchronize()
    idt = _dev(ids)
    for key, name in (("obs", "obs"), ("reward", "reward"), ("reward_f64", "reward64"), ("terminated", "terminated"), ("truncated", "truncated"),
                      ("status", "status"), ("energy", "energy")):
        _same(out[name].contiguous(), steps[1][key][..., idt].contiguous(), (solver, noise, layout, "ids", key))
    after = _state(b)
    listed = torch.zeros(n, dtype=torch.bool, device="cuda")
    listed[idt] = True
    for key in STATE_KEYS:
        _same(after[key][..., listed], states[1][key][..., listed], (solver, noise, layout, "ids: listed envs", key))
        _same(after[key][..., ~listed], before[key][..., ~listed], (solver, noise, layout, "ids: unlisted envs", key))
    b.close()


@pytest.mark.parametrize("method,noise", wcc.SHAPED_DIRECT)
def test_shaped_launch_vs_restatement(stg, oracle_mod, method, noise):
    """so that the chain above does not only compare the project with itself: one K = 3 launch of stg_step_shaped against K steps of the
    restatement under the knots (tau_j T, J s_j).  A launch hands back the fp64 state of its last step only, so the start rows of step k
    -- the energy goes with their resistance -- come from a launch of the first k steps on a twin context: every step's energy and
    the final total_energy are held to 1e-13 at the kernels' own start rows."""
    n, K = wcc.N, K_SHAPED
    s, refs = wcc.shaped_ref(method, noise, oracle_mod)
    c = dict(method=method, noise=noise, n=n)
    cfg, thermal = s["cfg"], noise is not None
    acts = _dev(np.ascontiguousarray(s["acts"].transpose(0, 2, 1)))
    starts = []                                                  # the kernels' own state before step k
    for k in range(K):
        twin = _step_backend(stg, c, s)
        twin.set_pulse_shape(s["shape"], s["fk"])
        if k:
            twin.step_shaped_many(acts[:k], out_every=False)
        starts.append(_state(twin))
        twin.close()
    e_refs = [wcc.pulse_energy(s, k, starts[k]["m"].cpu().numpy().T) for k in range(K)]
    b = _step_backend(stg, c, s)
    b.set_pulse_shape(s["shape"], s["fk"])
    res = b.step_shaped_many(acts, out_every=True)
    torch.cuda.synchronize()
    f = {key: v.clone() for key, v in zip(OUT_NAMES, res)}
    f["energy"] = b.energy_many.clone()
    st = _state(b)
    tol = tol_for(method, thermal)
    assert np.all(np.abs(e_refs[0] - refs[0]["energy"]) <= 1e-14 * np.abs(refs[0]["energy"]))       # (the reset normalises the given rows once more)
    for k in range(K):
        o = {key: f[key][k] for key in OUT_KEYS}
        e = o["energy"].cpu().numpy()
        assert np.all(np.abs(e - e_refs[k]) <= 1e-13 * np.abs(e_refs[k])), k
        for key in ("terminated", "truncated"):
            assert np.array_equal(o[key].cpu().numpy().astype(bool), refs[k][key]), (k, key)
        assert np.array_equal(o["status"].cpu().numpy(), refs[k]["status"])
        ob, ob_ref = o["obs"].cpu().numpy().T, refs[k]["obs"]
        assert np.all(np.abs(ob - ob_ref) <= wave_step_ref.F32_ULP * np.abs(ob_ref) + 2 * tol), k
        assert np.all(np.abs(o["reward_f64"].cpu().numpy() - refs[k]["reward"]) <= 1e-9 + 2 * tol), k
    _compare_step({key: f[key][K - 1] for key in OUT_KEYS}, st, refs[-1], n, tol, f"shaped launch {method} {noise}, last step", e_ref=e_refs[K - 1],
                  etot_ref=starts[K - 1]["total_energy"].cpu().numpy() + e_refs[K - 1])
    assert b.counters()["work_units"] == int(sum(r["n_sub"].sum() for r in refs))
    b.close()


# ------------------------------------------------------------------------------------------------
# RK45 max_attempts
# ------------------------------------------------------------------------------------------------
def test_rk45_attempt_budget_below_what_the_solve_needs(stg, golden):
    """A budget below the attempts the reference needed (G24 row 0: RK45 at rtol 1e-4, a trapezoid current and a ramped field): the solve
    fails -- success 0, m_final = m0, at most `budget` points -- and the env step is a no-op that keeps m.  Its energy is what the oracle
    charges for a failed solve (oracle/stg_oracle.c, env_step_parsed: the energy of the pulse is charged whether or not the solve
    succeeded, and the step counts), here the closed form of the current table."""
    g = golden("G24_wave_config")
    k = 0
    assert wcc.g24_solver(g, k) == "rk45" and not g["sv_thermal"][k] and g["sv_kj"][k] > 0
    budget = 100
    assert budget < int(g["sv_attempts"][k])
    p = stt_default_params(volume=float(g["sv_volume"][k]))
    cfg = dict(solver="rk45", include_thermal_fluctuations=False, rtol=float(g["sv_rtol"][k]), atol=float(g["sv_atol"][k]),
               max_step=float(g["sv_max_step"][k]), gamma=float(g["sv_gamma"][k]))
    cur, fld = wcc.g24_solve_knots(g, k)
    T = float(g["sv_T"][k])
    m0 = _dev(g["sv_m0"][k][:, None])
    for mx, want_ok in ((budget, False), (10 * int(g["sv_attempts"][k]), True)):
        b = _backend(stg, 1, [p], max_attempts=mx, **cfg)
        out = b.solve(m0, None, torch.tensor([T], dtype=F64), wave=_wave(cur, fld))
        torch.cuda.synchronize()
        assert bool(out["success"][0]) == want_ok, mx
        if want_ok:
            assert int(out["n_points"][0]) == int(g["sv_n_points"][k])
        else:
            assert int(out["n_points"][0]) <= budget
            _same(out["m_final"], m0, "m_final of a solve that ran out of attempts")
        # the env step with the same tables: the duration as a float64 action
        tgt = np.array([[0.0, 0.0, -1.0]])
        b.reset(init_m=m0, target=_dev(tgt.T))
        start = _state(b)
        act = np.array([[1e6, T]], dtype=np.float64)
        o = _outs(b, b.step_wave(_dev(act.T), _wave(cur, fld)))
        st = _state(b)
        m_before = start["m"].cpu().numpy().T
        r = wave_step_ref.resistance(m_before, p)
        ra = r * p["area"]
        e_ref = (ra * ra) / r * wave_step_ref.pulse_sq_integral(cur[0], cur[1], [T])
        assert e_ref[0] > 0
        assert abs(float(o["energy"][0]) - e_ref[0]) <= 1e-13 * e_ref[0], (mx, float(o["energy"][0]), e_ref[0])
        assert abs(float(st["total_energy"][0]) - e_ref[0]) <= 1e-13 * e_ref[0] and int(st["step_count"][0]) == 1 and int(st["rng_step"][0]) == 1
        if want_ok:
            assert int(o["status"][0]) == 0 and float((st["m"] - start["m"]).abs().max()) > 1e-3
        else:
            assert int(o["status"][0]) == STATUS_NOOP
            _same(st["m"], start["m"], "m of a step whose solve ran out of attempts")
            assert b.counters()["noop_steps"] == 1
        b.close()

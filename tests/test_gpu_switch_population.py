"""stg_switch_population -- stg_switch_times over a population of devices drawn per trial (include/spintorque_hip.h) -- held to EXACT
equality with existing code: `pytest -m gpu`.

  6. the draws: stg_switch_population_devices against the NumPy formula on the normals stg_thermal_normals dumps, bit for bit;
  7. their moments over 65 536 devices;
  8. sigma = 0 is stg_switch_times, integer for integer, all six outputs;
  9. a population of 64 devices against the UNCHANGED stg_solve / stg_solve_wave on a 64-row class table that holds the dumped devices,
     integer for integer, per-device counts included; once with lanes that loop;
 10. against the CPU oracle, which is handed the dumped devices as a class table;
 11. shapes and additivity; 12. a bad sigma column; 13. write footprint and refusals; 14. the public method.

Every test fails without the feature: the library has neither symbol."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import switch_population_ref as spr
import switch_stats_ref as ssr
import switch_stats_wave_ref as swr
import switch_times_ref as stref
from helpers import Guarded
from switch_stats_ref import G, SEED

pytestmark = pytest.mark.gpu

VS = spr.VAR_STEP
NAMES = ("n_switched", "n_failed", "hist", "n_crossed", "n_returned", "t_hist")
FORMS = (("rk4", "white"), ("rk4", "ou"), ("rk4", "brown"), ("euler", "white"), ("euler", "ou"), ("euler", "brown"), ("rk45", "white"))
SIGMA3 = np.array([[0.05, 0.10, 0.15], [0.02, 0.04, 0.06], [0.07, 0.03, 0.11], [0.20, 0.12, 0.08], [0.01, 0.09, 0.13]])       # [5, G]


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _same(got, want, what=None, names=NAMES):
    assert len(got) == len(want)
    for name, x, y in zip(names, got, want):
        assert (x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)), (what, name, x, y)


def _pulse(solver, g=G):
    m0, J, T, tgt = ssr.conditions()
    if solver == "rk45":
        J = J * ssr.RK45_J_SCALE
    return m0[:g], J[:g], T[:g], tgt[:g]


def _devices(b, g, d, sigma, **kw):
    out = b.switch_population_devices(g, d, torch.from_numpy(np.ascontiguousarray(sigma)), **kw)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out) if isinstance(out, tuple) else out.cpu().numpy()


# ------------------------------------------------------------------------------------------------
# 6. the draws
# ------------------------------------------------------------------------------------------------
def _stream_normals(stg, env_ids, var_step):
    """z [6, G, D]: calls 0 and 1 of stg_thermal_normals at counter word var_step for the env ids [G, D], one context per condition whose
    envs cover that condition's ids"""
    z = np.zeros((6,) + env_ids.shape)
    for g, ids in enumerate(env_ids):
        lo, n = int(ids.min()), int(ids.max() - ids.min()) + 1
        b = ssr.backend(stg, "rk4", "brown", n, env_id0=lo)
        zz = b.thermal_normals(var_step, 0, 2)
        torch.cuda.synchronize()
        z[:, g] = zz.cpu().numpy().reshape(6, n)[:, ids - lo]
        b.close()
    return z


@pytest.mark.parametrize("env_id0,dev0,Q,stride", ((0, 0, 3, 200), (37, 0, 3, 200), (37, 5, 1, 100), (11, 2 ** 33 + 5, 2, 2 ** 35)),
                         ids=("plain", "env_id0-37", "dev0-5", "device-beyond-2^33"))
def test_draws_equal_the_formula_on_the_streams_normals(stg, env_id0, dev0, Q, stride):
    D, clip, step = 64, 1.5, 12345
    b = ssr.backend(stg, "rk4", "brown", G, env_id0=env_id0)
    params, z = _devices(b, G, D, SIGMA3, dev0=dev0, trials_per_device=Q, trial_stride=stride, var_step=step, z_clip=clip, want_z=True)
    only = _devices(b, G, D, SIGMA3, dev0=dev0, trials_per_device=Q, trial_stride=stride, var_step=step, z_clip=clip)      # z = NULL
    b.close()
    ids = np.array([[spr.device_env(env_id0, g, stride, dev0 + j, Q) for j in range(D)] for g in range(G)], dtype=np.int64)
    assert ids.max() > 2 ** 33 or dev0 < 2 ** 33
    zs = _stream_normals(stg, ids, step)
    assert np.array_equal(z.view(np.uint64), zs.view(np.uint64))
    nominal = spr.nominal_values(ssr.flat_tables(stg)[0])
    want = spr.population(nominal, SIGMA3, zs, clip)
    assert np.array_equal(params.view(np.uint64), want.view(np.uint64)) and np.array_equal(only.view(np.uint64), want.view(np.uint64))
    # clipping occurred, on both sides, and the clipped devices sit on the bound
    assert (zs[:5] > clip).any() and (zs[:5] < -clip).any()
    hi = zs[:5] > clip
    assert np.array_equal(params[hi], np.broadcast_to((nominal[:, None] * (1.0 + SIGMA3 * clip))[:, :, None], params.shape)[hi])
    # another counter word, other devices
    b = ssr.backend(stg, "rk4", "brown", G, env_id0=env_id0)
    other = _devices(b, G, D, SIGMA3, dev0=dev0, trials_per_device=Q, trial_stride=stride, var_step=step + 1, z_clip=clip)
    b.close()
    assert not np.array_equal(other, params)


def test_devices_follow_the_conditions_class(stg):
    import brown_ref as br
    v = br.SWITCH["volume"]
    tables = [ssr.params(), ssr.params(0.7 * v), ssr.params(1.3 * v)]
    b = ssr.backend(stg, "rk4", "brown", G, tables, np.zeros(G, dtype=np.uint8))
    kw = dict(trial_stride=100, z_clip=4.0)
    base = _devices(b, G, 8, SIGMA3, **kw)
    got = _devices(b, G, 8, SIGMA3, cond_cls=torch.tensor([2, 0, 200], dtype=torch.uint8), **kw)                  # byte 200 reads class 0
    b.close()
    assert np.array_equal(got[:, 1:], base[:, 1:]) and np.array_equal(np.delete(got[:, 0], 3, axis=0), np.delete(base[:, 0], 3, axis=0))
    nom = [spr.nominal_values(r) for r in ssr.flat_tables(stg, tables)]
    sig = np.ascontiguousarray(SIGMA3)
    b = ssr.backend(stg, "rk4", "brown", G, tables, np.zeros(G, dtype=np.uint8))
    _, z = _devices(b, G, 8, sig, want_z=True, **kw)
    b.close()
    assert np.array_equal(got[3, 0], spr.vary_value(nom[2][3], sig[3, 0], z[3, 0], 4.0))      # class 2's volume, scattered
    assert nom[2][3] != nom[0][3]


# ------------------------------------------------------------------------------------------------
# 7. moments
# ------------------------------------------------------------------------------------------------
def test_moments_of_65536_devices(stg):
    D, s, c = 65536, 0.1, 4.0
    b = ssr.backend(stg, "rk4", "brown", 1)
    params = _devices(b, 1, D, np.full((5, 1), s), z_clip=c)[:, 0]
    b.close()
    nominal = spr.nominal_values(ssr.flat_tables(stg)[0])
    rel = params / nominal[:, None] - 1.0
    phi, Phi = math.exp(-0.5 * c * c) / math.sqrt(2 * math.pi), 0.5 * (1.0 + math.erf(c / math.sqrt(2.0)))
    sd = s * math.sqrt(1.0 - 2.0 * c * phi / (2.0 * Phi - 1.0))                    # the truncated normal's standard deviation
    for k, name in enumerate(spr.FIELDS):
        mean, std = rel[k].mean(), rel[k].std(ddof=1)
        print(f"{name}: mean {mean:+.2e} (bound {5 * s / math.sqrt(D):.2e}), std {std:.6f} (truncated normal {sd:.6f}, 5 standard errors {5 * sd / math.sqrt(2 * D):.2e})")
        assert abs(mean) < 5 * s / math.sqrt(D)
        assert abs(std - sd) < 5 * sd / math.sqrt(2 * D)                           # standard error of a standard deviation: sd / sqrt(2 D)
    corr = np.corrcoef(rel)
    assert np.abs(corr - np.eye(5)).max() < 0.02, corr


# ------------------------------------------------------------------------------------------------
# 8. sigma = 0 is the old kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", (192, 100))
@pytest.mark.parametrize("solver,noise", FORMS)
def test_sigma_zero_is_stg_switch_times(stg, solver, noise, R):
    m0, J, T, tgt = _pulse(solver)
    b = ssr.backend(stg, solver, noise, G)
    zero = np.zeros((5, G))
    for cur, fld in ((None, None), swr.knot_sets()["kj5-kh2"]):
        if solver == "rk45" and cur is not None:
            cur = (cur[0], cur[1] * ssr.RK45_J_SCALE)
        for n_tbins in (0, 16):
            kw = dict(n_bins=7, n_tbins=n_tbins, env_step=2)
            want = stref.fused(b, m0, J[None], T[None], tgt, R, 0, cur, fld, **kw)
            got, dev = spr.fused(b, m0, J[None], T[None], tgt, R, zero, cur, fld, dev_stride=R // 5 + 1, trials_per_device=5, passage=True, **kw)
            _same(got, want, (solver, noise, R, cur is not None, n_tbins))
            assert np.array_equal(dev.sum(axis=1), got[0])
            # without the first-passage counts: the three outputs of stg_switch_stats(_wave)
            got3, _ = spr.fused(b, m0, J[None], T[None], tgt, R, zero, cur, fld, n_bins=7, env_step=2)
            _same(got3, want[:3], (solver, noise, R, "three"))
    b.close()
    assert want[0].any() or solver == "rk45"


# ------------------------------------------------------------------------------------------------
# 9. exact, against the unchanged stg_solve / stg_solve_wave
# ------------------------------------------------------------------------------------------------
G2 = 2
SIGMA2 = SIGMA3[:, :G2] * 0.5


def _exact(stg, solver, noise, P, tabled=False, R=96, Q=3, D=32, T_all=None, n_tbins=0, **cfg):
    m0, Jp, Tp, tgt = _pulse(solver, G2)
    if T_all is not None:
        Tp = np.full(G2, T_all)
    J, T, wp = Jp[None], Tp[None], 0
    if P == 3:
        J, T, wp = np.stack([np.zeros(G2), Jp, np.zeros(G2)]), np.stack([np.full(G2, 3e-11), Tp, np.full(G2, 2e-11)]), 1
    cur = fld = None
    if tabled:
        c, f = swr.knot_sets()["kj5-kh2"]
        cur, fld = (c[0][:, :G2], c[1][:, :G2] * (ssr.RK45_J_SCALE if solver == "rk45" else 1.0)), (f[0][:, :G2], f[1][:, :G2])
    clip = 2.0
    b = ssr.backend(stg, solver, noise, G2, **cfg)
    params = _devices(b, G2, D, SIGMA2, trials_per_device=Q, trial_stride=R, z_clip=clip)
    got, dev = spr.fused(b, m0, J, T, tgt, R, SIGMA2, cur, fld, dev_stride=D, trials_per_device=Q, z_clip=clip, watch_phase=wp, n_bins=7, env_step=3,
                         n_tbins=n_tbins)
    b.close()
    assert (params > 0).all() and len(np.unique(params[3])) == G2 * D
    recs, _ = spr.table_of(stg, params)
    cls, dev_of_trial = spr.trial_classes(G2, R, Q, D)
    assert len(recs) == 64 and dev_of_trial.max() == D - 1
    m, failed = spr.host_path(stg, solver, noise, m0, J, T, R, recs, cls, env_step=3, cur=cur, fld=fld, wave_phase=wp, **cfg)
    want = ssr.host_counts(m, failed, tgt, R, n_bins=7)
    what = (solver, noise, P, tabled, cfg)
    _same(got[:3], want, what)
    assert np.array_equal(dev, spr.device_counts(m, failed, tgt, R, dev_of_trial, D)), what
    assert np.array_equal(dev.sum(axis=1), got[0])
    # the population matters: the nominal device's counts differ in the histogram
    b = ssr.backend(stg, solver, noise, G2, **cfg)
    nominal = ssr.fused(b, m0, J, T, tgt, R, n_bins=7, env_step=3) if not tabled else swr.fused(b, m0, J, T, tgt, R, cur, fld, wave_phase=wp, n_bins=7, env_step=3)
    b.close()
    return got, dev, nominal


@pytest.mark.parametrize("P,tabled", ((1, False), (3, False), (1, True)), ids=("P1", "P3", "tabled"))
@pytest.mark.parametrize("solver,noise", (("rk4", "brown"), ("euler", "ou"), ("rk45", "white")))
def test_population_equals_the_class_table_path(stg, solver, noise, P, tabled):
    got, dev, nominal = _exact(stg, solver, noise, P, tabled)
    print(f"{solver} {noise} P = {P} tabled {tabled}: switched {got[0].tolist()} (nominal device {nominal[0].tolist()}), failed {got[1].tolist()}, "
          f"devices by switched trials {np.bincount(dev.reshape(-1), minlength=4).tolist()}")
    assert not got[1].any() and (got[2].sum(axis=1) == 96).all()
    if noise == "brown":
        assert ((0 < got[0]) & (got[0] < 96)).all() and not np.array_equal(got[2], nominal[2])


def test_population_equals_the_class_table_path_without_the_thermal_field(stg):
    """no thermal field: the three trials of a device are one solve, so a device switches in all of them or in none"""
    got, dev, _ = _exact(stg, "rk4", "white", 1, include_thermal_fluctuations=False)
    assert set(dev.reshape(-1).tolist()) <= {0, 3} and not got[1].any()


def test_population_equals_the_class_table_path_with_time_bins(stg):
    """the watched phase runs on the device's row too: the first-passage counts of the population differ from the nominal device's, and
    every crossing is binned"""
    got, dev, _ = _exact(stg, "rk4", "brown", 3, n_tbins=16)
    assert np.array_equal(got[5].sum(axis=1), got[3]) and (got[3] >= got[0] - got[4]).all() and got[3].any()


def test_population_equals_the_class_table_path_when_lanes_loop(stg):
    """G = 2, Q = 12 290, 32 devices per condition: R = 393 280 needs 6145 wavefronts per condition at one trial per lane, one more than
    the launch rule allows, so every lane runs two trials (L = 2) and a lane's second trial is another device's than its first for
    the lanes of the wavefronts that straddle a device boundary; 20 ps pulses"""
    Q, D = 12290, 32
    R = Q * D
    assert -(-R // 64) == ssr.plan_cap(G2) + 1
    got, dev, _ = _exact(stg, "rk4", "brown", 1, R=R, Q=Q, D=D, T_all=2e-11)
    assert (dev <= Q).all() and len(np.unique(dev)) > 32 and not got[1].any()


# ------------------------------------------------------------------------------------------------
# 10. against the CPU oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise,P", spr.ORACLE_CASES)
def test_population_equals_the_oracle_on_the_dumped_devices(stg, oracle_mod, solver, noise, P):
    m0, _, _, tgt = ssr.conditions()
    cfg = ssr.settings_cfg(None, noise)
    R, Q, D = spr.ORACLE_R, spr.ORACLE_Q, spr.ORACLE_D
    b = ssr.backend(stg, solver, noise, G, **cfg)
    params = _devices(b, G, D, spr.ORACLE_SIGMA, trials_per_device=Q, trial_stride=R, z_clip=spr.ORACLE_CLIP)
    case = spr.oracle_case(stg, solver, noise, P, params)
    got, dev = spr.fused(b, m0, case["J"], case["T"], tgt, R, spr.ORACLE_SIGMA, dev_stride=D, trials_per_device=Q, z_clip=spr.ORACLE_CLIP,
                         n_bins=ssr.ORACLE_BINS, env_step=ssr.ORACLE_ENV_STEP)
    b.close()
    print(f"{solver} {noise} P = {P}: switched {got[0].tolist()} (oracle {case['counts'][0].tolist()}), distance to a decision {case['distance']:.2e}")
    spr.check_conditioned(case, solver, noise, P)                                  # on THESE devices; a case that is not conditioned fails
    # the GPU's devices are the CPU statement's to 2e-5 per normal
    cpu = spr.population(spr.nominal_values(ssr.flat_tables(stg)[0]), spr.ORACLE_SIGMA,
                         spr.oracle_normals(oracle_mod, SEED, G, D, Q, R), spr.ORACLE_CLIP)
    s_max = spr.ORACLE_SIGMA.max()
    assert np.abs(params / cpu - 1.0).max() < 2e-5 * s_max / (1.0 - s_max * spr.ORACLE_CLIP)      # |d value / value| <= sigma |dz| / (1 - sigma clip)
    _same(got, case["counts"], (solver, noise, P))
    assert np.array_equal(dev, case["dev_switched"])


# ------------------------------------------------------------------------------------------------
# 11. shapes and additivity
# ------------------------------------------------------------------------------------------------
def _args(m0, J, T, tgt):
    return (torch.from_numpy(m0.T.copy()), torch.from_numpy(np.ascontiguousarray(J)), torch.from_numpy(np.ascontiguousarray(T)),
            torch.from_numpy(tgt.T.copy()))


def test_lanes_that_loop_add_up_to_two_calls(stg):
    """G = 4097: 2 wavefronts per condition, so R = 256 runs two trials per lane and R = 128 one; the same dev_switched array takes both
    halves by absolute device id (Q = 100: devices straddle wavefronts and the two calls)"""
    big, R, Q = 4097, 256, 100
    assert ssr.plan_cap(big) == 2
    m3, J3, T3, t3 = ssr.conditions()
    idx = np.arange(big) % G
    m0, T, tgt = m3[idx], T3[idx][None].copy(), t3[idx]
    J = (J3[idx] * (0.8 + 0.4 * np.arange(big) / big))[None]
    sigma = np.ascontiguousarray(SIGMA3[:, idx] * 0.5)
    b = ssr.backend(stg, "rk4", "brown", big)
    kw = dict(n_bins=7, n_tbins=10, env_step=3, trials_per_device=Q, z_clip=2.0)
    whole, dev_whole = spr.fused(b, m0, J, T, tgt, R, sigma, dev_stride=3, **kw)
    dev = torch.zeros((big, 3), dtype=torch.int64, device="cuda")
    out = None
    for t0 in (0, 128):
        out = b.switch_population(*_args(m0, J, T, tgt), 128, torch.from_numpy(sigma), trial0=t0, trial_stride=R, dev_switched=dev, out=out, **kw)
    torch.cuda.synchronize()
    b.close()
    _same(whole, [x.cpu().numpy() for x in out])
    assert np.array_equal(dev.cpu().numpy(), dev_whole) and np.array_equal(dev_whole.sum(axis=1), whole[0])
    assert (whole[2].sum(axis=1) == R).all() and ((0 < whole[0]) & (whole[0] < R)).sum() > big // 2 and dev_whole[:, 2].any()


@pytest.mark.parametrize("Q,trial0", ((1, 0), (64, 0), (100, 0), (4, 10)))
def test_device_counts_for_every_q_and_prefilled_arrays(stg, Q, trial0):
    """Q = 1 (every lane its own device), Q = 64 (a wavefront is a device: one atomic per round), Q = 100 (devices straddle wavefronts),
    trial0 = 10 with Q = 4 (the first device partial): per-device counts against two half calls, prefilled arrays added to"""
    m0, J, T, tgt = _pulse("rk4")
    R = 200
    stride = trial0 + R
    n_dev = (trial0 + R + Q - 1) // Q
    b = ssr.backend(stg, "rk4", "brown", G)
    kw = dict(n_bins=7, n_tbins=8, env_step=1, trials_per_device=Q, z_clip=3.0, trial_stride=stride)
    fresh, dev = spr.fused(b, m0, J[None], T[None], tgt, R, SIGMA3, dev_stride=n_dev, trial0=trial0, **kw)
    first, last = spr.touched(trial0, R, Q)
    assert np.array_equal(dev.sum(axis=1), fresh[0]) and not dev[:, :first].any() and last == n_dev - 1
    assert (dev <= Q).all() and fresh[0].all() and (fresh[2].sum(axis=1) == R).all()
    # prefilled: every output and the device counts are added to; two halves by trial0
    rng = np.random.default_rng(5)
    pre = [rng.integers(1, 2 ** 40, s) for s in ((G,), (G,), (G, 7), (G,), (G,), (G, 8))]
    pre_dev = rng.integers(1, 2 ** 40, (G, n_dev))
    out, dsw = tuple(torch.from_numpy(p.copy()).cuda() for p in pre), torch.from_numpy(pre_dev.copy()).cuda()
    for t0, n in ((trial0, 90), (trial0 + 90, R - 90)):
        b.switch_population(*_args(m0, J[None], T[None], tgt), n, torch.from_numpy(SIGMA3), trial0=t0, dev_switched=dsw, out=out, **kw)
    torch.cuda.synchronize()
    b.close()
    _same([x.cpu().numpy() - p for x, p in zip(out, pre)], fresh, Q)
    assert np.array_equal(dsw.cpu().numpy() - pre_dev, dev)


# ------------------------------------------------------------------------------------------------
# 12. a bad sigma column
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", (-0.05, float("nan"), float("inf"), 0.25), ids=("negative", "nan", "inf", "sigma-clip-1"))
@pytest.mark.parametrize("solver,noise", (("rk4", "brown"), ("rk45", "white")))
def test_bad_sigma_column_fails_its_condition_alone(stg, solver, noise, bad):
    m0, Jp, Tp, tgt = _pulse(solver)
    J, T = np.stack([np.zeros(G), Jp]), np.stack([np.array([3e-11, 0.0, 3e-11]), Tp])      # (condition 1's first phase is skipped)
    R, clip, thr = 100, 4.0, -0.5                                                  # m0 . target = -0.1 ... -0.3 > thr: m0 is "switched" and would cross at row 0
    sigma = SIGMA3 * 0.5
    worse = sigma.copy()
    worse[3, 1] = bad
    assert not spr.column_ok(worse[:, 1], clip) and spr.column_ok(worse[:, 0], clip)
    b = ssr.backend(stg, solver, noise, G)
    kw = dict(trials_per_device=4, z_clip=clip, watch_phase=1, n_bins=8, n_tbins=16, threshold=thr, env_step=2, dev_stride=25)
    good, dev_good = spr.fused(b, m0, J, T, tgt, R, sigma, **kw)
    got, dev = spr.fused(b, m0, J, T, tgt, R, worse, **kw)
    params = _devices(b, G, 25, worse, trials_per_device=4, trial_stride=R, z_clip=clip)
    params_good = _devices(b, G, 25, sigma, trials_per_device=4, trial_stride=R, z_clip=clip)
    b.close()
    # the condition: every trial failed, is classified at m0 (proj = -0.2: switched for this threshold, bin floor(0.8 * 4) = 3), never crossed
    assert got[1][1] == R and got[0][1] == R and got[2][1].tolist() == [0, 0, 0, R, 0, 0, 0, 0]
    assert got[3][1] == 0 and got[4][1] == 0 and not got[5][1].any() and dev[1].tolist() == [4] * 25
    assert np.isnan(params[:, 1]).all()
    # the neighbours: unchanged against the run without the bad column
    for x, y in zip(got, good):
        assert np.array_equal(x[[0, 2]], y[[0, 2]])
    assert np.array_equal(dev[[0, 2]], dev_good[[0, 2]]) and np.array_equal(params[:, [0, 2]], params_good[:, [0, 2]])
    assert not good[1].any() and good[3].all()


# ------------------------------------------------------------------------------------------------
# 13. write footprint and refusals
# ------------------------------------------------------------------------------------------------
def _raw_call(lib, b, arrays, g=G, R=100, trial0=0, stride=None, P=1, watch_phase=0, kj=5, kh=2, n_bins=7, n_tbins=16, env_step=0, z_clip=3.0, var_step=VS,
              Q=4, dev_stride=None, null=()):
    """stg_switch_population through ctypes with Guarded outputs; `null`: names of pointer arguments passed as NULL"""
    ptr = lambda name: None if name in null else C.c_void_p(arrays[name].data_ptr())            # noqa: E731
    stride = trial0 + R if stride is None else stride
    dev_stride = arrays["dev_switched"].shape[1] if dev_stride is None else dev_stride
    return lib.stg_switch_population(None if "ctx" in null else b._ctx, g, R, trial0, stride, P, ptr("m0"), ptr("J"), ptr("T"), watch_phase,
                                     kj, ptr("tj"), ptr("jk"), kh, ptr("th"), ptr("hk"), ptr("cls"), env_step, ptr("target"), 0.0, n_bins,
                                     ptr("n_switched"), ptr("n_failed"), ptr("hist"), n_tbins, ptr("n_crossed"), ptr("n_returned"), ptr("t_hist"),
                                     ptr("sigma"), z_clip, var_step, Q, ptr("dev_switched"), dev_stride, None)


def _guards(g, n_tbins=16, n_dev=30):
    return {"n_switched": Guarded("n_switched", (g,), torch.float64), "n_failed": Guarded("n_failed", (g,), torch.float64),
            "hist": Guarded("hist", (g, 7), torch.float64, n_axis=0), "n_crossed": Guarded("n_crossed", (g,), torch.float64),
            "n_returned": Guarded("n_returned", (g,), torch.float64), "t_hist": Guarded("t_hist", (g, n_tbins), torch.float64, n_axis=0),
            "dev_switched": Guarded("dev_switched", (g, n_dev), torch.float64, n_axis=0)}


def test_write_footprint_and_refusals(stg):
    from spin_torque_gym_amd import _lib
    lib = _lib.load()
    m0, J, T, tgt = ssr.conditions()
    cur, fld = swr.knot_sets()["kj5-kh2"]
    R = 100
    b = ssr.backend(stg, "rk4", "brown", G)
    guards = _guards(G)
    wave = swr.wave_dict(cur, fld)
    sigma = SIGMA3 * 0.5
    arrays = dict(m0=torch.from_numpy(m0.T.copy()).cuda(), J=torch.from_numpy(np.stack([J, J])).cuda(), T=torch.from_numpy(np.stack([T, T])).cuda(),
                  target=torch.from_numpy(tgt.T.copy()).cuda(), cls=torch.zeros(G, dtype=torch.uint8, device="cuda"),
                  tj=wave["current"][0].cuda(), jk=wave["current"][1].cuda(), th=wave["field"][0].cuda(), hk=wave["field"][1].cuda(),
                  sigma=torch.from_numpy(sigma.copy()).cuda(), **{k: v.interior for k, v in guards.items()})
    # every refusal: an error code, a message, nothing launched -- the arrays still hold their sentinels
    refusals = [dict(null=(name,)) for name in ("ctx", "m0", "T", "target", "n_switched", "n_failed", "hist", "tj", "jk", "th", "hk", "n_crossed",
                                                "n_returned", "t_hist", "sigma")]
    refusals += [dict(null=("n_crossed", "n_returned")),                            # both NULL, but n_tbins > 0
                 dict(g=0), dict(R=-1), dict(P=0), dict(P=5), dict(n_bins=-1), dict(n_bins=65), dict(n_bins=0), dict(trial0=-1, stride=R),
                 dict(stride=R - 1), dict(trial0=10, stride=R + 9), dict(R=2 ** 62, trial0=2 ** 62, stride=2 ** 63 - 1), dict(stride=2 ** 62),
                 dict(watch_phase=-1), dict(watch_phase=1), dict(P=2, watch_phase=2), dict(kj=1), dict(kj=-2), dict(kj=33), dict(kh=1), dict(kh=-1),
                 dict(kh=33), dict(kj=0, null=("J",)), dict(P=2, null=("J",)), dict(n_tbins=-1), dict(n_tbins=1025), dict(n_tbins=0),
                 dict(z_clip=0.0), dict(z_clip=-1.0), dict(z_clip=float("inf")), dict(z_clip=float("nan")), dict(Q=0), dict(Q=-3),
                 dict(var_step=0), dict(var_step=5, env_step=5), dict(P=2, var_step=6, env_step=5), dict(P=2, var_step=0, env_step=2 ** 32 - 1),
                 dict(dev_stride=24), dict(trial0=4, stride=104, dev_stride=25), dict(Q=1, dev_stride=99), dict(dev_stride=-1),
                 dict(dev_stride=2 ** 62)]
    for kw in refusals:
        rc = _raw_call(lib, b, arrays, **kw)
        assert rc == _lib.STG_E_INVALID and lib.stg_last_error(), (kw, rc)
        torch.cuda.synchronize()
        for v in guards.values():
            v.check(written=False)
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    pe = HipBackend(G, EnvConfig(solver="rk4", include_thermal_fluctuations=True, noise_model="brown", seed=SEED))
    assert _raw_call(lib, pe, arrays) == _lib.STG_E_STATE                          # no parameters yet
    import spin_torque_gym_amd.devices as devices
    flat = stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", ssr.params()))
    block, dev_type, valid = devices.per_env_param_block(flat, G, {})
    pe.set_params_per_env(block, dev_type, valid)
    assert _raw_call(lib, pe, arrays) == _lib.STG_E_STATE and b"per-env" in lib.stg_last_error()
    out = torch.zeros((5, G, 4), dtype=torch.float64, device="cuda")
    devs = lambda ctx, **k: lib.stg_switch_population_devices(ctx, k.get("g", G), k.get("D", 4), k.get("dev0", 0), k.get("Q", 4), k.get("stride", 100), VS,        # noqa: E731
                                                              k.get("z_clip", 3.0), k.get("sigma", C.c_void_p(arrays["sigma"].data_ptr())), None,
                                                              k.get("params", C.c_void_p(out.data_ptr())), None, None)
    assert devs(pe._ctx) == _lib.STG_E_STATE
    pe.close()
    for k in (dict(g=0), dict(D=-1), dict(dev0=-1), dict(Q=0), dict(z_clip=0.0), dict(z_clip=float("nan")), dict(sigma=None), dict(params=None),
              dict(dev0=22), dict(D=26), dict(stride=2 ** 62)):
        assert devs(b._ctx, **k) == _lib.STG_E_INVALID and lib.stg_last_error(), k
    assert devs(None) == _lib.STG_E_INVALID and devs(b._ctx, D=0) == 0 and devs(b._ctx, dev0=21) == 0
    torch.cuda.synchronize()
    assert not out[:, :, :].isnan().any() and (out > 0).all()
    assert _raw_call(lib, b, arrays, R=0) == 0                                     # valid, does nothing
    torch.cuda.synchronize()
    for v in guards.values():
        v.check(written=False)
    # the real thing, at trial0 = 40 with Q = 4: devices 10 ... 34 of a 40-wide row.  The counts start from zero; dev_switched keeps its
    # sentinels, to which the kernel adds, so an element outside the stated range that was touched at all shows
    guards = _guards(G, n_dev=40)
    arrays.update({k: v.interior for k, v in guards.items()})
    for k, v in guards.items():
        if k != "dev_switched":
            v.bits().zero_()
    assert _raw_call(lib, b, arrays, trial0=40, null=("J",)) == 0, lib.stg_last_error()
    torch.cuda.synchronize()
    want, dev = spr.fused(b, m0, J[None], T[None], tgt, R, sigma, cur, fld, dev_stride=40, trials_per_device=4, z_clip=3.0, n_bins=7, n_tbins=16,
                          trial0=40)
    for (k, v), y in zip(guards.items(), want):
        v.check_guards()
        assert np.array_equal(v.bits().cpu().numpy(), y), k
    g = guards["dev_switched"]
    g.check_guards()
    assert spr.touched(40, R, 4) == (10, 34) and not dev[:, :10].any() and not dev[:, 35:].any() and dev.any()
    assert np.array_equal(g.bits().cpu().numpy() - g.sentinel, dev)
    assert g.untouched()[:, :10].all() and g.untouched()[:, 35:].all()
    # NULL first-passage arrays with n_tbins = 0, NULL dev_switched, NULL cond_cls, no tables: the three counts are added to, nothing else is touched
    before = {k: v.bits().clone() for k, v in guards.items()}
    rect, _ = spr.fused(b, m0, J[None], T[None], tgt, R, sigma, trials_per_device=4, z_clip=3.0, n_bins=7)
    assert _raw_call(lib, b, arrays, kj=0, kh=0, n_tbins=0, dev_stride=0,
                     null=("n_crossed", "n_returned", "t_hist", "dev_switched", "cls", "tj", "jk", "th", "hk")) == 0, lib.stg_last_error()
    torch.cuda.synchronize()
    for (k, v), y in zip(guards.items(), tuple(rect) + (None,) * 4):
        v.check_guards()
        assert np.array_equal((v.bits() - before[k]).cpu().numpy(), y if y is not None else np.zeros(v.shape, dtype=np.int64)), k
    b.close()


def test_write_footprint_when_lanes_loop(stg):
    """G = 4097, R = 256 (two trials per lane), Q = 100, 100 time bins: nothing beyond G, G, 7 G, G, G, 100 G and 3 G elements"""
    from spin_torque_gym_amd import _lib
    lib = _lib.load()
    big, R = 4097, 256
    m3, J3, T3, t3 = ssr.conditions()
    idx = np.arange(big) % G
    b = ssr.backend(stg, "rk4", "brown", big)
    guards = _guards(big, 100, n_dev=3)
    for v in guards.values():
        v.bits().zero_()
    arrays = dict(m0=torch.from_numpy(m3[idx].T.copy()).cuda(), J=torch.from_numpy(J3[idx].copy()).cuda(), T=torch.from_numpy(T3[idx].copy()).cuda(),
                  target=torch.from_numpy(t3[idx].T.copy()).cuda(), sigma=torch.from_numpy(np.ascontiguousarray(SIGMA3[:, idx] * 0.5)).cuda(),
                  **{k: v.interior for k, v in guards.items()})
    assert _raw_call(lib, b, arrays, g=big, R=R, kj=0, kh=0, n_tbins=100, Q=100, null=("cls", "tj", "jk", "th", "hk")) == 0, lib.stg_last_error()
    torch.cuda.synchronize()
    for v in guards.values():
        v.check_guards()
    got = {k: v.bits().cpu().numpy() for k, v in guards.items()}
    b.close()
    assert (got["hist"].sum(axis=1) == R).all() and np.array_equal(got["t_hist"].sum(axis=1), got["n_crossed"]) and got["n_crossed"][-1] > 0
    assert np.array_equal(got["dev_switched"].sum(axis=1), got["n_switched"]) and got["dev_switched"][-1].any() and got["dev_switched"][:, 2].max() <= 56


# ------------------------------------------------------------------------------------------------
# 14. the public method
# ------------------------------------------------------------------------------------------------
def test_public_api_per_device_counts_are_plain_calls_on_the_drawn_devices(stg):
    from spin_torque_gym_amd import physics
    m0, J, T, tgt = _pulse("rk4", G2)
    Q, D = 64, 8
    R = Q * D
    variation = {"volume": 0.1, "damping": 0.05}
    solver = physics.SimpleLLGSSolver(method="rk4", noise_model="brown", seed=SEED)
    res = solver.switching_statistics(m0, J, T, ssr.params(), R, n_bins=7, env_step=2, variation=variation, trials_per_device=Q, per_device=True)
    assert res["n_devices"].tolist() == [D] * G2 and res["dev_switched"].shape == (G2, D) and (res["dev_trials"] == Q).all()
    assert np.array_equal(res["dev_switched"].sum(axis=1), res["n_switched"]) and np.array_equal(res["dev_p_switch"], res["dev_switched"] / Q)
    chunked = solver.switching_statistics(m0, J, T, ssr.params(), R, n_bins=7, env_step=2, variation=variation, trials_per_device=Q, per_device=True,
                                          max_trials_per_launch=100)
    for k in res:
        assert np.array_equal(res[k], chunked[k]), k
    drawn = solver.draw_devices(ssr.params(), D, variation, n_conditions=G2, trials_per_device=Q)
    assert np.array_equal(drawn["saturation_magnetization"], np.full((G2, D), ssr.params()["saturation_magnetization"]))
    assert len(np.unique(drawn["volume"])) == G2 * D and len(np.unique(drawn["damping"])) == G2 * D
    assert np.array_equal(drawn["volume"], spr.vary_value(ssr.params()["volume"], 0.1, drawn["z"][3], 4.0))
    hist = np.zeros((G2, 7), dtype=np.int64)
    for d in range(D):
        for g in range(G2):
            # condition g alone would sit at env id 0: both conditions are run, with the same stride, and condition g's count is read
            one = solver.switching_statistics(m0, J, T, drawn["device_params"][g][d], Q, n_bins=7, env_step=2, trial_offset=Q * d, trial_stride=R)
            assert one["n_switched"][g] == res["dev_switched"][g, d], (g, d)
            hist[g] += one["hist"][g]
    assert np.array_equal(hist, res["hist"]) and ((0 < res["n_switched"]) & (res["n_switched"] < R)).all()
    # variation = None is today's call
    plain = solver.switching_statistics(m0, J, T, ssr.params(), R, n_bins=7, env_step=2)
    none = solver.switching_statistics(m0, J, T, ssr.params(), R, n_bins=7, env_step=2, variation=None, trials_per_device=Q, per_device=True)
    assert set(plain) == set(none) == {"p_switch", "wer", "n_switched", "n_failed", "stderr", "hist", "bin_edges"}
    for k in plain:
        assert np.array_equal(plain[k], none[k]), k
    assert not np.array_equal(plain["hist"], res["hist"])

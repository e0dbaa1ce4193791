"""stg_switch_population off its defaults and against references that are not the kernel: `pytest -m gpu`.
tests/test_gpu_switch_population.py holds the VARY instantiations of stg_switch_kernel to stg_solve on the three classification
outputs, at class 0, at the default configuration and at env_id0 = trial0 = 0.  Here every case compares ALL SIX outputs and
dev_switched, integer for integer, with switch_population_cases.population_host_path: one unchanged stg_solve / stg_solve_traj /
stg_solve_wave context per condition, created at the env id of the condition's first trial, whose class table holds that condition's
dumped devices; the watched phase's recorded rows go through switch_times_ref.first_passage.  The dump itself is asserted bit for bit
against the NumPy formula on stg_thermal_normals' values in every case that uses it.

  A. first passage of a varied population: (rk4, brown), (euler, ou), (rk45, white) x rectangular and the three knot sets x P = 1 and
     P = 3 watched first, middle, last, each with n_tbins 0, 16 and 100; a threshold m0 already exceeds; max_attempts = 3 on RK45;
  B. the nominal class: three classes that differ in volume AND in a field the draw leaves alone (easy axis / demagnetisation),
     cond_cls = [2, 0, 200], cond_cls = None, an invalid class as a condition's nominal record;
  C. configuration: the three (max_step, gamma, temperature) settings, gamma alone, temperature 0, the thermal field off -- every form;
  D. stream identity: env_id0, trial0 with a partial first device, trial_stride beyond trial0 + R and beyond 2^34, var_step, a phase
     counter that wraps;
  E. geometry with everything on: G = 4097, two trials per lane, tabled, 100 time bins, Q = 100;
  F. the CPU oracle off its defaults: four fixed-step forms x three settings at P = 3, RK45 at its own tolerances;
  G. the Python method.

The LLGS solver (rk45) has no parameter-validity gate (csrc/stg_kernels.hpp: only the fixed-step solvers read C_VALID), so in B an
invalid nominal class fails its condition under rk4 and is an ordinary device under rk45; both are what stg_solve does.
switching_statistics takes current_knots only with a single pulse ([G] or [1,G]; equilibrate / relax add the phases around it), so G
runs the [P,G] pulse with watch_phase = 1 rectangular and the tabled pulse behind an equilibration.

At threshold 0 the weak fields (ou, white) cross in all of a condition's trials or in none, which would not tell a device's row from
the nominal one: sections A and C put their threshold at the median, over condition 0's trials, of the largest projection the
reference reaches in the watched phase (48 of 96 trials cross, each device at its own time), and give RK45 -- which runs below its
current gate and relaxes towards +z -- the target +z.  Under brown the threshold is 0.

Measured on an MI355X: the 132 cases take 3.8 s in all (the slowest 0.2 s; an oracle case 0.03 - 0.12 s; G = 4097 with its 34 host
paths 0.07 s), and every one returned the reference's integers.  profiles/NOTEBOOK.md (round 25) has the smallest oracle distances
per form and the ten deliberate miscounts, each of which at least one case here catches."""
import numpy as np
import pytest
import torch

import switch_population_cases as spc
import switch_population_ref as spr
import switch_stats_ref as ssr
import switch_stats_wave_ref as swr
import switch_times_ref as stref
from switch_stats_ref import SEED
from test_gpu_switch_population import FORMS, SIGMA3
from test_gpu_switch_stats_config import RK45_CFG

pytestmark = pytest.mark.gpu

THREE = (("rk4", "brown"), ("euler", "ou"), ("rk45", "white"))
KNOT_SETS = (None, "kj5-kh2", "kj5-kh0", "kj0-kh2")
PLACES = ((1, 0), (3, 0), (3, 1), (3, 2))                  # (P, watched phase)
TBINS = (0, 16, 100)                                       # 100: lanes own two bins of t_hist


@pytest.fixture(scope="module")
def stg(oracle_mod):
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _pulse(solver, g):
    m0, J, T, tgt = ssr.conditions()
    if solver == "rk45":
        J = J * ssr.RK45_J_SCALE
    return m0[:g], J[:g], T[:g], tgt[:g]


def _case(stg, solver, noise, J, T, wp, g=2, R=96, Q=3, sigma=None, cur=None, fld=None, tbins=(16,), threshold=0.0, env_step=3, trial0=0,
          trial_stride=None, env_id0=0, var_step=spr.VAR_STEP, z_clip=2.0, tables=None, cond_cls=None, nominal_too=False, flip=False, what=None, **cfg):
    """One comparison.  The context under test (created at env_id0, with `tables` as its classes) dumps the devices of the trial
    range, which are checked against the stream; the reference runs on them; the fused call is made once per n_tbins of `tbins` and
    compared in all six outputs and dev_switched.  Returns dict(got: the last call's six, dev, ref, params, nominal: stg_switch_times
    on the same context and arguments, i.e. the nominal device's six)."""
    m0, _, _, tgt = ssr.conditions()
    m0, tgt = m0[:g], (-tgt[:g] if flip else tgt[:g])
    sigma = SIGMA3[:, :g] * 0.5 if sigma is None else sigma
    stride = trial0 + R if trial_stride is None else trial_stride
    _, dev0, n_dev = spc.trial_classes(R, Q, trial0)
    cc = None if cond_cls is None else np.asarray(cond_cls, dtype=np.uint8)
    b = ssr.backend(stg, solver, noise, g, tables, None if tables is None or len(tables) < 2 else np.zeros(g, dtype=np.uint8), env_id0=env_id0, **cfg)
    nominal = spc.nominal_records(stg, tables, cc, g)
    params = spc.checked_devices(stg, b, g, n_dev, sigma, Q, stride, nominal, dev0=dev0, var_step=var_step, z_clip=z_clip, cond_cls=cc, env_id0=env_id0)
    host = lambda thr: spc.population_host_path(stg, solver, noise, m0, J, T, tgt, R, Q, params, nominal=nominal, watch_phase=wp, cur=cur, fld=fld,       # noqa: E731
                                                threshold=thr, env_step=env_step, trial0=trial0, trial_stride=stride, env_id0=env_id0, **cfg)
    if threshold == "median-0":
        # the median of condition 0's final projections on the reference: half of its trials are switched, so any change of a trial's end shows
        threshold = float(np.median(ssr.proj(host(0.0)["m"], np.repeat(tgt, R, axis=0))[:R]))
    elif threshold == "median-peak-0":
        # the median, over condition 0's trials, of the largest projection a trial reaches in the watched phase after its row 0: half of them cross
        threshold = float(np.median(host(np.inf)["peak"][:R]))
    ref = host(threshold)
    kw = dict(trials_per_device=Q, z_clip=z_clip, var_step=var_step, watch_phase=wp, n_bins=7, env_step=env_step, threshold=threshold, trial0=trial0,
              trial_stride=stride, cond_cls=None if cc is None else torch.from_numpy(cc))
    got = dev = None
    for n_tbins in tbins:
        got, dev = spr.fused(b, m0, J, T, tgt, R, sigma, cur, fld, dev_stride=dev0 + n_dev, n_tbins=n_tbins, passage=True, **kw)
        want, want_dev = spc.reference_counts(ref, tgt, T[wp], R, dev0 + n_dev, threshold=threshold, n_bins=7, n_tbins=n_tbins)
        spc.same(got, want, (what, solver, noise, n_tbins))
        assert np.array_equal(dev, want_dev), (what, solver, noise, n_tbins, dev, want_dev)
        assert np.array_equal(dev.sum(axis=1), got[0]) and not dev[:, :dev0].any()
        assert (got[2].sum(axis=1) == R).all() and (got[5] is None or np.array_equal(got[5].sum(axis=1), got[3]))
    nom = None
    if nominal_too:
        kn = {k: kw[k] for k in ("n_bins", "env_step", "threshold", "trial0", "trial_stride", "cond_cls")}
        nom = stref.fused(b, m0, J, T, tgt, R, wp, cur, fld, n_tbins=tbins[-1], **kn)
    b.close()
    return dict(got=got, dev=dev, ref=ref, params=params, nominal=nom, threshold=threshold)


# ------------------------------------------------------------------------------------------------
# A. first passage of a varied population
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,wp", PLACES, ids=lambda v: str(v))
@pytest.mark.parametrize("knots", KNOT_SETS, ids=lambda v: str(v))
@pytest.mark.parametrize("solver,noise", THREE)
def test_first_passage_of_a_population_equals_the_host_path(stg, solver, noise, knots, P, wp):
    """n_crossed, n_returned and t_hist of a varied population -- the watched phase, rectangular or tabled, on each device's own row --
    against the rows stg_solve_traj / stg_solve_wave record for the dumped devices"""
    _, Jp, Tp, _ = _pulse(solver, 2)
    J, T = spc.chain(Jp, Tp, P, wp)
    cur, fld = spc.knots(knots, solver, 2)
    # Under brown the field decides at threshold 0.  The weak fields (ou, white) leave a device's trials next to each other, and at
    # threshold 0 a condition crosses in all trials or in none: there the threshold is put at the median of the largest projection
    # condition 0's trials reach in the watched phase, so that half of them cross, each device at its own time.  RK45 runs below its
    # current gate and relaxes towards +z: its target is +z, so that the projection rises.
    weak = noise != "brown"
    res = _case(stg, solver, noise, J, T, wp, cur=cur, fld=fld, tbins=TBINS, nominal_too=True, what=(knots, P, wp),
                threshold="median-peak-0" if weak else 0.0, flip=solver == "rk45")
    got, nom = res["got"], res["nominal"]
    print(f"{solver} {noise} {knots} P = {P} watched {wp} threshold {res['threshold']:.6g}: switched {got[0].tolist()}, crossed {got[3].tolist()} "
          f"(nominal device {nom[3].tolist()}), returned {got[4].tolist()}, failed {got[1].tolist()}, time bins in use {np.count_nonzero(got[5], axis=1).tolist()}")
    assert not got[1].any() and len(np.unique(res["params"][3])) == res["params"][3].size
    # the case tells the device's row from the nominal one: the nominal device crosses elsewhere
    assert got[3].any() and (not np.array_equal(got[3], nom[3]) or not np.array_equal(got[5], nom[5]))
    if weak:
        assert 0 < got[3][0] < 96


@pytest.mark.parametrize("solver,noise", THREE)
def test_a_threshold_m0_already_exceeds_crosses_at_row_zero(stg, solver, noise):
    """threshold -0.5 < m0 . target = -0.1, -0.2: every trial crosses at row 0 of the watched phase with t_x = 0.0 -- on P = 1, where the
    watched phase starts at m0 itself"""
    _, Jp, Tp, _ = _pulse(solver, 2)
    res = _case(stg, solver, noise, Jp[None], Tp[None], 0, tbins=(16,), threshold=-0.5)
    got = res["got"]
    assert not res["ref"]["t_x"].any() and res["ref"]["crossed"].all()
    assert got[3].tolist() == [96, 96] and got[5][:, 0].tolist() == [96, 96] and not got[5][:, 1:].any()


@pytest.mark.parametrize("max_attempts", (3, 19, 20))
def test_failed_watched_phases_discard_their_crossings_on_the_devices_own_row(stg, max_attempts):
    """RK45 short of attempts: a watched phase that runs out of them fails, and a trial that crossed in it (threshold -0.5: at row 0)
    has NOT crossed.  With 3 attempts every trial fails.  Measured: the 20 ps pulse of condition 0 takes exactly 20 attempts on every
    one of these devices (all 96 trials fail at 19, none at 20; the 60 ps pulse of condition 1 fails up to 40 and passes at 60), so
    19 and 20 hold the attempt count itself to stg_solve; no budget was found at which only some devices of a condition fail"""
    _, Jp, Tp, _ = _pulse("rk45", 2)
    res = _case(stg, "rk45", "white", Jp[None], Tp[None], 0, tbins=(0, 16), threshold=-0.5, max_attempts=max_attempts)
    got, ref = res["got"], res["ref"]
    print(f"rk45 max_attempts = {max_attempts}: failed {got[1].tolist()}, crossed {got[3].tolist()}, returned {got[4].tolist()}, "
          f"devices with 0 / 1 / 2 / 3 failed trials in condition 0 {np.bincount(np.bincount(ref['dev'], weights=ref['failed'][:96]).astype(int), minlength=4).tolist()}")
    # m0 lies beyond the threshold, so a trial has crossed exactly when its watched phase -- the only one -- did not fail
    assert got[1].any() and np.array_equal(got[3], 96 - got[1]) and not (ref["crossed"] & ref["failed"]).any()


# ------------------------------------------------------------------------------------------------
# B. the nominal class
# ------------------------------------------------------------------------------------------------
B_FORMS = (("rk4", "brown"), ("rk45", "white"))


def _class_case(stg, solver, noise, knots, tables, cond_cls, **kw):
    _, Jp, Tp, _ = _pulse(solver, 3)
    cur, fld = spc.knots(knots, solver, 3)
    return _case(stg, solver, noise, Jp[None], Tp[None], 0, g=3, sigma=SIGMA3 * 0.5, cur=cur, fld=fld, tbins=(16,), tables=tables, cond_cls=cond_cls,
                 what=(knots, cond_cls), **kw)


@pytest.mark.parametrize("cond_cls", ([2, 0, 200], None), ids=("cls-2-0-200", "cls-none"))
@pytest.mark.parametrize("knots", (None, "kj5-kh2"), ids=("rect", "tabled"))
@pytest.mark.parametrize("solver,noise", B_FORMS)
def test_the_nominal_record_is_the_conditions_class(stg, solver, noise, knots, cond_cls):
    """the whole record of class cond_cls[g] -- byte 200 and a NULL cond_cls read class 0 -- is what the draw scales and the trial
    integrates on: against the host path on that record, and NOT equal to the host path on class 0's record with the right class's
    five varied fields, nor to the one on class 0's record"""
    tables = spc.class_tables(solver)
    # (rk45's trials of a condition end 1e-6 apart, all in one bin and on one side of 0: the threshold is put among them)
    res = _class_case(stg, solver, noise, knots, tables, cond_cls, threshold="median-0" if solver == "rk45" else 0.0)
    got, thr = res["got"], res["threshold"]
    assert not got[1].any()
    if cond_cls is None:
        return
    # what two wrong kernels would count for condition 0 (class 2): the drawn five fields on class 0's other fields (`out = ptab[0]`
    # with the five scaled from the right class), and class 0's devices altogether (`ptab[0]`) -- the case must tell both from the truth
    m0, _, _, tgt = ssr.conditions()
    _, Jp, Tp, _ = _pulse(solver, 3)
    cur, fld = spc.knots(knots, solver, 3)
    flat = ssr.flat_tables(stg, tables)
    z = spc.stream_normals(stg, np.array([[spr.device_env(0, 0, 96, j, 3) for j in range(32)]], dtype=np.int64), spr.VAR_STEP)
    of_class_0 = res["params"].copy()
    of_class_0[:, :1] = spr.population(spr.nominal_values(flat[0]), SIGMA3[:, :1] * 0.5, z, 2.0)
    assert not np.array_equal(of_class_0[3, 0], res["params"][3, 0]) and np.array_equal(of_class_0[0, 0], res["params"][0, 0])      # volume differs, damping does not
    for nominal, params in (([spc.mixed_record(flat[2], flat[0])] * 3, res["params"]), ([flat[0]] * 3, of_class_0)):
        ref = spc.population_host_path(stg, solver, noise, m0, Jp[None], Tp[None], tgt, 96, 3, params, nominal=nominal, cur=cur, fld=fld, threshold=thr,
                                       env_step=3, conds=[0])
        wrong = spc.reference_counts(ref, tgt[:1], Tp[:1], 96, 32, threshold=thr, n_bins=7, n_tbins=16)[0]
        assert any(not np.array_equal(x[0], y[0]) for x, y in zip(got, wrong)), "the case does not tell the classes apart"


@pytest.mark.parametrize("knots", (None, "kj5-kh2"), ids=("rect", "tabled"))
@pytest.mark.parametrize("solver,noise", B_FORMS)
def test_an_invalid_nominal_class_fails_its_condition_alone(stg, solver, noise, knots):
    """condition 1's nominal record is a class whose parameter set is invalid.  Under rk4 every trial of it fails in its first phase,
    is classified at m0 (proj = -0.2 > threshold -0.5: switched, bin floor(0.8 * 3.5) = 2 of 7) and has not crossed although m0 lies
    beyond the threshold; under rk45, which has no validity gate, the record is a device like any other.  Either way the six outputs
    are the host path's, and the neighbours' are those of the run with a valid class in its place"""
    from conftest import sot_default_params
    invalid = stg.flatten_params(stg.DeviceFactory().create_device("sot_mram", sot_default_params()))
    assert invalid.params_valid == 0
    tables = spc.class_tables(solver)
    bad = _class_case(stg, solver, noise, knots, [tables[0], invalid, tables[2]], [0, 1, 2], threshold=-0.5)
    good = _class_case(stg, solver, noise, knots, tables, [0, 1, 2], threshold=-0.5)
    got, dev = bad["got"], bad["dev"]
    if solver != "rk45":
        assert got[1][1] == 96 and got[0][1] == 96 and got[2][1].tolist() == [0, 0, 96, 0, 0, 0, 0]
        assert got[3][1] == 0 and got[4][1] == 0 and not got[5][1].any() and dev[1].tolist() == [3] * 32
    for x, y in zip(got, good["got"]):
        assert np.array_equal(x[[0, 2]], y[[0, 2]])
    assert np.array_equal(dev[[0, 2]], good["dev"][[0, 2]]) and np.array_equal(bad["params"][:, [0, 2]], good["params"][:, [0, 2]])
    assert not good["got"][1].any() and good["got"][3].all()


# ------------------------------------------------------------------------------------------------
# C. configuration
# ------------------------------------------------------------------------------------------------
def _settings(solver, noise):
    """name -> configuration keywords; each is a context of its own on both sides"""
    out = {}
    for k in (0, 1, 2):
        out[f"setting-{k}"] = dict(ssr.settings_cfg(k, noise), **(RK45_CFG if solver == "rk45" else {}))
    out["gamma-alone"] = dict(gamma=1.9e5)
    out["temperature-0"] = dict(temperature=0.0)
    out["thermal-off"] = dict(include_thermal_fluctuations=False)
    if noise == "ou":
        for name in ("gamma-alone", "temperature-0", "thermal-off"):
            out[name]["correlation_time"] = ssr.CORR_TIME
    return out


@pytest.mark.parametrize("name", ("setting-0", "setting-1", "setting-2", "gamma-alone", "temperature-0", "thermal-off"))
@pytest.mark.parametrize("solver,noise", FORMS)
def test_configuration_off_its_defaults_equals_the_host_path(stg, solver, noise, name):
    """max_step, gamma and temperature (the ou correlation time; rtol, atol and max_attempts for RK45) reach every phase and
    derive_row: P = 3, the middle phase watched, 16 time bins"""
    cfg = _settings(solver, noise)[name]
    _, Jp, Tp, _ = _pulse(solver, 2)
    J, T = spc.chain(Jp, Tp, 3, 1)
    # (the weak fields get the threshold and RK45 the target of section A, so that half of condition 0's trials cross; not at 0 K, where
    # the fixed-step solvers never reach the watched phase)
    weak = noise != "brown" and name != "temperature-0"
    res = _case(stg, solver, noise, J, T, 1, tbins=(16,), what=name, threshold="median-peak-0" if weak else 0.0, flip=weak and solver == "rk45", **cfg)
    got = res["got"]
    print(f"{solver} {noise} {name} threshold {res['threshold']:.6g}: switched {got[0].tolist()}, failed {got[1].tolist()}, crossed {got[3].tolist()}, "
          f"time bins in use {np.count_nonzero(got[5], axis=1).tolist()}")
    assert not weak or 0 < got[3][0] < 96
    if name == "temperature-0" and solver != "rk45":
        # the fixed-step solvers reject a solve at 0 K with the field on: every trial fails in its first phase and stays at m0
        assert got[1].tolist() == [96, 96] and not got[0].any() and not got[3].any()
    elif name != "temperature-0":
        assert not got[1].any()
    if name == "thermal-off":
        assert set(res["dev"].reshape(-1).tolist()) <= {0, 3}                      # a device's three trials are one solve


@pytest.mark.parametrize("solver,noise", (("rk4", "brown"), ("rk45", "white")))
def test_gamma_alone_changes_the_counts(stg, solver, noise):
    """the case with only gamma off its default is not the default's: the histogram or the crossing times move"""
    _, Jp, Tp, _ = _pulse(solver, 2)
    J, T = spc.chain(Jp, Tp, 3, 1)
    a = _case(stg, solver, noise, J, T, 1, tbins=(100,), gamma=1.9e5)["got"]
    b = _case(stg, solver, noise, J, T, 1, tbins=(100,))["got"]
    assert not np.array_equal(a[2], b[2]) or not np.array_equal(a[5], b[5])


# ------------------------------------------------------------------------------------------------
# D. stream identity
# ------------------------------------------------------------------------------------------------
IDENTITIES = {"env_id0-37": dict(env_id0=37), "trial0-7": dict(trial0=7), "stride-500": dict(trial0=7, trial_stride=500),
              "stride-2^34+3": dict(trial_stride=2 ** 34 + 3), "var_step-12345": dict(var_step=12345),
              "phase-counter-wraps": dict(env_step=2 ** 32 - 2, var_step=1)}


@pytest.mark.parametrize("name", tuple(IDENTITIES))
def test_stream_identity_of_the_trial_kernel(stg, name):
    """the trial kernel's own env_id0, trial0, trial_stride, var_step and env_step + p against contexts created at the header's ids:
    rk4 + brown, P = 3 with the middle phase watched"""
    kw = IDENTITIES[name]
    _, Jp, Tp, _ = _pulse("rk4", 2)
    J, T = spc.chain(Jp, Tp, 3, 1)
    res = _case(stg, "rk4", "brown", J, T, 1, tbins=(16,), what=name, **kw)
    got, dev = res["got"], res["dev"]
    assert not got[1].any() and ((0 < got[0]) & (got[0] < 96)).all()
    if name.startswith("trial0") or name == "stride-500":
        # trials 7 ... 102 are devices 2 ... 34, the first of them with trials 7 and 8 alone
        assert spr.touched(7, 96, 3) == (2, 34) and dev.shape == (2, 35) and not dev[:, :2].any() and (dev[:, 2] <= 2).all()
    if name == "stride-2^34+3":
        assert spr.device_env(0, 1, 2 ** 34 + 3, 0, 3) > 2 ** 33
    if name == "var_step-12345":
        other = _case(stg, "rk4", "brown", J, T, 1, tbins=(16,))
        assert not np.array_equal(other["params"], res["params"])
        assert not np.array_equal(other["got"][2], got[2]) or not np.array_equal(other["got"][5], got[5])
    if name == "phase-counter-wraps":
        assert [(2 ** 32 - 2 + p) % 2 ** 32 for p in range(3)] == [2 ** 32 - 2, 2 ** 32 - 1, 0]


# ------------------------------------------------------------------------------------------------
# E. geometry with everything on
# ------------------------------------------------------------------------------------------------
def test_many_conditions_looping_lanes_tables_and_time_bins(stg):
    """G = 4097 (cap 2): R = 256 runs two trials per lane; Q = 100, so devices straddle wavefronts and a lane's two trials are two
    devices'; the watched pulse is tabled (trapezoid and field ramp per condition), 100 time bins.  34 conditions -- the first, the
    last and 32 drawn between -- against the host path, the others by the sums"""
    big, R, Q = 4097, 256, 100
    assert ssr.plan_cap(big) == 2 and -(-R // 64) // ssr.plan_cap(big) == 2
    m3, J3, T3, t3 = ssr.conditions()
    idx = np.arange(big) % ssr.G
    m0, tgt = m3[idx], t3[idx]
    Jp, Tp = J3[idx] * (0.8 + 0.4 * np.arange(big) / big), T3[idx].copy()
    cur = swr.trapezoid(Jp, Tp)
    ang = swr.FIELD_ANGLES[idx]
    fld = (np.stack([np.zeros(big), Tp]), np.stack([np.zeros((big, 3)), swr.FIELD * np.stack([np.cos(ang), np.sin(ang), np.zeros(big)], axis=1)]))
    sigma = np.ascontiguousarray(SIGMA3[:, idx] * 0.5)
    sample = np.unique(np.concatenate([[0, big - 1], np.random.default_rng(25).integers(1, big - 1, 32)])).tolist()
    assert 30 <= len(sample) <= 34 and sample[0] == 0 and sample[-1] == big - 1
    b = ssr.backend(stg, "rk4", "brown", big)
    params = spc.checked_devices(stg, b, big, 3, sigma, Q, R, z_clip=2.0, conds=sample)
    got, dev = spr.fused(b, m0, Jp[None], Tp[None], tgt, R, sigma, cur, fld, dev_stride=3, trials_per_device=Q, z_clip=2.0, n_bins=7, n_tbins=100,
                         passage=True, env_step=3)
    b.close()
    ref = spc.population_host_path(stg, "rk4", "brown", m0, Jp[None], Tp[None], tgt, R, Q, params, cur=cur, fld=fld, env_step=3, trial_stride=R, conds=sample)
    want, want_dev = spc.reference_counts(ref, tgt[sample], Tp[sample], R, 3, n_bins=7, n_tbins=100)
    spc.same([x[sample] for x in got], want, "sample")
    assert np.array_equal(dev[sample], want_dev)
    assert (got[2].sum(axis=1) == R).all() and np.array_equal(got[5].sum(axis=1), got[3]) and np.array_equal(dev.sum(axis=1), got[0])
    assert not got[1].any() and (dev[:, :2] <= Q).all() and (dev[:, 2] <= 56).all() and got[3].all()
    assert (np.count_nonzero(got[5], axis=1) > 2).all() and got[5][:, 64:].any()                 # (bins 64 ... 99: the second one a lane owns)


# ------------------------------------------------------------------------------------------------
# F. the CPU oracle, off its defaults
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise,k", spc.ORACLE_CASES)
def test_population_equals_the_oracle_off_its_defaults(stg, oracle_mod, solver, noise, k):
    """spr.oracle_path's construction at setting k, P = 3: the oracle is handed the dumped devices as class tables; conditioning is
    asserted on THESE devices (margin ssr.margin()) before the counts are compared"""
    m0, _, _, tgt = ssr.conditions()
    sigma, env_step, J, T = spc.oracle_inputs(solver, noise, k)
    cfg = spc.oracle_cfg(solver, noise, k)
    R, Q, D = spr.ORACLE_R, spr.ORACLE_Q, spr.ORACLE_D
    b = ssr.backend(stg, solver, noise, ssr.G, **cfg)
    params = spc.checked_devices(stg, b, ssr.G, D, sigma, Q, R, z_clip=spr.ORACLE_CLIP)
    case = spc.oracle_case(stg, solver, noise, k, params)
    got, dev = spr.fused(b, m0, J, T, tgt, R, sigma, dev_stride=D, trials_per_device=Q, z_clip=spr.ORACLE_CLIP, n_bins=ssr.ORACLE_BINS, env_step=env_step)
    b.close()
    print(f"{solver} {noise} setting {k}: switched {got[0].tolist()} (oracle {case['counts'][0].tolist()}), distance to a decision {case['distance']:.2e}")
    spc.check_conditioned(case, solver, noise, k)
    cpu = spr.population(spr.nominal_values(ssr.flat_tables(stg)[0]), sigma, spr.oracle_normals(oracle_mod, SEED, ssr.G, D, Q, R), spr.ORACLE_CLIP)
    s_max = sigma.max()
    assert np.abs(params / cpu - 1.0).max() < 2e-5 * s_max / (1.0 - s_max * spr.ORACLE_CLIP)      # |d value / value| <= sigma |dz| / (1 - sigma clip)
    spc.same(got, case["counts"], (solver, noise, k), names=spc.NAMES[:3])
    assert np.array_equal(dev, case["dev_switched"])


# ------------------------------------------------------------------------------------------------
# G. the Python method
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tabled", (False, True), ids=("P3-rect", "tabled-behind-equilibrate"))
def test_python_method_equals_the_backend_call(stg, tabled):
    from spin_torque_gym_amd import physics
    m0, Jp, Tp, tgt = _pulse("rk4", 2)
    R, Q = 128, 4
    variation = {"volume": 0.1, "damping": [0.05, 0.02], "polarization": 0.03}
    solver = physics.SimpleLLGSSolver(method="rk4", noise_model="brown", seed=SEED)
    J, T = spc.chain(Jp, Tp, 3, 1)
    kw = dict(n_bins=7, env_step=2, variation=variation, variation_step=12345, variation_clip=3.0, trials_per_device=Q, per_device=True, time_bins=16)
    cur = fld = None
    if tabled:
        cur, _ = spc.knots("kj5-kh0", "rk4", 2)
        call = lambda **k: solver.switching_statistics(m0, None, Tp, ssr.params(), R, equilibrate=3e-11, relax=2e-11, current_knots=cur, **kw, **k)       # noqa: E731
    else:
        call = lambda **k: solver.switching_statistics(m0, J, T, ssr.params(), R, watch_phase=1, **kw, **k)       # noqa: E731
    res = call()
    sigma = physics._variation_sigma(variation, 2, 3.0)
    assert sigma.tolist() == [[0.05, 0.02], [0.0, 0.0], [0.0, 0.0], [0.1, 0.1], [0.03, 0.03]]
    b = ssr.backend(stg, "rk4", "brown", 2)
    got, dev = spr.fused(b, m0, J, T, tgt, R, sigma, cur, fld, dev_stride=R // Q, trials_per_device=Q, z_clip=3.0, var_step=12345, watch_phase=1, n_bins=7,
                         n_tbins=16, env_step=2)
    b.close()
    for name, x in zip(spc.NAMES, got):
        assert np.array_equal(res[name], x), name
    assert np.array_equal(res["dev_switched"], dev) and res["n_devices"].tolist() == [32, 32] and (res["dev_trials"] == Q).all()
    # what follows from the integers
    n_cr, t_hist = got[3], got[5]
    edges = np.linspace(0.0, 1.0, 17)[None, :] * Tp[:, None]
    centres = 0.5 * (edges[:, :-1] + edges[:, 1:])
    assert np.array_equal(res["p_cross"], n_cr / R) and np.array_equal(res["t_edges"], edges) and np.array_equal(res["p_cross_by"], np.cumsum(t_hist, axis=1) / R)
    assert n_cr.all() and np.array_equal(res["t_mean"], (t_hist * centres).sum(axis=1) / t_hist.sum(axis=1))
    assert np.array_equal(res["p_switch"], got[0] / R) and np.array_equal(res["dev_p_switch"], dev / Q)
    # chunks of 50 trials: devices straddle the chunks (50 = 12 devices and a half)
    chunked = call(max_trials_per_launch=50)
    assert set(chunked) == set(res)
    for k in res:
        assert np.array_equal(res[k], chunked[k], equal_nan=True), k
    # and the variation matters: the default counter word draws another chip
    other = solver.switching_statistics(m0, J, T, ssr.params(), R, watch_phase=1, **dict(kw, variation_step=2 ** 31)) if not tabled else None
    assert other is None or not np.array_equal(other["dev_switched"], res["dev_switched"])

"""RK45 under waveforms against the C oracle at many lanes, on the GPU: `pytest -m gpu`.

Every RK45 waveform path of the library ends in llgs_solve_wave (csrc/stg_wave.hpp), a second statement of the Dormand-Prince attempt
with ballots and masks of its own, a forward-only cursor pair per lane, a scratch copy of the cursors per attempt and a probe copy for
select_initial_step.  The reference's recorded rows (G22, G24) reach it on contexts of ONE env, where a mask that is wave-wide instead
of per lane, a `low` flag that ends a neighbour or a cursor copy that survives a rejected attempt cannot show.  Here the oracle's
waveform solve (oracle/stg_oracle.c: stgo_llgs_solve_wave, a linear table scan from zero on every call; held to G22 / G24 by
tests/test_wave_oracle.py on the CPU) is the reference at N = 130 -- two wavefronts and a two-lane tail -- plus one case each at N = 1
and N = 64:

  stg_solve_wave   default configuration, thermal off: current + field, current only, field only (K = 2, 3, 17, 32), with success,
                   accepted points and m_final of every lane, every lane's energy and torque rows at its own recorded (t, m), and the
                   t / m / energy / torques rows against the oracle's while the lane steps at max_step (_check_rows); the four RK45 settings of
                   env_config_cases (two of them with 32 knots inside 3 max_step); two volumes by class; the thermal field (white, the
                   model RK45 takes) on a stream with non-zero env_id0 and env_step; a T = 0 lane, a bad-table lane and a NaN start row
                   among live lanes of one wavefront; an attempt budget that splits the wavefronts;
  stg_step_wave    two chained steps, thermal off and on, per-env tables, float32 and float64 actions, against
                   tests/wave_step_ref.py with the oracle's solve handed in;
  stg_step_knots   one launch of three steps with amplitudes that differ per env and per knot, against the same restatement.

The inputs and why their amplitudes are what they are: tests/wave_rk45_cases.py; tests/test_wave_oracle.py shows on the CPU that every
compared lane is well conditioned (one ulp on the start row: same points and attempts, m_final within tolerance / 100, no attempt within
1e-6 of an accept/reject tie) and that the sweep is not vacuous.  Tolerances are the project's: tol_for('rk45', thermal) = 1e-8, x 50
under the thermal field; 1e-9 T on times; energies and torques 1e-8 of the lane's largest magnitude; step level as
tests/test_gpu_wave_config.py.  profiles/NOTEBOOK.md (round 26) lists the worst errors measured on an MI355X (m_final 1.6e-15 ... 7.4e-11
thermal off, at most 7.0e-9 under the thermal field) and what is known about six mutations of llgs_lane_attempt_wave /
llgs_lane_begin_wave."""
import numpy as np
import pytest
import torch

from env_config_cases import tol_for
from knots_ref import wave_rows
from test_gpu_wave_config import OUT_KEYS, OUT_NAMES, _backend, _compare_step, _dev, _outs, _same, _state, _wave
import wave_config_cases as wcc
import wave_rk45_cases as wrc
import wave_step_ref

pytestmark = pytest.mark.gpu

F64 = torch.float64


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _solve(stg, c, p, traj_cap=0, **over):
    b = _backend(stg, c["n"], p["plist"], cls=p["cls"] if c["classes"] > 1 else None, env_id0=wrc.ENV_ID0, solver="rk45", seed=wrc.SEED,
                 include_thermal_fluctuations=c["thermal"], temperature=c["temperature"], **{**c["cfg"], **over})
    out = b.solve(_dev(p["m0"].T), _dev(p["J"]), _dev(p["T"]), env_step=wrc.ENV_STEP, traj_cap=traj_cap, want_energy=traj_cap > 0,
                  wave=_wave(p["cur"], p["fld"]))
    torch.cuda.synchronize()
    res = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    b.close()
    return res


def _check_lanes(name, c, res, ref, keep):
    """success, accepted points and m_final of the lanes `keep` against the oracle; returns the worst |m - m_ref|"""
    tol = tol_for("rk45", c["thermal"])
    mf = res["m_final"].T
    err = np.abs(mf - ref["m_final"]).max(axis=1)
    sure = keep & (ref["tie"] >= wrc.TIE_MARGIN) if c["thermal"] else keep
    loose = keep & ~sure
    differ = int((res["n_points"][loose] != ref["n_points"][loose]).sum())
    print(f"{name}: {int(keep.sum())} lanes, worst |m - m_ref| = {err[keep].max():.2e} (bound {tol:.0e}); points {ref['n_points'][keep].min()} ... "
          f"{ref['n_points'][keep].max()}, attempts {ref['attempts'][keep].min()} ... {ref['attempts'][keep].max()}, "
          f"{int((ref['attempts'] > ref['n_points'])[keep].sum())} lanes with rejections; point counts printed, not asserted: {int(loose.sum())} lanes "
          f"({differ} differ)")
    assert np.array_equal(res["success"].astype(bool)[keep], ref["success"][keep]), np.flatnonzero(keep & (res["success"].astype(bool) != ref["success"]))
    assert np.array_equal(res["n_points"][sure], ref["n_points"][sure]), np.flatnonzero(sure & (res["n_points"] != ref["n_points"]))[:8]
    assert err[keep].max() <= tol, (np.flatnonzero(keep & (err > tol))[:8], err[keep].max())
    return float(err[keep].max())


def _check_rows(name, c, p, res, ref, keep):
    """The recorded rows of the lanes `keep`.  Every lane: as many rows as accepted points, times increasing from 0 to T exactly, and
    the by-products at the lane's OWN recorded (t, m) against wave_rk45_cases.by_products -- the Zeeman term and current(t_i) --, to 1e-8
    of the lane's largest magnitude.  Row by row against the oracle (t to 1e-9 T, m to the tolerance, energy and torques to 1e-8 of the
    lane's largest magnitude): each lane's rows up to the start of its first step that is not max_step (wave_rk45_cases.clamped_rows says
    why no further); the row at t = T is m_final, compared in every lane by _check_lanes.  That is narrower than "the rows of every
    lane": 1 813 ... 2 069 of about 2 900 rows in the three default cases (63 ... 70 %; 77 ... 88 of 130 lanes in full), 6 408 of 13 304 in
    s1-dense, 256 of 971 in s0-dense, and row 0 alone in most lanes of s2 (184 of 772) and s3-rect (131 of 1 441), whose first step is
    not max_step.  The rows after a rejection are held through m_final, the point count and the by-products only."""
    assert ref["n_points"].max() + 1 <= wrc.TRAJ_CAP
    lanes = np.flatnonzero(keep)
    worst_e = worst_q = 0.0
    n_tq = 0
    for i in lanes:
        k = int(res["n_points"][i]) + 1
        t, m = res["t"][:k, i], res["m"][:k, :, i]
        assert t[0] == 0.0 and t[-1] == p["T"][i] and (np.diff(t) > 0).all(), i
        e, q = wrc.by_products(p, c, i, t, m)
        de, dq = np.abs(res["energy"][:k, i] - e).max(), np.abs(res["torques"][:k, i] - q).max()
        worst_e, worst_q = max(worst_e, de / np.abs(e).max()), max(worst_q, dq / max(np.abs(q).max(), 1e-300))
        n_tq += int(np.abs(q).max() > 0)
        assert de <= 1e-8 * np.abs(e).max() and dq <= 1e-8 * np.abs(q).max(), (i, de, dq)
    cnt = np.where(keep, wrc.clamped_rows(c, p, ref), 0)
    have = np.arange(wrc.TRAJ_CAP)[:, None] < cnt[None, :]                # [cap, n]: the rows compared with the oracle's
    assert (np.isfinite(ref["t"]) | ~have).all()
    tol = tol_for("rk45", False)
    gap = lambda key: np.where(have, np.abs(res[key] - ref[key]), 0.0).max(axis=0)          # noqa: E731
    big = lambda key: np.where(have, np.abs(ref[key]), 0.0).max(axis=0)                     # noqa: E731
    dm = np.where(have[:, :, None], np.abs(res["m"].transpose(0, 2, 1) - ref["m"]), 0.0).max(axis=(0, 2))
    rel = lambda d, b: float(np.max(np.where(b > 0, d / np.where(b > 0, b, 1.0), 0.0)))     # noqa: E731
    total = int((ref["n_points"][keep] + 1).sum())
    print(f"{name} rows: by-products at the lane's own rows, all {len(lanes)} lanes: energy {worst_e:.2e}, torques {worst_q:.2e} of the lane's largest "
          f"magnitude (bound 1e-08; {n_tq} lanes with torques); against the oracle, {int(have.sum())} of {total} rows ({int((cnt[keep] == ref['n_points'][keep] + 1).sum())} "
          f"lanes in full): t {rel(gap('t'), p['T']):.2e} T (bound 1e-09), m {dm.max():.2e} (bound {tol:.0e}), energy {rel(gap('energy'), big('energy')):.2e}, "
          f"torques {rel(gap('torques'), big('torques')):.2e} (bound 1e-08)")
    assert (gap("t") <= 1e-9 * p["T"]).all(), np.flatnonzero(gap("t") > 1e-9 * p["T"])[:8]
    assert dm.max() <= tol, np.flatnonzero(dm > tol)[:8]
    for key in ("energy", "torques"):
        assert (gap(key) <= 1e-8 * big(key)).all(), (key, np.flatnonzero(gap(key) > 1e-8 * big(key))[:8])


SOLVE_NAMES = [c["name"] for c in wrc.solve_cases() if not c["bad_lanes"]]


@pytest.mark.parametrize("name", SOLVE_NAMES)
def test_solve_wave_vs_oracle(stg, oracle_mod, name):
    c = wrc.case(name)
    p, ref = wrc.solve_ref(c, oracle_mod)
    keep = wrc.compared_lanes(c)
    assert keep.all() and ref["success"].all()
    res = _solve(stg, c, p, traj_cap=0 if c["thermal"] else wrc.TRAJ_CAP)
    _check_lanes(f"solve {name}", c, res, ref, keep)
    if not c["thermal"]:
        _check_rows(f"solve {name}", c, p, res, ref, keep)


def test_bad_and_rejected_lanes_among_good_ones(stg, oracle_mod):
    """A T = 0 lane, a lane whose current table is not strictly increasing and a NaN start row in wavefront 0, among live lanes of which
    every ninth rejects attempts.  The good lanes are held to the oracle in full.  The bad ones to include/spintorque_hip.h: a bad table
    and a failed RK45 solve (the NaN row: every attempt rejected until the step underflows) give success 0, m_final = m0 bit for bit and no
    accepted point; T = 0 has nothing to integrate -- as SciPy and the oracle, success with no accepted point and m_final the normalised
    start row."""
    c = wrc.case("bad-lanes")
    p, ref = wrc.solve_ref(c, oracle_mod)
    keep = wrc.compared_lanes(c)
    assert ref["success"][keep].all() and (ref["attempts"] > ref["n_points"])[:64][keep[:64]].sum() >= 5
    res = _solve(stg, c, p, traj_cap=wrc.TRAJ_CAP)
    _check_lanes("bad lanes: the good ones", c, res, ref, keep)
    _check_rows("bad lanes: the good ones", c, p, res, ref, keep)
    ok, npts, mf = res["success"].astype(bool), res["n_points"], torch.from_numpy(np.ascontiguousarray(res["m_final"].T))
    m0 = torch.from_numpy(p["m0"])
    for lane in (wrc.BAD_TABLE, wrc.BAD_NAN):
        assert not ok[lane] and npts[lane] == 0, (lane, ok[lane], npts[lane])
        _same(mf[lane], m0[lane], f"m_final of bad lane {lane}")
        assert not ref["success"][lane] and ref["n_points"][lane] == 0
    lane = wrc.BAD_T0
    assert ok[lane] and npts[lane] == 0 and ref["success"][lane] and ref["n_points"][lane] == 0
    assert np.abs(res["m_final"][:, lane] - ref["m_final"][lane]).max() <= tol_for("rk45", False)


def test_attempt_budget_that_splits_the_wavefronts(stg, oracle_mod):
    """max_attempts between the smallest and the largest attempt count of the 130 lanes.  Lanes within the budget are held to the
    oracle in full.  For a lane over it the library documents success 0, m_final = m0 and n_points = the points accepted until then
    (include/spintorque_hip.h: stg_solve_wave); the oracle leaves m_final at the last accepted row instead (oracle/stg_oracle.h says
    so).  The documented behaviour is what is asserted: m_final against m0 bit for bit, n_points against the oracle's count of accepted
    points under the same budget."""
    c = wrc.case("default-jh")
    p, full = wrc.solve_ref(c, oracle_mod)
    budget = int(np.sort(full["attempts"])[len(full["attempts"]) // 2]) + 1
    under = full["attempts"] <= budget
    assert full["attempts"].min() < budget < full["attempts"].max() and 20 <= under.sum() <= c["n"] - 20
    assert all(0 < under[w:w + 64].sum() < len(under[w:w + 64]) for w in (0, 64))          # both full wavefronts are split
    ref = wrc.run_oracle(oracle_mod, c, p, cap=wrc.TRAJ_CAP, max_attempts=budget)
    assert np.array_equal(ref["success"], under)
    res = _solve(stg, c, p, traj_cap=wrc.TRAJ_CAP, max_attempts=budget)
    _check_lanes(f"budget {budget}: lanes within it", c, res, ref, under)
    _check_rows(f"budget {budget}: lanes within it", c, p, res, ref, under)
    over = ~under
    print(f"budget {budget}: {int(over.sum())} lanes over it, accepted points until then {ref['n_points'][over].min()} ... {ref['n_points'][over].max()}")
    assert not res["success"].astype(bool)[over].any()
    assert np.array_equal(res["n_points"][over], ref["n_points"][over])
    _same(torch.from_numpy(np.ascontiguousarray(res["m_final"].T[over])), torch.from_numpy(np.ascontiguousarray(p["m0"][over])), "m_final of lanes over the budget")


# ------------------------------------------------------------------------------------------------
# stg_step_wave, stg_step_knots
# ------------------------------------------------------------------------------------------------
def _step_backend(stg, p, thermal, **extra):
    b = _backend(stg, wrc.N, p["plist"], cls=p["cls"], env_id0=wrc.ENV_ID0, solver="rk45", seed=wrc.SEED, include_thermal_fluctuations=thermal,
                 **p["cfg"], **extra)
    st = p["state"]
    b.reset(init_m=_dev(st["m"].T), target=_dev(st["target"].T))
    b.set_state(dict(total_energy=st["total_energy"], step_count=st["step_count"].astype(np.int32)))
    return b


def _pulse_energy(p, k, m_before):
    """wave_config_cases.pulse_energy for a class table of STT records"""
    _, T = wave_step_ref.parse_actions(p["acts"][k], p["cfg"]["max_current"], p["cfg"]["max_duration"])
    I = wave_step_ref.pulse_sq_integral(p["cur"][k][0], p["cur"][k][1], T)
    e = np.zeros(len(T))
    for ci, d in enumerate(p["plist"]):
        sel = p["cls"] == ci
        r = wave_step_ref.resistance(m_before[sel], d)
        ra = r * d["area"]
        e[sel] = (ra * ra) / r * I[sel]
    return e


@pytest.mark.parametrize("name", [c["name"] for c in wrc.step_cases()])
def test_step_wave_vs_oracle_plus_tail(stg, oracle_mod, name):
    c = wrc.step_case(name)
    p, refs = wrc.step_ref(c, oracle_mod)
    tol = tol_for("rk45", c["thermal"])
    b = _step_backend(stg, p, c["thermal"])
    for k, ref in enumerate(refs):
        assert (ref["status"] == 0).all()
        before = _state(b)
        o = _outs(b, b.step_wave(_dev(p["acts"][k].T), _wave(p["cur"][k], p["fld"][k])))
        e_ref = _pulse_energy(p, k, before["m"].cpu().numpy().T)
        if k == 0:
            assert np.all(np.abs(e_ref - ref["energy"]) <= 1e-14 * np.abs(ref["energy"]))       # (the reset normalises the given rows once more)
        _compare_step(o, _state(b), ref, wrc.N, tol, f"{name}, step {k}", e_ref=e_ref, etot_ref=before["total_energy"].cpu().numpy() + e_ref)
    b.close()


def test_step_knots_vs_oracle_plus_tail_with_amplitudes_that_are_not_flat(stg, oracle_mod):
    """One K = 3 launch of stg_step_knots under RK45 with amplitudes drawn per env and per knot (wave_config_cases.knots_problem at
    wave_rk45_cases.KNOTS_SEED): the tables tests/knots_ref.py builds from the parsed actions, the oracle's waveform solve and the
    restatement's tail.  As tests/test_gpu_knots_config.py: test_knots_launch_vs_restatement does for the fixed-step solvers, a launch
    hands back the fp64 state of its last step only, so the start rows of step k -- the energy goes with their resistance -- come from
    a launch of the first k steps on a twin context.  The flat-pulse oracle test of tests/test_gpu_step_knots.py stays as it is."""
    from test_gpu_wave_config import _step_backend as shaped_backend
    p, refs = wrc.knots_ref(oracle_mod)
    K, n, tol = wrc.KNOTS_STEPS, wcc.N, tol_for("rk45", False)
    acts = _dev(np.ascontiguousarray(p["acts"].transpose(0, 2, 1)))

    def backend():
        b = shaped_backend(stg, dict(method="rk45", noise=None, n=n), p)
        b.set_pulse_knots(p["tau"], p["limit"], p["fk"])
        return b
    starts = []                                                  # the kernels' own state before step k
    for k in range(K):
        twin = backend()
        if k:
            twin.step_knots_many(acts[:k], out_every=False)
        starts.append(_state(twin))
        twin.close()
    pe = dict(p, acts=[wave_rows(a) for a in p["acts"]])
    e_refs = [wcc.pulse_energy(pe, k, starts[k]["m"].cpu().numpy().T) for k in range(K)]
    b = backend()
    res = b.step_knots_many(acts, out_every=True)
    torch.cuda.synchronize()
    f = {key: v.clone() for key, v in zip(OUT_NAMES, res)}
    f["energy"] = b.energy_many.clone()
    st = _state(b)
    for k in range(K):
        o = {key: f[key][k] for key in OUT_KEYS}
        assert (refs[k]["status"] == 0).all()
        if k + 1 < K:                                            # the state after step k: the twin's start rows of step k + 1
            err = float(np.abs(starts[k + 1]["m"].cpu().numpy().T - refs[k]["m"]).max())
            print(f"knots launch rk45, amplitudes not flat, step {k}: worst |m - m_ref| = {err:.2e} (bound {tol:.0e})")
            assert err <= tol, k
        e = o["energy"].cpu().numpy()
        assert np.all(np.abs(e - e_refs[k]) <= 1e-13 * np.abs(e_refs[k])), k
        for key in ("terminated", "truncated"):
            assert np.array_equal(o[key].cpu().numpy().astype(bool), refs[k][key]), (k, key)
        assert np.array_equal(o["status"].cpu().numpy(), refs[k]["status"])
        ob, ob_ref = o["obs"].cpu().numpy().T, refs[k]["obs"]
        assert np.all(np.abs(ob - ob_ref) <= wave_step_ref.F32_ULP * np.abs(ob_ref) + 2 * tol), k
        assert np.all(np.abs(o["reward_f64"].cpu().numpy() - refs[k]["reward"]) <= 1e-9 + 2 * tol), k
    _compare_step({key: f[key][K - 1] for key in OUT_KEYS}, st, refs[K - 1], n, tol, f"knots launch rk45, amplitudes not flat, step {K - 1}",
                  e_ref=e_refs[K - 1], etot_ref=starts[K - 1]["total_energy"].cpu().numpy() + e_refs[K - 1])
    b.close()

"""stg_switch_stats_wave -- stg_switch_stats with one phase of the trial driven by piecewise-linear current and field tables
(include/spintorque_hip.h) -- held to EXACT integer equality with existing code: `pytest -m gpu`.

Every trial of the fused kernel is, by the header's stream rule, problem g * trial_stride + r of stg_solve_wave (the wave phase) and of
stg_solve (the rectangular phases).  The reference of every test here is therefore the host path of tests/switch_stats_wave_ref.py:
stg_solve_wave / stg_solve over the G * R replicated problems with the tables replicated per trial, phase after phase, reduced with
NumPy by the header's classification and bin arithmetic (switch_stats_ref.host_counts).

  1. equality, one trial per lane: R in {1, 63, 64, 65, 130}, P = 1, five forms, thresholds 0 and the median, three knot sets;
  2. lanes loop over two trials (the cursors are opened anew per trial);
  3. 32 + 32 knots with a knot in every sub-step of a window, tables that end before T / start after 0;
  4. phases: P = 3 with wave_phase = 1 and a T == 0 wave phase, wave_phase = 0 and P - 1;
  5. histogram; 6. additivity; 7. class table; 8. a bad table in one condition; 9. the Python method; 10. write footprint and
  refusals; 11. the NumPy statement under the oracle's normals (no stg_solve_wave involved).

Inputs: switch_stats_ref.conditions() with a 5-knot trapezoid and a 2-knot in-plane field ramp per condition (switch_stats_wave_ref).
Every test fails without the feature: the library has no symbol stg_switch_stats_wave."""
import ctypes as C

import numpy as np
import pytest
import torch

import brown_ref as br
from helpers import Guarded
import switch_stats_ref as ssr
import switch_stats_wave_ref as swr
from switch_stats_ref import G, SEED, host_counts as _host_counts, proj as _proj

pytestmark = pytest.mark.gpu

SMALL_R = (1, 63, 64, 65, 130)
FORMS = (("rk4", "brown"), ("euler", "brown"), ("rk4", "ou"), ("rk4", "white"), ("rk45", "white"))
KNOT_SETS = ("kj5-kh2", "kj5-kh0", "kj0-kh2")


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _median_threshold(m, tgt, R, g=1):
    """a threshold that splits condition g's trials in two: the median of its projections on the host path"""
    return float(np.median(_proj(m, np.repeat(tgt, R, axis=0))[g * R:(g + 1) * R]))


def _same(got, want, what=None):
    for x, y in zip(got, want):
        assert (x is None and y is None) or np.array_equal(x, y), (what, x, y)


# ------------------------------------------------------------------------------------------------
# 1. equality with stg_solve_wave, one trial per lane
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knots", KNOT_SETS)
@pytest.mark.parametrize("solver,noise", FORMS)
def test_counts_equal_stg_solve_wave(stg, solver, noise, knots):
    """P = 1, trial_stride = R: the counts equal the host reduction of ONE stg_solve_wave over the G R replicated problems and tables"""
    m0, J, T, tgt = ssr.conditions()
    cur, fld = swr.knot_sets()[knots]
    b = ssr.backend(stg, solver, noise, G)
    for R in SMALL_R:
        m, failed = swr.host_path(stg, solver, noise, m0, J[None], T[None], tgt, R, cur, fld, env_step=2)
        want_sw, want_failed, _ = _host_counts(m, failed, tgt, R)
        n_sw, n_failed, hist = swr.fused(b, m0, J[None], T[None], tgt, R, cur, fld, env_step=2)
        print(f"{solver} {noise} {knots} R = {R}: switched {n_sw.tolist()} (host {want_sw.tolist()}), failed {n_failed.tolist()}")
        assert hist is None
        assert np.array_equal(n_sw, want_sw) and np.array_equal(n_failed, want_failed), (solver, noise, knots, R)
        assert not want_failed.any()
        if noise == "brown" and R >= 63:
            assert ((0 < want_sw) & (want_sw < R)).all(), (R, want_sw)           # the field decides: neither 0 nor R (asserted on the reference)
        thr = _median_threshold(m, tgt, R)
        want_thr = _host_counts(m, failed, tgt, R, threshold=thr)[0]
        got_thr = swr.fused(b, m0, J[None], T[None], tgt, R, cur, fld, env_step=2, threshold=thr)[0]
        assert np.array_equal(got_thr, want_thr), (solver, noise, knots, R, want_thr)
    b.close()


# ------------------------------------------------------------------------------------------------
# 2. lanes loop
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise", (("rk4", "brown"), ("rk45", "white")))
def test_counts_equal_when_lanes_loop(stg, solver, noise):
    """one trial more than SWITCH_STATS_WAVES // G wavefronts hold at one trial per lane: every lane runs two trials, and the second one
    must start from cursors opened anew (a cursor left at the end of the first trial's table would hand it the tail value throughout)"""
    from spin_torque_gym_amd import _lib
    R = 64 * (_lib.SWITCH_STATS_WAVES // G) + 1
    m0, J, T, tgt = ssr.conditions()
    cur, fld = swr.knot_sets()["kj5-kh2"]
    m, failed = swr.host_path(stg, solver, noise, m0, J[None], T[None], tgt, R, cur, fld)
    want = _host_counts(m, failed, tgt, R, n_bins=7)
    thr = _median_threshold(m, tgt, R)
    want_thr = _host_counts(m, failed, tgt, R, threshold=thr)[0]
    b = ssr.backend(stg, solver, noise, G)
    got = swr.fused(b, m0, J[None], T[None], tgt, R, cur, fld, n_bins=7)
    got_thr = swr.fused(b, m0, J[None], T[None], tgt, R, cur, fld, threshold=thr)[0]
    b.close()
    print(f"{solver} {noise} R = {R}: switched {got[0].tolist()} (host {want[0].tolist()}), failed {got[1].tolist()}; above the median {got_thr.tolist()}")
    _same(got, want)
    assert np.array_equal(got_thr, want_thr)


# ------------------------------------------------------------------------------------------------
# 3. knot count and crossings
# ------------------------------------------------------------------------------------------------
def _dense_tables(J, T, first, spacing):
    """32 + 32 knots per condition: the first at `first` x T, then every `spacing` sub-steps (dt = T / 100 for these pulses) -- below one
    sub-step, so every sub-step of the window crosses a knot (two now and then) -- with the current wobbling around the plateau and the
    field turning in the plane"""
    k = np.arange(32)
    tk = (first + k * spacing / 100.0)[:, None] * T[None, :]
    jk = (1.0 + 0.2 * np.cos(1.3 * k))[:, None] * J[None, :]
    ang = 0.45 * k[:, None] + swr.FIELD_ANGLES[None, :]
    hk = swr.FIELD * np.stack([np.cos(ang), np.sin(ang), np.zeros_like(ang)], axis=2)
    assert (np.diff(tk, axis=0) > 0).all()
    return (tk, jk), (tk * 1.01 + 1e-13, hk)


@pytest.mark.parametrize("where", ("ends-before-T", "starts-after-0", "covers"))
@pytest.mark.parametrize("solver,noise", (("rk4", "brown"), ("euler", "brown"), ("rk45", "white")))
def test_thirty_two_knots_and_crossings(stg, solver, noise, where):
    m0, J, T, tgt = ssr.conditions()
    if solver == "rk45":
        J = J * ssr.RK45_J_SCALE              # below the LLGS solver's current gate, where its trials do not saturate: the field table decides
    first, spacing = {"ends-before-T": (0.0, 0.7), "starts-after-0": (0.6, 0.9), "covers": (-0.05, 3.6)}[where]
    cur, fld = _dense_tables(J, T, first, spacing)
    if where == "ends-before-T":
        assert (cur[0][-1] < 0.25 * T).all() and (cur[0][0] == 0).all()           # the tail value holds for three quarters of the pulse
    elif where == "starts-after-0":
        assert (cur[0][0] > 0.5 * T).all() and (cur[0][-1] < T).all()             # the head value holds for the first half
    else:
        assert (cur[0][0] < 0).all() and (cur[0][-1] > T).all()
    R = 130
    m, failed = swr.host_path(stg, solver, noise, m0, J[None], T[None], tgt, R, cur, fld, env_step=1)
    want = _host_counts(m, failed, tgt, R, n_bins=7)
    assert not want[1].any()
    b = ssr.backend(stg, solver, noise, G)
    got = swr.fused(b, m0, J[None], T[None], tgt, R, cur, fld, env_step=1, n_bins=7)
    thr = _median_threshold(m, tgt, R)
    got_thr = swr.fused(b, m0, J[None], T[None], tgt, R, cur, fld, env_step=1, threshold=thr)[0]
    # the tables matter: the 5 + 2 knot set leaves other trials
    other = swr.fused(b, m0, J[None], T[None], tgt, R, *swr.knot_sets()["kj5-kh2"], env_step=1, n_bins=7)
    b.close()
    print(f"{solver} {noise} {where}: switched {got[0].tolist()} (host {want[0].tolist()}); hist {got[2].tolist()}; above the median {got_thr.tolist()}")
    _same(got, want, where)
    assert np.array_equal(got_thr, _host_counts(m, failed, tgt, R, threshold=thr)[0])
    if noise == "brown":
        assert not np.array_equal(other[2], got[2])


# ------------------------------------------------------------------------------------------------
# 4. phases
# ------------------------------------------------------------------------------------------------
def _three_phases():
    """equilibrate 30 ps, the shaped pulse, relax 20 ps; condition 1's pulse has T == 0 (skipped; its tables are those of its 60 ps pulse)"""
    m0, Jp, Tp, tgt = ssr.conditions()
    cur, fld = swr.knot_sets()["kj5-kh2"]
    Tw = Tp.copy()
    Tw[1] = 0.0
    J = np.stack([np.zeros(G), Jp, np.zeros(G)])
    T = np.stack([np.full(G, 3e-11), Tw, np.full(G, 2e-11)])
    return m0, J, T, tgt, cur, fld


PHASES_R, PHASES_STEP = 130, 5
_PHASES = {}


def _phases_host(stg, solver, noise):
    key = (solver, noise)
    if key not in _PHASES:
        m0, J, T, tgt, cur, fld = _three_phases()
        m, failed = swr.host_path(stg, solver, noise, m0, J, T, tgt, PHASES_R, cur, fld, wave_phase=1, env_step=PHASES_STEP)
        _PHASES[key] = _host_counts(m, failed, tgt, PHASES_R, n_bins=7)
    return _PHASES[key]


@pytest.mark.parametrize("solver,noise", (("rk4", "brown"), ("euler", "brown"), ("rk45", "white")))
def test_three_phases_equal_chained_solves(stg, solver, noise):
    m0, J, T, tgt, cur, fld = _three_phases()
    want = _phases_host(stg, solver, noise)
    assert not want[1].any()
    b = ssr.backend(stg, solver, noise, G)
    got = swr.fused(b, m0, J, T, tgt, PHASES_R, cur, fld, wave_phase=1, env_step=PHASES_STEP, n_bins=7)
    print(f"{solver} {noise} three phases: switched {got[0].tolist()} (host {want[0].tolist()}), failed {got[1].tolist()}")
    _same(got, want)
    # which phase the tables drive matters, and so do the phases around the pulse
    if noise == "brown":
        first = swr.fused(b, m0, J, T, tgt, PHASES_R, cur, fld, wave_phase=0, env_step=PHASES_STEP, n_bins=7)
        alone = swr.fused(b, m0, J[1:2], T[1:2], tgt, PHASES_R, cur, fld, env_step=PHASES_STEP, n_bins=7)
        assert not np.array_equal(first[2], got[2]) and not np.array_equal(alone[2], got[2])
    b.close()


@pytest.mark.parametrize("wave_phase", (0, 1))
@pytest.mark.parametrize("solver,noise", (("rk4", "brown"), ("rk45", "white")))
def test_wave_phase_first_and_last(stg, solver, noise, wave_phase):
    """P = 2: (pulse, relax) with wave_phase = 0 and (equilibrate, pulse) with wave_phase = P - 1"""
    m0, Jp, Tp, tgt = ssr.conditions()
    cur, fld = swr.knot_sets()["kj5-kh2"]
    rect = (np.zeros(G), np.array([3e-11, 0.0, 2e-11]))                          # (condition 1 has no rectangular phase)
    J = np.stack([Jp, rect[0]] if wave_phase == 0 else [rect[0], Jp])
    T = np.stack([Tp, rect[1]] if wave_phase == 0 else [rect[1], Tp])
    R = 130
    m, failed = swr.host_path(stg, solver, noise, m0, J, T, tgt, R, cur, fld, wave_phase=wave_phase, env_step=9)
    want = _host_counts(m, failed, tgt, R, n_bins=7)
    b = ssr.backend(stg, solver, noise, G)
    got = swr.fused(b, m0, J, T, tgt, R, cur, fld, wave_phase=wave_phase, env_step=9, n_bins=7)
    b.close()
    _same(got, want, wave_phase)


# ------------------------------------------------------------------------------------------------
# 5. histogram, 6. additivity
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def thousand(stg):
    """the rk4 + brown host path of the three conditions under the 5 + 2 knot set with R = 1000, shared"""
    m0, J, T, tgt = ssr.conditions()
    cur, fld = swr.knot_sets()["kj5-kh2"]
    return swr.host_path(stg, "rk4", "brown", m0, J[None], T[None], tgt, 1000, cur, fld)


@pytest.mark.parametrize("n_bins", (1, 7, 64))
def test_histogram_equals_numpy_on_stg_solve_wave(stg, thousand, n_bins):
    m0, J, T, tgt = ssr.conditions()
    cur, fld = swr.knot_sets()["kj5-kh2"]
    R = 1000
    edges = np.linspace(-1.0, 1.0, n_bins + 1)
    k = n_bins // 2 + 1 if n_bins > 1 else 0
    threshold = float(edges[k])                                      # on a bin edge: the bins from k up hold exactly the switched trials
    want = _host_counts(*thousand, tgt, R, threshold=threshold, n_bins=n_bins)
    b = ssr.backend(stg, "rk4", "brown", G)
    got = swr.fused(b, m0, J[None], T[None], tgt, R, cur, fld, threshold=threshold, n_bins=n_bins)
    b.close()
    assert got[2].shape == (G, n_bins) and (got[2].sum(axis=1) == R).all()
    _same(got, want, n_bins)
    assert np.array_equal(got[2][:, k:].sum(axis=1), got[0])


def test_chunks_add_up(stg, thousand):
    m0, J, T, tgt = ssr.conditions()
    cur, fld = swr.knot_sets()["kj5-kh2"]
    R = 1000
    want = _host_counts(*thousand, tgt, R, n_bins=7)
    b = ssr.backend(stg, "rk4", "brown", G)
    whole = swr.fused(b, m0, J[None], T[None], tgt, R, cur, fld, n_bins=7)
    _same(whole, want)
    args = (torch.from_numpy(m0.T.copy()), torch.from_numpy(J[None]), torch.from_numpy(T[None]), torch.from_numpy(tgt.T.copy()))
    out = None
    for t0, n in ((0, 600), (600, 400)):                              # two chunks added into one set of arrays
        out = b.switch_stats_wave(*args, n, swr.wave_dict(cur, fld), trial0=t0, trial_stride=R, n_bins=7, out=out)
    torch.cuda.synchronize()
    _same([x.cpu().numpy() for x in out], whole)
    first = swr.fused(b, m0, J[None], T[None], tgt, 600, cur, fld, trial0=0, trial_stride=R)
    b.close()
    assert not np.array_equal(first[0], whole[0])
    from spin_torque_gym_amd import physics
    solver = physics.SimpleLLGSSolver(method="rk4", noise_model="brown", seed=SEED)
    a = solver.switching_statistics(m0, J, T, ssr.params(), R, n_bins=7, current_knots=cur, field_knots=fld)
    c = solver.switching_statistics(m0, J, T, ssr.params(), R, n_bins=7, current_knots=cur, field_knots=fld, max_trials_per_launch=300)
    for k in a:
        assert np.array_equal(a[k], c[k]), k
    _same((a["n_switched"], a["n_failed"], a["hist"]), want)


# ------------------------------------------------------------------------------------------------
# 7. class table
# ------------------------------------------------------------------------------------------------
def test_two_volumes_by_cond_cls(stg):
    m0, J, T, tgt = ssr.conditions()
    cur, fld = swr.knot_sets()["kj5-kh2"]
    tables = [ssr.params(), ssr.params(0.7 * br.SWITCH["volume"])]
    cond_cls = np.array([1, 0, 1], dtype=np.uint8)
    R = 130
    m, failed = swr.host_path(stg, "rk4", "brown", m0, J[None], T[None], tgt, R, cur, fld, tables=tables, cond_cls=cond_cls)
    want = _host_counts(m, failed, tgt, R, n_bins=7)
    b = ssr.backend(stg, "rk4", "brown", G, tables, cond_cls)
    got = swr.fused(b, m0, J[None], T[None], tgt, R, cur, fld, cond_cls=torch.from_numpy(cond_cls), n_bins=7)
    _same(got, want)
    # cond_cls = NULL: class 0 for every condition
    m1, f1 = swr.host_path(stg, "rk4", "brown", m0, J[None], T[None], tgt, R, cur, fld, tables=tables, cond_cls=np.zeros(G, dtype=np.uint8))
    want0 = _host_counts(m1, f1, tgt, R, n_bins=7)
    got0 = swr.fused(b, m0, J[None], T[None], tgt, R, cur, fld, n_bins=7)
    b.close()
    _same(got0, want0)
    assert not np.array_equal(want0[2], want[2])


# ------------------------------------------------------------------------------------------------
# 8. a bad table in one condition
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise", (("rk4", "brown"), ("rk45", "white")))
def test_bad_tables_fail_their_condition_only(stg, solver, noise):
    """non-increasing times in condition 1's current table, a NaN in condition 2's field table: every trial of the two is failed and
    classified by m0 (above the equator: not switched); condition 0 is the host path's"""
    m0, J, T, tgt = ssr.conditions()
    cur, fld = swr.knot_sets()["kj5-kh2"]
    tk, jk = cur[0].copy(), cur[1].copy()
    th, hk = fld[0].copy(), fld[1].copy()
    tk[3, 1] = tk[2, 1]
    hk[1, 2, 0] = np.nan
    R = 130
    m, failed = swr.host_path(stg, solver, noise, m0, J[None], T[None], tgt, R, (tk, jk), (th, hk))
    assert failed.reshape(G, R).all(axis=1).tolist() == [False, True, True] and not failed[:R].any()     # what stg_solve_wave reports
    assert np.array_equal(m[:, R:], np.repeat(m0[1:], R, axis=0).T)
    want = _host_counts(m, failed, tgt, R, n_bins=7)
    assert want[1].tolist() == [0, R, R] and want[0][1] == 0 and want[0][2] == 0
    b = ssr.backend(stg, solver, noise, G)
    got = swr.fused(b, m0, J[None], T[None], tgt, R, (tk, jk), (th, hk), n_bins=7)
    good = swr.fused(b, m0, J[None], T[None], tgt, R, cur, fld, n_bins=7)
    b.close()
    _same(got, want)
    assert good[1].tolist() == [0, 0, 0] and np.array_equal(good[2][0], got[2][0])                     # condition 0 is untouched


# ------------------------------------------------------------------------------------------------
# 9. the Python method
# ------------------------------------------------------------------------------------------------
def test_python_method(stg):
    from spin_torque_gym_amd import physics
    m0, J, T, tgt, cur, fld = _three_phases()
    want = _phases_host(stg, "rk4", "brown")
    solver = physics.SimpleLLGSSolver(method="rk4", noise_model="brown", seed=SEED)
    res = solver.switching_statistics(m0, J[1], T[1], ssr.params(), PHASES_R, equilibrate=3e-11, relax=2e-11, n_bins=7, env_step=PHASES_STEP,
                                      current_knots=cur, field_knots=fld)
    assert set(res) == {"p_switch", "wer", "n_switched", "n_failed", "stderr", "hist", "bin_edges"}
    _same((res["n_switched"], res["n_failed"], res["hist"]), want)
    # current=None: the table replaces it
    res2 = solver.switching_statistics(m0, None, T[1], ssr.params(), PHASES_R, equilibrate=3e-11, relax=2e-11, n_bins=7, env_step=PHASES_STEP,
                                       current_knots=cur, field_knots=fld)
    assert np.array_equal(res2["hist"], res["hist"])
    # one table for all conditions, against switching_probability's replicated tables
    _, Jp, Tp, _ = ssr.conditions()
    one_cur = (cur[0][:, 1].copy(), cur[1][:, 1].copy())
    one_fld = (fld[0][:, 1].copy(), fld[1][:, 1].copy())
    R = 130
    new = solver.switching_statistics(m0, Jp, Tp, ssr.params(), R, current_knots=one_cur, field_knots=one_fld)
    old = solver.switching_probability(m0, Jp, Tp, ssr.params(), R, current_knots=one_cur, field_knots=one_fld)
    print(f"python method: p_switch {new['p_switch'].tolist()}")
    assert np.array_equal(new["p_switch"], old["n_switched"] / R) and np.array_equal(new["n_failed"], old["n_failed"])
    assert ((0 < old["n_switched"]) & (old["n_switched"] < R)).any()


# ------------------------------------------------------------------------------------------------
# 10. write footprint and checked errors
# ------------------------------------------------------------------------------------------------
def _raw_call(lib, b, arrays, g=G, R=130, trial0=0, stride=None, P=1, wave_phase=0, kj=5, kh=2, n_bins=7, null=()):
    """stg_switch_stats_wave through ctypes with Guarded outputs; `null`: names of pointer arguments passed as NULL"""
    ptr = lambda name: None if name in null else C.c_void_p(arrays[name].data_ptr())            # noqa: E731
    stride = trial0 + R if stride is None else stride
    return lib.stg_switch_stats_wave(None if "ctx" in null else b._ctx, g, R, trial0, stride, P, ptr("m0"), ptr("J"), ptr("T"), wave_phase,
                                     kj, ptr("tj"), ptr("jk"), kh, ptr("th"), ptr("hk"), ptr("cls"), 0, ptr("target"), 0.0, n_bins,
                                     ptr("n_switched"), ptr("n_failed"), ptr("hist"), None)


def test_write_footprint_and_refusals(stg):
    from spin_torque_gym_amd import _lib
    lib = _lib.load()
    m0, J, T, tgt = ssr.conditions()
    cur, fld = swr.knot_sets()["kj5-kh2"]
    R = 130
    b = ssr.backend(stg, "rk4", "brown", G)
    guards = {"n_switched": Guarded("n_switched", (G,), torch.float64), "n_failed": Guarded("n_failed", (G,), torch.float64),
              "hist": Guarded("hist", (G, 7), torch.float64, n_axis=0)}
    wave = swr.wave_dict(cur, fld)
    # (J and T hold two phases, so that P = 2 reads inside them)
    arrays = dict(m0=torch.from_numpy(m0.T.copy()).cuda(), J=torch.from_numpy(np.stack([J, J])).cuda(), T=torch.from_numpy(np.stack([T, T])).cuda(),
                  target=torch.from_numpy(tgt.T.copy()).cuda(), cls=torch.zeros(G, dtype=torch.uint8, device="cuda"),
                  tj=wave["current"][0].cuda(), jk=wave["current"][1].cuda(), th=wave["field"][0].cuda(), hk=wave["field"][1].cuda(),
                  **{k: v.interior for k, v in guards.items()})
    # every refusal: an error code, a message, nothing launched -- the arrays still hold their sentinels
    refusals = [(dict(null=(name,)), _lib.STG_E_INVALID) for name in ("ctx", "m0", "T", "target", "n_switched", "n_failed", "hist", "tj", "jk", "th", "hk")]
    refusals += [(kw, _lib.STG_E_INVALID) for kw in (
        dict(g=0), dict(R=-1), dict(P=0), dict(P=5), dict(n_bins=-1), dict(n_bins=65), dict(n_bins=0), dict(trial0=-1, stride=R),
        dict(stride=R - 1), dict(trial0=10, stride=R + 9), dict(R=2 ** 62, trial0=2 ** 62, stride=2 ** 63 - 1), dict(stride=2 ** 62),
        dict(wave_phase=-1), dict(wave_phase=1), dict(P=2, wave_phase=2), dict(kj=1), dict(kj=-2), dict(kj=33), dict(kh=1), dict(kh=-1), dict(kh=33),
        dict(kj=0, kh=0), dict(kj=0, null=("J",)), dict(P=2, null=("J",)))]
    for kw, code in refusals:
        rc = _raw_call(lib, b, arrays, **kw)
        assert rc == code and lib.stg_last_error(), (kw, rc)
        torch.cuda.synchronize()
        for v in guards.values():
            v.check(written=False)
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    pe = HipBackend(G, EnvConfig(solver="rk4", include_thermal_fluctuations=True, noise_model="brown", seed=SEED))
    assert _raw_call(lib, pe, arrays) == _lib.STG_E_STATE                                       # no parameters yet
    import spin_torque_gym_amd.devices as devices
    flat = stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", ssr.params()))
    block, dev_type, valid = devices.per_env_param_block(flat, G, {})
    pe.set_params_per_env(block, dev_type, valid)
    assert _raw_call(lib, pe, arrays) == _lib.STG_E_STATE and b"per-env" in lib.stg_last_error()
    pe.close()
    assert _raw_call(lib, b, arrays, R=0) == 0                                                   # valid, does nothing
    torch.cuda.synchronize()
    for v in guards.values():
        v.check(written=False)
    # the real thing: zeroed interiors, the counts of the host path, guards intact; J = NULL is fine with a current table and P = 1
    for v in guards.values():
        v.bits().zero_()
    assert _raw_call(lib, b, arrays, null=("J",)) == 0, lib.stg_last_error()
    torch.cuda.synchronize()
    m, failed = swr.host_path(stg, "rk4", "brown", m0, J[None], T[None], tgt, R, cur, fld)
    want = _host_counts(m, failed, tgt, R, n_bins=7)
    for v, y in zip(guards.values(), want):
        v.check_guards()
        assert np.array_equal(v.bits().cpu().numpy(), y), v.name
    # it ADDS: a second call doubles the counts; hist = NULL with n_bins = 0 leaves the histogram alone
    assert _raw_call(lib, b, arrays, n_bins=0, null=("hist", "cls")) == 0, lib.stg_last_error()
    torch.cuda.synchronize()
    for v, y, f in zip(guards.values(), want, (2, 2, 1)):
        v.check_guards()
        assert np.array_equal(v.bits().cpu().numpy(), f * y), v.name
    b.close()


# ------------------------------------------------------------------------------------------------
# 11. the NumPy statement under the oracle's normals
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise", swr.NUMPY_FORMS)
def test_counts_equal_the_numpy_statement(stg, oracle_mod, solver, noise):
    """R = 192, 7 bins: the fused counts against tests/brown_ref.py under the oracle's Philox stream -- no stg_solve_wave in between.  The
    statement's projections lie further than margin() from every decision (asserted here again; tests/test_switch_stats_wave_host.py)"""
    case = swr.numpy_case(oracle_mod, solver)
    assert case["distance"] > ssr.margin() and not case["counts"][1].any()
    m0, J, T, tgt = ssr.conditions()
    b = ssr.backend(stg, solver, noise, G)
    got = swr.fused(b, m0, J[None], T[None], tgt, swr.NUMPY_R, case["cur"], case["fld"], env_step=swr.NUMPY_ENV_STEP, n_bins=swr.NUMPY_BINS)
    b.close()
    print(f"{solver} {noise}: switched {got[0].tolist()} (NumPy {case['counts'][0].tolist()})")
    _same(got, case["counts"], solver)

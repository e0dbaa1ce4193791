"""stg_switch_stats off its defaults and against references that are not stg_solve: `pytest -m gpu`.  tests/test_gpu_switch_stats.py holds the
fused kernel to stg_solve + a host reduction at the default configuration, G = 3 and stream ids below 3000.  Here:

  2. classification against NumPy alone: every phase duration 0.0 or -0.0 (a trial's m is then the condition's m0 untouched, whatever
     double it holds), ~270 conditions x R = 65, one launch per (n_bins, threshold): projections on every bin edge and one ulp either
     side, +-1, +-(1 + 2^-52), +-3, +-1e300, +-0.0, +-inf, NaN, thresholds 0 / an edge / one ulp below it / NaN / +-inf, and witnesses
     whose outcome a fused multiply-add in the projection would change;
  3. counts against the CPU oracle (tests/switch_stats_ref.py oracle_path; conditioned: tests/test_switch_stats_oracle.py), integer for
     integer, four fixed-step forms x (defaults + three settings) x P in {1, 3}, RK45, and the Python method;
  4. the three off-default settings, the thermal field off and temperature 0 against stg_solve, all five forms;
  5. launch geometry: G = 4097 x R = 321 (cap 2, L = 3, a lone trial in the last round) and G = 12289 x R = 130 (cap 1, L = 3);
  6. stream ids beyond 2^33 and env_step across 2^32;
  7. class table edges: three classes, a class index beyond the table, cond_cls on a one-class context, an invalid class.

Sections 4-7 are exact against stg_solve (switch_stats_ref.host_path), as the header's stream rule promises.

Measured on an MI355X: the 37 cases take 4.0 s in all (the slowest, the classification test with its 53 launches, 0.34 s); every one of
the 34 oracle cases returned the oracle's counts.  profiles/NOTEBOOK.md (round 20) has the smallest oracle distances per form and the
seven deliberate miscounts each of which a test here catches."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import brown_ref as br
import switch_stats_ref as ssr
from helpers import Guarded

pytestmark = pytest.mark.gpu

G, SEED = ssr.G, ssr.SEED
FORMS = (("rk4", "brown"), ("euler", "brown"), ("rk4", "ou"), ("rk4", "white"), ("rk45", "white"))
RK45_CFG = dict(rtol=1e-5, atol=1e-8, max_attempts=100_000)


@pytest.fixture(scope="module")
def stg(oracle_mod):
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _same_counts(got, want, tag):
    for name, x, y in zip(("n_switched", "n_failed", "hist"), got, want):
        assert (x is None) == (y is None), (tag, name)
        assert x is None or np.array_equal(x, y), (tag, name, np.asarray(x).tolist()[:8], np.asarray(y).tolist()[:8])


# ------------------------------------------------------------------------------------------------
# 2. classification against NumPy alone
# ------------------------------------------------------------------------------------------------
E30 = 2.0 ** -30
# (m0 row, target row, threshold at which the header's value and a contracted one classify differently)
WITNESSES = (
    ((-1.0, 1.0 + E30, 0.0), (1.0, 1.0 - E30, 0.0), -2.0 ** -61),       # fma(my, ty, mx tx): -2^-60 in place of 0.0
    ((1.0 + E30, -1.0, 0.0), (1.0 - E30, 1.0, 0.0), -2.0 ** -61),       # fma(mx, tx, my ty)
    ((-1.0, 0.0, 1.0 + E30), (1.0, 1.0, 1.0 - E30), -2.0 ** -61),       # the second addition: fma(mz, tz, -1.0)
    ((-1.0, 1.0 + E30, 0.0), (1.0, 1.0 + E30, 0.0), 2.0 ** -29),        # upwards: 2^-29 + 2^-60 in place of 2^-29 -- switched only if fused
    ((-1.0, 0.0, 1.0 + E30), (1.0, 1.0, 1.0 + E30), 2.0 ** -29),
)
THRESHOLDS = (0.0, 0.5, float(np.nextafter(0.5, -np.inf)), float(np.linspace(-1.0, 1.0, 8)[5]), -1.0, float("nan"), float("inf"), float("-inf"),
              -2.0 ** -61, 2.0 ** -29)
N_BINS = (1, 2, 7, 63, 64)


def test_the_witnesses_tell_a_contracted_projection_apart():
    """exact rational arithmetic: for each witness, the header's value (every operation rounded) and each way of fusing a product into
    an addition -- of which at least one differs -- lie on opposite sides of the witness's threshold"""
    def rnd(x):
        return Fraction(float(x))                                       # Fraction -> float rounds to nearest even

    for m, t, thr in WITNESSES:
        m, t = [Fraction(x) for x in m], [Fraction(x) for x in t]
        px, py, pz = (rnd(a * b) for a, b in zip(m, t))
        header = rnd(rnd(px + py) + pz)
        fused = {rnd(rnd(px + m[1] * t[1]) + pz), rnd(rnd(m[0] * t[0] + py) + pz), rnd(rnd(px + py) + m[2] * t[2])}
        assert float(header) == float(ssr.proj(np.array([[float(x)] for x in m]), np.array([[float(x) for x in t]]))[0])
        other = [f for f in fused if f != header]
        assert len(other) == 1, (m, t, fused)
        assert (header > Fraction(thr)) != (other[0] > Fraction(thr)), (m, t, header, other)
        if hasattr(math, "fma"):
            mf, tf = [float(x) for x in m], [float(x) for x in t]
            ways = {math.fma(mf[1], tf[1], mf[0] * tf[0]) + mf[2] * tf[2], math.fma(mf[0], tf[0], mf[1] * tf[1]) + mf[2] * tf[2],
                    math.fma(mf[2], tf[2], mf[0] * tf[0] + mf[1] * tf[1])}
            assert ways == {float(f) for f in fused}


def _classification_conditions():
    """(m0 [G,3], target [G,3]): each projection below is formed as ((0 0) + (0 0)) + (v 1) = v unless the row says otherwise"""
    vals = []
    for nb in (64, 7):                                                  # the dyadic edges (those of 1 and 2 bins are among the 64's), and 7's
        for e in np.linspace(-1.0, 1.0, nb + 1):
            vals += [e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf)]
    for e in np.linspace(-1.0, 1.0, 64)[::8]:                           # a few of 63's
        vals += [e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf)]
    assert all(float(e) == -1.0 + k / 32.0 for k, e in enumerate(np.linspace(-1.0, 1.0, 65)))         # exact: dyadic
    vals += [1.0 + 2.0 ** -52, -(1.0 + 2.0 ** -52), 3.0, -3.0, 1e300, -1e300, 0.0, 2.0 ** -61, -2.0 ** -61, 2.0 ** -29, np.nextafter(2.0 ** -29, 1.0)]
    m0 = [(0.0, 0.0, float(v)) for v in vals]
    tg = [(0.0, 0.0, 1.0)] * len(vals)
    inf, nan = float("inf"), float("nan")
    rows = [((0.0, 0.0, 0.0), (-1.0, -1.0, -1.0)),                      # -0.0: every product and both sums
            ((0.0, 0.0, 1.0), (0.0, 0.0, inf)), ((0.0, 0.0, 1.0), (0.0, 0.0, -inf)), ((1.0, 0.0, 0.0), (inf, 0.0, 0.0)), ((0.0, -2.0, 0.0), (0.0, inf, 0.0)),
            ((nan, 0.0, 1.0), (0.0, 0.0, 1.0)), ((0.0, 0.0, nan), (0.0, 0.0, 1.0)), ((0.0, 0.0, 1.0), (inf, 0.0, 0.0)),        # NaN in m0; 0 inf
            ((1.0, 1.0, 0.0), (inf, -inf, 0.0)), ((0.3, 0.4, 0.5), (nan, 0.0, 0.0)),                                          # inf - inf; NaN target
            ((0.6, 0.0, 0.8), (0.6, 0.0, 0.8)), ((1e200, 1e200, 0.0), (1e200, -1e200, 0.0))]                                   # an ordinary row; inf - inf by overflow
    rows += [(m, t) for m, t, _ in WITNESSES]
    m0 += [r[0] for r in rows]
    tg += [r[1] for r in rows]
    return np.array(m0), np.array(tg)


def _raw(lib, b, arrays, g, R, P, threshold, n_bins, hist):
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())                                  # noqa: E731
    return lib.stg_switch_stats(b._ctx, g, R, 0, R, P, ptr(arrays["m0"]), ptr(arrays["J"]), ptr(arrays["T"]), None, 7, ptr(arrays["target"]),
                                threshold, n_bins, ptr(arrays["n_switched"]), ptr(arrays["n_failed"]), ptr(hist), None)


def test_classification_equals_numpy_when_every_phase_is_skipped(stg):
    from spin_torque_gym_amd import _lib
    lib = _lib.load()
    m0, tgt = _classification_conditions()
    g, R = len(m0), 65
    assert 250 <= g <= 350 and g > 64
    with np.errstate(all="ignore"):
        pr = ssr.proj(m0.T, tgt)
    assert np.isnan(pr).sum() >= 6 and np.isposinf(pr).sum() >= 2 and np.isneginf(pr).sum() >= 2 and (np.abs(pr[np.isfinite(pr)]) > 1.0).sum() >= 6
    assert any(v == 0.0 and np.signbit(v) for v in pr) and any(v == 0.0 and not np.signbit(v) for v in pr)
    T4 = np.zeros((4, g))
    T4[:, 1::2] = -0.0
    T4[1::2, ::3] = -0.0
    assert np.signbit(T4).any() and not np.signbit(T4).all() and (T4 == 0.0).all()
    b = ssr.backend(stg, "rk4", "brown", G)
    sw_g, fail_g = Guarded("n_switched", (g,), torch.float64), Guarded("n_failed", (g,), torch.float64)
    arrays = dict(m0=torch.from_numpy(m0.T.copy()).cuda(), J=torch.full((4, g), 1e-9, dtype=torch.float64, device="cuda"), T=torch.from_numpy(T4).cuda(),
                  target=torch.from_numpy(tgt.T.copy()).cuda(), n_switched=sw_g.interior, n_failed=fail_g.interior)
    launches = [(nb, thr, 1) for nb in N_BINS for thr in THRESHOLDS] + [(0, 0.0, 1), (7, 0.5, 4), (64, 0.0, 4)]
    flips = 0
    for nb, thr, P in launches:
        hist_g = Guarded("hist", (g, nb), torch.float64, n_axis=0) if nb else None
        for v in (sw_g, fail_g, hist_g):
            if v is not None:
                v.bits().zero_()
        assert _raw(lib, b, arrays, g, R, P, thr, nb, None if hist_g is None else hist_g.interior) == 0, lib.stg_last_error()
        torch.cuda.synchronize()
        with np.errstate(all="ignore"):
            want_sw = R * (pr > thr).astype(np.int64)
        for v in (sw_g, fail_g, hist_g):
            if v is not None:
                v.check_guards()
        got_sw = sw_g.bits().cpu().numpy()
        bad = np.nonzero(got_sw != want_sw)[0]
        assert bad.size == 0, (nb, thr, P, [(int(i), m0[i].tolist(), tgt[i].tolist(), float(pr[i]), int(got_sw[i])) for i in bad[:4]])
        assert not fail_g.bits().any().item(), (nb, thr, P)
        if nb:
            with np.errstate(all="ignore"):
                want_hist = np.zeros((g, nb), dtype=np.int64)
                want_hist[np.arange(g), ssr.bins(pr, nb)] = R
            got_hist = hist_g.bits().cpu().numpy()
            bad = np.nonzero((got_hist != want_hist).any(axis=1))[0]
            assert bad.size == 0, (nb, thr, P, [(int(i), float(pr[i]), got_hist[i].nonzero()[0].tolist(), int(ssr.bins(pr[i:i + 1], nb)[0])) for i in bad[:4]])
        flips += int(np.isnan(thr)) * int(want_sw.sum() == 0) + int(thr == float("-inf")) * int(want_sw.sum() == R * (g - int(np.isnan(pr).sum()) - int(np.isneginf(pr).sum())))
    assert flips == 2 * len(N_BINS)                                   # a NaN threshold switches nothing; -inf everything but NaN and -inf itself
    # what the set holds: strictness at the threshold, the edges on the upper side, NaN and the infinities in the outer bins
    i_half = int(np.nonzero(pr == 0.5)[0][0])
    assert pr[i_half + 1] == np.nextafter(0.5, 1.0) and pr[i_half + 2] == np.nextafter(0.5, 0.0)
    # (one ulp below +0.5 is still bin 48 of 64: proj + 1.0 rounds up to 1.5 -- the header's arithmetic, not the real line; below -0.5 it does not)
    assert ssr.bins(pr[i_half:i_half + 3], 64).tolist() == [48, 48, 48] and ssr.bins(pr[i_half:i_half + 3], 2).tolist() == [1, 1, 1]
    i_neg = int(np.nonzero(pr == -0.5)[0][0])
    assert ssr.bins(pr[i_neg:i_neg + 3], 64).tolist() == [16, 16, 15] and ssr.bins(pr[i_neg:i_neg + 3], 2).tolist() == [0, 0, 0]
    with np.errstate(all="ignore"):
        assert set(ssr.bins(pr[np.isnan(pr)], 7)) == {0} and set(ssr.bins(pr[np.isposinf(pr)], 7)) == {6} and set(ssr.bins(pr[np.isneginf(pr)], 7)) == {0}
    b.close()


# ------------------------------------------------------------------------------------------------
# 3. counts against the CPU oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise", ssr.ORACLE_FORMS)
def test_counts_equal_the_cpu_oracle(stg, solver, noise):
    """n_switched, n_failed and the 7-bin histogram are integer for integer those of the oracle's chain on the same streams, at the
    defaults and at the three settings, P = 1 and P = 3; the condition of the comparison (no oracle projection within 1e-8 of a
    decision) is asserted first, from the oracle alone"""
    m0, _, _, tgt = ssr.conditions()
    for k in (None, 0, 1, 2):
        b = ssr.backend(stg, solver, noise, G, **ssr.settings_cfg(k, noise))
        for P in (1, 3):
            case = ssr.oracle_case(stg, solver, noise, k, P)
            ssr.check_conditioned(case, solver, noise, k, P)
            got = ssr.fused(b, m0, case["J"], case["T"], tgt, ssr.ORACLE_R, env_step=ssr.ORACLE_ENV_STEP, n_bins=ssr.ORACLE_BINS)
            print(f"{solver} {noise} setting {k} P = {P}: switched {got[0].tolist()} (oracle {case['counts'][0].tolist()}), oracle distance {case['distance']:.2e}")
            _same_counts(got, case["counts"], (solver, noise, k, P))
        b.close()


@pytest.mark.parametrize("P", (1, 3))
def test_rk45_counts_equal_the_cpu_oracle(stg, P):
    """RK45 + white at the one unsaturated input there is (switch_stats_ref.RK45_J_SCALE: a current below the solver's gate): |proj| <
    0.99 in every condition, the conditioning rule holds, and the counts and the histogram are the oracle's"""
    m0, _, _, tgt = ssr.conditions()
    case = ssr.oracle_case(stg, "rk45", "white", None, P)
    ssr.check_conditioned(case, "rk45", "white", None, P)
    b = ssr.backend(stg, "rk45", "white", G)
    got = ssr.fused(b, m0, case["J"], case["T"], tgt, ssr.ORACLE_R, env_step=ssr.ORACLE_ENV_STEP, n_bins=ssr.ORACLE_BINS)
    b.close()
    _same_counts(got, case["counts"], ("rk45", P))


@pytest.mark.parametrize("noise", ("brown", "ou"))
def test_python_method_carries_its_settings_to_the_context(stg, noise):
    """switching_statistics on a solver constructed with gamma, max_step and correlation_time off their defaults, at 450 K, with
    equilibrate and relax: the oracle's counts of setting 1, P = 3"""
    from spin_torque_gym_amd import physics
    m0, Jp, Tp, _ = ssr.conditions()
    max_step, gamma, temperature = ssr.SETTINGS[1]
    case = ssr.oracle_case(stg, "rk4", noise, 1, 3)
    ssr.check_conditioned(case, "rk4", noise, 1, 3)
    assert np.array_equal(case["T"][0], np.full(G, 3e-11)) and np.array_equal(case["T"][2], np.full(G, 2e-11))
    solver = physics.SimpleLLGSSolver(method="rk4", noise_model=noise, seed=SEED, gamma=gamma, max_step=max_step, correlation_time=ssr.CORR_TIME)
    res = solver.switching_statistics(m0, Jp, Tp, ssr.params(), ssr.ORACLE_R, equilibrate=3e-11, relax=2e-11, temperature=temperature,
                                      env_step=ssr.ORACLE_ENV_STEP, n_bins=ssr.ORACLE_BINS)
    _same_counts((res["n_switched"], res["n_failed"], res["hist"]), case["counts"], noise)
    base = ssr.oracle_case(stg, "rk4", noise, None, 3)["counts"]
    assert not (np.array_equal(case["counts"][0], base[0]) and np.array_equal(case["counts"][2], base[2]))           # (not the defaults' counts)
    if noise == "ou":
        # the counts above do not feel correlation_time (the trials of a condition end 1e-10 apart); against condition 1's median on the
        # host path they do, and stg_solve is the reference there: the method's count is the host path's at 7e-13 and not at 1e-12
        _, _, _, tgt = ssr.conditions()
        R, cfg = ssr.ORACLE_R, ssr.settings_cfg(1, "ou")
        m, failed = ssr.host_path(stg, "rk4", "ou", m0, case["J"], case["T"], tgt, R, env_step=ssr.ORACLE_ENV_STEP, **cfg)
        thr = float(np.median(ssr.proj(m, np.repeat(tgt, R, axis=0))[R:2 * R]))
        want = ssr.host_counts(m, failed, tgt, R, threshold=thr)[0]
        res = solver.switching_statistics(m0, Jp, Tp, ssr.params(), R, equilibrate=3e-11, relax=2e-11, temperature=temperature,
                                          env_step=ssr.ORACLE_ENV_STEP, threshold=thr)
        assert np.array_equal(res["n_switched"], want) and want[1] == R // 2
        m1, f1 = ssr.host_path(stg, "rk4", "ou", m0, case["J"], case["T"], tgt, R, env_step=ssr.ORACLE_ENV_STEP, **dict(cfg, correlation_time=1e-12))
        assert not np.array_equal(m1, m)


# ------------------------------------------------------------------------------------------------
# 4. off-default configuration against stg_solve
# ------------------------------------------------------------------------------------------------
def _cfg_for(solver, noise, k):
    cfg = ssr.settings_cfg(k, noise)
    if solver == "rk45":
        cfg.update(RK45_CFG)
    return cfg


def _against_host_path(stg, solver, noise, J, T, R, cfg, tag, env_step=4, thresholds=(0.0,)):
    m0, _, _, tgt = ssr.conditions()
    m, failed = ssr.host_path(stg, solver, noise, m0, J, T, tgt, R, env_step=env_step, **cfg)
    b = ssr.backend(stg, solver, noise, G, **cfg)
    want = None
    for thr in thresholds + (float(np.median(ssr.proj(m, np.repeat(tgt, R, axis=0))[R:2 * R])),):
        want = ssr.host_counts(m, failed, tgt, R, threshold=thr, n_bins=7)
        got = ssr.fused(b, m0, J, T, tgt, R, env_step=env_step, threshold=thr, n_bins=7)
        print(f"{tag} threshold {thr:.6g}: switched {got[0].tolist()} (host {want[0].tolist()}), failed {got[1].tolist()}")
        _same_counts(got, want, (tag, thr))
    b.close()
    return m, failed, ssr.host_counts(m, failed, tgt, R, n_bins=7)


@pytest.mark.parametrize("k", (0, 1, 2))
@pytest.mark.parametrize("solver,noise", FORMS)
def test_off_default_settings_equal_stg_solve(stg, solver, noise, k):
    """max_step, gamma and temperature off their defaults (correlation_time for ou; rtol, atol and max_attempts for RK45), three phases,
    R = 130, 7 bins, thresholds 0 and condition 1's median: exact against the host path"""
    J, T = ssr.phases(k, 3)
    _, failed, want = _against_host_path(stg, solver, noise, J, T, 130, _cfg_for(solver, noise, k), f"{solver} {noise} setting {k}")
    assert not failed.any()
    if noise == "brown":
        assert ((0 < want[0]) & (want[0] < 130)).all()


@pytest.mark.parametrize("solver", ("rk4", "euler", "rk45"))
def test_thermal_field_off_equals_stg_solve(stg, solver):
    """include_thermal_fluctuations=False: the kernels without a field (THERMAL = false) -- every trial of a condition is the same
    solve, so the counts are 0 or R, and they are the host path's"""
    J, T = ssr.phases(None, 3)
    noise = "white" if solver == "rk45" else "brown"
    _, failed, want = _against_host_path(stg, solver, noise, J, T, 130, dict(include_thermal_fluctuations=False), f"{solver} thermal off")
    assert not failed.any() and set(want[0].tolist()) <= {0, 130} and (want[2].max(axis=1) == 130).all()
    # ... and the field is what was switched off: with it the histogram spreads
    if solver != "rk45":
        _, _, on = _against_host_path(stg, solver, noise, J, T, 130, {}, f"{solver} thermal on")
        assert (on[2].max(axis=1) < 130).all()


@pytest.mark.parametrize("solver", ("rk4", "euler", "rk45"))
def test_temperature_zero_with_the_field_on_equals_stg_solve(stg, solver):
    """temperature = 0.0, include_thermal_fluctuations=True: the fixed-step solvers reject every solve (the header's rule), so every
    trial is failed and classified by m0 (above the equator: not switched); RK45 draws its (zero) field and n_failed is stg_solve's"""
    m0, _, _, tgt = ssr.conditions()
    J, T = ssr.phases(None, 3)
    noise = "white" if solver == "rk45" else "brown"
    m, failed, want = _against_host_path(stg, solver, noise, J, T, 130, dict(temperature=0.0), f"{solver} 0 K")
    if solver != "rk45":
        assert failed.all() and np.array_equal(m, np.repeat(m0, 130, axis=0).T) and not want[0].any()
        assert np.array_equal(want[2], ssr.host_counts(np.repeat(m0, 130, axis=0).T, failed, tgt, 130, n_bins=7)[2])


# ------------------------------------------------------------------------------------------------
# 5. launch geometry beyond three conditions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,R,n_bins,plan", ((4097, 321, 64, (2, 3, 2)), (12289, 130, 0, (1, 3, 1))))
def test_many_conditions_with_looping_lanes_equal_stg_solve(stg, g, R, n_bins, plan):
    """G beyond STG_SWITCH_STATS_WAVES / 2 and beyond it: (cap, L, wavefronts per condition) = (2, 3, 2) with the 321st trial alone in
    the last round of the second wavefront, and (1, 3, 1) with two live lanes in the third round; m0, J and the target vary per
    condition (a condition that read its neighbour's row would count other trials); rk4 + brown, 20 ps pulses"""
    cap = max(1, ssr.WAVES // g)
    w1 = -(-R // 64)
    L = -(-w1 // cap)
    assert (cap, L, -(-w1 // L)) == plan and w1 > cap
    rng = np.random.default_rng(50 + g)
    mz, ph = rng.uniform(0.05, 0.35, g), rng.uniform(0.0, 2 * np.pi, g)
    s = np.sqrt(1.0 - mz * mz)
    m0 = np.stack([s * np.cos(ph), s * np.sin(ph), mz], axis=1)
    J = (br.SWITCH["J"] * rng.uniform(0.4, 0.7, g))[None]
    T = np.full((1, g), 2e-11)
    tgt = br.sphere(rng, g)
    tgt[::2] = [0.0, 0.0, -1.0]                                          # half on -z, where the field decides; the others anywhere on the sphere
    m, failed = ssr.host_path(stg, "rk4", "brown", m0, J, T, tgt, R, env_step=9)
    want = ssr.host_counts(m, failed, tgt, R, n_bins=n_bins)
    del m, failed
    torch.cuda.empty_cache()
    b = ssr.backend(stg, "rk4", "brown", G)
    got = ssr.fused(b, m0, J, T, tgt, R, env_step=9, n_bins=n_bins)
    b.close()
    bad = np.nonzero(got[0] != want[0])[0]
    assert bad.size == 0, (bad[:8].tolist(), got[0][bad[:8]].tolist(), want[0][bad[:8]].tolist())
    _same_counts(got, want, (g, R))
    assert not want[1].any() and 0.05 * g * R / 2 < want[0][::2].sum() < 0.95 * g * R / 2 and len(set(want[0].tolist())) > 20       # the field decides
    if n_bins:
        assert (got[2].sum(axis=1) == R).all() and np.count_nonzero(got[2], axis=1).mean() > 2


# ------------------------------------------------------------------------------------------------
# 6. stream ids and counter words
# ------------------------------------------------------------------------------------------------
def _per_condition_path(stg, solver, noise, m0, J, T, R, ids, steps, **cfg):
    """the header's stream rule with one stg_solve context of R problems per condition, created at env_id0 = ids[g]; phase p at counter
    word steps[p].  Returns (m_final [3, G R], failed [G R])."""
    ms, fs = [], []
    for g in range(m0.shape[0]):
        b = ssr.backend(stg, solver, noise, R, env_id0=int(ids[g]), **cfg)
        m = torch.from_numpy(np.repeat(m0[g:g + 1], R, axis=0).T.copy()).cuda()
        failed = torch.zeros(R, dtype=torch.bool, device="cuda")
        for p in range(J.shape[0]):
            if T[p, g] == 0.0:
                continue
            out = b.solve(m, torch.full((R,), float(J[p, g]), dtype=torch.float64), torch.full((R,), float(T[p, g]), dtype=torch.float64),
                          env_step=int(steps[p]))
            live = ~failed
            m = torch.where(live[None, :], out["m_final"], m)
            failed = failed | (live & (out["success"] == 0))
        torch.cuda.synchronize()
        ms.append(m.cpu().numpy())
        fs.append(failed.cpu().numpy())
        b.close()
    return np.concatenate(ms, axis=1), np.concatenate(fs)


@pytest.mark.parametrize("ctx_id0", (0, 2 ** 40))
def test_stream_ids_beyond_2_to_33(stg, ctx_id0):
    """trial0 = 2^33 + 5, trial_stride = 2^34: env_id0 + g * trial_stride + trial0 + r needs 64 bits -- against three stg_solve contexts
    created at those ids (and with the fused context itself created at env_id0 = 2^40)"""
    m0, J, T, tgt = ssr.conditions()
    R, trial0, stride = 130, 2 ** 33 + 5, 2 ** 34
    ids = [ctx_id0 + g * stride + trial0 for g in range(G)]
    m, failed = _per_condition_path(stg, "rk4", "brown", m0, J[None], T[None], R, ids, [2])
    want = ssr.host_counts(m, failed, tgt, R, n_bins=7)
    b = ssr.backend(stg, "rk4", "brown", G, env_id0=ctx_id0)
    got = ssr.fused(b, m0, J[None], T[None], tgt, R, trial0=trial0, trial_stride=stride, env_step=2, n_bins=7)
    _same_counts(got, want, ctx_id0)
    assert ((0 < want[0]) & (want[0] < R)).all()
    # the high words are part of the key: the same trials at the ids' low 32 bits are other trials
    low = ssr.fused(b, m0, J[None], T[None], tgt, R, trial0=5, trial_stride=stride % 2 ** 32 + R + 5, env_step=2, n_bins=7)
    b.close()
    assert not np.array_equal(low[2][0], want[2][0])                            # (condition 0: ids 5 + r against 2^33 + 5 + r)


def test_env_step_plus_phase_wraps_modulo_2_to_32(stg):
    """env_step = 2^32 - 2 with four phases: the counter words are 2^32 - 2, 2^32 - 1, 0, 1 (the header's stream rule, modulo 2^32)"""
    m0, Jp, Tp, tgt = ssr.conditions()
    J = np.stack([np.zeros(G), Jp, np.zeros(G), 0.5 * Jp])
    T = np.stack([np.full(G, 2e-11), Tp, np.full(G, 2e-11), np.full(G, 2e-11)])
    R, step = 130, 2 ** 32 - 2
    steps = [(step + p) % 2 ** 32 for p in range(4)]
    assert steps == [2 ** 32 - 2, 2 ** 32 - 1, 0, 1]
    m, failed = _per_condition_path(stg, "rk4", "brown", m0, J, T, R, [g * R for g in range(G)], steps)
    want = ssr.host_counts(m, failed, tgt, R, n_bins=7)
    b = ssr.backend(stg, "rk4", "brown", G)
    got = ssr.fused(b, m0, J, T, tgt, R, env_step=step, n_bins=7)
    b.close()
    _same_counts(got, want, "wrap")
    assert not want[1].any()


# ------------------------------------------------------------------------------------------------
# 7. class table edges
# ------------------------------------------------------------------------------------------------
def _class_case(stg, tables, cond_cls, ref_tables=None, ref_cls="same", R=130):
    m0, J, T, tgt = ssr.conditions()
    cond_cls = np.asarray(cond_cls, dtype=np.uint8)
    m, failed = ssr.host_path(stg, "rk4", "brown", m0, J[None], T[None], tgt, R, tables=tables if ref_tables is None else ref_tables,
                              cond_cls=cond_cls if isinstance(ref_cls, str) else ref_cls)
    want = ssr.host_counts(m, failed, tgt, R, n_bins=7)
    b = ssr.backend(stg, "rk4", "brown", G, tables, np.zeros(G, dtype=np.uint8) if len(tables) > 1 else None)      # (the context's own cls plays no part)
    got = ssr.fused(b, m0, J[None], T[None], tgt, R, cond_cls=torch.from_numpy(cond_cls), n_bins=7)
    b.close()
    _same_counts(got, want, cond_cls.tolist())
    return want


def test_class_table_edges(stg):
    """three volumes by cond_cls = [2, 0, 1]; a class index beyond the table reads class 0 (the reference passes the same byte through
    stg_solve's cls); cond_cls on a one-class context is ignored; a class whose parameter set is invalid fails every trial of its
    conditions and leaves the others alone"""
    from conftest import sot_default_params
    v = br.SWITCH["volume"]
    three = [ssr.params(), ssr.params(0.7 * v), ssr.params(1.3 * v)]
    a = _class_case(stg, three, [2, 0, 1])
    zero = _class_case(stg, three, [0, 0, 0])
    assert not np.array_equal(a[2][0], zero[2][0]) and not np.array_equal(a[2][2], zero[2][2]) and np.array_equal(a[2][1], zero[2][1])
    c = _class_case(stg, three, [200, 1, 0])
    assert np.array_equal(c[2][0], zero[2][0]) and np.array_equal(c[2][2], zero[2][2]) and not np.array_equal(c[2][1], zero[2][1])
    one = _class_case(stg, [ssr.params()], [2, 0, 1], ref_cls=None)
    _same_counts(one, zero, "one class")
    invalid = stg.flatten_params(stg.DeviceFactory().create_device("sot_mram", sot_default_params()))
    assert invalid.params_valid == 0
    d = _class_case(stg, [ssr.params(), invalid, ssr.params(0.7 * v)], [1, 0, 1])
    m0, _, _, tgt = ssr.conditions()
    assert d[1].tolist() == [130, 0, 130] and d[0][0] == 0 and d[0][2] == 0                      # failed, classified by m0 (above the equator)
    assert np.array_equal(d[2][1], zero[2][1]) and d[0][1] == zero[0][1]
    assert np.array_equal(d[2][[0, 2]], ssr.host_counts(np.repeat(m0[[0, 2]], 130, axis=0).T, np.ones(260, dtype=bool), tgt[[0, 2]], 130, n_bins=7)[2])

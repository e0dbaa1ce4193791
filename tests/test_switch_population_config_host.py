"""The CPU side of stg_switch_population's second test round (tests/test_gpu_switch_population_config.py; no GPU here):

  1. the class and index arithmetic of switch_population_cases.population_host_path -- trial0, dev0, a partial first device, strides,
     ids beyond 2^33 -- against switch_population_ref.trial_classes, touched and device_env on small integers;
  2. the classes of the nominal-class tests differ in a varied field AND in a field the draw does not vary but the solver reads;
  3. the conditioning of the oracle cases off the defaults (12 fixed-step cases = four forms x three settings, and RK45 at its own
     tolerances, all P = 3), on the devices drawn from the oracle's own normals: it is known here that the reference alone meets the
     rule, margin ssr.margin() = 1e-8.

Measured here (3.), smallest distance of any projection to a decision per form over its cases: rk4 + brown 2.19e-5 (setting 2), euler +
brown 7.37e-6 (setting 0), rk4 + ou 1.14e-4 and rk4 + white 1.14e-4 (setting 2), rk45 + white 9.60e-3; under brown 43 ... 108 of 192
trials switch.  No case needed another env_step or sigma (ORACLE_OVERRIDES is empty)."""
import numpy as np
import pytest

import switch_population_cases as spc
import switch_population_ref as spr
import switch_stats_ref as ssr


# ------------------------------------------------------------------------------------------------
# 1. index arithmetic
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Q,trial0,dev0", ((96, 3, 0, 0), (96, 3, 7, 2), (96, 3, 7, None), (100, 4, 10, 2), (100, 4, 10, 0), (50, 1, 13, 13),
                                             (30, 1000, 100, 0), (192, 3, 0, None), (5, 7, 6, None)))
def test_trial_classes_equal_the_references(R, Q, trial0, dev0):
    cls, d0, n_dev = spc.trial_classes(R, Q, trial0, dev0)
    first, last = spr.touched(trial0, R, Q)
    assert d0 == (first if dev0 is None else dev0) and n_dev == last - d0 + 1
    assert cls.dtype == np.uint8 and cls.shape == (R,)
    for G in (1, 3):
        flat, dev = spr.trial_classes(G, R, Q, n_dev, trial0=trial0, dev0=d0)
        assert np.array_equal(dev, cls)
        if G * n_dev <= 256:
            # the one-table layout of switch_population_ref puts condition g's device j in row g n_dev + j: the same device
            assert np.array_equal(flat.reshape(G, R), np.arange(G)[:, None] * n_dev + cls[None, :])
    # trial r of the range is ABSOLUTE trial trial0 + r, of device (trial0 + r) // Q: the first device partial when Q does not divide trial0
    assert cls[0] == trial0 // Q - d0 and cls[-1] == last - d0
    assert np.bincount(cls, minlength=n_dev)[first - d0] == min(R, Q - trial0 % Q)
    assert (np.diff(cls.astype(np.int64)) >= 0).all() and set(np.diff(cls.astype(np.int64)).tolist()) <= {0, 1}


def test_a_table_beyond_64_devices_is_refused():
    with pytest.raises(AssertionError):
        spc.trial_classes(195, 3, 0)                                               # 65 devices
    with pytest.raises(AssertionError):
        spc.trial_classes(96, 3, 7, dev0=3)                                        # trial 7 is device 2's
    assert spc.trial_classes(192, 3, 0)[2] == 64 == spc.MAX_CLASSES


@pytest.mark.parametrize("env_id0,stride,trial0,Q", ((0, 96, 0, 3), (37, 96, 0, 3), (0, 103, 7, 3), (0, 500, 7, 3), (0, 2 ** 34 + 3, 0, 3),
                                                     (11, 2 ** 35, 2 ** 33 + 5, 2)))
def test_contexts_sit_on_the_headers_stream_ids(env_id0, stride, trial0, Q):
    """env r of condition g's context is absolute trial trial0 + r: problem g stride + trial0 + r counted from env_id0; and the stream
    that draws a device is the one of the device's first trial"""
    for g in (0, 1, 2):
        e = spc.condition_env(env_id0, g, stride, trial0)
        assert e == env_id0 + g * stride + trial0
        for r in (0, 1, 95):
            d = int(spr.device_of(trial0 + r, Q))
            assert spr.device_env(env_id0, g, stride, d, Q) == e + r - (trial0 + r) % Q
            assert spr.device_env(env_id0, g, stride, d, Q) == spc.condition_env(env_id0, g, stride, d * Q)
    assert spc.condition_env(0, 2, 2 ** 34 + 3, 0) > 2 ** 33


def test_chains_put_the_pulse_where_it_is_watched():
    _, Jp, Tp, _ = ssr.conditions()
    J, T = spc.chain(Jp, Tp, 1, 0)
    assert J.shape == T.shape == (1, ssr.G) and np.array_equal(J[0], Jp) and np.array_equal(T[0], Tp)
    for w in (0, 1, 2):
        J, T = spc.chain(Jp, Tp, 3, w)
        assert np.array_equal(J[w], Jp) and np.array_equal(T[w], Tp) and not np.delete(J, w, axis=0).any() and (T > 0).all()
    for name in ("kj5-kh2", "kj5-kh0", "kj0-kh2"):
        cur, fld = spc.knots(name, "rk45", 2)
        assert (cur is None) == name.startswith("kj0") and (fld is None) == name.endswith("kh0")
        if cur is not None:
            assert cur[0].shape == (5, 2) and np.array_equal(cur[1], spc.knots(name, "rk4", 2)[0][1] * ssr.RK45_J_SCALE)
    assert spc.knots(None, "rk4", 2) == (None, None)


# ------------------------------------------------------------------------------------------------
# 2. the classes of the nominal-class tests
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stg(oracle_mod):
    import spin_torque_gym_amd as s
    return s


@pytest.mark.parametrize("solver", ("rk4", "rk45"))
def test_classes_differ_in_a_field_the_draw_does_not_vary(stg, solver):
    recs = ssr.flat_tables(stg, spc.class_tables(solver))
    assert len(recs) == 3 and all(r.params_valid == 1 for r in recs)
    fixed = "demag" if solver == "rk45" else "easy_axis"
    assert fixed not in spr.FIELDS
    for a in range(3):
        for b in range(a + 1, 3):
            assert recs[a].volume != recs[b].volume                                # a varied field
            assert list(getattr(recs[a], fixed)) != list(getattr(recs[b], fixed))  # one that is not
            for f in ("damping", "ms", "ku", "polarization"):
                assert getattr(recs[a], f) == getattr(recs[b], f)
    # the record a kernel would integrate on that took the five varied fields from class c and the rest from class 0
    mix = spc.mixed_record(recs[2], recs[0])
    assert mix.volume == recs[2].volume and list(getattr(mix, fixed)) == list(getattr(recs[0], fixed)) != list(getattr(recs[2], fixed))
    assert bytes(mix) != bytes(recs[2]) and bytes(mix) != bytes(recs[0])
    # the nominal record of a condition: its class, class 0 for a byte beyond the table and without cond_cls
    nom = spc.nominal_records(stg, spc.class_tables(solver), [2, 0, 200])
    assert [bytes(r) for r in nom] == [bytes(recs[2]), bytes(recs[0]), bytes(recs[0])]
    assert [bytes(r) for r in spc.nominal_records(stg, spc.class_tables(solver), None)] == [bytes(recs[0])] * 3


# ------------------------------------------------------------------------------------------------
# 3. the oracle cases off the defaults are conditioned
# ------------------------------------------------------------------------------------------------
def test_oracle_cases_are_the_issues():
    assert len(spc.ORACLE_CASES) == 13 and set(spc.ORACLE_CASES[:12]) == {(s, n, k) for s, n in ssr.ORACLE_FORMS for k in (0, 1, 2)}
    assert spc.ORACLE_CASES[12] == ("rk45", "white", None) and spc.oracle_cfg("rk45", "white", None) == dict(rtol=1e-5, atol=1e-8, max_attempts=100_000)
    for s, n, k in spc.ORACLE_CASES[:12]:
        cfg = spc.oracle_cfg(s, n, k)
        assert (cfg["max_step"], cfg["gamma"], cfg["temperature"]) == ssr.SETTINGS[k] and (cfg.get("correlation_time") == ssr.CORR_TIME) == (n == "ou")
    for key, (sigma, env_step) in spc.ORACLE_OVERRIDES.items():
        assert key in spc.ORACLE_CASES and all(spr.column_ok(sigma[:, g], spr.ORACLE_CLIP) for g in range(ssr.G))
        assert spr.VAR_STEP not in [(env_step + p) % 2 ** 32 for p in range(spc.ORACLE_P)]


@pytest.mark.parametrize("solver,noise,k", spc.ORACLE_CASES)
def test_oracle_cases_off_the_defaults_are_conditioned(stg, oracle_mod, solver, noise, k):
    """Every projection further than ssr.margin() from threshold 0 and from the inner edges of the 7 bins, no trial failed, and under
    brown 0 < n_switched < R -- on the oracle's own devices; the GPU test asserts the same on the devices the library dumps"""
    case = spc.oracle_case_cpu(stg, oracle_mod, solver, noise, k)
    print(f"{solver} {noise} setting {k}: switched {case['counts'][0].tolist()}, smallest distance to a decision {case['distance']:.2e} "
          f"(margin {ssr.margin():.0e}), devices with 0 / 1 / 2 / 3 switched trials {np.bincount(case['dev_switched'].reshape(-1), minlength=4).tolist()}")
    spc.check_conditioned(case, solver, noise, k)
    # the population matters: the nominal device's trials end elsewhere
    if solver != "rk45":
        nominal = ssr.oracle_case(stg, solver, noise, k, spc.ORACLE_P)
        assert not np.array_equal(case["proj"], nominal["proj"])

"""The condition under which test_gpu_wave_config.py and test_gpu_knots_config.py may hold the waveform kernels to the project's tolerances (TOL_RK4 = 1e-10, x 50 with
the thermal field): every restatement case must be well conditioned.  Checked here on the CPU, on the same cases
(tests/wave_config_cases.py): when the largest component of every start row moves by one ulp, the restatement's own answer has the same
flags and sub-step counts and moves by less than tolerance / 100, in every step.  The env-level cases also show here that the 20-seed
bound of their redraw holds for the committed seeds with no env left out.  An input that fails this is to be replaced, not met with a
wider tolerance."""
import numpy as np
import pytest

import wave_config_cases as wcc

SOLVE_CASES, STEP_CASES = wcc.solve_cases(), wcc.step_cases()


@pytest.mark.parametrize("name", [c["name"] for c in SOLVE_CASES])
def test_solve_case_moves_less_than_a_hundredth_of_the_tolerance_per_ulp(oracle_mod, name):
    c = wcc.case(SOLVE_CASES, name)
    p, base = wcc.solve_ref(c, oracle_mod)
    _, moved = wcc.solve_ref(c, oracle_mod, ulp=True)
    tol = wcc.tol_for(c["method"], c["noise"] is not None)
    d = float(np.abs(base["m_final"] - moved["m_final"]).max())
    print(f"{name}: |dm| per ulp of m0 = {d:.3e} (tolerance / 100 = {tol / 100:.1e})")
    assert base["success"].all() and moved["success"].all() and np.array_equal(base["n_steps"], moved["n_steps"])
    assert not np.array_equal(base["m_final"], moved["m_final"])             # (the ulp did reach the solver)
    assert d < tol / 100, (name, d)


@pytest.mark.parametrize("name", [c["name"] for c in STEP_CASES])
def test_step_case_moves_less_than_a_hundredth_of_the_tolerance_per_ulp(oracle_mod, name):
    c = wcc.case(STEP_CASES, name)
    p, base = wcc.step_ref(c, oracle_mod)              # (raises if no seed of 20 keeps every alignment away from the threshold)
    _, moved = wcc.step_ref(c, oracle_mod, ulp=True)
    tol = wcc.tol_for(c["method"], c["noise"] is not None)
    worst = 0.0
    for k, (a, b) in enumerate(zip(base, moved)):
        assert (np.abs(a["alignment"] - p["cfg"]["success_threshold"]) > 1e-6).all(), (name, k)
        for key in ("status", "terminated", "truncated", "n_sub", "step_count"):
            assert np.array_equal(a[key], b[key]), (name, k, key)
        worst = max(worst, float(np.abs(a["m"] - b["m"]).max()))
    print(f"{name}: |dm| per ulp of m0 = {worst:.3e} (tolerance / 100 = {tol / 100:.1e})")
    assert not np.array_equal(base[0]["m"], moved[0]["m"])
    assert worst < tol / 100, (name, worst)


@pytest.mark.parametrize("method,noise", wcc.SHAPED_DIRECT)
def test_shaped_case_moves_less_than_a_hundredth_of_the_tolerance_per_ulp(oracle_mod, method, noise):
    _, base = wcc.shaped_ref(method, noise, oracle_mod)
    _, moved = wcc.shaped_ref(method, noise, oracle_mod, ulp=True)
    tol = wcc.tol_for(method, noise is not None)
    worst = 0.0
    for k, (a, b) in enumerate(zip(base, moved)):
        for key in ("status", "terminated", "truncated", "n_sub", "step_count"):
            assert np.array_equal(a[key], b[key]), (method, noise, k, key)
        worst = max(worst, float(np.abs(a["m"] - b["m"]).max()))
    print(f"shaped {method} {noise}: |dm| per ulp of m0 = {worst:.3e} (tolerance / 100 = {tol / 100:.1e})")
    assert not np.array_equal(base[0]["m"], moved[0]["m"])
    assert worst < tol / 100, (method, noise, worst)


@pytest.mark.parametrize("method,noise", wcc.SHAPED_DIRECT)
def test_knots_case_moves_less_than_a_hundredth_of_the_tolerance_per_ulp(oracle_mod, method, noise):
    """the cases test_gpu_knots_config.py compares with the restatement directly (actions that carry the knot amplitudes)"""
    p, base = wcc.knots_ref(method, noise, oracle_mod)
    _, moved = wcc.knots_ref(method, noise, oracle_mod, ulp=True)
    tol = wcc.tol_for(method, noise is not None)
    worst = 0.0
    for k, (a, b) in enumerate(zip(base, moved)):
        assert (np.abs(a["alignment"] - p["cfg"]["success_threshold"]) > 1e-6).all(), (method, noise, k)
        for key in ("status", "terminated", "truncated", "n_sub", "step_count"):
            assert np.array_equal(a[key], b[key]), (method, noise, k, key)
        worst = max(worst, float(np.abs(a["m"] - b["m"]).max()))
    near = min(float(np.abs(a["alignment"] - p["cfg"]["success_threshold"]).min()) for a in base)
    print(f"knots {method} {noise}: |dm| per ulp of m0 = {worst:.3e} (tolerance / 100 = {tol / 100:.1e}), nearest alignment {near:.1e} from the threshold")
    assert not np.array_equal(base[0]["m"], moved[0]["m"])
    assert worst < tol / 100, (method, noise, worst)


@pytest.mark.parametrize("method,noise", wcc.SHAPED_DIRECT)
def test_knots_case_is_not_vacuous(oracle_mod, method, noise):
    """what the knots case is there to exercise is in it: amplitudes on both sides of the limit, currents at max_current, the three
    classes, and at every step envs that terminate next to envs that do not; every env is solved and the last step truncates them all"""
    p, refs = wcc.knots_ref(method, noise, oracle_mod)
    amp = np.abs(p["acts"][:, :, 2:].astype(np.float64))
    beyond = float((amp > p["limit"]).mean())
    print(f"knots {method} {noise}: {100 * beyond:.0f} % of the amplitudes beyond the limit, terminated per step "
          f"{[int(r['terminated'].sum()) for r in refs]} of {wcc.N}")
    assert p["acts"].shape == (wcc.K_SHAPED, wcc.N, 2 + wcc.P_KNOTS) and p["limit"] == wcc.KNOT_LIMIT <= 0.25
    assert 0.2 <= beyond <= 0.6
    assert p["tau"][0] == 0.0 and p["tau"][-1] == 1.0 and (np.diff(p["tau"]) > 0).all()
    assert set(p["cls"].tolist()) == {0, 1, 2}
    for k, r in enumerate(refs):
        assert (r["status"] == 0).all(), k
        assert (np.abs(r["J"]) == p["cfg"]["max_current"]).any() and (r["J"] == 0.0).any(), k
        assert 0 < int(r["terminated"].sum()) < wcc.N, k
        # the tables are those of the clamped amplitudes: no knot value beyond limit * max_current, some exactly there
        assert (np.abs(p["cur"][k][1]) <= p["limit"] * p["cfg"]["max_current"]).all() and (np.abs(p["cur"][k][1]) == p["limit"] * p["cfg"]["max_current"]).any(), k
    assert refs[-1]["truncated"].all() and not refs[0]["truncated"].all()
    # off the defaults: a parse against the default limits gives other tables
    import knots_ref as kr
    J, T, s = kr.parse_np(p["acts"][0], 2e6, 5e-9, 1.0)
    assert not np.array_equal(J, refs[0]["J"]) and (np.abs(s) > p["limit"]).any()

"""The condition under which tests/test_gpu_brown_config.py may hold the kernels under noise_model='brown' to TOL_RK4 = 1e-10: every
case of tests/brown_config_cases.py must be well conditioned, and none may be vacuous.  Checked here on the CPU, on the same inputs,
with the oracle's own stream in the place of the device's normals:

  * when the largest component of every start row moves by one ulp, and when every normal moves by one ulp, the restatement's answer
    keeps its flags, status bytes and sub-step counts and moves by at most tolerance / 100 = 1e-12, in every step, for every drive
    (rectangular, per-env tables, the pulse shape, the knot amplitudes) and for the K = 3 chain with autoreset;
  * the two references (tests/brown_ref.py and the C oracle's fed-normals step) agree within 1e-12 on the rectangular chain;
  * premises: lanes with dt = T / 100 and, at max_step = 3e-13, lanes where max_step decides (dt in [max_step, 1.01 max_step)); the
    clamps of the episode fields bite on at least a fifth of the actions; the field moves m by more than 1e-3; the K = 3 chain resets
    envs inside the launch; under the device torque model every class's own torque changes its lanes.

An input that fails this is to be replaced (shorter pulses, a larger volume), not met with a wider tolerance.

Measured here, worst over all cases, |dm| per ulp of the start rows / per ulp of the normals: rectangular chain 1.0e-13 / 5.8e-14,
K = 3 with autoreset 8.7e-14 / 1.1e-13, per-env tables 9.3e-14 / 5.5e-14, pulse shape 1.4e-13 / 6.2e-14, knot amplitudes 7.9e-14 /
6.3e-14, device torque model 3.9e-14 / 4.3e-14; restatement against the fed-normals oracle 4.6e-14.  The field moves m by 6e-3 ...
1.5 (volume 1e-23; at 1e-26 it moves m by 1.8 and the chains amplify an ulp to 1e-11)."""
import numpy as np
import pytest

import brown_config_cases as bcc
import brown_ref as br
import wave_step_ref as wsr

CASES, DEVICE_CASES = bcc.cases(), bcc.device_cases()
BOUND = bcc.TOL / 100


def _worst(base, moved, tag):
    worst = 0.0
    for k, (a, b) in enumerate(zip(base, moved)):
        for key in ("status", "terminated", "truncated", "n_sub", "step_count"):
            assert np.array_equal(a[key], b[key]), (tag, k, key)
        worst = max(worst, float(np.abs(a["m"] - b["m"]).max()))
    return worst


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_case_premises(oracle_mod, name):
    c = bcc.case(CASES, name)
    p = bcc.problem(c)
    cfg, n = p["cfg"], c["n"]
    assert cfg["max_step"] != 1e-12 and cfg["gamma"] != 2.21e5 and cfg["temperature"] not in (300.0, 250.0) and cfg["max_steps"] == 3
    raw_j = np.abs(p["acts"][:, :, 0].astype(np.float64))
    clamped = float((raw_j > cfg["max_current"]).mean())
    for k in range(bcc.K_MANY):
        J, T = wsr.parse_actions(p["acts"][k], cfg["max_current"], cfg["max_duration"])
        ns, dt = br.substeps(T, cfg["max_step"])
        by_t, by_ms = dt == T / 100, ns > 100
        if n > 1:
            assert by_t.any(), (name, k)
            assert set(p["cls"].tolist()) == {0, 1, 2} and (np.abs(J) == cfg["max_current"]).any()
        if cfg["max_step"] < 1e-12:
            assert (dt[by_ms] >= cfg["max_step"]).all() and (dt[by_ms] < 1.01 * cfg["max_step"]).all() and (dt[by_ms] < T[by_ms] / 100).all()
            # (the one-lane case: max_step decides in its first step, T / 100 in a later one)
            assert ((by_ms.any() if k == 0 else by_t.any() if k == 1 else True) if n == 1 else (by_t.sum() >= 10 and by_ms.sum() >= 10)), (name, k)
        else:
            assert (dt < cfg["max_step"]).all() and (np.abs(dt - 1e-12) > 4e-14).all() and not by_ms.any()
    if n > 1:
        assert 0.2 <= clamped <= 0.35, (name, clamped)                        # the clamp of max_current bites on a quarter of the actions
        assert len(np.unique(p["state"]["target"], axis=0)) == 5 and set(p["state"]["step_count"].tolist()) == {0, 1}
    if c["f64"]:
        assert p["acts"].dtype == np.float64 and p["kacts"].dtype == np.float64
    # the field moves the states: the same chain with strength 0
    normals_of = bcc.oracle_normals(oracle_mod, n)
    refs = bcc.run_chain(c, p, oracle_mod, normals_of)
    off = bcc.run_chain(c, p, oracle_mod, normals_of, field_on=False)
    moved = min(float(np.abs(a["m"] - b["m"]).max()) for a, b in zip(refs, off))
    print(f"{name}: {100 * clamped:.0f} % of the currents beyond max_current, the field moves m by {moved:.2e}")
    assert moved > 1e-3, (name, moved)
    assert all((r["status"] == 0).all() for r in refs)


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_rectangular_chain_per_ulp_and_against_the_oracle(oracle_mod, name):
    c = bcc.case(CASES, name)
    p = bcc.problem(c)
    normals_of = bcc.oracle_normals(oracle_mod, c["n"])
    base = bcc.run_chain(c, p, oracle_mod, normals_of)
    d_m0 = _worst(base, bcc.run_chain(c, p, oracle_mod, normals_of, ulp=True), (name, "m0"))
    d_z = _worst(base, bcc.run_chain(c, p, oracle_mod, normals_of, ulp_normals=True), (name, "normals"))
    ora = bcc.run_chain(c, p, oracle_mod, normals_of, engine="oracle")
    d_o = _worst(base, ora, (name, "oracle"))
    for a, b in zip(base, ora):
        assert np.allclose(a["obs"], b["obs"], rtol=3e-7, atol=1e-9) and np.allclose(a["reward"], b["reward"], rtol=1e-10, atol=1e-10)
        assert np.allclose(a["energy"], b["energy"], rtol=1e-13, atol=0.0) and np.allclose(a["total_energy"], b["total_energy"], rtol=1e-13, atol=0.0)
    near = min(float(np.abs(r["alignment"] - p["cfg"]["success_threshold"]).min()) for r in base)
    print(f"{name}: |dm| per ulp of m0 {d_m0:.2e}, per ulp of the normals {d_z:.2e}, restatement - oracle {d_o:.2e} (bound {BOUND:.0e}); "
          f"nearest alignment {near:.1e} from the threshold")
    assert c["n"] == 1 or (d_m0 > 0.0 and d_z > 0.0)                          # (the ulps did reach the solver)
    assert d_m0 <= BOUND and d_z <= BOUND and d_o <= BOUND, (name, d_m0, d_z, d_o)


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_fused_chain_with_autoreset_per_ulp(oracle_mod, name):
    """K = 3 with autoreset: resets fall inside the launch (max_steps = 3 with envs that start at step count 1; terminations at the
    threshold 0.6), and the chain through them is as well conditioned as the plain one"""
    c = bcc.case(CASES, name)
    p = bcc.problem(c)
    kw = dict(K=bcc.K_MANY, autoreset=True, reset_of=bcc.oracle_resets(p))
    normals_of = bcc.oracle_normals(oracle_mod, c["n"])
    base = bcc.run_chain(c, p, oracle_mod, normals_of, **kw)
    d_m0 = _worst(base, bcc.run_chain(c, p, oracle_mod, normals_of, ulp=True, **kw), (name, "m0"))
    d_z = _worst(base, bcc.run_chain(c, p, oracle_mod, normals_of, ulp_normals=True, **kw), (name, "normals"))
    ora = bcc.run_chain(c, p, oracle_mod, normals_of, engine="oracle", **kw)
    d_o = _worst(base, ora, (name, "oracle"))
    resets = [int(r["done"].sum()) for r in base]
    print(f"{name}: K = 3 with autoreset, resets per step {resets}: |dm| per ulp of m0 {d_m0:.2e}, of the normals {d_z:.2e}, restatement - oracle {d_o:.2e}")
    if c["n"] > 1:
        assert resets[0] > 0 and resets[1] > resets[0] // 2 and sum(resets[:2]) < 2 * c["n"]         # resets inside the launch, not everywhere
        assert base[1]["truncated"].any() and base[0]["terminated"].any() and not base[0]["truncated"].any()
    assert d_m0 <= BOUND and d_z <= BOUND and d_o <= BOUND, (name, d_m0, d_z, d_o)


@pytest.mark.parametrize("drive", ("wave", "shaped", "knots"))
@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_waveform_chain_per_ulp(oracle_mod, name, drive):
    c = bcc.case(CASES, name)
    p = bcc.problem(c)
    normals_of = bcc.oracle_normals(oracle_mod, c["n"])
    base = bcc.run_chain(c, p, oracle_mod, normals_of, drive=drive)
    rect = bcc.run_chain(c, p, oracle_mod, normals_of)
    d_m0 = _worst(base, bcc.run_chain(c, p, oracle_mod, normals_of, drive=drive, ulp=True), (name, drive, "m0"))
    d_z = _worst(base, bcc.run_chain(c, p, oracle_mod, normals_of, drive=drive, ulp_normals=True), (name, drive, "normals"))
    print(f"{name} {drive}: |dm| per ulp of m0 {d_m0:.2e}, per ulp of the normals {d_z:.2e} (bound {BOUND:.0e})")
    assert all((r["status"] == 0).all() for r in base)
    assert float(np.abs(base[0]["m"] - rect[0]["m"]).max()) > 1e-6                       # the tables do drive the solve
    if drive == "knots" and c["n"] > 1:
        beyond = float((np.abs(p["kacts"][:, :, 2:].astype(np.float64)) > p["limit"]).mean())
        assert 0.2 <= beyond <= 0.6                                                      # the amplitude clamp is at work
    assert (0.0 < d_m0 or c["n"] == 1) and d_m0 <= BOUND and d_z <= BOUND, (name, drive, d_m0, d_z)


@pytest.mark.parametrize("name", [c["name"] for c in DEVICE_CASES])
def test_device_torque_chain_per_ulp_and_every_class_at_work(oracle_mod, name):
    """torque_model='device' on the fed-normals oracle, J != 0 in every lane: the SOT and the VCMA lanes take their own torque (they move
    away from the reference torque model's answer by far more than the tolerance), the STT lanes keep the reference RHS bit for bit"""
    c = bcc.case(DEVICE_CASES, name)
    p = bcc.problem(c)
    normals_of = bcc.oracle_normals(oracle_mod, c["n"])
    kw = dict(engine="oracle", torque_model=1)
    base = bcc.run_chain(c, p, oracle_mod, normals_of, **kw)
    d_m0 = _worst(base, bcc.run_chain(c, p, oracle_mod, normals_of, ulp=True, **kw), (name, "m0"))
    d_z = _worst(base, bcc.run_chain(c, p, oracle_mod, normals_of, ulp_normals=True, **kw), (name, "normals"))
    ref_model = bcc.run_chain(c, p, oracle_mod, normals_of, engine="oracle", torque_model=0)
    d = np.abs(base[0]["m"] - ref_model[0]["m"]).max(axis=1)
    cls = p["cls"]
    print(f"{name}: |dm| per ulp of m0 {d_m0:.2e}, of the normals {d_z:.2e}; device - reference torque model, median per class: "
          f"STT {np.median(d[cls == 0]):.1e}, SOT {np.median(d[cls == 1]):.1e}, VCMA {np.median(d[cls == 2]):.1e}")
    J, _ = wsr.parse_actions(p["acts"][0], p["cfg"]["max_current"], p["cfg"]["max_duration"])
    assert (np.abs(J) > 1e-12).all() and (d[cls == 0] == 0.0).all()
    assert (d[cls == 1] > 1e-8).all() and (d[cls == 2] > 1e-8).all()
    assert all((r["status"] == 0).all() for r in base)
    assert 0.0 < d_m0 <= BOUND and d_z <= BOUND, (name, d_m0, d_z)


@pytest.mark.parametrize("n", (65537, 90112))
def test_launch_form_slices_per_ulp(oracle_mod, n):
    """the three slices tests/test_gpu_noise_launch_forms.py holds to 1e-10 at the hybrid sizes: one RK4 step of up to 0.3 ns under the
    Brown field at the default configuration (max_step 1e-12, 300 K), on the oracle's stream"""
    import waveform_ref
    m0, tgt, acts = bcc.launch_inputs(n, n)
    worst, moved = 0.0, 1.0
    for s0 in bcc.launch_slices(n):
        z = np.stack([waveform_ref.normals(oracle_mod, 3, s0 + i, 0, 300) for i in range(64)])
        base = bcc.launch_slice_ref(oracle_mod, m0, tgt, acts[0], s0, z)
        for kw in (dict(ulp=True), dict(ulp_normals=True)):
            other = bcc.launch_slice_ref(oracle_mod, m0, tgt, acts[0], s0, z, **kw)
            assert np.array_equal(base["status"], other["status"]) and np.array_equal(base["n_sub"], other["n_sub"])
            worst = max(worst, float(np.abs(base["m"] - other["m"]).max()))
        off = bcc.launch_slice_ref(oracle_mod, m0, tgt, acts[0], s0, 0.0 * z)
        moved = min(moved, float(np.abs(base["m"] - off["m"]).max()))
        assert (base["status"] == 0).all() and base["n_sub"].max() <= 300
    first, mid, _ = bcc.launch_slices(n)
    assert (acts[0, first:first + 64, 1] == acts[0, :, 1].max()).all() and (acts[0, mid:mid + 64, 1] == acts[0, :, 1].min()).all()
    print(f"launch-form slices at {n}: |dm| per ulp {worst:.2e} (bound {BOUND:.0e}), the field moves m by {moved:.2e}")
    assert worst <= BOUND and moved > 1e-3

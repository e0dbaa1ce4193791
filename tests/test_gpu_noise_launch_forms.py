"""Every launch form of the fixed-step env step under the two thermal fields that draw three normals per sub-step -- noise_model='ou'
and 'brown' -- on the GPU: `pytest -m gpu`.  csrc/stg_launch_plan.hpp promises that results never depend on the plan; for these fields
the suite had checked that up to 4 226 envs ('ou') and 320 envs ('brown') only, and never in the RK4 hybrid launch (65 537 ... 90 112
envs: producer / consumer pairs for the longest blocks -- whose chunk holds SHARED_SUBS3 = 8 sub-steps of 3 normals under these fields,
where the white field has 2 sub-steps of 12 -- and two inline-normal blocks in every other workgroup).

  hybrid sizes       65 537 (the smallest hybrid launch), 90 112 (the largest: 2048 - 22 * 64 = 640 pairs = STG_HYBRID_MIN_PAIRS_RK4) and
                     90 113 (the first size past it), one RK4 step, T <= 0.3 ns, under 'ou' (correlation time 3e-12) and 'brown':
                     env_steps == n, every output bit and the state equal to the identity schedule's (lane_sort=False) and to
                     wave_spec=False (all inline);
  65 537 extras      a two-class table with skip_done over two steps; K = 2 fused with float64 actions
                     (tests/test_gpu_fullsize.py: test_hybrid_launch_with_class_table_skip_done_and_fused_steps, there with the white field);
  values             at 65 537 and 90 112 under 'brown': three 64-env slices (the first wavefront with the longest durations, one in the
                     middle with the shortest, the end with the ragged tail) against tests/brown_ref.py fed the device's normals,
                     within TOL_RK4 = 1e-10 (tests/test_brown_config_conditioning.py: the slices move by 7e-14 per ulp);
  small forms        N = 130 and N = 4 226: wave_spec {forced on, off} x lane_sort {on, off}, both fields, both methods: bit-identical
                     (tests/test_gpu_brown.py: test_wave_specialised_pairs_bit_identical has wave_spec only, 'brown' only, N = 320).

Volume 1e-23 with currents scaled by the volume ratio (tests/brown_config_cases.py): the Brown field moves m by 1e-2 and more."""
import numpy as np
import pytest
import torch

import brown_config_cases as bcc
from conftest import stt_default_params, vcma_default_params

pytestmark = pytest.mark.gpu

TOL_RK4 = 1e-10
NOISES = ("ou", "brown")
CORR_TIME = 3e-12
SEED = 3


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _kw(noise, solver="rk4", **over):
    return dict(dict(device_params=stt_default_params(volume=bcc.VOL), include_thermal_fluctuations=True, solver=solver, seed=SEED, noise_model=noise,
                     correlation_time=CORR_TIME, max_current=bcc.LF_MAX_CURRENT), **over)


def _run(stg, n, m0, tgt, acts, cls=None, **kw):
    """steps the env through `acts`; the device tensors of every step (cloned), the work counters and the backend's plan-free state"""
    env = stg.SpinTorqueVecEnv(n, diagnostics=True, class_index=cls, **kw)
    env.reset(options={"initial_state": m0, "target_state": tgt})
    rec = []
    for a in acts:
        o, r, te, tr, info = env.step(torch.from_numpy(a))
        st = env.get_state()
        rec.append(dict(obs=o.clone(), reward=r.clone(), reward_f64=info["reward_f64"].clone(), term=te.clone(), trunc=tr.clone(),
                        status=info["status"].clone(), energy=info["energy"].clone(), m=st["m"].clone(), step_count=st["step_count"].clone(),
                        etot=st["total_energy"].clone(), rng_step=st["rng_step"].clone(), done=st["done"].clone()))
    counters = env.backend.counters()
    place = env.backend.placement(0)
    counters["launch"] = (place["workgroups"], place["waves_per_workgroup"])        # (the form the last launch took)
    env.close()
    return rec, counters


def _bits(t):
    t = t.contiguous()
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64, torch.bool: torch.uint8}.get(t.dtype, t.dtype))


def _assert_same_bits(a, b, tag):
    for k, (x, y) in enumerate(zip(a, b)):
        for key in x:
            bad = int((_bits(x[key]) != _bits(y[key])).sum())
            assert bad == 0, (tag, k, key, bad)


# ------------------------------------------------------------------------------------------------
# the hybrid sizes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("n", (65537, 90112, 90113))
def test_hybrid_sizes_equal_the_identity_schedule_and_all_inline(stg, oracle_mod, n, noise):
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    m0, tgt, acts = bcc.launch_inputs(n, n)
    kw = _kw(noise)
    a, ca = _run(stg, n, m0, tgt, acts, **kw)
    assert ca["env_steps"] == n and ca["noop_steps"] == 0, (n, noise, ca)
    assert bool((a[0]["status"] == 0).all()) and bool((a[0]["rng_step"] == 1).all())
    # the hybrid launch is 1024 two-wavefront workgroups; one size further it is not taken
    form_a = ca.pop("launch")
    print(f"{n} envs under {noise!r}: {form_a[0]} workgroups of {form_a[1]} wavefronts")
    assert (form_a == (1024, 2)) == (n <= 90112), (n, noise, form_a)
    for form, over in (("identity schedule", dict(lane_sort=False)), ("all inline", dict(wave_spec=False))):
        b, cb = _run(stg, n, m0, tgt, acts, **dict(kw, **over))
        assert cb.pop("launch") != (1024, 2), (n, noise, form)
        assert ca == cb, (n, noise, form, ca, cb)
        _assert_same_bits(a, b, (n, noise, form))
    assert float((a[0]["m"] - torch.from_numpy(m0.T).cuda()).abs().max()) > 1e-2
    if noise != "brown" or n == 90113:
        return
    # values: three slices against the restatement fed the device's normals (keyed by the global env index: a 64-env context at env_id0)
    m = a[0]["m"].cpu().numpy().T
    status = a[0]["status"].cpu().numpy()
    for s0 in bcc.launch_slices(n):
        small = HipBackend(64, EnvConfig(solver="rk4", include_thermal_fluctuations=True, noise_model="brown", seed=SEED), 0, s0)
        z = small.thermal_normals(0, 0, 300).permute(2, 0, 1).cpu().numpy()
        small.close()
        ref = bcc.launch_slice_ref(oracle_mod, m0, tgt, acts[0], s0, z)
        sl = slice(s0, s0 + 64)
        err = float(np.abs(m[sl] - ref["m"]).max())
        print(f"hybrid launch of {n} under 'brown', envs {s0} ... {s0 + 63} (T {acts[0, sl, 1].min():.2e} ... {acts[0, sl, 1].max():.2e}): "
              f"|m - m_ref| = {err:.2e}, sub-steps {int(ref['n_sub'].min())} ... {int(ref['n_sub'].max())}")
        assert err <= TOL_RK4, (n, s0, err)
        assert np.array_equal(status[sl], ref["status"]) and np.array_equal(a[0]["term"].cpu().numpy()[sl], ref["terminated"])
        assert np.allclose(a[0]["obs"].cpu().numpy()[sl], ref["obs"], rtol=3e-7, atol=1e-9)
        assert np.allclose(a[0]["reward_f64"].cpu().numpy()[sl], ref["reward"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("noise", NOISES)
def test_smallest_hybrid_launch_with_class_table_skip_done_and_fused_steps(stg, noise):
    """65 537 envs: a two-class table (MULTI kernels) with skip_done over two steps (finished envs are not integrated), then K = 2 fused
    steps with float64 actions under autoreset: every bit equal to the identity schedule's, which does not use the hybrid launch"""
    n = 65537
    cls = (np.arange(n) % 2).astype(np.uint8)
    m0, tgt, acts = bcc.launch_inputs(n, n + 1, steps=2)
    stt = stt_default_params(volume=bcc.VOL)
    vc = vcma_default_params(polarization=0.6, volume=0.8 * bcc.VOL)
    kw = _kw(noise, device_type=["stt_mram", "vcma_mram"], device_params=[stt, vc], max_steps=1, skip_done=True, autoreset=False)
    a, ca = _run(stg, n, m0, tgt, acts, cls=cls, **kw)
    b, cb = _run(stg, n, m0, tgt, acts, cls=cls, lane_sort=False, **kw)
    ca.pop("launch"), cb.pop("launch")
    assert ca == cb and ca["env_steps"] == n, (noise, ca, cb)                  # (second step: every env is done and skipped)
    _assert_same_bits(a, b, ("hybrid class table skip_done", noise))
    outs = []
    for ls in (None, False):
        env = stg.SpinTorqueVecEnv(n, diagnostics=True, class_index=cls, lane_sort=ls, **dict(kw, max_steps=100, skip_done=False, autoreset=True))
        env.reset(options={"initial_state": m0, "target_state": tgt})
        o, r, te, tr, info = env.step_many(torch.from_numpy(acts.astype(np.float64)))
        st = env.get_state()
        outs.append(dict(obs=o.clone(), reward=r.clone(), term=te.clone(), trunc=tr.clone(), status=info["status"].clone(), m=st["m"].clone(),
                         etot=st["total_energy"].clone(), rng_step=st["rng_step"].clone()))
        assert env.backend.counters()["env_steps"] == 2 * n
        env.close()
    _assert_same_bits(outs[:1], outs[1:], ("hybrid fused K = 2 float64", noise))
    assert bool((outs[0]["rng_step"] == 2).all())


# ------------------------------------------------------------------------------------------------
# the small, latency-bound forms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ("rk4", "euler"))
@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("n", (130, 4226))
def test_small_forms_wave_spec_by_lane_sort_bit_identical(stg, n, noise, solver):
    """two steps with a two-class table: the producer / consumer pairs (wave_spec=True) and the one-wavefront kernels (False), each on
    the sorted and on the identity schedule"""
    cls = (np.arange(n) % 2).astype(np.uint8)
    m0, tgt, acts = bcc.launch_inputs(n, 7 * n, steps=2)
    kw = _kw(noise, solver, device_type=["stt_mram", "vcma_mram"],
             device_params=[stt_default_params(volume=bcc.VOL), vcma_default_params(polarization=0.6, volume=0.8 * bcc.VOL)])
    base, c0 = _run(stg, n, m0, tgt, acts, cls=cls, wave_spec=False, lane_sort=False, **kw)
    assert c0.pop("launch")[1] == 1 and c0["env_steps"] == 2 * n and bool((base[1]["status"] == 0).all())
    for ws, ls in ((True, True), (True, False), (False, True)):
        other, c1 = _run(stg, n, m0, tgt, acts, cls=cls, wave_spec=ws, lane_sort=ls, **kw)
        assert (c1.pop("launch")[1] == 2) == ws                                # (pairs are two-wavefront workgroups)
        assert c0 == c1, (n, noise, solver, ws, ls, c0, c1)
        _assert_same_bits(base, other, (n, noise, solver, "wave_spec", ws, "lane_sort", ls))
    assert float((base[1]["m"] - torch.from_numpy(m0.T).cuda()).abs().max()) > 1e-2

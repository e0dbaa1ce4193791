"""stg_switch_verify -- write - verify - write switching statistics with the trial loop, the verify and the reduction on the GPU
(include/spintorque_hip.h) -- held to EXACT integer equality with chained stg_solve launches: `pytest -m gpu`.

By the header's stream rule phase p of attempt a of trial r of condition g is problem g * trial_stride + r of stg_solve at
env_step + a P + p.  The reference of every test is therefore tests/switch_verify_ref.py chain over HipBackend.solve, the unchanged
kernel: A P launches over the G R replicated problems with a host-side mask, reduced with NumPy.  All four arrays are compared.

Default shape: G = 3, R = 130 (two full wavefronts and one of two lanes), A = 3, P = 2 (a 0.1 ns pulse and a 0.05 ns relax), the
attempts' currents scaled 1.0 / 1.1 / 1.2.

  1. equality with the chain: rk4 / euler + brown (threshold 0; about 0.4 of the trials switch per attempt, and the reference itself
     has 0 < n_switched_at[a] < trials attempted for every a and g, so every attempt runs with a mixed wavefront), rk4 + ou and rk45 +
     white (threshold at the median of condition 1's projections after the first attempt.  Under these two fields the trials of a
     condition end within ~2e-6 of each other, so the first verify splits condition 1 in two halves by every trial's own stream, while
     the later attempts move the survivors of a condition together: the mixed-wavefront assertion is made where it can hold, at
     attempt 0 of condition 1);
  2. lanes that loop and refill: max_waves = G (one wavefront per condition: three trials per lane, ending at different attempts) and
     2 G give the counts of 1; one case at the library's own rule, R = 64 (SWITCH_STATS_WAVES // G) + 1;
  3. A = 1 equals stg_switch_stats, with and without a class table;
  4. invariants: sum_a n_ended_at = R, n_switched_at <= n_ended_at, chunks through trial0 and out=, env_id0;
  5. edge rules: a skipped phase, an attempt of skipped phases only, a NaN m0 row, a negative duration in attempt 1 only, A = 8;
  6. write footprint and every refusal;
  7. write_verify_statistics through the public solver classes.

Every test needs the symbol stg_switch_verify: none passes without the feature."""
import ctypes as C

import numpy as np
import pytest
import torch

import brown_ref as br
import switch_stats_ref as ssr
import switch_verify_ref as svr
from helpers import Guarded
from switch_verify_ref import A, ENV_STEP, FORMS, G, P, R

pytestmark = pytest.mark.gpu

N_BINS = 7
_REF = {}


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _inputs(solver):
    m0, J, T, tgt = svr.conditions()
    if solver == "rk45":
        J = J * ssr.RK45_J_SCALE                              # (switch_stats_ref.RK45_J_SCALE: the one unsaturated input of the LLGS solver)
    return m0, J, T, tgt


def _reference(stg, solver, noise):
    """the chain over stg_solve of the default case, computed once per form: dict(inputs, threshold, rec, counts with N_BINS bins)"""
    key = (solver, noise)
    if key not in _REF:
        m0, J, T, tgt = _inputs(solver)
        solve, close = svr.gpu_solve(stg, solver, noise, G, R)
        rec = svr.chain(solve, m0, J, T, tgt, R, env_step=ENV_STEP)
        thr = 0.0
        if noise != "brown":
            thr = svr.median_threshold(rec, R)
            rec = svr.chain(solve, m0, J, T, tgt, R, env_step=ENV_STEP, threshold=thr)
        close()
        _REF[key] = dict(inputs=(m0, J, T, tgt), threshold=thr, rec=rec, counts=svr.counts(rec, G, R, A, n_bins=N_BINS))
    return _REF[key]


def _same(got, want, what=""):
    for name, x, y in zip(("n_switched_at", "n_ended_at", "n_failed", "hist"), got, want):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), (what, name, None if x is None else x.tolist(),
                                                                                   None if y is None else y.tolist())


# ------------------------------------------------------------------------------------------------
# 1. equality with chained stg_solve
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise", FORMS)
def test_counts_equal_chained_stg_solve(stg, solver, noise):
    ref = _reference(stg, solver, noise)
    m0, J, T, tgt = ref["inputs"]
    n_sw, n_end, n_failed, hist = ref["counts"]
    att = svr.attempted(n_end, R)
    print(f"{solver} {noise} threshold {ref['threshold']!r}: reference switched_at {n_sw.tolist()}, attempted {att.tolist()}, failed {n_failed.tolist()}")
    assert not n_failed.any() and (n_end.sum(axis=0) == R).all()
    if noise == "brown":
        assert ((0 < n_sw) & (n_sw < att)).all()              # every attempt of every condition runs with a mixed wavefront
    else:
        assert n_sw[0, 1] == R // 2 and att[1, 1] == R - R // 2
    b = ssr.backend(stg, solver, noise, G)
    got = svr.fused(b, m0, J, T, tgt, R, env_step=ENV_STEP, threshold=ref["threshold"], n_bins=N_BINS)
    b.close()
    print(f"  kernel switched_at {got[0].tolist()}, ended_at {got[1].tolist()}, failed {got[2].tolist()}")
    _same(got, ref["counts"], (solver, noise))


# ------------------------------------------------------------------------------------------------
# 2. lanes that loop and refill
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise", FORMS)
@pytest.mark.parametrize("waves", (G, 2 * G))
def test_lanes_loop_and_refill(stg, solver, noise, waves):
    """max_waves = G: one wavefront per condition, so lane l runs trials l, l + 64 and (l < 2) l + 128, and its neighbours end theirs at
    other attempts; 2 G: two wavefronts, trials w 64 + l + 128 k.  The counts are those of the widest launch"""
    ref = _reference(stg, solver, noise)
    m0, J, T, tgt = ref["inputs"]
    b = ssr.backend(stg, solver, noise, G)
    got = svr.fused(b, m0, J, T, tgt, R, env_step=ENV_STEP, threshold=ref["threshold"], n_bins=N_BINS, max_waves=waves)
    b.close()
    _same(got, ref["counts"], (solver, noise, waves))


def test_lanes_loop_at_the_librarys_own_rule(stg):
    """R = 64 (SWITCH_STATS_WAVES // G) + 1 with max_waves = 0: one trial more than the wavefronts hold at one per lane, so lane 0 of the
    first wavefront of every condition runs two trials"""
    from spin_torque_gym_amd import _lib
    big = 64 * (_lib.SWITCH_STATS_WAVES // G) + 1
    m0, J, T, tgt = _inputs("rk4")
    solve, close = svr.gpu_solve(stg, "rk4", "brown", G, big)
    want = svr.counts(svr.chain(solve, m0, J, T, tgt, big, env_step=ENV_STEP), G, big, A, n_bins=N_BINS)
    close()
    b = ssr.backend(stg, "rk4", "brown", G)
    got = svr.fused(b, m0, J, T, tgt, big, env_step=ENV_STEP, n_bins=N_BINS)
    b.close()
    print(f"R = {big}: switched_at {got[0].tolist()}, ended_at {got[1].tolist()}")
    _same(got, want)
    assert ((0 < want[0]) & (want[0] < svr.attempted(want[1], big))).all()


# ------------------------------------------------------------------------------------------------
# 3. A = 1 equals stg_switch_stats
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_classes", (False, True))
def test_one_attempt_equals_switch_stats(stg, with_classes):
    m0, J, T, tgt = _inputs("rk4")
    tables = cond_cls = cls_t = None
    if with_classes:
        tables = [ssr.params(), ssr.params(0.7 * br.SWITCH["volume"]), ssr.params(1.3 * br.SWITCH["volume"])]
        cond_cls = np.array([2, 0, 1], dtype=np.uint8)
        cls_t = torch.from_numpy(cond_cls)
    b = ssr.backend(stg, "rk4", "brown", G, tables, cond_cls)
    want = ssr.fused(b, m0, J[0], T[0], tgt, R, env_step=ENV_STEP, n_bins=N_BINS, cond_cls=cls_t)
    n_sw, n_end, n_failed, hist = svr.fused(b, m0, J[:1], T[:1], tgt, R, env_step=ENV_STEP, n_bins=N_BINS, cond_cls=cls_t)
    plain = ssr.fused(b, m0, J[0], T[0], tgt, R, env_step=ENV_STEP, n_bins=N_BINS)
    b.close()
    assert n_sw.shape == (1, G) and np.array_equal(n_sw[0], want[0]) and np.array_equal(n_failed, want[1]) and np.array_equal(hist, want[2])
    assert (n_end == R).all() and ((0 < n_sw) & (n_sw < R)).all()
    if with_classes:
        assert not np.array_equal(plain[2], want[2])          # the classes reach the trials
        # ... and the chain over stg_solve on a context whose cls array replicates cond_cls per trial says the same for A = 3
        solve, close = svr.gpu_solve(stg, "rk4", "brown", G, R, tables=tables, cond_cls=cond_cls)
        ref = svr.counts(svr.chain(solve, m0, J, T, tgt, R, env_step=ENV_STEP), G, R, A, n_bins=N_BINS)
        close()
        bb = ssr.backend(stg, "rk4", "brown", G, tables, cond_cls)
        _same(svr.fused(bb, m0, J, T, tgt, R, env_step=ENV_STEP, n_bins=N_BINS, cond_cls=cls_t), ref)
        bb.close()


# ------------------------------------------------------------------------------------------------
# 4. invariants
# ------------------------------------------------------------------------------------------------
def test_invariants_chunks_and_env_id0(stg):
    ref = _reference(stg, "rk4", "brown")
    m0, J, T, tgt = ref["inputs"]
    n_sw, n_end, n_failed, hist = ref["counts"]
    b = ssr.backend(stg, "rk4", "brown", G)
    whole = svr.fused(b, m0, J, T, tgt, R, env_step=ENV_STEP, n_bins=N_BINS)
    _same(whole, ref["counts"])
    assert (whole[1].sum(axis=0) == R).all() and (whole[0] <= whole[1]).all() and (whole[3].sum(axis=1) == R).all()
    # chunks [0, 50) + [50, 130) through trial0, added into one set of arrays
    args = (torch.from_numpy(m0.T.copy()), torch.from_numpy(J), torch.from_numpy(T), torch.from_numpy(tgt.T.copy()))
    out = b.switch_verify(*args, 50, trial0=0, trial_stride=R, env_step=ENV_STEP, n_bins=N_BINS)
    first = tuple(x.cpu().numpy().copy() for x in out)
    sel = np.concatenate([np.arange(g * R, g * R + 50) for g in range(G)])
    _same(first, svr.counts(ref["rec"], G, R, A, n_bins=N_BINS, select=sel), "chunk [0, 50)")
    out = b.switch_verify(*args, 80, trial0=50, trial_stride=R, env_step=ENV_STEP, n_bins=N_BINS, out=out)
    torch.cuda.synchronize()
    _same(tuple(x.cpu().numpy() for x in out), whole, "chunks")
    b.close()
    # a context created at env_id0 = 37: the chain over a stg_solve context with that offset
    solve, close = svr.gpu_solve(stg, "rk4", "brown", G, R, env_id0=37)
    want = svr.counts(svr.chain(solve, m0, J, T, tgt, R, env_step=ENV_STEP), G, R, A, n_bins=N_BINS)
    close()
    bb = ssr.backend(stg, "rk4", "brown", G, env_id0=37)
    got = svr.fused(bb, m0, J, T, tgt, R, env_step=ENV_STEP, n_bins=N_BINS)
    bb.close()
    _same(got, want, "env_id0 = 37")
    assert not np.array_equal(got[0], whole[0])


# ------------------------------------------------------------------------------------------------
# 5. edge rules
# ------------------------------------------------------------------------------------------------
def _against_chain(stg, solver, noise, m0, J, T, tgt, n_att, **kw):
    solve, close = svr.gpu_solve(stg, solver, noise, G, R)
    rec = svr.chain(solve, m0, J, T, tgt, R, env_step=ENV_STEP)
    close()
    want = svr.counts(rec, G, R, n_att, n_bins=N_BINS)
    b = ssr.backend(stg, solver, noise, G)
    got = svr.fused(b, m0, J, T, tgt, R, env_step=ENV_STEP, n_bins=N_BINS, **kw)
    b.close()
    _same(got, want)
    return got, rec


def test_skipped_phases(stg):
    """T == 0 exactly: condition 0 has no relax in attempt 1 (skipped, not failed); condition 1's attempt 1 is made of skipped phases
    only, so its survivors of attempt 0 are verified again with the m they had and move on to attempt 2"""
    m0, J, T, tgt = _inputs("rk4")
    T[1, 1, 0] = 0.0
    T[1, :, 1] = 0.0
    for waves in (0, G):
        (n_sw, n_end, n_failed, _), rec = _against_chain(stg, "rk4", "brown", m0, J, T, tgt, A, max_waves=waves)
        assert not n_failed.any() and n_sw[1, 1] == 0 and n_end[1, 1] == 0 and n_sw[2, 1] > 0
    plain = _reference(stg, "rk4", "brown")["counts"]
    assert np.array_equal(n_sw[0], plain[0][0]) and not np.array_equal(n_sw[1:, :2], plain[0][1:, :2])


@pytest.mark.parametrize("solver", ("rk4", "euler"))
def test_failed_solves(stg, solver):
    """condition 1's m0 row is NaN: every trial fails at attempt 0, is not switched, lands in bin 0, n_ended_at[0] = R.  Condition 2 has a
    negative duration in attempt 1 only: attempt 0 decides normally, the survivors fail at attempt 1 with the m they had"""
    m0, J, T, tgt = _inputs(solver)
    m0[1] = [np.nan, 0.0, 1.0]
    T[1, 0, 2] = -1e-11
    for waves in (0, G):
        (n_sw, n_end, n_failed, hist), rec = _against_chain(stg, solver, "brown", m0, J, T, tgt, A, max_waves=waves)
        assert n_end[:, 1].tolist() == [R, 0, 0] and n_sw[:, 1].tolist() == [0, 0, 0] and n_failed[1] == R and hist[1, 0] == R
        assert 0 < n_sw[0, 2] < R and n_end[0, 2] == n_sw[0, 2] and n_end[1, 2] == R - n_sw[0, 2] == n_failed[2]
        assert n_sw[1, 2] == 0 and n_end[2, 2] == 0 and n_failed[0] == 0


def test_eight_attempts(stg):
    from spin_torque_gym_amd import _lib
    assert _lib.STG_MAX_VERIFY_ATTEMPTS == 8
    m0, J, T, tgt = svr.conditions(8, scales=(0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2))
    (n_sw, n_end, n_failed, _), _ = _against_chain(stg, "rk4", "brown", m0, J, T, tgt, 8, max_waves=G)
    print(f"A = 8: switched_at {n_sw.tolist()}, ended_at {n_end.tolist()}")
    # trials of every condition run all eight attempts, and end at early ones too: every counter row is reached
    assert n_sw.shape == (8, G) and (svr.attempted(n_end, R)[7] > 0).all() and (n_sw[0] > 0).all() and (n_end.sum(axis=0) == R).all()


# ------------------------------------------------------------------------------------------------
# 6. write footprint and checked errors
# ------------------------------------------------------------------------------------------------
def _raw_call(lib, b, arrays, g=G, R=R, trial0=0, stride=None, A=A, P=P, n_bins=N_BINS, max_waves=0, null=()):
    """stg_switch_verify through ctypes with Guarded outputs; `null`: names of pointer arguments passed as NULL"""
    ptr = lambda name: None if name in null else C.c_void_p(arrays[name].data_ptr())            # noqa: E731
    stride = trial0 + R if stride is None else stride
    return lib.stg_switch_verify(None if "ctx" in null else b._ctx, g, R, trial0, stride, A, P, ptr("m0"), ptr("J"), ptr("T"), ptr("cls"), ENV_STEP,
                                 ptr("target"), 0.0, n_bins, max_waves, ptr("n_switched_at"), ptr("n_ended_at"), ptr("n_failed"), ptr("hist"),
                                 None)


def test_write_footprint_and_refusals(stg):
    from spin_torque_gym_amd import _lib
    lib = _lib.load()
    ref = _reference(stg, "rk4", "brown")
    m0, J, T, tgt = ref["inputs"]
    b = ssr.backend(stg, "rk4", "brown", G)
    guards = {"n_switched_at": Guarded("n_switched_at", (A, G), torch.float64), "n_ended_at": Guarded("n_ended_at", (A, G), torch.float64),
              "n_failed": Guarded("n_failed", (G,), torch.float64), "hist": Guarded("hist", (G, N_BINS), torch.float64, n_axis=0)}
    arrays = dict(m0=torch.from_numpy(m0.T.copy()).cuda(), J=torch.from_numpy(J.copy()).cuda(), T=torch.from_numpy(T.copy()).cuda(),
                  target=torch.from_numpy(tgt.T.copy()).cuda(), cls=torch.zeros(G, dtype=torch.uint8, device="cuda"),
                  **{k: v.interior for k, v in guards.items()})
    # every refusal: an error code, a message, nothing launched -- the arrays still hold their sentinels
    refusals = [(dict(null=(name,)), _lib.STG_E_INVALID)
                for name in ("ctx", "m0", "J", "T", "target", "n_switched_at", "n_ended_at", "n_failed", "hist")]
    refusals += [(kw, _lib.STG_E_INVALID) for kw in (
        dict(g=0), dict(R=-1), dict(P=0), dict(P=5), dict(n_bins=-1), dict(n_bins=65), dict(n_bins=0), dict(trial0=-1, stride=R),
        dict(stride=R - 1), dict(trial0=10, stride=R + 9), dict(R=2 ** 62, trial0=2 ** 62, stride=2 ** 63 - 1), dict(stride=2 ** 62),
        dict(A=0), dict(A=-1), dict(A=9), dict(max_waves=-1), dict(max_waves=1), dict(max_waves=G - 1))]
    for kw, code in refusals:
        rc = _raw_call(lib, b, arrays, **kw)
        assert rc == code and lib.stg_last_error(), (kw, rc)
        torch.cuda.synchronize()
        for v in guards.values():
            v.check(written=False)
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    pe = HipBackend(G, EnvConfig(solver="rk4", include_thermal_fluctuations=True, noise_model="brown", seed=ssr.SEED))
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
    # the real thing: zeroed interiors, the counts of the chain, guards intact
    for v in guards.values():
        v.bits().zero_()
    assert _raw_call(lib, b, arrays) == 0, lib.stg_last_error()
    torch.cuda.synchronize()
    for v, y in zip(guards.values(), ref["counts"]):
        v.check_guards()
        assert np.array_equal(v.bits().cpu().numpy(), y), v.name
    # it ADDS: a second call -- one wavefront per condition, no histogram, no class bytes -- doubles the counts and leaves hist alone
    assert _raw_call(lib, b, arrays, n_bins=0, max_waves=G, null=("hist", "cls")) == 0, lib.stg_last_error()
    torch.cuda.synchronize()
    for v, y, f in zip(guards.values(), ref["counts"], (2, 2, 2, 1)):
        v.check_guards()
        assert np.array_equal(v.bits().cpu().numpy(), f * y), v.name
    b.close()


# ------------------------------------------------------------------------------------------------
# 7. the public method
# ------------------------------------------------------------------------------------------------
def _derived_ok(res, n_trials):
    n_sw, n_end = res["n_switched_at"], res["n_ended_at"]
    wer = 1.0 - np.cumsum(n_sw, axis=0) / n_trials
    assert np.array_equal(res["n_attempted"], svr.attempted(n_end, n_trials)) and np.array_equal(res["wer_after"], wer)
    assert np.array_equal(res["stderr"], np.sqrt(wer * (1.0 - wer) / n_trials)) and np.array_equal(res["p_switch"], 1.0 - wer[-1])
    assert np.array_equal(res["mean_attempts"], ((np.arange(n_sw.shape[0])[:, None] + 1) * n_end).sum(axis=0) / n_trials)


def test_write_verify_statistics(stg):
    from spin_torque_gym_amd import physics
    ref = _reference(stg, "rk4", "brown")
    m0, J, T, tgt = ref["inputs"]
    solver = physics.SimpleLLGSSolver(method="rk4", noise_model="brown", seed=ssr.SEED)
    keys = {"n_switched_at", "n_ended_at", "n_failed", "n_attempted", "wer_after", "stderr", "p_switch", "mean_attempts", "hist", "bin_edges"}
    # [A,P,G], and the same trial as [A,G] pulses with relax=
    full = solver.write_verify_statistics(m0, J, T, ssr.params(), R, n_bins=N_BINS, env_step=ENV_STEP)
    relax = solver.write_verify_statistics(m0, J[:, 0], T[:, 0], ssr.params(), R, relax=svr.RELAX, n_bins=N_BINS, env_step=ENV_STEP)
    chunked = solver.write_verify_statistics(m0, J, T, ssr.params(), R, n_bins=N_BINS, env_step=ENV_STEP, max_trials_per_launch=64)
    for res in (full, relax, chunked):
        assert set(res) == keys
        _same((res["n_switched_at"], res["n_ended_at"], res["n_failed"], res["hist"]), ref["counts"])
        _derived_ok(res, R)
        for k in keys:
            assert np.array_equal(res[k], full[k]), k
    assert np.array_equal(full["bin_edges"], np.linspace(-1.0, 1.0, N_BINS + 1)) and (full["mean_attempts"] > 1.0).all()
    # [A]: the same pulse train for every condition
    Ja, Ta = J[:, 0, 0].copy(), T[:, 0, 0].copy()
    one = solver.write_verify_statistics(m0, Ja, Ta, ssr.params(), R, relax=svr.RELAX, env_step=ENV_STEP)
    Jb = np.concatenate([np.repeat(Ja[:, None, None], G, axis=2), np.zeros((A, 1, G))], axis=1)
    Tb = np.concatenate([np.repeat(Ta[:, None, None], G, axis=2), np.full((A, 1, G), svr.RELAX)], axis=1)
    solve, close = svr.gpu_solve(stg, "rk4", "brown", G, R)
    want = svr.counts(svr.chain(solve, m0, Jb, Tb, tgt, R, env_step=ENV_STEP), G, R, A)
    close()
    _same((one["n_switched_at"], one["n_ended_at"], one["n_failed"], None), want)
    _derived_ok(one, R)
    assert one["hist"].shape == (G, 0) and np.array_equal(one["n_switched_at"][:, 0], full["n_switched_at"][:, 0])
    # the other two classes have the method too
    for cls, kw, form in ((physics.RobustLLGSSolver, dict(method="euler", noise_model="brown"), ("euler", "brown")),
                          (physics.LLGSSolver, dict(noise_model="white"), ("rk45", "white"))):
        r2 = _reference(stg, *form)
        res = cls(seed=ssr.SEED, **kw).write_verify_statistics(*r2["inputs"][:3], ssr.params(), R, n_bins=N_BINS, env_step=ENV_STEP,
                                                                threshold=r2["threshold"])
        _same((res["n_switched_at"], res["n_ended_at"], res["n_failed"], res["hist"]), r2["counts"], form)

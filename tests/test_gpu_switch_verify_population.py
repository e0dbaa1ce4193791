"""stg_switch_verify_population -- write - verify - write statistics over a population of varied devices, with the trial loop, the
draw, the verify and the reduction on the GPU (include/spintorque_hip.h) -- held to EXACT integer equality with existing code:
`pytest -m gpu`.

  a. sigma 0 is stg_switch_verify, all four arrays, for the four forms of switch_verify_ref.FORMS;
  b. A = 1 is stg_switch_population (no tables, no first passage), per-device counts included;
  c. a population of 2 x 26 devices against tests/switch_verify_population_ref.py: switch_verify_ref.chain over the UNCHANGED stg_solve
     on a class table that holds the devices stg_switch_population_devices dumps, a class byte per replicated problem;
  d. lanes that loop and refill: three trials of three devices per lane, and lanes that keep their device;
  e. additivity: chunks split inside a device, prefilled arrays, env_id0 != 0, trial_stride > trial0 + R;
  f. a bad sigma column fails its condition alone;
  g. edge rules with devices on: skipped phases, A = 8, a NaN m0 row;
  h. write footprint and every refusal;
  i. write_verify_statistics(variation=..., per_device=True) against plain calls on the drawn devices;
  j. against the CPU oracle, which is handed the dumped devices as class tables (rk4 + brown, euler + brown).

No tolerance appears: every comparison is integer for integer.  Every test needs the symbol stg_switch_verify_population or the new
keywords of write_verify_statistics: none passes without the feature."""
import ctypes as C

import numpy as np
import pytest
import torch

import switch_population_ref as spr
import switch_stats_ref as ssr
import switch_verify_population_ref as svpr
import switch_verify_ref as svr
from helpers import Guarded
from switch_verify_ref import A, ENV_STEP, P

pytestmark = pytest.mark.gpu

N_BINS = 7
NAMES = ("n_switched_at", "n_ended_at", "n_failed", "hist", "dev_switched_at")
SIGMA3 = np.array([[0.05, 0.10, 0.15], [0.02, 0.04, 0.06], [0.07, 0.03, 0.11], [0.20, 0.12, 0.08], [0.01, 0.09, 0.13]])       # [5, G]: that of tests/test_gpu_switch_population.py
G2, R, Q, D, CLIP = 2, 130, 5, 26, 2.0
SIGMA2 = SIGMA3[:, :G2] * 0.5
POP_FORMS = (("rk4", "brown"), ("euler", "ou"), ("rk45", "white"))
_REF = {}
_PLAIN = {}


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _same(got, want, what=None, names=NAMES):
    assert len(got) == len(want)
    for name, x, y in zip(names, got, want):
        assert (x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)), (
            what, name, None if x is None else x.tolist(), None if y is None else y.tolist())


def _inputs(solver, g=None):
    m0, J, T, tgt = svr.conditions()
    if solver == "rk45":
        J = J * ssr.RK45_J_SCALE
    g = m0.shape[0] if g is None else g
    return m0[:g].copy(), J[:, :, :g].copy(), T[:, :, :g].copy(), tgt[:g].copy()


def _devices(stg, solver, noise, g, d, sigma, **kw):
    b = ssr.backend(stg, solver, noise, g, env_id0=kw.pop("env_id0", 0))
    params = b.switch_population_devices(g, d, torch.from_numpy(np.ascontiguousarray(sigma)), **kw)
    torch.cuda.synchronize()
    params = params.cpu().numpy()
    b.close()
    return params


def _chain_counts(stg, solver, noise, params, m0, J, T, tgt, n_trials, q, threshold=None, env_id0=0, select=None):
    """the reference: the chain over stg_solve on the class table of the devices `params` -> (record, threshold, the five arrays)"""
    recs, cls, dev = svpr.class_table(stg, params, n_trials, q)
    solve, close = svpr.gpu_solve(stg, solver, noise, recs, cls, env_id0=env_id0)
    rec = svr.chain(solve, m0, J, T, tgt, n_trials, env_step=ENV_STEP, threshold=0.0 if threshold is None else threshold)
    if threshold is None and noise != "brown":
        threshold = svr.median_threshold(rec, n_trials)
        rec = svr.chain(solve, m0, J, T, tgt, n_trials, env_step=ENV_STEP, threshold=threshold)
    close()
    threshold = 0.0 if threshold is None else threshold
    return rec, threshold, svpr.all_counts(rec, m0.shape[0], n_trials, J.shape[0], dev, params.shape[2], n_bins=N_BINS, select=select)


def _reference(stg, solver, noise):
    """case (c), computed once per form: G = 2, R = 130, Q = 5 -- 26 devices per condition, 52 rows of the class table"""
    key = (solver, noise)
    if key not in _REF:
        m0, J, T, tgt = _inputs(solver, G2)
        params = _devices(stg, solver, noise, G2, D, SIGMA2, trials_per_device=Q, trial_stride=R, z_clip=CLIP)
        assert (params > 0).all() and len(np.unique(params[3])) == G2 * D
        rec, thr, counts = _chain_counts(stg, solver, noise, params, m0, J, T, tgt, R, Q)
        _REF[key] = dict(inputs=(m0, J, T, tgt), params=params, rec=rec, threshold=thr, counts=counts)
    return _REF[key]


def _fused(stg, solver, noise, ref, sigma=SIGMA2, g=G2, **kw):
    m0, J, T, tgt = ref["inputs"]
    b = ssr.backend(stg, solver, noise, g)
    kw = dict(dict(env_step=ENV_STEP, threshold=ref["threshold"], n_bins=N_BINS, trials_per_device=Q, z_clip=CLIP, dev_stride=D), **kw)
    got = svpr.fused(b, m0, J, T, tgt, R, sigma, **kw)
    b.close()
    return got


# ------------------------------------------------------------------------------------------------
# a. sigma 0 is stg_switch_verify
# ------------------------------------------------------------------------------------------------
def _plain_threshold(stg, solver, noise):
    """threshold 0 under brown; else the median of condition 1's projections after attempt 0 in the chain over stg_solve, as
    tests/test_gpu_switch_verify.py sets it"""
    if (solver, noise) not in _PLAIN:
        thr = 0.0
        if noise != "brown":
            m0, J, T, tgt = _inputs(solver)
            solve, close = svr.gpu_solve(stg, solver, noise, svr.G, R)
            thr = svr.median_threshold(svr.chain(solve, m0, J, T, tgt, R, env_step=ENV_STEP), R)
            close()
        _PLAIN[(solver, noise)] = thr
    return _PLAIN[(solver, noise)]


@pytest.mark.parametrize("solver,noise", svr.FORMS)
def test_sigma_zero_is_stg_switch_verify(stg, solver, noise):
    assert (svr.G, svr.R, A, P) == (3, 130, 3, 2)
    m0, J, T, tgt = _inputs(solver)
    thr = _plain_threshold(stg, solver, noise)
    b = ssr.backend(stg, solver, noise, svr.G)
    want = svr.fused(b, m0, J, T, tgt, R, env_step=ENV_STEP, threshold=thr, n_bins=N_BINS)
    got = svpr.fused(b, m0, J, T, tgt, R, np.zeros((5, svr.G)), dev_stride=D, trials_per_device=Q, env_step=ENV_STEP, threshold=thr, n_bins=N_BINS)
    # without the per-device counts, and with one wavefront per condition
    bare = svpr.fused(b, m0, J, T, tgt, R, np.zeros((5, svr.G)), trials_per_device=Q, env_step=ENV_STEP, threshold=thr, n_bins=N_BINS, max_waves=svr.G)
    b.close()
    print(f"{solver} {noise} threshold {thr!r}: switched_at {got[0].tolist()}, ended_at {got[1].tolist()}")
    _same(got[:4], want, (solver, noise))
    _same(bare[:4], want, (solver, noise, "bare"))
    assert bare[4] is None and np.array_equal(got[4].sum(axis=-1), got[0]) and got[0].any() and (got[1].sum(axis=0) == R).all()


# ------------------------------------------------------------------------------------------------
# b. A = 1 is stg_switch_population
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise", (("rk4", "brown"), ("rk45", "white")))
def test_one_attempt_is_stg_switch_population(stg, solver, noise):
    m0, J, T, tgt = _inputs(solver)
    g, var_step = svr.G, 77
    b = ssr.backend(stg, solver, noise, g)
    kw = dict(trials_per_device=Q, z_clip=3.0, var_step=var_step, env_step=ENV_STEP, n_bins=N_BINS, dev_stride=D)
    (n_sw, n_failed, hist), dev = spr.fused(b, m0, J[0], T[0], tgt, R, SIGMA3, **kw)
    got = svpr.fused(b, m0, J[:1], T[:1], tgt, R, SIGMA3, **kw)
    other = svpr.fused(b, m0, J[:1], T[:1], tgt, R, SIGMA3, **dict(kw, var_step=var_step + 1))
    b.close()
    assert got[0].shape == (1, g) and got[4].shape == (1, g, D)
    assert np.array_equal(got[0][0], n_sw) and np.array_equal(got[2], n_failed) and np.array_equal(got[3], hist) and np.array_equal(got[4][0], dev)
    assert (got[1] == R).all()
    if noise == "brown":
        assert ((0 < n_sw) & (n_sw < R)).all() and not np.array_equal(other[3], got[3])         # var_step reaches the draw


# ------------------------------------------------------------------------------------------------
# c. a population against the class-table path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise", POP_FORMS)
def test_population_equals_the_class_table_path(stg, solver, noise):
    ref = _reference(stg, solver, noise)
    m0, J, T, tgt = ref["inputs"]
    n_sw, n_end, n_failed, hist, dev = ref["counts"]
    att = svr.attempted(n_end, R)
    print(f"{solver} {noise} threshold {ref['threshold']!r}: reference switched_at {n_sw.tolist()}, attempted {att.tolist()}, failed {n_failed.tolist()}, "
          f"devices by switched trials at attempt 0 {np.bincount(dev[0].reshape(-1), minlength=Q + 1).tolist()}")
    assert not n_failed.any() and (n_end.sum(axis=0) == R).all() and np.array_equal(dev.sum(axis=-1), n_sw)
    if noise == "brown":
        assert ((0 < n_sw) & (n_sw < att)).all()              # every attempt of every condition runs with a mixed wavefront
    else:
        assert n_sw[0, 1] == R // 2 and att[1, 1] == R - R // 2
    total = dev.sum(axis=0)
    assert len(np.unique(total)) > 1                          # the devices' counts are not all equal
    got = _fused(stg, solver, noise, ref)
    print(f"  kernel switched_at {got[0].tolist()}, ended_at {got[1].tolist()}, failed {got[2].tolist()}")
    _same(got, ref["counts"], (solver, noise))
    # the population matters: the nominal device's stg_switch_verify counts differ
    b = ssr.backend(stg, solver, noise, G2)
    nominal = svr.fused(b, m0, J, T, tgt, R, env_step=ENV_STEP, threshold=ref["threshold"], n_bins=N_BINS)
    b.close()
    assert not np.array_equal(nominal[0], got[0]) and (noise != "brown" or not np.array_equal(nominal[3], got[3]))


# ------------------------------------------------------------------------------------------------
# d. lanes that loop and refill
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise", POP_FORMS)
@pytest.mark.parametrize("waves", (G2, 2 * G2))
def test_lanes_loop_and_refill(stg, solver, noise, waves):
    """max_waves = G: one wavefront per condition, so lane l runs trials l, l + 64 and (l < 2) l + 128 -- of devices l // 5,
    (l + 64) // 5 and (l + 128) // 5, three different ones -- and its neighbours end theirs at other attempts; 2 G: trials
    w 64 + l + 128 k.  The counts are those of the widest launch"""
    ref = _reference(stg, solver, noise)
    _same(_fused(stg, solver, noise, ref, max_waves=waves), ref["counts"], (solver, noise, waves))


def test_lanes_that_keep_their_device(stg):
    """G = 1, R = 256, Q = 128, max_waves = 1: lane l runs trials l, l + 64, l + 128, l + 192 of devices 0, 0, 1, 1 -- it keeps its row
    once and redraws once"""
    m0, J, T, tgt = _inputs("rk4", 1)
    n, q = 256, 128
    params = _devices(stg, "rk4", "brown", 1, 2, SIGMA2[:, :1], trials_per_device=q, trial_stride=n, z_clip=CLIP)
    _, _, want = _chain_counts(stg, "rk4", "brown", params, m0, J, T, tgt, n, q)
    b = ssr.backend(stg, "rk4", "brown", 1)
    kw = dict(dev_stride=2, trials_per_device=q, z_clip=CLIP, env_step=ENV_STEP, n_bins=N_BINS)
    got = svpr.fused(b, m0, J, T, tgt, n, SIGMA2[:, :1], max_waves=1, **kw)
    wide = svpr.fused(b, m0, J, T, tgt, n, SIGMA2[:, :1], **kw)
    b.close()
    print(f"kept devices: switched_at {got[0].tolist()}, per device {got[4].tolist()}")
    _same(got, want, "max_waves = 1")
    _same(wide, want, "the library's rule")
    assert got[4][..., 0].any() and got[4][..., 1].any()


# ------------------------------------------------------------------------------------------------
# e. additivity
# ------------------------------------------------------------------------------------------------
def test_chunks_prefilled_arrays_env_id0_and_stride(stg):
    """env_id0 = 37 and trial_stride = 160 > R = 130: the reference is the chain over a stg_solve context of G x 160 problems at that
    env id, of which each condition's first 130 count (32 devices per condition: 64 rows).  Then two chunks split at trial 47 -- inside
    device 9 -- into prefilled arrays add up to the one call"""
    stride, d, env_id0 = 160, 32, 37
    m0, J, T, tgt = _inputs("rk4", G2)
    params = _devices(stg, "rk4", "brown", G2, d, SIGMA2, trials_per_device=Q, trial_stride=stride, z_clip=CLIP, env_id0=env_id0)
    sel = np.concatenate([np.arange(g * stride, g * stride + R) for g in range(G2)])
    _, _, want = _chain_counts(stg, "rk4", "brown", params, m0, J, T, tgt, stride, Q, env_id0=env_id0, select=sel)
    assert not want[4][..., D:].any() and want[4][..., D - 1].any()
    b = ssr.backend(stg, "rk4", "brown", G2, env_id0=env_id0)
    kw = dict(trials_per_device=Q, z_clip=CLIP, env_step=ENV_STEP, n_bins=N_BINS, trial_stride=stride)
    whole = svpr.fused(b, m0, J, T, tgt, R, SIGMA2, dev_stride=d, **kw)
    _same(whole, want, "env_id0 = 37, stride 160")
    assert not np.array_equal(whole[0], _reference(stg, "rk4", "brown")["counts"][0])
    rng = np.random.default_rng(5)
    pre = [rng.integers(1, 2 ** 40, s) for s in ((A, G2), (A, G2), (G2,), (G2, N_BINS))]
    pre_dev = rng.integers(1, 2 ** 40, (A, G2, d))
    out, dsw = tuple(torch.from_numpy(p.copy()).cuda() for p in pre), torch.from_numpy(pre_dev.copy()).cuda()
    args = (torch.from_numpy(m0.T.copy()), torch.from_numpy(J), torch.from_numpy(T), torch.from_numpy(tgt.T.copy()))
    assert 47 % Q != 0
    for t0, n in ((0, 47), (47, R - 47)):
        res = b.switch_verify_population(*args, n, torch.from_numpy(SIGMA2.copy()), trial0=t0, dev_switched_at=dsw, out=out, **kw)
        assert all(x is y for x, y in zip(res, out))
    torch.cuda.synchronize()
    b.close()
    _same([x.cpu().numpy() - p for x, p in zip(out, pre)] + [dsw.cpu().numpy() - pre_dev], whole, "chunks")


# ------------------------------------------------------------------------------------------------
# f. a bad sigma column
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad,where", ((-0.05, 0), (float("nan"), 1), (0.5, 0)), ids=("negative", "nan", "sigma-clip-1"))
def test_bad_sigma_column_fails_its_condition_alone(stg, bad, where):
    ref = _reference(stg, "rk4", "brown")
    m0, J, T, tgt = ref["inputs"]
    worse = SIGMA2.copy()
    worse[3, where] = bad
    other = 1 - where
    assert not spr.column_ok(worse[:, where], CLIP) and spr.column_ok(worse[:, other], CLIP)
    got = _fused(stg, "rk4", "brown", ref, sigma=worse)
    # the condition: every trial fails at attempt 0 with m = m0 (proj = -m0.z < 0: not switched), classified and binned like any other
    pr0 = ssr.proj(m0.T.copy(), tgt)
    assert (pr0 < 0).all()
    assert got[2][where] == R and got[1][:, where].tolist() == [R, 0, 0] and not got[0][:, where].any() and not got[4][:, where].any()
    assert np.array_equal(got[3][where], R * np.bincount(np.asarray(ssr.bins(pr0[where:where + 1], N_BINS), dtype=np.int64), minlength=N_BINS))
    # the other condition keeps the integers of (c)
    for name, x, y in zip(NAMES, got, ref["counts"]):
        idx = (slice(None), other) if x.ndim >= 2 and name != "hist" else (other,)
        assert np.array_equal(x[idx], y[idx]), name
    # with a threshold below proj(m0) the failed trials ARE switched, at attempt 0, and every device of the condition counts its trials
    sw = _fused(stg, "rk4", "brown", ref, sigma=worse, threshold=-0.5)
    assert sw[0][:, where].tolist() == [R, 0, 0] and sw[2][where] == R and sw[4][0, where].tolist() == [Q] * D and not sw[4][1:, where].any()
    # a skipped first phase: the trial fails at its first phase that is not skipped
    T2 = T.copy()
    T2[0, 0, where] = 0.0
    skipped = _fused(stg, "rk4", "brown", dict(ref, inputs=(m0, J, T2, tgt)), sigma=worse)
    assert skipped[2][where] == R and skipped[1][:, where].tolist() == [R, 0, 0]


# ------------------------------------------------------------------------------------------------
# g. edge rules with devices on
# ------------------------------------------------------------------------------------------------
def _against_chain(stg, m0, J, T, tgt, **kw):
    ref = _reference(stg, "rk4", "brown")
    rec, _, want = _chain_counts(stg, "rk4", "brown", ref["params"], m0, J, T, tgt, R, Q)
    got = _fused(stg, "rk4", "brown", dict(inputs=(m0, J, T, tgt), threshold=0.0), **kw)
    _same(got, want)
    return got, rec


def test_skipped_phases(stg):
    """T == 0 exactly: condition 0 has no relax in attempt 1 (skipped, not failed); condition 1's attempt 1 is made of skipped phases
    only, so its survivors of attempt 0 are verified again with the m they had and move on to attempt 2"""
    m0, J, T, tgt = _inputs("rk4", G2)
    T[1, 1, 0] = 0.0
    T[1, :, 1] = 0.0
    for waves in (0, G2):
        (n_sw, n_end, n_failed, _, dev), _ = _against_chain(stg, m0, J, T, tgt, max_waves=waves)
        assert not n_failed.any() and n_sw[1, 1] == 0 and n_end[1, 1] == 0 and n_sw[2, 1] > 0 and not dev[1, 1].any()
    plain = _reference(stg, "rk4", "brown")["counts"]
    assert np.array_equal(n_sw[0], plain[0][0]) and not np.array_equal(n_sw[1:], plain[0][1:])


def test_nan_m0_row(stg):
    """condition 1's m0 row is NaN: every trial fails at attempt 0, is not switched, lands in bin 0"""
    m0, J, T, tgt = _inputs("rk4", G2)
    m0[1] = [np.nan, 0.0, 1.0]
    for waves in (0, G2):
        (n_sw, n_end, n_failed, hist, dev), _ = _against_chain(stg, m0, J, T, tgt, max_waves=waves)
        assert n_end[:, 1].tolist() == [R, 0, 0] and not n_sw[:, 1].any() and n_failed.tolist() == [0, R] and hist[1, 0] == R and not dev[:, 1].any()
        assert 0 < n_sw[0, 0] < R


def test_eight_attempts(stg):
    m0, J, T, tgt = svr.conditions(8, scales=(0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2))
    m0, J, T, tgt = m0[:G2], J[:, :, :G2].copy(), T[:, :, :G2].copy(), tgt[:G2]
    (n_sw, n_end, n_failed, _, dev), _ = _against_chain(stg, m0, J, T, tgt, max_waves=G2)
    print(f"A = 8: switched_at {n_sw.tolist()}, ended_at {n_end.tolist()}")
    assert n_sw.shape == (8, G2) and dev.shape == (8, G2, D) and (svr.attempted(n_end, R)[7] > 0).all() and (n_sw[0] > 0).all()
    assert np.array_equal(dev.sum(axis=-1), n_sw) and (n_end.sum(axis=0) == R).all()


# ------------------------------------------------------------------------------------------------
# h. write footprint and every refusal
# ------------------------------------------------------------------------------------------------
def _raw_call(lib, b, arrays, g=G2, R=R, trial0=0, stride=None, A=A, P=P, n_bins=N_BINS, max_waves=0, env_step=ENV_STEP, z_clip=CLIP,
              var_step=spr.VAR_STEP, Q=Q, dev_stride=None, null=()):
    """stg_switch_verify_population through ctypes with Guarded outputs; `null`: names of pointer arguments passed as NULL"""
    ptr = lambda name: None if name in null else C.c_void_p(arrays[name].data_ptr())            # noqa: E731
    stride = trial0 + R if stride is None else stride
    dev_stride = arrays["dev_switched_at"].shape[2] if dev_stride is None else dev_stride
    return lib.stg_switch_verify_population(None if "ctx" in null else b._ctx, g, R, trial0, stride, A, P, ptr("m0"), ptr("J"), ptr("T"), ptr("cls"),
                                            env_step, ptr("target"), 0.0, n_bins, max_waves, ptr("n_switched_at"), ptr("n_ended_at"),
                                            ptr("n_failed"), ptr("hist"), ptr("sigma"), z_clip, var_step, Q, ptr("dev_switched_at"), dev_stride,
                                            None)


def _guards(n_dev):
    return {"n_switched_at": Guarded("n_switched_at", (A, G2), torch.float64), "n_ended_at": Guarded("n_ended_at", (A, G2), torch.float64),
            "n_failed": Guarded("n_failed", (G2,), torch.float64), "hist": Guarded("hist", (G2, N_BINS), torch.float64, n_axis=0),
            "dev_switched_at": Guarded("dev_switched_at", (A, G2, n_dev), torch.float64, n_axis=0)}


def test_write_footprint_and_refusals(stg):
    from spin_torque_gym_amd import _lib
    lib = _lib.load()
    ref = _reference(stg, "rk4", "brown")
    m0, J, T, tgt = ref["inputs"]
    b = ssr.backend(stg, "rk4", "brown", G2)
    guards = _guards(D)
    arrays = dict(m0=torch.from_numpy(m0.T.copy()).cuda(), J=torch.from_numpy(J.copy()).cuda(), T=torch.from_numpy(T.copy()).cuda(),
                  target=torch.from_numpy(tgt.T.copy()).cuda(), cls=torch.zeros(G2, dtype=torch.uint8, device="cuda"),
                  sigma=torch.from_numpy(SIGMA2.copy()).cuda(), **{k: v.interior for k, v in guards.items()})
    m_before = {k: arrays[k].clone() for k in ("m0", "J", "T", "target", "sigma")}
    # every refusal: an error code, a message, nothing launched -- the arrays still hold their sentinels
    refusals = [dict(null=(name,)) for name in ("ctx", "m0", "J", "T", "target", "n_switched_at", "n_ended_at", "n_failed", "hist", "sigma")]
    refusals += [dict(g=0), dict(R=-1), dict(P=0), dict(P=5), dict(n_bins=-1), dict(n_bins=65), dict(n_bins=0), dict(trial0=-1, stride=R),
                 dict(stride=R - 1), dict(trial0=10, stride=R + 9), dict(R=2 ** 62, trial0=2 ** 62, stride=2 ** 63 - 1), dict(stride=2 ** 62),
                 dict(A=0), dict(A=-1), dict(A=9), dict(max_waves=-1), dict(max_waves=1), dict(max_waves=G2 - 1),
                 dict(z_clip=0.0), dict(z_clip=-1.0), dict(z_clip=float("inf")), dict(z_clip=float("nan")), dict(Q=0), dict(Q=-3),
                 dict(var_step=ENV_STEP), dict(var_step=ENV_STEP + 1), dict(var_step=ENV_STEP + A * P - 1),
                 dict(var_step=1, env_step=2 ** 32 - 2), dict(var_step=3, env_step=2 ** 32 - 2),         # modulo 2^32: k = 3 and k = 5 < A P = 6
                 dict(dev_stride=D - 1), dict(trial0=5, stride=R + 5, dev_stride=D), dict(Q=1, dev_stride=R - 1), dict(dev_stride=-1),
                 dict(dev_stride=2 ** 62)]
    for kw in refusals:
        rc = _raw_call(lib, b, arrays, **kw)
        assert rc == _lib.STG_E_INVALID and lib.stg_last_error(), (kw, rc)
        torch.cuda.synchronize()
        for v in guards.values():
            v.check(written=False)
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    pe = HipBackend(G2, EnvConfig(solver="rk4", include_thermal_fluctuations=True, noise_model="brown", seed=ssr.SEED))
    assert _raw_call(lib, pe, arrays) == _lib.STG_E_STATE                                       # no parameters yet
    import spin_torque_gym_amd.devices as devices
    flat = stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", ssr.params()))
    block, dev_type, valid = devices.per_env_param_block(flat, G2, {})
    pe.set_params_per_env(block, dev_type, valid)
    assert _raw_call(lib, pe, arrays) == _lib.STG_E_STATE and b"per-env" in lib.stg_last_error()
    pe.close()
    assert _raw_call(lib, b, arrays, R=0) == 0                                                   # valid, does nothing
    torch.cuda.synchronize()
    for v in guards.values():
        v.check(written=False)
    for k, x in m_before.items():
        assert torch.equal(arrays[k].view(torch.int64), x.view(torch.int64)), k                 # the inputs are as they were
    # var_step = env_step + A P is the first counter word behind the trial's: accepted.  The counts start from zero; dev_switched_at
    # keeps its sentinels, to which the kernel adds, so an element outside the stated range that was touched at all shows.  trial0 = 40
    # with Q = 5: devices 8 ... 33 of a 40-wide row
    n_dev, t0 = 40, 40
    guards = _guards(n_dev)
    arrays.update({k: v.interior for k, v in guards.items()})
    for k, v in guards.items():
        if k != "dev_switched_at":
            v.bits().zero_()
    step = ENV_STEP + A * P
    assert _raw_call(lib, b, arrays, trial0=t0, var_step=step) == 0, lib.stg_last_error()
    torch.cuda.synchronize()
    want = svpr.fused(b, m0, J, T, tgt, R, SIGMA2, dev_stride=n_dev, trials_per_device=Q, z_clip=CLIP, env_step=ENV_STEP, n_bins=N_BINS, trial0=t0,
                      var_step=step)
    for (k, v), y in zip(guards.items(), want[:4]):
        v.check_guards()
        assert np.array_equal(v.bits().cpu().numpy(), y), k
    g = guards["dev_switched_at"]
    g.check_guards()
    first, last = spr.touched(t0, R, Q)
    assert (first, last) == (8, 33) and want[4][..., first:last + 1].any() and np.array_equal(want[4].sum(axis=-1), want[0])
    assert np.array_equal(g.bits().cpu().numpy() - g.sentinel, want[4])
    assert g.untouched()[..., :first].all() and g.untouched()[..., last + 1:].all()              # per (a, g) row
    # it ADDS: a second call -- one wavefront per condition, no histogram, no class bytes, no per-device counts -- doubles the three
    # counts and leaves hist and dev_switched_at alone
    before = {k: v.bits().clone() for k, v in guards.items()}
    assert _raw_call(lib, b, arrays, trial0=t0, var_step=step, n_bins=0, max_waves=G2, dev_stride=0, null=("hist", "cls", "dev_switched_at")) == 0, \
        lib.stg_last_error()
    torch.cuda.synchronize()
    for (k, v), y in zip(guards.items(), want[:3] + (None, None)):
        v.check_guards()
        assert np.array_equal((v.bits() - before[k]).cpu().numpy(), y if y is not None else np.zeros(v.shape, dtype=np.int64)), k
    b.close()


# ------------------------------------------------------------------------------------------------
# i. the public method
# ------------------------------------------------------------------------------------------------
def test_write_verify_statistics_per_device_counts_are_plain_calls_on_the_drawn_devices(stg):
    from spin_torque_gym_amd import physics
    m0, J, T, tgt = _inputs("rk4", G2)
    q, d = 32, 5
    n = q * d
    variation = {"volume": 0.1, "damping": 0.05}
    solver = physics.SimpleLLGSSolver(method="rk4", noise_model="brown", seed=ssr.SEED)
    kw = dict(n_bins=N_BINS, env_step=ENV_STEP)
    res = solver.write_verify_statistics(m0, J, T, ssr.params(), n, variation=variation, trials_per_device=q, per_device=True, **kw)
    chunked = solver.write_verify_statistics(m0, J, T, ssr.params(), n, variation=variation, trials_per_device=q, per_device=True,
                                             max_trials_per_launch=50, **kw)
    plain_keys = {"n_switched_at", "n_ended_at", "n_failed", "n_attempted", "wer_after", "stderr", "p_switch", "mean_attempts", "hist", "bin_edges"}
    assert set(res) == plain_keys | {"dev_switched_at", "dev_trials", "dev_wer_after"}
    for k in res:
        assert np.array_equal(res[k], chunked[k]), k
    assert res["dev_switched_at"].shape == (A, G2, d) and (res["dev_trials"] == q).all()
    assert np.array_equal(res["dev_switched_at"].sum(axis=-1), res["n_switched_at"])
    assert np.array_equal(res["dev_wer_after"], 1.0 - np.cumsum(res["dev_switched_at"], axis=0) / q)
    drawn = solver.draw_devices(ssr.params(), d, variation, n_conditions=G2, trials_per_device=q)
    hist, n_end = np.zeros((G2, N_BINS), dtype=np.int64), np.zeros((A, G2), dtype=np.int64)
    for j in range(d):
        for g in range(G2):
            # condition g alone would sit at env id 0: both conditions are run, with the same stride, and condition g's counts are read
            one = solver.write_verify_statistics(m0, J, T, drawn["device_params"][g][j], q, trial_offset=q * j, trial_stride=n, **kw)
            assert np.array_equal(one["n_switched_at"][:, g], res["dev_switched_at"][:, g, j]), (g, j)
            hist[g] += one["hist"][g]
            n_end[:, g] += one["n_ended_at"][:, g]
    assert np.array_equal(hist, res["hist"]) and np.array_equal(n_end, res["n_ended_at"])
    assert ((0 < res["n_switched_at"][0]) & (res["n_switched_at"][0] < n)).all()
    # without per_device the dict is the plain one; variation = None is the plain call
    bare = solver.write_verify_statistics(m0, J, T, ssr.params(), n, variation=variation, trials_per_device=q, **kw)
    plain = solver.write_verify_statistics(m0, J, T, ssr.params(), n, **kw)
    none = solver.write_verify_statistics(m0, J, T, ssr.params(), n, variation=None, trials_per_device=q, per_device=True, **kw)
    assert set(bare) == set(plain) == set(none) == plain_keys
    for k in plain_keys:
        assert np.array_equal(bare[k], res[k]) and np.array_equal(plain[k], none[k]), k
    assert not np.array_equal(plain["hist"], res["hist"])


# ------------------------------------------------------------------------------------------------
# j. against the CPU oracle on the dumped devices
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,noise", svpr.ORACLE_FORMS)
def test_population_equals_the_oracle_on_the_dumped_devices(stg, oracle_mod, solver, noise):
    n, q, d, clip = svpr.ORACLE_R, svpr.ORACLE_Q, svpr.ORACLE_D, svpr.ORACLE_CLIP
    g = svr.G
    params = _devices(stg, solver, noise, g, d, spr.ORACLE_SIGMA, trials_per_device=q, trial_stride=n, z_clip=clip)
    (m0, J, T, tgt), rec, dev = svpr.oracle_run(stg, solver, noise, params)
    want = svpr.all_counts(rec, g, n, A, dev, d, n_bins=0)
    distance = svpr.threshold_distance(rec)
    print(f"{solver} {noise}: oracle switched_at {want[0].tolist()}, attempted {svr.attempted(want[1], n).tolist()}, "
          f"smallest |proj - threshold| over all attempts {distance:.2e}")
    assert distance > svr.MARGIN and not want[2].any()        # on THESE devices; a case that is not conditioned fails
    b = ssr.backend(stg, solver, noise, g)
    got = svpr.fused(b, m0, J, T, tgt, n, spr.ORACLE_SIGMA, dev_stride=d, trials_per_device=q, z_clip=clip, env_step=ENV_STEP)
    b.close()
    _same(got, want, (solver, noise))

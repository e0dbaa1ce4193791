"""stg_switch_verify / write_verify_statistics, host side (no GPU):

  * the binding: the symbol, its argument types against the header's declaration, the attempt limit;
  * the Python method through a recording fake backend: the shapes [A], [A,G], [A,P,G], relax, chunking and trial_stride, classes, the
    derived fields recomputed from the integers, refusals;
  * tests/switch_verify_ref.py chain -- the host statement of the rule the GPU tests hold the kernel to -- against the CPU oracle: the
    vectorised, masked chain equals a trial-by-trial loop over the oracle's single solves on the header's streams;
  * conditioning, a hard condition: in the oracle's run of the conditions of tests/test_gpu_switch_verify.py no projection, after any
    attempt, lies within switch_verify_ref.MARGIN = 1e-6 of threshold 0; no trial is excluded.  (A trial misclassified once changes
    everything after it.)  Measured here, smallest distance over all attempts: rk4 + brown 1.4e-3, euler + brown 5.0e-5, rk4 + ou
    4.0e-2, rk45 + white 2.2e-1.  The GPU tests of rk4 + ou and rk45 + white move the threshold to a median of stg_solve's own
    projections, whose neighbours are ~2e-8 away: that comparison is exact because both sides classify the SAME doubles, not because it
    is conditioned, and no oracle count is compared there."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import switch_stats_ref as ssr
import switch_verify_ref as svr
from conftest import stt_default_params
from switch_verify_ref import A, ENV_STEP, G, P, R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------
# the binding
# ------------------------------------------------------------------------------------------------
def test_symbol_and_argument_types():
    from spin_torque_gym_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "stg_switch_verify")
    header = open(os.path.join(ROOT, "include", "spintorque_hip.h")).read()
    decl = re.search(r"int stg_switch_verify\(([^;]*)\);", header)
    assert decl
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "double": C.c_double}
    want = [C.c_void_p if "*" in arg else ctype[arg.split()[0]] for arg in (a.strip() for a in decl.group(1).split(","))]
    assert len(want) == 21 and _lib.SYMBOLS["stg_switch_verify"] == (C.c_int, want)
    assert re.search(r"#define STG_MAX_VERIFY_ATTEMPTS 8\b", header) and _lib.STG_MAX_VERIFY_ATTEMPTS == 8
    assert _lib.ABI_VERSION == 5 and lib.stg_abi_version() == 5
    # argument checks come before the device: a NULL context is refused without a GPU
    assert lib.stg_switch_verify(None, 1, 1, 0, 1, 1, 1, None, None, None, None, 0, None, 0.0, 0, 0, None, None, None, None, None) == _lib.STG_E_INVALID


# ------------------------------------------------------------------------------------------------
# the Python method through a fake backend
# ------------------------------------------------------------------------------------------------
class _FakeBackend:
    """HipBackend's constructor signature and what write_verify_statistics calls.  switch_verify records its arguments; trial r of
    condition g (r counted from trial 0 of the whole range) ends at attempt (g + r) % A, switched unless r % 5 == 0, failed if
    r % 50 == 7, and lands in bin (g + r) % n_bins."""
    made = []

    def __init__(self, n, cfg, device_index=0, env_id0=0):
        self.n, self.cfg, self.closed, self.calls = n, cfg, False, []
        _FakeBackend.made.append(self)

    def set_params(self, table, cls=None):
        self.table, self.cls = table, cls

    def switch_verify(self, m0, J, T, target, n_trials, trial0=0, trial_stride=None, cond_cls=None, env_step=0, threshold=0.0, n_bins=0,
                      max_waves=0, out=None):
        g, a = m0.shape[1], J.shape[0]
        self.calls.append(dict(m0=m0.clone(), J=J.clone(), T=T.clone(), target=target.clone(), n_trials=n_trials, trial0=trial0,
                               trial_stride=trial_stride, cond_cls=cond_cls, env_step=env_step, threshold=threshold, n_bins=n_bins,
                               max_waves=max_waves, fresh=out is None))
        if out is None:
            out = (torch.zeros((a, g), dtype=torch.int64), torch.zeros((a, g), dtype=torch.int64), torch.zeros(g, dtype=torch.int64),
                   torch.zeros((g, n_bins), dtype=torch.int64) if n_bins else None)
        for k in range(g):
            for r in range(trial0, trial0 + n_trials):
                out[1][(k + r) % a, k] += 1
                out[0][(k + r) % a, k] += r % 5 != 0
                out[2][k] += r % 50 == 7
                if n_bins:
                    out[3][k, (k + r) % n_bins] += 1
        return out

    def close(self):
        self.closed = True


@pytest.fixture()
def fake():
    _FakeBackend.made = []
    return _FakeBackend


M0 = np.array([[0.0, 0.0, 1.0], [0.0, 0.6, 0.8], [0.0, 0.8, 0.6]])
JA, TA = np.array([1e9, 2e9]), np.array([1e-10, 2e-10])                              # [A]
JAG, TAG = np.outer(JA, [1.0, 2.0, 3.0]), np.outer(TA, [1.0, 1.5, 2.0])              # [A,G]


def _solver(fake, cls="SimpleLLGSSolver", **kw):
    from spin_torque_gym_amd import physics
    return getattr(physics, cls)(backend=fake, **kw)


def test_every_solver_class_has_the_method(fake):
    for cls, kw in (("SimpleLLGSSolver", dict(method="rk4", noise_model="brown")), ("RobustLLGSSolver", dict(method="euler", noise_model="brown")),
                    ("LLGSSolver", {})):
        out = _solver(fake, cls, **kw).write_verify_statistics(M0, JA, TA, stt_default_params(), 10)
        b = fake.made[-1]
        assert b.n == 3 and b.closed and b.cfg.include_thermal_fluctuations and len(b.calls) == 1
        assert b.cfg.solver == {"SimpleLLGSSolver": "rk4", "RobustLLGSSolver": "euler", "LLGSSolver": "rk45"}[cls]
        assert out["n_ended_at"].sum(axis=0).tolist() == [10, 10, 10]


def test_shapes_and_relax(fake):
    s = _solver(fake, method="rk4", noise_model="brown")
    s.write_verify_statistics(M0, JA, TA, stt_default_params(), 5, env_step=4)
    c = fake.made[-1].calls[0]
    assert c["J"].shape == (2, 1, 3) and np.array_equal(c["J"].numpy(), np.repeat(JA[:, None, None], 3, axis=2))
    assert np.array_equal(c["T"].numpy(), np.repeat(TA[:, None, None], 3, axis=2))
    assert np.array_equal(c["m0"].numpy(), M0.T) and np.array_equal(c["target"].numpy(), np.tile([0.0, 0.0, -1.0], (3, 1)).T)
    assert (c["n_trials"], c["trial0"], c["trial_stride"], c["env_step"], c["threshold"], c["n_bins"], c["cond_cls"]) == (5, 0, 5, 4, 0.0, 0, None)
    s.write_verify_statistics(M0, JAG, TAG, stt_default_params(), 5)
    c = fake.made[-1].calls[0]
    assert np.array_equal(c["J"].numpy(), JAG[:, None, :]) and np.array_equal(c["T"].numpy(), TAG[:, None, :])
    # mixed forms broadcast: [A,G] currents with [A] durations
    s.write_verify_statistics(M0, JAG, TA, stt_default_params(), 5)
    c = fake.made[-1].calls[0]
    assert np.array_equal(c["J"].numpy(), JAG[:, None, :]) and np.array_equal(c["T"].numpy(), np.repeat(TA[:, None, None], 3, axis=2))
    # [A,P,G] passes through; relax appends a J = 0 phase to every attempt (scalar or [G])
    J3, T3 = np.stack([JAG, -JAG], axis=1), np.stack([TAG, 2 * TAG], axis=1)
    s.write_verify_statistics(M0, J3, T3, stt_default_params(), 5)
    c = fake.made[-1].calls[0]
    assert c["J"].shape == (2, 2, 3) and np.array_equal(c["J"].numpy(), J3) and np.array_equal(c["T"].numpy(), T3)
    s.write_verify_statistics(M0, J3, T3, stt_default_params(), 5, relax=np.array([1e-10, 0.0, 3e-10]))
    c = fake.made[-1].calls[0]
    assert c["J"].shape == (2, 3, 3) and np.array_equal(c["J"].numpy()[:, :2], J3) and not c["J"].numpy()[:, 2].any()
    assert np.array_equal(c["T"].numpy()[:, :2], T3) and np.array_equal(c["T"].numpy()[:, 2], np.tile([1e-10, 0.0, 3e-10], (2, 1)))
    s.write_verify_statistics(M0, JA, TA, stt_default_params(), 5, relax=5e-11)
    c = fake.made[-1].calls[0]
    assert c["J"].shape == (2, 2, 3) and (c["T"].numpy()[:, 1] == 5e-11).all() and c["J"].is_contiguous() and c["T"].is_contiguous()
    n_made = len(fake.made)
    for args, kw in (((np.ones(9), np.ones(9)), {}), ((np.ones((2, 4, 3)), np.ones((2, 4, 3))), dict(relax=1e-10)),
                     ((np.ones((2, 5, 3)), np.ones((2, 5, 3))), {}), ((JA, np.ones(3)), {}), ((np.ones((2, 2)), TA), {}),
                     ((np.ones((2, 2, 3)), np.ones((2, 3, 3))), {}), ((JA, TA), dict(relax=-1e-10)), ((1e9, 1e-10), {}),
                     ((JA, TA), dict(n_bins=65)), ((JA, TA), dict(max_trials_per_launch=0)), ((JA, TA), dict(trial_offset=-1)),
                     ((JA, TA), dict(trial_offset=3, trial_stride=7))):
        with pytest.raises(ValueError):
            s.write_verify_statistics(M0, *args, stt_default_params(), 5, **kw)
    for n in (0, -3):
        with pytest.raises(ValueError, match="n_trials"):
            s.write_verify_statistics(M0, JA, TA, stt_default_params(), n)
    assert len(fake.made) == n_made                                                    # refused before a context exists


def test_chunking_classes_and_derived_fields(fake):
    s = _solver(fake, method="rk4", noise_model="brown")
    n_trials = 1000
    whole = s.write_verify_statistics(M0, JA, TA, stt_default_params(), n_trials, n_bins=7)
    parts = s.write_verify_statistics(M0, JA, TA, stt_default_params(), n_trials, n_bins=7, max_trials_per_launch=300)
    calls = fake.made[-1].calls
    assert len(fake.made[-2].calls) == 1 and len(fake.made) == 2
    assert [(c["trial0"], c["n_trials"], c["trial_stride"], c["fresh"]) for c in calls] == \
        [(0, 300, 1000, True), (300, 300, 1000, False), (600, 300, 1000, False), (900, 100, 1000, False)]
    assert set(whole) == {"n_switched_at", "n_ended_at", "n_failed", "n_attempted", "wer_after", "stderr", "p_switch", "mean_attempts", "hist",
                          "bin_edges"}
    for k in whole:
        assert np.array_equal(whole[k], parts[k]), k
    n_sw, n_end = whole["n_switched_at"], whole["n_ended_at"]
    assert n_sw.dtype == np.int64 and n_sw.shape == (2, 3) and (n_end.sum(axis=0) == n_trials).all() and whole["n_failed"].tolist() == [20, 20, 20]
    assert np.array_equal(whole["n_attempted"], np.stack([np.full(3, n_trials), n_trials - n_end[0]]))
    wer = 1.0 - np.cumsum(n_sw, axis=0) / n_trials
    assert np.array_equal(whole["wer_after"], wer) and np.array_equal(whole["stderr"], np.sqrt(wer * (1 - wer) / n_trials))
    assert np.array_equal(whole["p_switch"], 1.0 - wer[1]) and np.array_equal(whole["mean_attempts"], (n_end[0] + 2 * n_end[1]) / n_trials)
    assert whole["mean_attempts"].tolist() == [1.5, 1.5, 1.5]
    assert (whole["hist"].sum(axis=1) == n_trials).all() and np.array_equal(whole["bin_edges"], np.linspace(-1.0, 1.0, 8))
    assert s.solve_count == 2 * 3 * n_trials
    # a rank of a sharded job: its own trial range inside a common stride
    s.write_verify_statistics(M0, JA, TA, stt_default_params(), 500, trial_offset=500, trial_stride=1000, max_trials_per_launch=400)
    assert [(c["trial0"], c["n_trials"], c["trial_stride"]) for c in fake.made[-1].calls] == [(500, 400, 1000), (900, 100, 1000)]
    # classes, targets, threshold
    tables = [stt_default_params(), stt_default_params(volume=5e-24)]
    tg = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    s.write_verify_statistics(M0, JA, TA, tables, 5, class_index=[1, 0, 1], target=tg, threshold=0.25)
    b = fake.made[-1]
    assert len(b.table) == 2 and b.table[1].volume == 5e-24 and b.cls.dtype == torch.uint8 and b.cls.tolist() == [1, 0, 1]
    c = b.calls[0]
    assert c["cond_cls"].tolist() == [1, 0, 1] and c["threshold"] == 0.25 and np.array_equal(c["target"].numpy(), tg.T)
    for kw in (dict(), dict(class_index=[0, 1, 2])):
        with pytest.raises(ValueError, match="class_index"):
            s.write_verify_statistics(M0, JA, TA, tables, 5, **kw)
    with pytest.raises(ValueError, match="attempts"):
        s.write_verify_statistics(M0, np.ones(9), np.ones(9), stt_default_params(), 5)


# ------------------------------------------------------------------------------------------------
# the reference against the CPU oracle, and its conditioning
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stg(oracle_mod):
    import spin_torque_gym_amd as s
    return s


_RUNS = {}


def _oracle_run(stg, solver, noise):
    if (solver, noise) not in _RUNS:
        m0, J, T, tgt = svr.conditions()
        if solver == "rk45":
            J = J * ssr.RK45_J_SCALE
        rec = svr.chain(svr.oracle_solve(stg, solver, noise, G, R), m0, J, T, tgt, R, env_step=ENV_STEP)
        _RUNS[(solver, noise)] = (m0, J, T, tgt), rec
    return _RUNS[(solver, noise)]


@pytest.mark.parametrize("solver,noise", svr.FORMS)
def test_oracle_run_is_conditioned(stg, solver, noise):
    """the hard condition: every projection after every attempt further than MARGIN from threshold 0, with no trial excluded"""
    _, rec = _oracle_run(stg, solver, noise)
    pa = rec["proj_after"]
    ran = ~np.isnan(pa)
    n_sw, n_end, n_failed, _ = svr.counts(rec, G, R, A)
    att = svr.attempted(n_end, R)
    distance = float(np.abs(pa[ran]).min())
    print(f"{solver} {noise}: switched_at {n_sw.tolist()}, attempted {att.tolist()}, smallest |proj - threshold| over all attempts {distance:.2e}")
    assert svr.MARGIN == 1e-6 and distance > svr.MARGIN
    assert not n_failed.any() and np.array_equal(ran.reshape(A, G, R).sum(axis=2), att) and (n_end.sum(axis=0) == R).all()
    if noise == "brown":
        assert ((0 < n_sw) & (n_sw < att)).all()                                       # the field decides at every attempt of every condition
        assert (np.abs(n_sw[0] / R - 0.4) < 0.1).all()                                 # about 0.4 per attempt


@pytest.mark.parametrize("solver", ("rk4", "euler"))
def test_chain_is_the_headers_rule_trial_by_trial(stg, oracle_mod, solver):
    """trial r of condition g, spelled out with the oracle's single solve on the stream of env id g R + r at env_step + a P + p: the
    attempts until the trial is switched, failed or out of attempts.  The vectorised chain ends every trial at the same attempt with the
    same final projection"""
    from helpers import oracle_config, oracle_params
    (m0, J, T, tgt), rec = _oracle_run(stg, solver, "brown")
    cfg = oracle_config(ssr.env_config(solver, "brown"))
    po = oracle_params(ssr.flat_tables(stg))[0]
    for g in range(G):
        for r in range(0, R, 3):
            x = m0[g]
            for a in range(A):
                for p in range(P):
                    o = oracle_mod.simple_solve(x, T[a, p, g], po, cfg, J[a, p, g], env_id=g * R + r, env_step=ENV_STEP + a * P + p)
                    assert o["success"]
                    x = o["m_final"]
                pr = ((x[0] * tgt[g, 0]) + (x[1] * tgt[g, 1])) + (x[2] * tgt[g, 2])
                assert rec["proj_after"][a, g * R + r] == pr, (g, r, a)
                if pr > 0.0 or a == A - 1:
                    break
            i = g * R + r
            assert rec["ended_at"][i] == a and rec["switched"][i] == (pr > 0.0) and rec["proj"][i] == pr and not rec["failed"][i]
            assert np.isnan(rec["proj_after"][a + 1:, i]).all()


def test_chain_masks_skipped_and_failed_phases(stg):
    """a skipped phase passes m through; an attempt of skipped phases only verifies the same m again; a failed solve ends the trial at
    its attempt with the m it had, classified like any other"""
    (m0, J, T, tgt), plain = _oracle_run(stg, "rk4", "brown")
    T = T.copy()
    T[1, :, 1] = 0.0                                                                   # condition 1: attempt 1 does nothing
    T[1, 0, 2] = -1e-11                                                                # condition 2: attempt 1's pulse fails
    rec = svr.chain(svr.oracle_solve(stg, "rk4", "brown", G, R), m0, J, T, tgt, R, env_step=ENV_STEP)
    n_sw, n_end, n_failed, _ = svr.counts(rec, G, R, A)
    c1, c2 = slice(R, 2 * R), slice(2 * R, 3 * R)
    went_on = ~np.isnan(rec["proj_after"][1, c1])
    assert np.array_equal(rec["proj_after"][1, c1][went_on], rec["proj_after"][0, c1][went_on]) and n_end[1, 1] == 0 and n_sw[2, 1] > 0
    assert np.array_equal(rec["proj_after"][0], plain["proj_after"][0])
    survivors = plain["proj_after"][0, c2] <= 0.0
    assert n_failed.tolist() == [0, 0, int(survivors.sum())] and np.array_equal(rec["failed"][c2], survivors)
    assert (rec["ended_at"][c2][survivors] == 1).all() and not rec["switched"][c2][survivors].any() and n_end[2, 2] == 0
    assert np.array_equal(rec["proj"][c2][survivors], plain["proj_after"][0, c2][survivors])
    # counts of a selection add up to the whole
    sel = np.concatenate([np.arange(g * R, g * R + 50) for g in range(G)])
    rest = np.setdiff1d(np.arange(G * R), sel)
    for x, y, z in zip(svr.counts(rec, G, R, A, n_bins=7, select=sel), svr.counts(rec, G, R, A, n_bins=7, select=rest), svr.counts(rec, G, R, A, n_bins=7)):
        assert np.array_equal(x + y, z)

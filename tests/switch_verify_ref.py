"""The host statement of stg_switch_verify's rule (include/spintorque_hip.h), shared by tests/test_gpu_switch_verify.py and
tests/test_switch_verify_host.py: given a `solve(m, J, T, env_step)` over the G R replicated problems (problem g R + r = trial r of
condition g) it chains attempts and phases, masks the trials that have ended, and reduces with NumPy to the four arrays.

  * chain: attempt a, phase p is ONE solve of all G R problems at env_step + a P + p, of which only the live trials take the result --
    a phase with T == 0 is skipped, a trial whose solve failed keeps the m that solve handed back and ends with this attempt; after
    every attempt the live trials are classified with switch_stats_ref.proj, and a trial ends when it is switched, failed, or a = A - 1;
  * counts: n_switched_at [A,G], n_ended_at [A,G], n_failed [G], hist [G,n_bins] from the per-trial record of chain;
  * gpu_solve / oracle_solve: the two solves the tests chain -- HipBackend.solve (stg_solve, the unchanged kernel) and the CPU oracle;
  * the conditions of the tests: switch_stats_ref.conditions() with a 0.1 ns pulse and a 0.05 ns relax per attempt, J scaled
    1.0 / 1.1 / 1.2 over the attempts.

Nothing here imports the GPU at module level."""
import numpy as np

import switch_stats_ref as ssr

G, R, A, P = ssr.G, 130, 3, 2
ENV_STEP = 3
PULSE, RELAX = 1e-10, 5e-11
SCALES = (1.0, 1.1, 1.2)
FORMS = (("rk4", "brown"), ("euler", "brown"), ("rk4", "ou"), ("rk45", "white"))
MARGIN = 1e-6                                              # no projection of the oracle's run may lie this close to the threshold
# the current of attempt 0 as a fraction of brown_ref.SWITCH["J"], per condition: about 0.4 of the trials switch per attempt under the
# Brown field (measured on the CPU oracle, tests/test_switch_verify_host.py prints the counts)
J_FRACTION = np.array([0.1, 0.25, 0.38])


def conditions(n_attempts=A, scales=SCALES):
    """m0 [G,3], J [A,P,G], T [A,P,G], target [G,3]: the starts of switch_stats_ref.conditions(); attempt a is a PULSE at J_FRACTION x
    SWITCH["J"] x scales[a] followed by a RELAX at J = 0"""
    import brown_ref as br
    m0, _, _, tgt = ssr.conditions()
    J = np.zeros((n_attempts, P, G))
    T = np.empty((n_attempts, P, G))
    for a in range(n_attempts):
        J[a, 0] = br.SWITCH["J"] * J_FRACTION * scales[a % len(scales)]
    T[:, 0], T[:, 1] = PULSE, RELAX
    return m0, J, T, tgt


def chain(solve, m0, J, T, tgt, n_trials, env_step=0, threshold=0.0):
    """solve(m [3,n], J [n], T [n], env_step) -> (m_final [3,n], success [n]) over the n = G n_trials replicated problems.  m0, tgt
    [G,3]; J, T [A,P,G].  Returns the per-trial record: dict(ended_at [n] -- the trial's last attempt --, switched [n], failed [n],
    proj [n] -- the final projection --, proj_after [A,n] -- the projection after attempt a, NaN where the trial did not run it)."""
    g = m0.shape[0]
    n = g * n_trials
    n_att, n_ph = J.shape[0], J.shape[1]
    rep = lambda x: np.repeat(x, n_trials)                                        # noqa: E731
    tg = np.repeat(tgt, n_trials, axis=0)
    m = np.repeat(m0, n_trials, axis=0).T.copy()
    live = np.ones(n, dtype=bool)
    ended_at = np.full(n, -1, dtype=np.int64)
    switched, failed = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    proj_after = np.full((n_att, n), np.nan)
    for a in range(n_att):
        bad = np.zeros(n, dtype=bool)                                             # a solve of this attempt failed
        for p in range(n_ph):
            Tp = rep(T[a, p])
            runs = live & ~bad & (Tp != 0.0)
            if not runs.any():
                continue
            mf, ok = solve(m, rep(J[a, p]), Tp, (env_step + a * n_ph + p) % 2 ** 32)
            m = np.where(runs[None, :], mf, m)
            bad |= runs & ~ok
        pr = ssr.proj(m, tg)
        sw = live & (pr > threshold)
        proj_after[a, live] = pr[live]
        ends = live & (sw | bad | (a == n_att - 1))
        ended_at[ends] = a
        switched |= ends & sw
        failed |= live & bad
        live &= ~ends
    assert not live.any() and (ended_at >= 0).all()
    return dict(ended_at=ended_at, switched=switched, failed=failed, proj=ssr.proj(m, tg), proj_after=proj_after)


def counts(rec, g, n_trials, n_attempts, n_bins=0, select=None):
    """(n_switched_at [A,G], n_ended_at [A,G], n_failed [G], hist [G,n_bins] or None) of a chain's record; `select`: a bool mask [n]
    or index array of the trials that count (a chunk of the trial range)"""
    cond = np.repeat(np.arange(g), n_trials)
    keep = np.ones(g * n_trials, dtype=bool) if select is None else np.zeros(g * n_trials, dtype=bool)
    if select is not None:
        keep[select] = True
    n_end = np.zeros((n_attempts, g), dtype=np.int64)
    n_sw = np.zeros((n_attempts, g), dtype=np.int64)
    np.add.at(n_end, (rec["ended_at"][keep], cond[keep]), 1)
    np.add.at(n_sw, (rec["ended_at"][keep & rec["switched"]], cond[keep & rec["switched"]]), 1)
    n_failed = np.bincount(cond[keep & rec["failed"]], minlength=g).astype(np.int64)
    hist = None
    if n_bins:
        hist = np.zeros((g, n_bins), dtype=np.int64)
        np.add.at(hist, (cond[keep], ssr.bins(rec["proj"], n_bins)[keep]), 1)
    return n_sw, n_end, n_failed, hist


def attempted(n_end, n_trials):
    """trials that ran attempt a: R - sum_{b<a} n_ended_at[b]"""
    return n_trials - (np.cumsum(n_end, axis=0) - n_end)


def gpu_solve(stg, solver, noise, g, n_trials, tables=None, cond_cls=None, env_id0=0, **cfg):
    """(solve, close) over HipBackend.solve -- stg_solve -- on a context of g n_trials problems"""
    import torch
    cls = None if cond_cls is None else np.repeat(cond_cls, n_trials).astype(np.uint8)
    b = ssr.backend(stg, solver, noise, g * n_trials, tables, cls, env_id0=env_id0, **cfg)

    def solve(m, J, T, env_step):
        out = b.solve(torch.from_numpy(np.ascontiguousarray(m)), torch.from_numpy(np.ascontiguousarray(J)),
                      torch.from_numpy(np.ascontiguousarray(T)), env_step=env_step)
        torch.cuda.synchronize()
        return out["m_final"].cpu().numpy(), out["success"].cpu().numpy() != 0
    return solve, b.close


def oracle_solve(stg, solver, noise, g, n_trials, env_id0=0, **cfg):
    """solve over the CPU oracle (helpers.OracleBackend), which reproduces the Philox streams: one backend of g n_trials problems, so
    its problem g R + r has the stream of env id env_id0 + g R + r -- trial_stride = R"""
    import torch
    from helpers import OracleBackend
    b = OracleBackend(g * n_trials, ssr.env_config(solver, noise, **cfg), 0, env_id0=env_id0)
    b.set_params(ssr.flat_tables(stg))

    def solve(m, J, T, env_step):
        out = b.solve(torch.from_numpy(np.ascontiguousarray(m)), torch.from_numpy(np.ascontiguousarray(J)),
                      torch.from_numpy(np.ascontiguousarray(T)), env_step=env_step)
        return out["m_final"].numpy(), out["success"].numpy() != 0
    return solve


def median_threshold(rec, n_trials, g=1):
    """the median of condition g's projections after the FIRST attempt (every trial runs it): under the white and the
    Ornstein-Uhlenbeck field the trials of a condition end close to each other, all on one side of 0; against this threshold the first
    verify still depends on every trial's own stream"""
    return float(np.median(rec["proj_after"][0, g * n_trials:(g + 1) * n_trials]))


def fused(b, m0, J, T, tgt, n_trials, **kw):
    """HipBackend.switch_verify on condition-major NumPy inputs -> the four arrays as NumPy (hist None without bins)"""
    import torch
    out = b.switch_verify(torch.from_numpy(m0.T.copy()), torch.from_numpy(np.ascontiguousarray(J)), torch.from_numpy(np.ascontiguousarray(T)),
                          torch.from_numpy(tgt.T.copy()), n_trials, **kw)
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in out)

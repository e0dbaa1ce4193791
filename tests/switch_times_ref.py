"""References of stg_switch_times shared by its GPU and its CPU tests (tests/test_gpu_switch_times.py, tests/test_switch_times_host.py),
next to tests/switch_stats_ref.py and tests/switch_stats_wave_ref.py, whose conditions, tables, classification and margin they use:

  * first_passage / time_bins / counts: the header's crossing rule, crossing-time estimate and time bin in NumPy, each operation
    rounded, from recorded rows (t [rows,N], m [rows,3,N], n_points, success), reduced to the six arrays of the entry;
  * host_path: the definition through EXISTING code -- HipBackend.solve(traj_cap=) / solve(wave=, traj_cap=) over the replicated
    problems, phase after phase, one context per condition created at the env id of the condition's first trial (so trial0,
    trial_stride and env_id0 are free);
  * numpy_case: an independent statement that goes through no library solve -- tests/brown_ref.py (NumPy) with trajectory=True under
    the oracle's Philox normals by the header's stream rule: the pulse of switch_stats_ref.conditions() watched, a relax phase behind it;
  * fused: HipBackend.switch_times on the same condition-major inputs.

Nothing here imports the GPU at module level."""
import numpy as np

import brown_ref as br
import switch_stats_ref as ssr
import switch_stats_wave_ref as swr

G = ssr.G
NUMPY_R, NUMPY_ENV_STEP, NUMPY_BINS = ssr.ORACLE_R, ssr.ORACLE_ENV_STEP, ssr.ORACLE_BINS
# 25 divides the n = 100 sub-steps of the pulses: a midpoint (k - 1/2) T / 100 scaled by 25 / T is (2 k - 1) / 8, never an integer
NUMPY_TBINS = 25
NUMPY_RELAX = 2e-11                      # the J = 0 phase behind the watched pulse [s]
NUMPY_FORMS = (("rk4", "brown"), ("euler", "brown"))


# ------------------------------------------------------------------------------------------------
# (a) the header's first passage in NumPy
# ------------------------------------------------------------------------------------------------
def first_passage(t, m, n_points, success, tgt, threshold=0.0):
    """t [rows,N], m [rows,3,N]: the recorded rows of N solves, row k <= n_points[i] valid for problem i; tgt [N,3] the target rows.
    proj_k = ((m_k.x tx) + (m_k.y ty)) + (m_k.z tz); the problem crosses at the first valid k with proj_k > threshold (NaN: never) and
    only if its solve succeeded; t_x = 0.0 for k = 0, else 0.5 * (t_{k-1} + t_k).  Returns dict(crossed [N], t_x [N], k [N], proj
    [rows,N], valid [rows,N])."""
    t, m = np.asarray(t), np.asarray(m)
    rows, n = t.shape
    pr = ((m[:, 0] * tgt[None, :, 0]) + (m[:, 1] * tgt[None, :, 1])) + (m[:, 2] * tgt[None, :, 2])
    valid = np.arange(rows)[:, None] <= np.asarray(n_points)[None, :]
    with np.errstate(invalid="ignore"):
        hit = (pr > threshold) & valid
    k = hit.argmax(axis=0)
    i = np.arange(n)
    t_x = np.where(k == 0, 0.0, 0.5 * (t[np.maximum(k - 1, 0), i] + t[k, i]))
    return dict(crossed=hit.any(axis=0) & np.asarray(success, dtype=bool), t_x=t_x, k=k, proj=pr, valid=valid)


def time_bins(t_x, T, n_tbins):
    """the header's time bin: min(n_tbins - 1, max(0, (int)floor(t_x * ((double)n_tbins / T)))), clamped before the conversion"""
    with np.errstate(all="ignore"):
        b = np.floor(t_x * (float(n_tbins) / T))
    b = np.where(np.isnan(b), 0.0, b)
    return np.minimum(n_tbins - 1, np.maximum(0, b)).astype(np.int64)


def counts(m, failed, crossed, t_x, tgt, T_watch, R, threshold=0.0, n_bins=0, n_tbins=0):
    """m [3, G R], failed, crossed, t_x [G R] (problem g R + r = trial r of condition g), tgt [G,3], T_watch [G] -> the six arrays of
    stg_switch_times: (n_switched, n_failed, hist | None, n_crossed, n_returned, t_hist | None)"""
    g = tgt.shape[0]
    n_sw, n_failed, hist = ssr.host_counts(m, failed, tgt, R, threshold=threshold, n_bins=n_bins)
    with np.errstate(invalid="ignore"):
        switched = ssr.proj(m, np.repeat(tgt, R, axis=0)) > threshold
    n_cr = crossed.reshape(g, R).sum(axis=1)
    n_ret = (crossed & ~switched).reshape(g, R).sum(axis=1)
    t_hist = None
    if n_tbins:
        b = time_bins(t_x, np.repeat(T_watch, R), n_tbins).reshape(g, R)
        c = crossed.reshape(g, R)
        t_hist = np.stack([np.bincount(b[k][c[k]], minlength=n_tbins) for k in range(g)])
    return n_sw, n_failed, hist, n_cr, n_ret, t_hist


# ------------------------------------------------------------------------------------------------
# (b) the definition through existing code
# ------------------------------------------------------------------------------------------------
def host_path(stg, solver, noise, m0, J, T, tgt, R, watch_phase=0, cur=None, fld=None, threshold=0.0, env_step=0, trial0=0,
              trial_stride=None, tables=None, cond_cls=None, env_id0=0, **cfg):
    """The existing path.  Condition g's R trials are the problems of ONE context of R envs created at env id env_id0 + g trial_stride +
    trial0 (the header's stream rule); one solve per phase at env_step + p with m_final fed back as m0.  The watched phase is solved
    twice: once for n_points, then with traj_cap = max(n_points) + 1 -- stg_solve_traj, or stg_solve_wave with the condition's tables
    replicated per trial when cur / fld (condition-major knots, as swr.trapezoid / swr.field_ramp give them) are given -- and its rows
    go through first_passage.  A phase with T == 0 is skipped, a trial whose solve failed keeps the m that solve handed back and takes
    no further phase; a trial whose watched phase is skipped, is not reached or fails has not crossed.  J, T [P,G].
    Returns dict(m [3, G R], failed [G R], crossed [G R], t_x [G R])."""
    import torch
    g = m0.shape[0]
    stride = trial0 + R if trial_stride is None else trial_stride
    wave = cur is not None or fld is not None
    ms, fs, cs, ts = [], [], [], []
    for k in range(g):
        cls = None if tables is None or len(tables) < 2 else np.full(R, 0 if cond_cls is None else cond_cls[k], dtype=np.uint8)
        b = ssr.backend(stg, solver, noise, R, tables, cls, env_id0=env_id0 + k * stride + trial0, **cfg)
        m = torch.from_numpy(np.repeat(m0[k:k + 1], R, axis=0).T.copy()).cuda()
        failed = torch.zeros(R, dtype=torch.bool, device="cuda")
        crossed, t_x = np.zeros(R, dtype=bool), np.zeros(R)
        for p in range(T.shape[0]):
            if T[p, k] == 0.0:
                continue
            Jp, Tp = torch.full((R,), float(J[p, k]), dtype=torch.float64), torch.full((R,), float(T[p, k]), dtype=torch.float64)
            kw = {}
            if p == watch_phase and wave:
                one = lambda kn: None if kn is None else tuple(np.asarray(a)[:, k:k + 1] for a in kn)         # noqa: E731
                kw["wave"] = swr.wave_dict(one(cur), one(fld), R)
            out = b.solve(m, Jp, Tp, env_step=env_step + p, **kw)
            if p == watch_phase:
                cap = max(1, int(out["n_points"].max().item()) + 1)
                out = b.solve(m, Jp, Tp, env_step=env_step + p, traj_cap=cap, **kw)
                torch.cuda.synchronize()
                live = (~failed).cpu().numpy()
                fp = first_passage(out["t"].cpu().numpy(), out["m"].cpu().numpy(), out["n_points"].cpu().numpy(),
                                   out["success"].cpu().numpy() != 0, np.repeat(tgt[k:k + 1], R, axis=0), threshold)
                crossed, t_x = fp["crossed"] & live, fp["t_x"]
            live = ~failed
            m = torch.where(live[None, :], out["m_final"], m)
            failed = failed | (live & (out["success"] == 0))
        torch.cuda.synchronize()
        ms.append(m.cpu().numpy())
        fs.append(failed.cpu().numpy())
        cs.append(crossed)
        ts.append(t_x)
        b.close()
    return dict(m=np.concatenate(ms, axis=1), failed=np.concatenate(fs), crossed=np.concatenate(cs), t_x=np.concatenate(ts))


def host_counts(h, tgt, T_watch, R, threshold=0.0, n_bins=0, n_tbins=0):
    """counts() of a host_path result"""
    return counts(h["m"], h["failed"], h["crossed"], h["t_x"], tgt, T_watch, R, threshold=threshold, n_bins=n_bins, n_tbins=n_tbins)


def fused(b, m0, J, T, tgt, R, watch_phase=0, cur=None, fld=None, **kw):
    """HipBackend.switch_times on condition-major NumPy inputs (m0, tgt [G,3]; J, T [P,G]; knots as swr.trapezoid / swr.field_ramp give
    them, or none) -> the six arrays as NumPy (None for an absent histogram)"""
    import torch
    wave = None if cur is None and fld is None else swr.wave_dict(cur, fld)
    out = b.switch_times(torch.from_numpy(m0.T.copy()), torch.from_numpy(np.ascontiguousarray(J)), torch.from_numpy(np.ascontiguousarray(T)),
                         torch.from_numpy(tgt.T.copy()), R, watch_phase=watch_phase, wave=wave, **kw)
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in out)


# ------------------------------------------------------------------------------------------------
# (c) the independent statement: NumPy under the oracle's normals, by the header's stream rule
# ------------------------------------------------------------------------------------------------
_CASES = {}


def numpy_case(oracle, method, R=NUMPY_R):
    """P = 2, trial_stride = R, env_step = NUMPY_ENV_STEP: the rectangular pulse of ssr.conditions(), watched, and NUMPY_RELAX at J = 0
    behind it.  Trial r of condition g is brown_ref.solve(trajectory=True) of (m0[g], J[g],
    T[g]) under the Brown field, its sub-step i taking draw i of the oracle's stream (ssr.SEED, g R + r, NUMPY_ENV_STEP), then
    brown_ref.solve of the relax phase on the stream at NUMPY_ENV_STEP + 1.  (brown_ref.solve records the trajectory of one problem per call, so the
    pulses are G R calls: about 50 ms each under rk4, once per process.)  Returns dict(J, T [2,G], m [3, G R], failed,
    crossed, t_x, counts at threshold 0 with NUMPY_BINS and NUMPY_TBINS bins, and the three conditioning distances: row_distance --
    of any proj_k up to and including the crossing row to the threshold; bin_distance -- of any crossed trial's scaled t_x to an
    integer; distance -- of a final projection to a decision, ssr.edge_distance)."""
    import waveform_ref
    key = (method, R)
    if key not in _CASES:
        m0, Jp, Tp, tgt = ssr.conditions()
        J, T = np.stack([Jp, np.zeros(G)]), np.stack([Tp, np.full(G, NUMPY_RELAX)])
        s = br.strength(oracle, ssr.params())
        n = G * R
        n_sub, _ = br.substeps(np.repeat(Tp, R))
        rows = int(n_sub.max()) + 1
        t, m = np.zeros((rows, n)), np.zeros((rows, 3, n))
        ok, mf = np.zeros(n, dtype=bool), np.zeros((n, 3))
        for i in range(n):
            g = i // R
            z = waveform_ref.normals(oracle, ssr.SEED, i, NUMPY_ENV_STEP, int(n_sub[i]))[None]
            res = br.solve(m0[g:g + 1], Tp[g:g + 1], ssr.params(), s, z, method, J=Jp[g:g + 1], trajectory=True)
            k = int(n_sub[i]) + 1
            t[:k, i], m[:k, :, i] = res["t"], res["m"]
            ok[i], mf[i] = res["success"][0], res["m_final"][0]
        rep = lambda a: np.repeat(a, R, axis=0)                                       # noqa: E731
        fp = first_passage(t, m, n_sub, ok, rep(tgt), 0.0)
        # the relax phase, for the trials whose pulse succeeded
        n_rel, _ = br.substeps(rep(T[1]))
        z = np.stack([waveform_ref.normals(oracle, ssr.SEED, i, NUMPY_ENV_STEP + 1, int(n_rel[i])) for i in range(n)])
        rel = br.solve(mf, rep(T[1]), ssr.params(), s, z, method, J=np.zeros(n))
        m_end = np.where(ok[:, None], rel["m_final"], mf).T.copy()
        failed = ~ok | ~rel["success"]
        pr = ssr.proj(m_end, rep(tgt))
        upto = fp["valid"] & (np.arange(rows)[:, None] <= np.where(fp["crossed"], fp["k"], rows)[None, :])
        scaled = fp["t_x"][fp["crossed"]] * (float(NUMPY_TBINS) / rep(Tp)[fp["crossed"]])
        _CASES[key] = dict(J=J, T=T, m=m_end, failed=failed, crossed=fp["crossed"], t_x=fp["t_x"], proj=pr,
                           counts=counts(m_end, failed, fp["crossed"], fp["t_x"], tgt, Tp, R, n_bins=NUMPY_BINS, n_tbins=NUMPY_TBINS),
                           row_distance=float(np.abs(fp["proj"][upto]).min()),
                           bin_distance=float(np.abs(scaled - np.round(scaled)).min()) if len(scaled) else np.inf,
                           distance=ssr.edge_distance(pr, NUMPY_BINS))
    return _CASES[key]

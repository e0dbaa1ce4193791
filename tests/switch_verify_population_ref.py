"""The host statement of stg_switch_verify_population's rule (include/spintorque_hip.h), shared by
tests/test_gpu_switch_verify_population.py and tests/test_switch_verify_population_host.py.  It composes two existing references and
adds nothing of its own to either rule:

  * switch_verify_ref.chain -- attempts, phases, the host-side mask, the verify -- over a `solve` of the G R replicated problems;
  * switch_population_ref -- the draw (population, oracle_normals), the devices as ONE class table (table_of, records) and the class
    byte of every replicated problem (trial_classes): problem g R + r is trial r of condition g, of device r // Q.

So the reference of a population under verify is the chain over the UNCHANGED stg_solve (or the CPU oracle's solve) on a class table
that holds the dumped devices.  device_counts reduces a chain's record to dev_switched_at [A, G, n_dev].

Nothing here imports the GPU at module level."""
import numpy as np

import switch_population_ref as spr
import switch_stats_ref as ssr
import switch_verify_ref as svr

# the oracle case: switch_verify_ref.conditions() (G = 3, A = 3, P = 2) at R = 192, three trials per device, 64 devices per condition
ORACLE_R, ORACLE_Q, ORACLE_D, ORACLE_CLIP = spr.ORACLE_R, spr.ORACLE_Q, spr.ORACLE_D, spr.ORACLE_CLIP
ORACLE_FORMS = (("rk4", "brown"), ("euler", "brown"))


def class_table(stg, params, n_trials, Q):
    """the devices params [5, G, D] as one class table and the replicated problems' place in it: (records [G D], cls [G n_trials],
    dev [n_trials] -- the device of trial r, counted from trial 0)"""
    g, d = params.shape[1:]
    recs, _ = spr.table_of(stg, params)
    cls, dev = spr.trial_classes(g, n_trials, Q, d)
    return recs, cls, dev


def gpu_solve(stg, solver, noise, recs, cls, env_id0=0, **cfg):
    """(solve, close) over HipBackend.solve -- stg_solve, the unchanged kernel -- on a context of len(cls) problems whose class table
    is `recs` and whose problem i has class cls[i]"""
    import torch
    b = ssr.backend(stg, solver, noise, len(cls), recs, cls, env_id0=env_id0, **cfg)

    def solve(m, J, T, env_step):
        out = b.solve(torch.from_numpy(np.ascontiguousarray(m)), torch.from_numpy(np.ascontiguousarray(J)),
                      torch.from_numpy(np.ascontiguousarray(T)), env_step=env_step)
        torch.cuda.synchronize()
        return out["m_final"].cpu().numpy(), out["success"].cpu().numpy() != 0
    return solve, b.close


def oracle_solve(stg, solver, noise, params, n_trials, Q, **cfg):
    """solve over the CPU oracle, which knows nothing of populations: as switch_population_ref.oracle_path, one OracleBackend of
    n_trials problems per condition g at env_id0 = g n_trials (trial_stride = n_trials, trial0 = 0), its class table the condition's
    devices params[:, g] and its cls the device of each trial"""
    import torch
    from helpers import OracleBackend
    g = params.shape[1]
    nominal = ssr.flat_tables(stg)[0]
    dev = spr.device_of(np.arange(n_trials), Q)
    backends = []
    for k in range(g):
        b = OracleBackend(n_trials, ssr.env_config(solver, noise, **cfg), 0, env_id0=k * n_trials)
        b.set_params(spr.records(nominal, params[:, k]), dev.astype(np.uint8))
        backends.append(b)

    def solve(m, J, T, env_step):
        mf, ok = [], []
        for k, b in enumerate(backends):
            s = slice(k * n_trials, (k + 1) * n_trials)
            out = b.solve(torch.from_numpy(np.ascontiguousarray(m[:, s])), torch.from_numpy(np.ascontiguousarray(J[s])),
                          torch.from_numpy(np.ascontiguousarray(T[s])), env_step=env_step)
            mf.append(out["m_final"].numpy())
            ok.append(out["success"].numpy() != 0)
        return np.concatenate(mf, axis=1), np.concatenate(ok)
    return solve


def device_counts(rec, g, n_trials, n_attempts, dev, n_dev, select=None):
    """dev_switched_at [A, G, n_dev] of a chain's record: dev [n_trials] is each trial's device index; `select` as
    switch_verify_ref.counts takes it"""
    cond = np.repeat(np.arange(g), n_trials)
    d = np.tile(np.asarray(dev), g)
    keep = np.ones(g * n_trials, dtype=bool) if select is None else np.zeros(g * n_trials, dtype=bool)
    if select is not None:
        keep[select] = True
    keep &= rec["switched"]
    out = np.zeros((n_attempts, g, n_dev), dtype=np.int64)
    np.add.at(out, (rec["ended_at"][keep], cond[keep], d[keep]), 1)
    return out


def all_counts(rec, g, n_trials, n_attempts, dev, n_dev, n_bins=0, select=None):
    """switch_verify_ref.counts and device_counts: (n_switched_at, n_ended_at, n_failed, hist or None, dev_switched_at)"""
    return svr.counts(rec, g, n_trials, n_attempts, n_bins=n_bins, select=select) + (
        device_counts(rec, g, n_trials, n_attempts, dev, n_dev, select=select),)


def fused(b, m0, J, T, tgt, n_trials, sigma, dev_stride=None, **kw):
    """HipBackend.switch_verify_population on condition-major NumPy inputs -> the four arrays and dev_switched_at [A, G, dev_stride]
    (None without dev_stride) as NumPy"""
    import torch
    dev = None if dev_stride is None else torch.zeros((J.shape[0], m0.shape[0], dev_stride), dtype=torch.int64, device="cuda")
    out = b.switch_verify_population(torch.from_numpy(m0.T.copy()), torch.from_numpy(np.ascontiguousarray(J)),
                                     torch.from_numpy(np.ascontiguousarray(T)), torch.from_numpy(tgt.T.copy()), n_trials,
                                     torch.from_numpy(np.ascontiguousarray(sigma, dtype=np.float64)), dev_switched_at=dev, **kw)
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in out) + (None if dev is None else dev.cpu().numpy(),)


def oracle_run(stg, solver, noise, params):
    """the CPU oracle's run of the oracle case on the devices params [5, G, ORACLE_D]: (inputs, the chain's record, dev [ORACLE_R])"""
    m0, J, T, tgt = svr.conditions()
    rec = svr.chain(oracle_solve(stg, solver, noise, params, ORACLE_R, ORACLE_Q), m0, J, T, tgt, ORACLE_R, env_step=svr.ENV_STEP)
    return (m0, J, T, tgt), rec, spr.device_of(np.arange(ORACLE_R), ORACLE_Q)


def threshold_distance(rec, threshold=0.0):
    """the smallest distance of any projection, after any attempt that ran, to the threshold"""
    pa = rec["proj_after"]
    return float(np.abs(pa[~np.isnan(pa)] - threshold).min())

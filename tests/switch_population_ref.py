"""References of stg_switch_population shared by its CPU and its GPU tests (tests/test_switch_population_host.py,
tests/test_gpu_switch_population.py):

  * the draw of include/spintorque_hip.h restated in NumPy: device identity (device_of, device_env, touched), the clipped scaling of the
    five parameters (vary_value, each operation rounded) and the validity rule of a sigma column (column_ok);
  * records: the C-ABI records of drawn devices, fit for a class table;
  * host_path: the counts' definition through the UNCHANGED stg_solve / stg_solve_wave on the GPU -- the G R replicated problems on a
    class table that holds the devices, `cls` per problem;
  * oracle_path: the same chain on the CPU oracle, which knows nothing of populations: it is handed the devices as a class table;
  * the cases of the oracle comparison and their conditioning rule.

Nothing here imports the GPU at module level."""
import numpy as np

import switch_stats_ref as ssr

NVARY = 5
FIELDS = ("damping", "ms", "ku", "volume", "polarization")                 # the first five doubles of stg_device_params
KEYS = ("damping", "saturation_magnetization", "uniaxial_anisotropy", "volume", "polarization")     # their names in a device_params dict
VAR_STEP = 2 ** 31


# ------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------
def device_of(r, Q):
    """the device of ABSOLUTE trial r"""
    return np.asarray(r) // Q


def device_env(env_id0, g, trial_stride, d, Q):
    """the env id whose stream draws device d of condition g: the id of the device's first trial"""
    return env_id0 + g * trial_stride + d * Q


def touched(trial0, R, Q):
    """(first, last) device, both inclusive, whose dev_switched element a call on trials trial0 ... trial0 + R - 1 may touch"""
    return trial0 // Q, (trial0 + R - 1) // Q


def vary_value(nominal, sigma, z, z_clip):
    """nominal * (1.0 + sigma * min(max(z, -z_clip), z_clip)): NumPy rounds every operation and contracts nothing"""
    zc = np.minimum(np.maximum(z, -z_clip), z_clip)
    return nominal * (1.0 + sigma * zc)


def column_ok(col, z_clip):
    """a condition's sigma column [5]: no entry negative or not finite, and sigma * z_clip < 1.0"""
    col = np.asarray(col, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.isfinite(col)) and np.all(col >= 0.0) and np.all(col * z_clip < 1.0))


def nominal_values(rec):
    return np.array([getattr(rec, f) for f in FIELDS], dtype=np.float64)


def population(nominal, sigma, z, z_clip):
    """params [5, G, D] from the nominal values [5, G] (or [5]), sigma [5, G] and normals z [>= 5, G, D]"""
    nominal = np.asarray(nominal, dtype=np.float64)
    nominal = nominal[:, None] if nominal.ndim == 1 else nominal
    return vary_value(nominal[:, :, None], np.asarray(sigma)[:, :, None], np.asarray(z)[:NVARY], z_clip)


def records(nominal_rec, values):
    """the C-ABI records of devices: values [5, D] -> D copies of the nominal record with the five varied fields replaced"""
    out = []
    for j in range(values.shape[1]):
        rec = type(nominal_rec).from_buffer_copy(nominal_rec)
        for k, f in enumerate(FIELDS):
            setattr(rec, f, float(values[k, j]))
        out.append(rec)
    return out


def oracle_normals(oracle, seed, G, D, Q, trial_stride, dev0=0, env_id0=0, var_step=VAR_STEP):
    """z [6, G, D]: calls 0 and 1 of the oracle's restatement of the thermal stream of each device's env id at counter word var_step"""
    z = np.zeros((6, G, D))
    for g in range(G):
        for j in range(D):
            e = device_env(env_id0, g, trial_stride, dev0 + j, Q)
            z[:3, g, j] = oracle.thermal_normals(seed, e, var_step, 0)
            z[3:, g, j] = oracle.thermal_normals(seed, e, var_step, 1)
    return z


# ------------------------------------------------------------------------------------------------
# the existing path on a class table that holds the devices
# ------------------------------------------------------------------------------------------------
def table_of(stg, params, nominal=None):
    """(records [G D], cls_of(g, d)): the devices params [5, G, D] as ONE class table, device d of condition g in row g D + d"""
    nominal = ssr.flat_tables(stg)[0] if nominal is None else nominal
    g, d = params.shape[1:]
    recs = [r for k in range(g) for r in records(nominal, params[:, k])]
    return recs, lambda k, j: k * d + j


def trial_classes(G, R, Q, D, trial0=0, dev0=0):
    """cls [G R] of the replicated problems: problem g R + r is trial trial0 + r of condition g, of device (trial0 + r) // Q, whose row
    in table_of's table is g D + (device - dev0)"""
    dev = device_of(trial0 + np.arange(R), Q) - dev0
    assert dev.min() >= 0 and dev.max() < D
    return (np.arange(G)[:, None] * D + dev[None, :]).reshape(-1).astype(np.uint8), dev


def host_path(stg, solver, noise, m0, J, T, R, recs, cls, env_step=0, cur=None, fld=None, wave_phase=0, **cfg):
    """ssr.host_path / swr.host_path with a class byte per replicated problem: stg_solve (stg_solve_wave for phase `wave_phase` with
    tables) over the G R problems, problem g R + r = trial r of condition g (trial_stride = R, trial0 = 0), one call per phase at
    env_step + p with m_final fed back; a phase with T == 0 is skipped, a failed row keeps the m its solve handed back and takes no
    further phase.  Returns (m_final [3, G R], failed [G R])."""
    import torch
    import switch_stats_wave_ref as swr
    g = m0.shape[0]
    n = g * R
    b = ssr.backend(stg, solver, noise, n, recs, cls, **cfg)
    wave = None if cur is None and fld is None else swr.wave_dict(cur, fld, R)
    m = torch.from_numpy(np.repeat(m0, R, axis=0).T.copy()).cuda()
    failed = torch.zeros(n, dtype=torch.bool, device="cuda")
    for p in range(J.shape[0]):
        Tp = torch.from_numpy(np.repeat(T[p], R)).cuda()
        kw = {"wave": wave} if wave is not None and p == wave_phase else {}
        out = b.solve(m, torch.from_numpy(np.repeat(J[p], R)), Tp, env_step=env_step + p, **kw)
        live = ~failed & (Tp != 0.0)
        m = torch.where(live[None, :], out["m_final"], m)
        failed = failed | (live & (out["success"] == 0))
    torch.cuda.synchronize()
    res = m.cpu().numpy(), failed.cpu().numpy()
    b.close()
    return res


def device_counts(m, failed, tgt, R, dev, n_dev, threshold=0.0):
    """dev_switched [G, n_dev] of a path's result: dev [R] is each trial's device index"""
    g = tgt.shape[0]
    sw = (ssr.proj(m, np.repeat(tgt, R, axis=0)) > threshold).reshape(g, R)
    return np.stack([np.bincount(dev, weights=row, minlength=n_dev).astype(np.int64) for row in sw])


def fused(b, m0, J, T, tgt, R, sigma, cur=None, fld=None, dev_stride=None, **kw):
    """HipBackend.switch_population on condition-major NumPy inputs -> (the output tuple as NumPy, dev_switched [G, dev_stride] or None)"""
    import torch
    import switch_stats_wave_ref as swr
    wave = None if cur is None and fld is None else swr.wave_dict(cur, fld)
    dev = None if dev_stride is None else torch.zeros((m0.shape[0], dev_stride), dtype=torch.int64, device="cuda")
    out = b.switch_population(torch.from_numpy(m0.T.copy()), torch.from_numpy(np.ascontiguousarray(J)), torch.from_numpy(np.ascontiguousarray(T)),
                              torch.from_numpy(tgt.T.copy()), R, torch.from_numpy(np.ascontiguousarray(sigma, dtype=np.float64)), wave=wave,
                              dev_switched=dev, **kw)
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in out), None if dev is None else dev.cpu().numpy()


# ------------------------------------------------------------------------------------------------
# the CPU oracle's statement, and the cases of the oracle comparison
# ------------------------------------------------------------------------------------------------
def oracle_path(stg, solver, noise, m0, J, T, R, Q, params, env_step=0, **cfg):
    """ssr.oracle_path on a population: one OracleBackend of R problems per condition g at env_id0 = g R (trial_stride = R, trial0 = 0),
    its class table the condition's devices params[:, g] and its cls the device of each trial.  Returns (m_final [3, G R], failed)."""
    import torch
    from helpers import OracleBackend
    g = m0.shape[0]
    nominal = ssr.flat_tables(stg)[0]
    dev = device_of(np.arange(R), Q)
    ms, fs = [], []
    for k in range(g):
        b = OracleBackend(R, ssr.env_config(solver, noise, **cfg), 0, env_id0=k * R)
        b.set_params(records(nominal, params[:, k]), dev.astype(np.uint8))
        m = np.repeat(m0[k:k + 1], R, axis=0).T.copy()
        failed = np.zeros(R, dtype=bool)
        for p in range(J.shape[0]):
            if T[p, k] == 0.0:
                continue
            out = b.solve(torch.from_numpy(m), torch.full((R,), float(J[p, k]), dtype=torch.float64),
                          torch.full((R,), float(T[p, k]), dtype=torch.float64), env_step=env_step + p)
            live = ~failed
            m = np.where(live[None, :], out["m_final"].numpy(), m)
            failed = failed | (live & (out["success"].numpy() == 0))
        ms.append(m)
        fs.append(failed)
    return np.concatenate(ms, axis=1), np.concatenate(fs)


# R = 192 trials of 64 devices per condition, three trials each; every parameter scatters, each by another sigma per condition
ORACLE_R, ORACLE_Q, ORACLE_D, ORACLE_CLIP = ssr.ORACLE_R, 3, 64, 3.0
ORACLE_SIGMA = np.array([[0.05, 0.03, 0.08], [0.02, 0.04, 0.03], [0.04, 0.06, 0.02], [0.10, 0.05, 0.07], [0.03, 0.02, 0.05]])
# (solver, noise, P): the fixed-step forms of ssr.ORACLE_FORMS on the pulse alone and on the three-phase chain, and the LLGS solver
ORACLE_CASES = tuple((s, n, P) for s, n in ssr.ORACLE_FORMS for P in (1, 3)) + (("rk45", "white", 1),)
_CASES = {}


def oracle_case(stg, solver, noise, P, params):
    """the oracle's statement of case (solver, noise, P) on the devices params [5, G, ORACLE_D]: dict(J, T, m, failed, proj, counts at
    threshold 0 and ssr.ORACLE_BINS bins, dev_switched, distance)"""
    m0, _, _, tgt = ssr.conditions()
    J, T = ssr.phases(None, P)
    if solver == "rk45":
        J = J * ssr.RK45_J_SCALE
    cfg = ssr.settings_cfg(None, noise)
    m, failed = oracle_path(stg, solver, noise, m0, J, T, ORACLE_R, ORACLE_Q, params, env_step=ssr.ORACLE_ENV_STEP, **cfg)
    pr = ssr.proj(m, np.repeat(tgt, ORACLE_R, axis=0))
    dev = device_of(np.arange(ORACLE_R), ORACLE_Q)
    return dict(cfg=cfg, J=J, T=T, m=m, failed=failed, proj=pr, counts=ssr.host_counts(m, failed, tgt, ORACLE_R, n_bins=ssr.ORACLE_BINS),
                dev_switched=device_counts(m, failed, tgt, ORACLE_R, dev, ORACLE_D), distance=ssr.edge_distance(pr, ssr.ORACLE_BINS))


def oracle_case_cpu(stg, oracle, solver, noise, P):
    """oracle_case on the devices drawn from the oracle's own normals (no GPU): computed once per process"""
    key = (solver, noise, P)
    if key not in _CASES:
        z = oracle_normals(oracle, ssr.SEED, ssr.G, ORACLE_D, ORACLE_Q, ORACLE_R)
        params = population(nominal_values(ssr.flat_tables(stg)[0]), ORACLE_SIGMA, z, ORACLE_CLIP)
        _CASES[key] = oracle_case(stg, solver, noise, P, params)
    return _CASES[key]


def check_conditioned(case, solver, noise, P):
    """ssr.check_conditioned's rule at the defaults: every trial solved, every projection further than ssr.margin() from threshold 0
    and from every inner bin edge; under brown the field decides"""
    ssr.check_conditioned(case, solver, noise, None, P)
    assert case["dev_switched"].sum(axis=1).tolist() == case["counts"][0].tolist()

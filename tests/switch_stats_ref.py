"""References of stg_switch_stats shared by its GPU and its CPU tests (tests/test_gpu_switch_stats.py, test_gpu_switch_stats_config.py,
test_switch_stats_oracle.py, test_switch_stats_plan_host.py):

  * the header's classification in NumPy (proj, bins), each operation rounded, and the reduction to counts (host_counts);
  * host_path: the counts' definition through stg_solve on the GPU -- the G R replicated problems, phase after phase;
  * oracle_path: the same chain on the CPU oracle (helpers.OracleBackend), which reproduces the Philox streams and knows the three
    thermal fields: an INDEPENDENT statement of what the counts should be;
  * the launch rule and the kernel's index map restated in Python (plan_cap, trial_index_map);
  * the off-default settings and the conditioning rule of the oracle comparison.

Nothing here imports the GPU at module level: host_path and backend take the package as their first argument."""
import numpy as np

import brown_ref as br

SEED = 41
G = 3
WAVES = 12288                                             # STG_SWITCH_STATS_WAVES (tests/test_switch_stats_host.py pins it to the header)

# (max_step, gamma, temperature): the three off-default settings of tests/test_wave_config_host.py (tests/test_brown_oracle.py SETTINGS)
SETTINGS = ((2.5e-12, 1.9e5, 77.0), (3e-13, 2.5e5, 450.0), (1e-10, 2.21e5, 250.0))
CORR_TIME = 7e-13                                          # wave_config_cases.CORR_TIME: the ou correlation time off its default
MARGIN_FACTOR = 100                                        # x the tolerance stg_solve is held to the oracle at: three chained phases and the projection
ORACLE_FORMS = (("rk4", "brown"), ("euler", "brown"), ("rk4", "ou"), ("rk4", "white"))


def params(volume=br.SWITCH["volume"]):
    return br.physics_params(volume, br.SWITCH["damping"])


def conditions():
    """m0 [G,3] a little above the equator, J [G], T [G] (20, 60, 100 ps), target -z.  The NumPy restatement (tests/brown_ref.py, NumPy's
    own generator, 1500 samples) switches 0.36, ~0.6 and ~0.45 of the trials of these conditions under the Brown field"""
    mz = np.array([0.1, 0.2, 0.3])
    ph = np.array([0.3, 1.7, 4.0])
    s = np.sqrt(1.0 - mz * mz)
    m0 = np.stack([s * np.cos(ph), s * np.sin(ph), mz], axis=1)
    J = br.SWITCH["J"] * np.array([0.5, 0.6, 0.45])
    T = np.array([2e-11, 6e-11, 1e-10])
    return m0, J, T, np.tile([0.0, 0.0, -1.0], (G, 1))


def env_config(solver, noise, **cfg):
    from spin_torque_gym_amd.backend import EnvConfig
    kw = dict(solver=solver, include_thermal_fluctuations=True, noise_model=noise, seed=SEED)
    kw.update(cfg)
    return EnvConfig(**kw)


def flat_tables(stg, tables=None):
    """the C-ABI records of a class table: dicts as STT classes; an entry that is a record already passes through"""
    tables = [params()] if tables is None else tables
    return [stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", p)) if isinstance(p, dict) else p for p in tables]


def backend(stg, solver, noise, n, tables=None, cls=None, env_id0=0, **cfg):
    from spin_torque_gym_amd.backend import HipBackend
    b = HipBackend(n, env_config(solver, noise, **cfg), 0, env_id0)
    flat = flat_tables(stg, tables)
    if cls is not None and len(flat) > 1 and int(np.max(np.asarray(cls))) >= len(flat):
        # a class byte beyond the table, which the header says reads class 0: the Python binding refuses it, but the C-ABI keeps the
        # caller's device array (stg_set_params), so the bytes are written into that array after the call
        import torch
        b.set_params(flat, np.zeros(n, dtype=np.uint8))
        b._cls.copy_(torch.as_tensor(np.asarray(cls, dtype=np.uint8)))
        torch.cuda.synchronize()
    else:
        b.set_params(flat, cls)
    return b


def proj(m, tgt):
    """the header's projection, [n] from m [3,n] and target rows [n,3]: ((mx tx) + (my ty)) + (mz tz), each operation rounded"""
    return ((m[0] * tgt[:, 0]) + (m[1] * tgt[:, 1])) + (m[2] * tgt[:, 2])


def bins(proj, n_bins):
    """the header's bin rule: min(n_bins - 1, max(0, (int)floor((proj + 1.0) * (0.5 * n_bins)))); NaN -> bin 0"""
    b = np.floor((proj + 1.0) * (0.5 * n_bins))
    b = np.where(np.isnan(b), 0.0, b)
    return np.minimum(n_bins - 1, np.maximum(0, b)).astype(np.int64)


def host_path(stg, solver, noise, m0, J, T, tgt, R, env_step=0, tables=None, cond_cls=None, env_id0=0, **cfg):
    """The existing path: stg_solve over the G R replicated problems (problem g R + r = trial r of condition g), one call per phase at
    env_step + p with m_final fed back as m0; a phase with T == 0 is skipped, a row whose solve failed keeps the m that solve handed
    back and takes no further phase.  J, T [P,G].  Returns (m_final [3, G R], failed [G R]) as NumPy arrays."""
    import torch
    g = m0.shape[0]
    n = g * R
    cls = None if cond_cls is None else np.repeat(cond_cls, R).astype(np.uint8)
    b = backend(stg, solver, noise, n, tables, cls, env_id0=env_id0, **cfg)
    m = torch.from_numpy(np.repeat(m0, R, axis=0).T.copy()).cuda()
    failed = torch.zeros(n, dtype=torch.bool, device="cuda")
    for p in range(J.shape[0]):
        Tp = torch.from_numpy(np.repeat(T[p], R)).cuda()
        out = b.solve(m, torch.from_numpy(np.repeat(J[p], R)), Tp, env_step=env_step + p)
        live = ~failed & (Tp != 0.0)
        m = torch.where(live[None, :], out["m_final"], m)
        failed = failed | (live & (out["success"] == 0))
    torch.cuda.synchronize()
    res = m.cpu().numpy(), failed.cpu().numpy()
    b.close()
    return res


def host_counts(m, failed, tgt, R, threshold=0.0, n_bins=0):
    g = tgt.shape[0]
    pr = proj(m, np.repeat(tgt, R, axis=0))
    n_sw = (pr > threshold).reshape(g, R).sum(axis=1)
    n_failed = failed.reshape(g, R).sum(axis=1)
    hist = None
    if n_bins:
        b = bins(pr, n_bins).reshape(g, R)
        hist = np.stack([np.bincount(row, minlength=n_bins) for row in b])
    return n_sw, n_failed, hist


# ------------------------------------------------------------------------------------------------
# the CPU oracle's statement of the same trials
# ------------------------------------------------------------------------------------------------
def oracle_path(stg, solver, noise, m0, J, T, R, env_step=0, trial0=0, trial_stride=None, tables=None, cond_cls=None, **cfg):
    """host_path's chain on the CPU oracle, by the header's stream rule: one OracleBackend of R problems per condition g, created at
    env_id0 = g * trial_stride + trial0, so that its problem r is trial trial0 + r of condition g; phase p is its solve at env_step + p
    with m_final fed back; a phase with T == 0 is skipped, a trial whose solve failed keeps the m that solve handed back and takes no
    further phase.  `stg` is the package (flatten_params, DeviceFactory: host code).  Returns (m_final [3, G R], failed [G R])."""
    import torch
    from helpers import OracleBackend
    g = m0.shape[0]
    stride = trial0 + R if trial_stride is None else trial_stride
    flat = flat_tables(stg, tables)
    ms, fs = [], []
    for k in range(g):
        b = OracleBackend(R, env_config(solver, noise, **cfg), 0, env_id0=k * stride + trial0)
        c = 0 if cond_cls is None or len(flat) == 1 else int(cond_cls[k])
        b.set_params([flat[c if c < len(flat) else 0]])
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


def settings_cfg(k, noise):
    """the configuration keywords of setting k (None: the defaults) for a fixed-step form; ou also takes its correlation time off its default"""
    cfg = {} if k is None else dict(max_step=SETTINGS[k][0], gamma=SETTINGS[k][1], temperature=SETTINGS[k][2])
    if noise == "ou":
        cfg["correlation_time"] = CORR_TIME
    return cfg


# a duration per setting at which max_step, not T / 100, is the sub-step (dt = min(max_step, T / 100)): the relax phase of condition 0
# in the three-phase chain (n = 150 at the defaults, 120 at max_step = 2.5e-12).  Setting 1 needs none: the pulses of conditions()
# themselves reach it (60 and 100 ps at max_step = 3e-13: n = 200, 333).  Setting 2 (max_step = 1e-10) has none: max_step decides there
# only from T > 1e-8 s on, in sub-steps of 1e-10 s = ~22 rad of precession each, where the fixed-step integrators are unstable --
# measured on the oracle with a 1.2e-8 s relax phase, a change of 1e-9 in m0 moves the final m by 5e-6 under rk4 and by 1.9 under
# euler (against 2e-7 for the durations used here), so no exact comparison is conditioned there.
LONG_RELAX = {None: 1.5e-10, 0: 3e-10, 1: None, 2: None}


def phases(k, P):
    """(J [P,G], T [P,G]) of the oracle comparison at setting k: the pulse of conditions() alone, or equilibrate 30 ps / pulse / relax
    20 ps with condition 0's relax at LONG_RELAX[k]"""
    _, Jp, Tp, _ = conditions()
    if P == 1:
        return Jp[None].copy(), Tp[None].copy()
    relax = np.full(G, 2e-11)
    if LONG_RELAX[k] is not None:
        relax[0] = LONG_RELAX[k]
    return np.stack([np.zeros(G), Jp, np.zeros(G)]), np.stack([np.full(G, 3e-11), Tp, relax])


def edge_distance(pr, n_bins, threshold=0.0):
    """smallest distance of any projection to the threshold or to an inner edge of the n_bins bins over [-1, 1]"""
    edges = np.concatenate([[threshold], np.linspace(-1.0, 1.0, n_bins + 1)[1:-1]]) if n_bins else np.array([threshold])
    return float(np.abs(np.asarray(pr)[:, None] - edges[None, :]).min())


# ------------------------------------------------------------------------------------------------
# the launch rule and the kernel's index map
# ------------------------------------------------------------------------------------------------
def plan_cap(G_):
    """wavefronts per condition the launch rule allows: max(1, 12288 / G)"""
    return max(1, WAVES // G_)


def trial_index_map(R, L, waves_per_cond):
    """the kernel's index map: lane `lane` of wavefront w of a condition runs, in its round l, trial r = (w L + l) 64 + lane if r < R.
    Returns the trials that are run, in launch order."""
    w, l, lane = np.meshgrid(np.arange(waves_per_cond), np.arange(L), np.arange(64), indexing="ij")
    r = (w * L + l) * 64 + lane
    return r[r < R]


# ------------------------------------------------------------------------------------------------
# the cases of the oracle comparison, computed once per process and shared (tests/test_switch_stats_oracle.py on the CPU,
# tests/test_gpu_switch_stats_config.py on the GPU)
# ------------------------------------------------------------------------------------------------
ORACLE_R, ORACLE_ENV_STEP, ORACLE_BINS = 192, 3, 7
# RK45 (the LLGS solver, white field): with the device of these tests every current above the solver's |J| > 1e-12 gate saturates all
# trials at proj = 1.0 within the shortest pulse (measured on the oracle from 1.06e-12 A/m^2 up), so the one unsaturated input is a
# current below the gate: the file's J / 1000.  The trials then relax under the white field, 4e-7 ... 1e-6 apart within a condition.
RK45_J_SCALE = 1e-3
_CASES = {}


def margin():
    """the conditioning margin: 100 x the tolerance tests/test_gpu_brown_config.py holds stg_solve to the oracle at"""
    from test_gpu_brown_config import TOL
    return MARGIN_FACTOR * TOL


def oracle_case(stg, solver, noise, k, P):
    """the oracle's statement of form (solver, noise) at setting k (None: the defaults) with P phases: dict(cfg, J, T, m, failed, proj
    [G R], counts = (n_switched, n_failed, hist) at threshold 0 and ORACLE_BINS bins, distance = edge_distance)"""
    key = (solver, noise, k, P)
    if key not in _CASES:
        m0, _, _, tgt = conditions()
        J, T = phases(k, P)
        if solver == "rk45":
            J = J * RK45_J_SCALE
        cfg = settings_cfg(k, noise)
        m, failed = oracle_path(stg, solver, noise, m0, J, T, ORACLE_R, env_step=ORACLE_ENV_STEP, **cfg)
        pr = proj(m, np.repeat(tgt, ORACLE_R, axis=0))
        _CASES[key] = dict(cfg=cfg, J=J, T=T, m=m, failed=failed, proj=pr, counts=host_counts(m, failed, tgt, ORACLE_R, n_bins=ORACLE_BINS),
                           distance=edge_distance(pr, ORACLE_BINS))
    return _CASES[key]


def check_conditioned(case, solver, noise, k, P):
    """the condition of the exact comparison, from the oracle alone: every trial solved, every projection finite and further than
    margin() from threshold 0 and from every inner edge of the ORACLE_BINS bins; under brown the field decides (0 < n_switched < R)"""
    n_sw, n_failed, hist = case["counts"]
    assert np.isfinite(case["proj"]).all() and not n_failed.any(), (solver, noise, k, P)
    assert case["distance"] > margin(), (solver, noise, k, P, case["distance"])
    assert (hist.sum(axis=1) == ORACLE_R).all()
    if noise == "brown":
        assert ((0 < n_sw) & (n_sw < ORACLE_R)).all(), (solver, k, P, n_sw)
    if solver == "rk45":
        assert (np.abs(case["proj"]) < 0.99).all()


def fused(b, m0, J, T, tgt, R, **kw):
    """HipBackend.switch_stats on condition-major NumPy inputs (m0, tgt [G,3]; J, T [P,G]) -> (n_switched, n_failed, hist or None) as NumPy"""
    import torch
    out = b.switch_stats(torch.from_numpy(m0.T.copy()), torch.from_numpy(np.ascontiguousarray(J)), torch.from_numpy(np.ascontiguousarray(T)),
                         torch.from_numpy(tgt.T.copy()), R, **kw)
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in out)

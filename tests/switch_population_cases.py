"""The reference and the inputs of stg_switch_population's second test round (tests/test_gpu_switch_population_config.py on the GPU,
tests/test_switch_population_config_host.py on the CPU), next to tests/switch_population_ref.py:

  * population_host_path: all six outputs through EXISTING code at any stream identity -- switch_times_ref.host_path (one context per
    condition at the env id of the condition's first trial, the watched phase solved again with traj_cap and put through
    switch_times_ref.first_passage) with switch_population_ref.host_path's class byte per problem: condition g's context holds that
    condition's devices as its class table;
  * trial_classes: the class byte of every trial of such a context;
  * checked_devices: the dump of stg_switch_population_devices, asserted bit for bit against the NumPy formula on the normals
    stg_thermal_normals hands out, so that a reference built on the dump does not lean on the dump alone;
  * the classes of the nominal-class tests, the pulse chains, and the oracle cases off the defaults with their conditioning rule.

Nothing here imports the GPU at module level."""
import numpy as np

import switch_population_ref as spr
import switch_stats_ref as ssr
import switch_stats_wave_ref as swr
import switch_times_ref as stref

MAX_CLASSES = 64                                           # STG_MAX_CLASSES: a condition's devices must fit one class table
NAMES = ("n_switched", "n_failed", "hist", "n_crossed", "n_returned", "t_hist")


# ------------------------------------------------------------------------------------------------
# index arithmetic
# ------------------------------------------------------------------------------------------------
def trial_classes(R, Q, trial0=0, dev0=None):
    """(cls [R], dev0, n_dev): the class byte of trials trial0 ... trial0 + R - 1 in a table that holds devices dev0, dev0 + 1, ... --
    trial r's class is (trial0 + r) // Q - dev0; dev0 None: the first device the range touches"""
    first, last = spr.touched(trial0, R, Q)
    dev0 = first if dev0 is None else int(dev0)
    cls = (trial0 + np.arange(R, dtype=np.int64)) // Q - dev0
    assert dev0 <= first and 0 <= cls.min() and cls.max() == last - dev0 < MAX_CLASSES, (trial0, R, Q, dev0)
    return cls.astype(np.uint8), dev0, last - dev0 + 1


def condition_env(env_id0, g, trial_stride, trial0):
    """the env id of condition g's trial trial0: where its context is created"""
    return env_id0 + g * trial_stride + trial0


def nominal_records(stg, tables=None, cond_cls=None, G=ssr.G):
    """the nominal record of each condition: class cond_cls[g] of the table, class 0 for a byte beyond it or without cond_cls"""
    flat = ssr.flat_tables(stg, tables)
    cc = np.zeros(G, dtype=np.int64) if cond_cls is None else np.asarray(cond_cls, dtype=np.int64)
    return [flat[c if c < len(flat) else 0] for c in cc]


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def population_host_path(stg, solver, noise, m0, J, T, tgt, R, Q, params, nominal=None, watch_phase=0, cur=None, fld=None, threshold=0.0,
                         env_step=0, trial0=0, trial_stride=None, dev0=None, env_id0=0, conds=None, **cfg):
    """Condition g's R trials are the problems of ONE context of R envs created at env id env_id0 + g trial_stride + trial0, whose class
    table holds the condition's devices -- copies of nominal[g] (a record per condition; None: the default device) with the five
    fields of params[:, g, j], device dev0 + j -- and whose cls is trial_classes.  One solve per phase at env_step + p (modulo 2^32)
    with m_final fed back; the watched phase is solved a second time with traj_cap = max(n_points) + 1 -- with the condition's
    tables replicated per trial when cur / fld are given -- and its rows go through switch_times_ref.first_passage.  A phase with
    T == 0 is skipped, a trial whose solve failed keeps the m that solve handed back and takes no further phase; a trial whose
    watched phase is skipped, not reached or failed has not crossed.  `conds`: the conditions to compute (others are left out of
    the result, which is then ordered as conds).  Returns dict(m [3, n R], failed, crossed, t_x [n R], dev [R]: each trial's
    ABSOLUTE device)."""
    import torch
    g_all = m0.shape[0]
    stride = trial0 + R if trial_stride is None else trial_stride
    cls, dev0, n_dev = trial_classes(R, Q, trial0, dev0)
    assert params.shape[1] == g_all and params.shape[2] >= n_dev
    wave = cur is not None or fld is not None
    ms, fs, cs, ts, ps = [], [], [], [], []
    for k in (range(g_all) if conds is None else conds):
        nom = ssr.flat_tables(stg)[0] if nominal is None else nominal[k]
        recs = spr.records(nom, params[:, k, :n_dev])
        b = ssr.backend(stg, solver, noise, R, recs, cls if len(recs) > 1 else None, env_id0=condition_env(env_id0, k, stride, trial0), **cfg)
        m = torch.from_numpy(np.repeat(m0[k:k + 1], R, axis=0).T.copy()).cuda()
        failed = torch.zeros(R, dtype=torch.bool, device="cuda")
        crossed, t_x, peak = np.zeros(R, dtype=bool), np.zeros(R), np.full(R, -np.inf)
        for p in range(T.shape[0]):
            if T[p, k] == 0.0:
                continue
            Jp, Tp = torch.full((R,), float(J[p, k]), dtype=torch.float64), torch.full((R,), float(T[p, k]), dtype=torch.float64)
            kw = {}
            if p == watch_phase and wave:
                one = lambda kn: None if kn is None else tuple(np.asarray(a)[:, k:k + 1] for a in kn)         # noqa: E731
                kw["wave"] = swr.wave_dict(one(cur), one(fld), R)
            step = (env_step + p) % 2 ** 32
            out = b.solve(m, Jp, Tp, env_step=step, **kw)
            if p == watch_phase:
                cap = max(1, int(out["n_points"].max().item()) + 1)
                out = b.solve(m, Jp, Tp, env_step=step, traj_cap=cap, **kw)
                torch.cuda.synchronize()
                fp = stref.first_passage(out["t"].cpu().numpy(), out["m"].cpu().numpy(), out["n_points"].cpu().numpy(),
                                         out["success"].cpu().numpy() != 0, np.repeat(tgt[k:k + 1], R, axis=0), threshold)
                crossed, t_x = fp["crossed"] & (~failed).cpu().numpy(), fp["t_x"]
                if cap > 1:
                    peak = np.where(fp["valid"][1:], fp["proj"][1:], -np.inf).max(axis=0)
            live = ~failed
            m = torch.where(live[None, :], out["m_final"], m)
            failed = failed | (live & (out["success"] == 0))
        torch.cuda.synchronize()
        ms.append(m.cpu().numpy())
        fs.append(failed.cpu().numpy())
        cs.append(crossed)
        ts.append(t_x)
        ps.append(peak)
        b.close()
    return dict(m=np.concatenate(ms, axis=1), failed=np.concatenate(fs), crossed=np.concatenate(cs), t_x=np.concatenate(ts),
                peak=np.concatenate(ps), dev=cls.astype(np.int64) + dev0)


def reference_counts(h, tgt, T_watch, R, n_dev, threshold=0.0, n_bins=0, n_tbins=0):
    """(the six arrays, dev_switched [G, n_dev] by ABSOLUTE device) of a population_host_path result"""
    six = stref.counts(h["m"], h["failed"], h["crossed"], h["t_x"], tgt, T_watch, R, threshold=threshold, n_bins=n_bins, n_tbins=n_tbins)
    return six, spr.device_counts(h["m"], h["failed"], tgt, R, h["dev"], n_dev, threshold=threshold)


def same(got, want, what=None, names=NAMES):
    assert len(got) == len(want), (what, len(got), len(want))
    for name, x, y in zip(names, got, want):
        assert (x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)), (what, name, x, y)


# ------------------------------------------------------------------------------------------------
# the dump, checked against the stream
# ------------------------------------------------------------------------------------------------
def stream_normals(stg, env_ids, var_step):
    """z [6, n, D]: calls 0 and 1 of stg_thermal_normals at counter word var_step for the env ids [n, D], one context per row whose envs
    cover that row's ids (tests/test_gpu_switch_population.py's _stream_normals)"""
    import torch
    z = np.zeros((6,) + env_ids.shape)
    for g, ids in enumerate(env_ids):
        lo, n = int(ids.min()), int(ids.max() - ids.min()) + 1
        b = ssr.backend(stg, "rk4", "brown", n, env_id0=lo)
        zz = b.thermal_normals(var_step, 0, 2)
        torch.cuda.synchronize()
        z[:, g] = zz.cpu().numpy().reshape(6, n)[:, ids - lo]
        b.close()
    return z


def checked_devices(stg, b, G, D, sigma, Q, trial_stride, nominal=None, dev0=0, var_step=spr.VAR_STEP, z_clip=4.0, cond_cls=None, env_id0=0,
                    conds=None):
    """params [5, G, D] as context b (created at env_id0) dumps them, asserted bit for bit -- for the conditions `conds`, None: all --
    against spr.population on the normals of the devices' own streams and the conditions' nominal records"""
    import torch
    out = b.switch_population_devices(G, D, torch.from_numpy(np.ascontiguousarray(sigma)), dev0=dev0, trials_per_device=Q, trial_stride=trial_stride,
                                      var_step=var_step, z_clip=z_clip, cond_cls=None if cond_cls is None else torch.as_tensor(cond_cls, dtype=torch.uint8))
    torch.cuda.synchronize()
    params = out.cpu().numpy()
    conds = list(range(G)) if conds is None else list(conds)
    ids = np.array([[spr.device_env(env_id0, g, trial_stride, dev0 + j, Q) for j in range(D)] for g in conds], dtype=np.int64)
    zs = stream_normals(stg, ids, var_step)
    nom = np.stack([spr.nominal_values(ssr.flat_tables(stg)[0] if nominal is None else nominal[g]) for g in conds], axis=1)
    want = spr.population(nom, np.asarray(sigma)[:, conds], zs, z_clip)
    assert np.array_equal(params[:, conds].view(np.uint64), want.view(np.uint64)), "the dump is not the formula on the stream's normals"
    return params


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def chain(Jp, Tp, P, watch):
    """(J [P,G], T [P,G]): the pulse alone, or the pulse as phase `watch` of three with J = 0 phases of 30 and 20 ps around it"""
    if P == 1:
        return Jp[None].copy(), Tp[None].copy()
    g = len(Jp)
    J, T = np.zeros((3, g)), np.stack([np.full(g, 3e-11), np.full(g, 3e-11), np.full(g, 2e-11)])
    J[watch], T[watch] = Jp, Tp
    return J, T


def knots(name, solver, g):
    """(cur, fld) of swr.knot_sets()[name] for the first g conditions (None: rectangular); rk45 takes the current at its scale"""
    if name is None:
        return None, None
    cur, fld = swr.knot_sets()[name]
    if cur is not None:
        cur = (cur[0][:, :g], cur[1][:, :g] * (ssr.RK45_J_SCALE if solver == "rk45" else 1.0))
    if fld is not None:
        fld = (fld[0][:, :g], fld[1][:, :g])
    return cur, fld


# The three classes of the nominal-class tests differ in a VARIED field (volume) and in fields the draw leaves alone but the solvers
# integrate on: the easy axis, tilted 0 / 0.25 / 0.5 rad in the x-z plane, for the fixed-step solvers, and the demagnetisation factors
# for RK45.  A kernel that took only the five varied fields from the condition's class would integrate on class 0's others.
CLASS_VOLUMES = (1.0, 0.7, 1.3)
CLASS_TILTS = (0.0, 0.25, 0.5)
CLASS_DEMAG = ((0.0, 0.0, 1.0), (0.1, 0.0, 0.9), (0.0, 0.3, 0.7))


def class_tables(solver):
    import brown_ref as br
    v = br.SWITCH["volume"]
    out = []
    for k in range(3):
        p = ssr.params(CLASS_VOLUMES[k] * v)
        if solver == "rk45":
            p["demag_factors"] = np.array(CLASS_DEMAG[k])
        else:
            p["easy_axis"] = np.array([np.sin(CLASS_TILTS[k]), 0.0, np.cos(CLASS_TILTS[k])])
        out.append(p)
    return out


def mixed_record(rec_c, rec_0):
    """class 0's record with the five varied fields of class c: what a kernel would integrate on that took `out = ptab[0]` and scaled
    the right class's five"""
    rec = type(rec_0).from_buffer_copy(rec_0)
    for f in spr.FIELDS:
        setattr(rec, f, getattr(rec_c, f))
    return rec


# ------------------------------------------------------------------------------------------------
# the oracle, off its defaults
# ------------------------------------------------------------------------------------------------
ORACLE_P = 3
# (solver, noise, setting): the fixed-step forms x the three settings, and RK45 at its own tolerances (setting None)
ORACLE_CASES = tuple((s, n, k) for s, n in ssr.ORACLE_FORMS for k in (0, 1, 2)) + (("rk45", "white", None),)
# per case: (sigma, env_step) where the case is not conditioned at spr.ORACLE_SIGMA and ssr.ORACLE_ENV_STEP
ORACLE_OVERRIDES = {}
_CASES = {}


def oracle_cfg(solver, noise, k):
    """the configuration keywords of form (solver, noise) at setting k (None: the defaults); RK45 also takes rtol, atol and max_attempts
    off their defaults"""
    cfg = ssr.settings_cfg(k, noise)
    if solver == "rk45":
        from test_gpu_switch_stats_config import RK45_CFG
        cfg.update(RK45_CFG)
    return cfg


def oracle_inputs(solver, noise, k):
    """(sigma [5, G], env_step, J, T [3, G]) of case (solver, noise, k)"""
    sigma, env_step = ORACLE_OVERRIDES.get((solver, noise, k), (spr.ORACLE_SIGMA, ssr.ORACLE_ENV_STEP))
    J, T = ssr.phases(k, ORACLE_P)
    if solver == "rk45":
        J = J * ssr.RK45_J_SCALE
    return sigma, env_step, J, T


def oracle_case(stg, solver, noise, k, params):
    """spr.oracle_case at setting k, P = 3: the oracle's statement on the devices params [5, G, ORACLE_D]"""
    m0, _, _, tgt = ssr.conditions()
    _, env_step, J, T = oracle_inputs(solver, noise, k)
    cfg = oracle_cfg(solver, noise, k)
    R, Q, D = spr.ORACLE_R, spr.ORACLE_Q, spr.ORACLE_D
    m, failed = spr.oracle_path(stg, solver, noise, m0, J, T, R, Q, params, env_step=env_step, **cfg)
    pr = ssr.proj(m, np.repeat(tgt, R, axis=0))
    dev = spr.device_of(np.arange(R), Q)
    return dict(cfg=cfg, J=J, T=T, m=m, failed=failed, proj=pr, counts=ssr.host_counts(m, failed, tgt, R, n_bins=ssr.ORACLE_BINS),
                dev_switched=spr.device_counts(m, failed, tgt, R, dev, D), distance=ssr.edge_distance(pr, ssr.ORACLE_BINS))


def oracle_case_cpu(stg, oracle, solver, noise, k):
    """oracle_case on the devices drawn from the oracle's own normals (no GPU): computed once per process"""
    key = (solver, noise, k)
    if key not in _CASES:
        sigma = oracle_inputs(solver, noise, k)[0]
        z = spr.oracle_normals(oracle, ssr.SEED, ssr.G, spr.ORACLE_D, spr.ORACLE_Q, spr.ORACLE_R)
        params = spr.population(spr.nominal_values(ssr.flat_tables(stg)[0]), sigma, z, spr.ORACLE_CLIP)
        _CASES[key] = oracle_case(stg, solver, noise, k, params)
    return _CASES[key]


def check_conditioned(case, solver, noise, k):
    """ssr.check_conditioned at setting k, P = 3 (margin ssr.margin()), and the per-device counts add up"""
    ssr.check_conditioned(case, solver, noise, k, ORACLE_P)
    assert case["dev_switched"].sum(axis=1).tolist() == case["counts"][0].tolist()

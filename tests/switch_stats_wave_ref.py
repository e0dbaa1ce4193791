"""References of stg_switch_stats_wave shared by its GPU and its CPU tests (tests/test_gpu_switch_stats_wave.py,
tests/test_switch_stats_wave_host.py), next to tests/switch_stats_ref.py, whose conditions, classification and margin they use:

  * the inputs: a 5-knot trapezoid current per condition (rise and fall of T / 10, plateau at PLATEAU_SCALE x the file's J) and a
    2-knot in-plane field ramp per condition, condition-major as the Python method takes them (tk [K,G], jk [K,G], hk [K,G,3]);
  * host_path: the counts' definition through EXISTING code -- stg_solve_wave (and stg_solve for the rectangular phases) over the G R
    replicated problems with the tables replicated per trial, phase after phase;
  * numpy_case: an independent statement that does not go through stg_solve_wave -- tests/brown_ref.py (NumPy) under the oracle's
    Philox normals by the header's stream rule;
  * fused: HipBackend.switch_stats_wave on the same condition-major inputs.

Nothing here imports the GPU at module level."""
import numpy as np

import brown_ref as br
import switch_stats_ref as ssr

G = ssr.G
# The plateau of the trapezoid as a factor on conditions()' J.  The trapezoid carries 0.9 of the rectangle's charge.  Chosen on the CPU
# with numpy_case (tests/test_switch_stats_wave_host.py runs the check again): at this scale, R = 192, rk4 and euler under the Brown
# field, every condition has 0 < n_switched < R and no projection within margin() of threshold 0 or of an inner edge of 7 bins.
PLATEAU_SCALE = 1.0
# the field ramp ends at this magnitude [A/m]: the bound of the field values wave_config_cases.tables draws (uniform in +-1e5), 5 % of
# the anisotropy field of the "switching" device
FIELD = 1e5
FIELD_ANGLES = np.array([0.4, 2.1, 3.9])                  # in-plane direction of each condition's ramp
NUMPY_R, NUMPY_ENV_STEP, NUMPY_BINS = ssr.ORACLE_R, ssr.ORACLE_ENV_STEP, ssr.ORACLE_BINS
NUMPY_FORMS = (("rk4", "brown"), ("euler", "brown"))


def trapezoid(J, T, scale=PLATEAU_SCALE):
    """current_knots (tk [5,G], jk [5,G]): 0 -> plateau over T / 10, plateau (one knot mid-way), plateau -> 0 over the last T / 10;
    the times differ per condition"""
    tau = np.array([0.0, 0.1, 0.5, 0.9, 1.0])
    s = np.array([0.0, 1.0, 1.0, 1.0, 0.0])
    return tau[:, None] * T[None, :], s[:, None] * (scale * J)[None, :]


def field_ramp(T, magnitude=FIELD):
    """field_knots (tk [2,G], hk [2,G,3]): zero at t = 0 to `magnitude` in the plane at t = T, another direction per condition"""
    g = len(T)
    d = np.stack([np.cos(FIELD_ANGLES[:g]), np.sin(FIELD_ANGLES[:g]), np.zeros(g)], axis=1)
    return np.stack([np.zeros(g), T]), np.stack([np.zeros((g, 3)), magnitude * d])


def knot_sets():
    """the three knot sets of the equality tests: name -> (current_knots | None, field_knots | None) on conditions()"""
    _, J, T, _ = ssr.conditions()
    return {"kj5-kh2": (trapezoid(J, T), field_ramp(T)), "kj5-kh0": (trapezoid(J, T), None), "kj0-kh2": (None, field_ramp(T))}


def wave_dict(cur, fld, rep=1):
    """condition-major knots -> the backend's dict(current=(tj [K,N], jk [K,N]) | None, field=(th [K,N], hk [K,3,N]) | None) with every
    condition's column repeated `rep` times (N = G rep: the replicated tables of the existing path)"""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.repeat(a, rep, axis=-1)))         # noqa: E731
    return {"current": None if cur is None else (t(np.asarray(cur[0], dtype=np.float64)), t(np.asarray(cur[1], dtype=np.float64))),
            "field": None if fld is None else (t(np.asarray(fld[0], dtype=np.float64)),
                                               t(np.transpose(np.asarray(fld[1], dtype=np.float64), (0, 2, 1))))}


def host_path(stg, solver, noise, m0, J, T, tgt, R, cur, fld, wave_phase=0, env_step=0, tables=None, cond_cls=None, **cfg):
    """The existing path: the G R replicated problems (problem g R + r = trial r of condition g), one call per phase at env_step + p
    with m_final fed back as m0 -- stg_solve_wave with the tables replicated per trial for phase `wave_phase`, stg_solve for the
    others; a phase with T == 0 is skipped, a row whose solve failed keeps the m that solve handed back and takes no further phase.
    J, T [P,G].  Returns (m_final [3, G R], failed [G R]) as NumPy arrays."""
    import torch
    g = m0.shape[0]
    n = g * R
    cls = None if cond_cls is None else np.repeat(cond_cls, R).astype(np.uint8)
    b = ssr.backend(stg, solver, noise, n, tables, cls, **cfg)
    wave = wave_dict(cur, fld, R)
    m = torch.from_numpy(np.repeat(m0, R, axis=0).T.copy()).cuda()
    failed = torch.zeros(n, dtype=torch.bool, device="cuda")
    for p in range(T.shape[0]):
        Tp = torch.from_numpy(np.repeat(T[p], R)).cuda()
        kw = dict(wave=wave) if p == wave_phase else {}
        out = b.solve(m, torch.from_numpy(np.repeat(J[p], R)), Tp, env_step=env_step + p, **kw)
        live = ~failed & (Tp != 0.0)
        m = torch.where(live[None, :], out["m_final"], m)
        failed = failed | (live & (out["success"] == 0))
    torch.cuda.synchronize()
    res = m.cpu().numpy(), failed.cpu().numpy()
    b.close()
    return res


def fused(b, m0, J, T, tgt, R, cur, fld, **kw):
    """HipBackend.switch_stats_wave on condition-major NumPy inputs (m0, tgt [G,3]; J, T [P,G]; knots as trapezoid / field_ramp give
    them) -> (n_switched, n_failed, hist or None) as NumPy"""
    import torch
    out = b.switch_stats_wave(torch.from_numpy(m0.T.copy()), torch.from_numpy(np.ascontiguousarray(J)), torch.from_numpy(np.ascontiguousarray(T)),
                              torch.from_numpy(tgt.T.copy()), R, wave_dict(cur, fld), **kw)
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in out)


# ------------------------------------------------------------------------------------------------
# the independent statement: NumPy under the oracle's normals, by the header's stream rule
# ------------------------------------------------------------------------------------------------
_CASES = {}


def numpy_case(oracle, method, scale=PLATEAU_SCALE, R=NUMPY_R):
    """P = 1, trial_stride = R, env_step = NUMPY_ENV_STEP, the trapezoid at `scale` and the field ramp: trial r of condition g is
    brown_ref.solve (tests/waveform_ref.py's arithmetic) of (m0[g], T[g], condition g's tables) under the Brown field, its sub-step i
    taking draw i of the oracle's stream (ssr.SEED, g R + r, NUMPY_ENV_STEP).  Returns dict(m [3, G R], failed, proj, counts at
    threshold 0 and NUMPY_BINS bins, distance = the smallest distance of a projection to a decision)."""
    import waveform_ref
    key = (method, scale, R)
    if key not in _CASES:
        m0, J, T, tgt = ssr.conditions()
        cur, fld = trapezoid(J, T, scale), field_ramp(T)
        rep = lambda a: np.repeat(a, R, axis=0)                                       # noqa: E731
        n_sub, _ = br.substeps(rep(T))
        normals = np.stack([waveform_ref.normals(oracle, ssr.SEED, i, NUMPY_ENV_STEP, int(n_sub[i])) for i in range(G * R)])
        res = br.solve(rep(m0), rep(T), ssr.params(), br.strength(oracle, ssr.params()), normals, method,
                       current=(rep(cur[0].T), rep(cur[1].T)), field=(rep(fld[0].T), rep(np.transpose(fld[1], (1, 0, 2)))))
        m, failed = res["m_final"].T.copy(), ~res["success"]
        pr = ssr.proj(m, rep(tgt))
        _CASES[key] = dict(cur=cur, fld=fld, m=m, failed=failed, proj=pr, counts=ssr.host_counts(m, failed, tgt, R, n_bins=NUMPY_BINS),
                           distance=ssr.edge_distance(pr, NUMPY_BINS))
    return _CASES[key]

"""NumPy restatement of the fixed-step solve with piecewise-linear current and field waveforms (stg_solve_wave; RK4 and Euler, no
thermal field, RobustLLGSSolver's gates included), vectorised over problems.  Written from the algorithm -- the macrospin LLGS equation
the reference's fixed-step solver integrates and the waveform semantics of include/spintorque_hip.h -- to check the kernels on inputs
the golden file does not hold; tests/test_waveform_host.py pins it against the golden rows recorded from the reference itself.

Everything is elementwise float64 NumPy (IEEE, no fused multiply-add), so the waveform values are the ones
`physics.PiecewiseLinear` computes, bit for bit."""
import numpy as np

MU0 = 4 * np.pi * 1e-7
GAMMA = 2.21e5


def pwl(tk, vk, t):
    """tk [N,K], vk [N,K] or [N,K,3], t [N] -> value at t per problem, [N] or [N,3]."""
    tk, vk, t = np.asarray(tk, float), np.asarray(vk, float), np.asarray(t, float)
    n, K = tk.shape
    rows = np.arange(n)
    # the largest k <= K-2 with tk[k] <= t (0 when t is below the table)
    k = np.minimum((tk[:, 1:] <= t[:, None]).sum(axis=1), K - 2)
    t0, t1 = tk[rows, k], tk[rows, k + 1]
    v0, v1 = vk[rows, k], vk[rows, k + 1]
    vec = vk.ndim == 3
    ex = (lambda a: a[:, None]) if vec else (lambda a: a)
    slope = (v1 - v0) / ex(t1 - t0)
    v = v0 + ex(t - t0) * slope
    v = np.where(ex(t <= tk[:, 0]), vk[:, 0], v)
    v = np.where(ex(t >= tk[:, -1]), vk[:, -1], v)
    return v


def _unit_or_default(m):
    """rows -> rows / |row|; a non-finite row or |row| < 1e-12 becomes +z.  Also returns the rows whose norm overflowed (m / inf)."""
    finite = np.isfinite(m).all(axis=1)
    with np.errstate(all="ignore"):
        norm = np.sqrt((m * m).sum(axis=1))
        out = m / norm[:, None]
    bad = ~finite | (norm < 1e-12) | ~np.isfinite(out).all(axis=1)
    out[bad] = (0.0, 0.0, 1.0)
    return out, finite & np.isinf(norm)


def solve(m0, T, params, method="rk4", current=None, J=None, field=None, max_step=1e-12, temperature=300.0, params_valid=True,
          trajectory=False):
    """m0 [N,3], T [N].  current = (tk [N,K], jk [N,K]) or None: then the rectangular J [N] while t <= T (None: no current).
    field = (th [N,K], hk [N,K,3]) or None.  Returns dict(success [N], m_final [N,3], n_steps [N]) and, with trajectory=True (N = 1),
    t [n+1] and m [n+1,3]."""
    m0 = np.array(m0, dtype=float).reshape(-1, 3)
    T = np.array(T, dtype=float).reshape(-1)
    N = len(T)
    alpha, ms, ku = params["damping"], params["saturation_magnetization"], params["uniaxial_anisotropy"]
    vol, pol = params["volume"], params["polarization"]
    e = np.asarray(params["easy_axis"], dtype=float)
    e = e / np.linalg.norm(e)
    hk = (2 * ku) / (MU0 * ms)
    geff = GAMMA / (1 + alpha ** 2)
    J = np.zeros(N) if J is None else np.array(J, dtype=float).reshape(-1)
    with np.errstate(all="ignore"):
        rejected = ~np.isfinite(m0).all(axis=1) | (np.sqrt((m0 * m0).sum(axis=1)) < 1e-12) | ~(T > 0) | (not params_valid) | \
            (not temperature > 0)
    Tn = np.where(rejected, 1.0, T)
    dt0 = np.minimum(max_step, Tn / 100)
    n = np.maximum(10, (Tn / dt0).astype(np.int64))
    dt = Tn / n
    n = np.where(rejected, 0, n)

    def rhs(m, t):
        cur = pwl(current[0], current[1], t) if current is not None else np.where(t <= T, J, 0.0)
        h = pwl(field[0], field[1], t) if field is not None else np.zeros((N, 3))
        H = h + (hk * (m @ e))[:, None] * e
        H[:, 2] += -ms * m[:, 2]
        prec = np.cross(m, H)
        damp = alpha * np.cross(m, prec)
        a = np.where(np.abs(cur) > 1e-12, (pol * cur) / (ms * vol), 0.0)
        return -geff * (prec + damp) + a[:, None] * np.cross(m, np.cross(m, e))

    m, _ = _unit_or_default(m0.copy())
    fail = np.zeros(N, dtype=bool)
    traj = [m[0].copy()] if trajectory else None
    h = dt[:, None]
    with np.errstate(all="ignore"):
        for i in range(int(n.max()) if N else 0):
            ti = i * dt
            if method == "euler":
                mn = m + h * rhs(m, ti)
            else:
                k1 = h * rhs(m, ti)
                k2 = h * rhs(m + k1 / 2, ti + dt / 2)
                k3 = h * rhs(m + k2 / 2, ti + dt / 2)
                k4 = h * rhs(m + k3, ti + dt)
                mn = m + (k1 + 2 * k2 + 2 * k3 + k4) / 6
            mn, zero_row = _unit_or_default(mn)
            live = i < n
            fail |= live & zero_row
            m = np.where(live[:, None], mn, m)
            if trajectory:
                traj.append(m[0].copy())
    ok = ~rejected & ~fail
    out = dict(success=ok, m_final=np.where(ok[:, None], m, m0), n_steps=n)
    if trajectory:
        out["m"] = np.array(traj)
        out["t"] = np.append(np.arange(int(n[0])) * dt[0], T[0])
    return out

"""NumPy restatement of the fixed-step solve with piecewise-linear current and field waveforms (stg_solve_wave; RK4 and Euler, the
thermal field white or Ornstein-Uhlenbeck, RobustLLGSSolver's gates included), vectorised over problems.  Written from the algorithm -- the macrospin LLGS equation
the reference's fixed-step solver integrates and the waveform semantics of include/spintorque_hip.h -- to check the kernels on inputs
the golden file does not hold; tests/test_waveform_host.py pins it against the golden rows recorded from the reference itself.

Everything is elementwise float64 NumPy (IEEE, no fused multiply-add), so the waveform values are the ones
`physics.PiecewiseLinear` computes, bit for bit.

The thermal field takes its strength and its standard normals from the C oracle (oracle.thermal_strength, oracle.thermal_normals:
`thermal_field`), never from the library under test; tests/test_wave_config_host.py pins both noise models against oracle.simple_solve
and the white one against solves of the reference itself (tests/golden/G24_wave_config.npz)."""
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


NORMALS = {}        # (seed, env_id, env_step) -> [calls,3]: the oracle's stream, fetched once (it replays from call 0 on every fetch)


def normals(oracle, seed, env_id, env_step, count):
    """the first `count` draws of the stream (seed, env_id, env_step), in call order"""
    key = (int(seed), int(env_id), int(env_step))
    have = NORMALS.get(key, np.zeros((0, 3)))
    if len(have) < count:
        more = [oracle.thermal_normals(key[0], key[1], key[2], c) for c in range(len(have), count)]
        have = NORMALS[key] = np.concatenate([have, np.array(more).reshape(-1, 3)])
    return have[:count]


def thermal_field(oracle, params, device_type, gamma, temperature, seed, env_ids, env_steps, noise="white", corr_time=1e-12):
    """the `thermal` argument of solve(): the fixed-step solvers' field strength for this class and the key of every problem's stream"""
    strength = oracle.thermal_strength(oracle.make_params(params, device_type), gamma, temperature, 0)
    return dict(strength=strength, oracle=oracle, seed=seed, env_id=np.asarray(env_ids), env_step=np.broadcast_to(env_steps, np.shape(env_ids)),
                noise=noise, corr_time=corr_time)


def solve(m0, T, params, method="rk4", current=None, J=None, field=None, max_step=1e-12, temperature=300.0, params_valid=True,
          trajectory=False, gamma=GAMMA, thermal=None):
    """m0 [N,3], T [N].  current = (tk [N,K], jk [N,K]) or None: then the rectangular J [N] while t <= T (None: no current).
    field = (th [N,K], hk [N,K,3]) or None.  thermal = None or dict(strength, noise 'white' | 'ou', corr_time, and either normals
    [N,calls,3] or oracle, seed, env_id [N], env_step [N]): white -- strength z joins H in every RHS call, the call index running as in
    the reference (four per RK4 sub-step, one per Euler sub-step); ou -- once per sub-step x <- d x + sqrt(1 - d^2) xi with
    d = exp(-dt / corr_time), x = 0 at the start, xi the sub-step's one draw, the field strength x for all stages (oracle/stg_oracle.c,
    stgo_simple_solve).  Returns dict(success [N], m_final [N,3], n_steps [N]) and, with trajectory=True (N = 1), t [n+1] and m [n+1,3]."""
    m0 = np.array(m0, dtype=float).reshape(-1, 3)
    T = np.array(T, dtype=float).reshape(-1)
    N = len(T)
    alpha, ms, ku = params["damping"], params["saturation_magnetization"], params["uniaxial_anisotropy"]
    vol, pol = params["volume"], params["polarization"]
    e = np.asarray(params["easy_axis"], dtype=float)
    e = e / np.linalg.norm(e)
    hk = (2 * ku) / (MU0 * ms)
    geff = gamma / (1 + alpha ** 2)
    J = np.zeros(N) if J is None else np.array(J, dtype=float).reshape(-1)
    with np.errstate(all="ignore"):
        rejected = ~np.isfinite(m0).all(axis=1) | (np.sqrt((m0 * m0).sum(axis=1)) < 1e-12) | ~(T > 0) | (not params_valid) | \
            (not temperature > 0)
    Tn = np.where(rejected, 1.0, T)
    dt0 = np.minimum(max_step, Tn / 100)
    n = np.maximum(10, (Tn / dt0).astype(np.int64))
    dt = Tn / n
    n = np.where(rejected, 0, n)

    nstage = 1 if method == "euler" else 4
    ou = thermal is not None and thermal.get("noise", "white") == "ou"
    z_all = None
    if thermal is not None:
        calls = n * (1 if ou else nstage)
        z_all = np.zeros((N, max(1, int(calls.max()) if N else 0), 3))
        for i in range(N):
            z_all[i, :calls[i]] = thermal["normals"][i][:calls[i]] if "normals" in thermal else \
                normals(thermal["oracle"], thermal["seed"], thermal["env_id"][i], thermal["env_step"][i], int(calls[i]))
        if ou:
            with np.errstate(all="ignore"):
                decay = np.exp(-dt / thermal["corr_time"]) if thermal["corr_time"] > 0 else np.zeros(N)
            ou_w = np.sqrt(1 - decay * decay)
            ou_x = np.zeros((N, 3))
    hth = [None]

    def draw(call):
        idx = np.minimum(call, z_all.shape[1] - 1)
        return thermal["strength"] * z_all[np.arange(N), idx]

    def rhs(m, t, call=None):
        cur = pwl(current[0], current[1], t) if current is not None else np.where(t <= T, J, 0.0)
        h = pwl(field[0], field[1], t) if field is not None else np.zeros((N, 3))
        H = h + (hk * (m @ e))[:, None] * e
        H[:, 2] += -ms * m[:, 2]
        if thermal is not None:
            H = H + (hth[0] if ou else draw(call))
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
            if ou:
                ou_x = decay[:, None] * ou_x + ou_w[:, None] * z_all[:, min(i, z_all.shape[1] - 1)]
                hth[0] = thermal["strength"] * ou_x
            c0 = nstage * i
            if method == "euler":
                mn = m + h * rhs(m, ti, c0)
            else:
                k1 = h * rhs(m, ti, c0)
                k2 = h * rhs(m + k1 / 2, ti + dt / 2, c0 + 1)
                k3 = h * rhs(m + k2 / 2, ti + dt / 2, c0 + 2)
                k4 = h * rhs(m + k3, ti + dt, c0 + 3)
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

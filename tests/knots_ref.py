"""NumPy restatement of the action parse of stg_step_knots (include/spintorque_hip.h, the four steps stated there) and the action rows
that hit its branches.  Shared by tests/test_step_knots_host.py and tests/test_gpu_step_knots.py; everything is elementwise NumPy."""
import numpy as np

import wave_step_ref


def parse_np(a, max_current, max_duration, limit):
    """actions a [N,2+P] float32 or float64 -> (J [N], T [N], s [N,P]) float64: rows 0 and 1 as stg_step parses them; the amplitudes in
    fp64, clamped by two compares that are both false for a NaN; one NaN amplitude voids the env's action to J = 0, T = 1e-12, s = 0"""
    a = np.asarray(a)
    J, T = wave_step_ref.parse_actions(a[:, :2], max_current, max_duration)
    s = a[:, 2:].astype(np.float64)
    with np.errstate(invalid="ignore"):
        s = np.where(s < -limit, -limit, np.where(s > limit, limit, s))
    void = np.isnan(s).any(axis=1)
    return np.where(void, 0.0, J), np.where(void, 1e-12, T), np.where(void[:, None], 0.0, s)


def knot_tables_np(tau, J, T, s):
    """the current table of the parsed action, env-major as wave_step_ref.step takes it: (tj [N,P], jk [N,P]) = (tau_j * T, J * s_j)"""
    return np.asarray(tau, dtype=np.float64)[None, :] * T[:, None], J[:, None] * s


def wave_rows(a):
    """the two rows stg_step_wave is handed for actions a [N,2+P] so that it parses the (J, T) of parse_np: a void action goes in as a
    NaN current, which stg_step parses to (0, 1e-12)"""
    a = np.asarray(a)
    void = np.isnan(a[:, 2:]).any(axis=1)
    return np.stack([np.where(void, a.dtype.type(np.nan), a[:, 0]), a[:, 1]], axis=1)


def edge_actions(dtype, P=4, limit=1.0):
    """rows that hit every branch of the parse, P amplitudes each: 0 ordinary; 1 beyond +-limit; 2 +-Inf; 3, 4 a NaN amplitude (void);
    5, 6 NaN in (J, T) with finite amplitudes; 7 Inf J; 8, 9 all-zero amplitudes; 10 J, T beyond their clips, denormal-small amplitudes;
    11 T below its clip; 12 J = 0"""
    rows = [[1.5e6, 1e-10] + [0.5] * P,
            [1.5e6, 1e-10] + ([2.0 * limit, -3.0 * limit, limit, -limit] + [0.25] * P)[:P],
            [1.5e6, 1e-10] + [np.inf, -np.inf] + [0.5] * (P - 2),
            [1.5e6, 1e-10] + [0.5] * (P - 1) + [np.nan],
            [1.5e6, 1e-10] + [np.nan] + [np.inf] * (P - 1),
            [np.nan, 1e-10] + [0.5] * P,
            [1e6, np.nan] + [0.5] * P,
            [np.inf, 1e-10] + [-0.5] * P,
            [1.5e6, 1e-10] + [0.0] * P,
            [-1.5e6, 8e-11] + [-0.0] * P,
            [9e9, 1e-3] + [1e-30] * P,
            [1.5e6, 1e-13] + [0.5] * P,
            [0.0, 1e-10] + [0.5] * P]
    return np.array(rows, dtype=dtype)

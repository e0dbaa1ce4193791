"""WHERE the macrospin C-ABI entry points write (include/spintorque_hip.h): stg_step_many, stg_step_ids, stg_reset, stg_get_state,
stg_set_state, stg_solve, stg_solve_traj, stg_thermal_normals and stg_device_terms are called directly, through `backend.lib` and
`backend._ctx`, with every caller-owned output in the interior of a larger sentinel-filled allocation (tests/helpers.py: Guarded).

  * every guard element behind and in front of each array still holds the sentinel afterwards (back guards are at least the array at
    N rounded up to whole 4096-slot tiles plus a row: a store one row, one record or one ragged tile too far fails an assertion
    and never leaves the allocation),
  * every element the contract says is written no longer holds it, every element it says is left alone still does,
  * the interiors, and the state after the call, equal bit for bit what a second, identically configured context gives through the
    normal HipBackend methods (the plain runs the oracle tests pin; asserted finite first, so the NaN sentinels cannot collide).

The step cases force every launch form through configuration alone; test_table_covers_what_it_claims (no GPU needed) evaluates
csrc/stg_launch_plan.hpp for each row and pins the form it takes."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from conftest import sot_default_params, stt_default_params, vcma_default_params
from helpers import GUARD_TILE, Guarded
from test_launch_plan import CSRC, DEFAULTS as PLAN_DEFAULTS, DRIVER, FIELDS, PLAN

gpu = pytest.mark.gpu

VOL_RK4, VOL_RK45 = 8.75e-11, 9.7e-6          # the regimes in which the current drives switching (bench.py: volume_for)
T_FIXED, T_RK45 = 1e-10, 3e-11                # longest pulses: 100 RK4 / Euler sub-steps, some 45 RK45 attempts
STATE_KEYS = ("m", "target", "total_energy", "step_count", "rng_step", "done")
STATE_DTYPES = dict(m=torch.float64, target=torch.float64, total_energy=torch.float64, step_count=torch.int32, rng_step=torch.int32,
                    done=torch.uint8)
F32, F64, U8, I32 = torch.float32, torch.float64, torch.uint8, torch.int32

# configurations by name: SpinTorqueVecEnv keyword arguments (+ `mode`: how the device parameters are given)
BASES = {
    "rk4-thermal": dict(solver="rk4"),
    "rk4-T0": dict(solver="rk4", include_thermal_fluctuations=False),
    "rk4-thermal-identity": dict(solver="rk4", lane_sort=False),
    "euler-thermal-inline": dict(solver="euler", wave_spec=False),
    "rk45-thermal": dict(solver="rk45"),
    "rk45-T0": dict(solver="rk45", include_thermal_fluctuations=False),
    "rk45-thermal-inline": dict(solver="rk45", wave_spec=False),
    "rk45-T0-refill": dict(solver="rk45", include_thermal_fluctuations=False, lane_refill=2),
    "rk45-thermal-refill": dict(solver="rk45", lane_refill=2),
    "rk4-T0-classes3": dict(solver="rk4", include_thermal_fluctuations=False, mode="classes"),
    "rk4-devphys-mixed": dict(solver="rk4", torque_model="device", mode="classes-uneven"),
    "rk4-thermal-per-env": dict(solver="rk4", mode="per-env"),
    "rk4-thermal-skip-done": dict(solver="rk4", skip_done=True),
}


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as stg
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return stg


def _unit_rows(rng, n):
    v = rng.normal(0, 1, (n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _make(stg, base, n, layout, **extra):
    kw = dict(BASES[base], **extra)
    mode = kw.pop("mode", None)
    vol = VOL_RK45 if kw["solver"] == "rk45" else VOL_RK4
    rng = np.random.default_rng(5)
    if mode in ("classes", "classes-uneven"):
        kw.update(device_type=["stt_mram", "sot_mram", "vcma_mram"],
                  device_params=[stt_default_params(volume=vol), sot_default_params(volume=vol, polarization=0.7),
                                 vcma_default_params(volume=vol, polarization=0.7)],
                  # (uneven: a ragged tile then holds a whole 256-slot group of one kind and a mixed, partly filled one)
                  class_index=(np.arange(n) % 3).astype(np.uint8) if mode == "classes"
                  else rng.choice(3, n, p=[0.6, 0.25, 0.15]).astype(np.uint8))
    elif mode == "per-env":
        kw.update(device_params=stt_default_params(volume=vol),
                  per_env_params={"damping": rng.uniform(0.005, 0.03, n), "polarization": rng.uniform(0.5, 0.8, n)})
    else:
        kw.update(device_params=stt_default_params(volume=vol))
    return stg.SpinTorqueVecEnv(n, diagnostics=True, seed=11, out_layout=layout, **kw)


def _start(env, base, n):
    """Both contexts of a case start from the same given rows; the skip_done row then marks a third of the envs as finished."""
    rng = np.random.default_rng(17)
    m0, tgt = _unit_rows(rng, n), np.where(rng.integers(0, 2, (n, 1)) == 0, 1.0, -1.0) * np.array([[0.0, 0.0, 1.0]])
    env.reset(options={"initial_state": m0, "target_state": tgt})
    if BASES[base].get("skip_done"):
        env.backend.set_state({"done": (torch.arange(n) % 3 == 0).to(torch.uint8)})


def _actions(seed, K, n, solver, f64=False):
    rng = np.random.default_rng(seed)
    a = np.empty((K, 2, n), dtype=np.float64 if f64 else np.float32)
    a[:, 0] = rng.uniform(-2e6, 2e6, (K, n))
    a[:, 1] = rng.uniform(1e-11, T_RK45 if solver == "rk45" else T_FIXED, (K, n))
    return torch.tensor(a, device="cuda")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _gptr(g, name):
    return _ptr(g[name].interior) if name in g else None


def _bits(t):
    t = t.contiguous()
    return t.view({F32: torch.int32, F64: torch.int64}.get(t.dtype, t.dtype))


def _same(x, y, what):
    """bit for bit (floats compared as integers: -0.0 is not 0.0, and a NaN would not equal itself otherwise)"""
    assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape, x.dtype, y.dtype)
    bad = (_bits(x) != _bits(y)).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements differ from the plain run, first at {bad[:4].tolist()}"


def _state(b):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in b.get_state().items()}


def _same_state(sa, sb, what):
    for k in STATE_KEYS:
        _same(sa[k], sb[k], (what, "state", k))


def _check(rc, b):
    assert rc == 0, (rc, b.lib.stg_last_error())
    torch.cuda.synchronize()


def _step_guards(ko, n, layout, final, nulls=()):
    """Guarded outputs of one step launch: [ko] blocks of n envs (n = M for an id launch)."""
    g = {}
    if layout == "records":
        g["records"] = Guarded("records", (ko, n, 14), I32, n_axis=1)       # 56-byte records as 14 words: the sentinel is 0xA5 in every byte
        if final:
            g["final_obs"] = Guarded("final_obs", (ko, n, 12), F32, n_axis=1)
    else:
        g["obs"] = Guarded("obs", (ko, 12, n), F32)
        g["reward"] = Guarded("reward", (ko, n), F32)
        g["terminated"], g["truncated"] = Guarded("terminated", (ko, n), U8), Guarded("truncated", (ko, n), U8)
        if final:
            g["final_obs"] = Guarded("final_obs", (ko, 12, n), F32)
    for name, dt in (("reward_f64", F64), ("energy", F64), ("status", U8)):
        if name not in nulls:
            g[name] = Guarded(name, (ko, n), dt)
    return g


def _out_args(g):
    return (_gptr(g, "records") if "records" in g else _gptr(g, "obs"), _gptr(g, "final_obs"), _gptr(g, "reward"), _gptr(g, "reward_f64"),
            _gptr(g, "energy"), _gptr(g, "terminated"), _gptr(g, "truncated"), _gptr(g, "status"))


def _guarded_step_many(env, a, out_every, autoreset, layout, final=None, nulls=()):
    b = env.backend
    K, n = int(a.shape[0]), b.n
    g = _step_guards(K if out_every else 1, n, layout, bool(autoreset) if final is None else final, nulls)
    _check(b.lib.stg_step_many(b._ctx, K, _ptr(a), int(a.dtype == F64), int(out_every), int(autoreset), *_out_args(g), b._stream()), b)
    return g


def _plain_step_many(env, a, out_every, autoreset):
    """The plain run through HipBackend.step_many: dict of [ko, ...] tensors, obs and final_obs component-major [ko, 12, n]."""
    b = env.backend
    obs, reward, reward64, term, trunc, status = b.step_many(a, out_every=bool(out_every), autoreset=bool(autoreset))
    torch.cuda.synchronize()
    w = dict(obs=obs.contiguous(), reward=reward.contiguous(), reward_f64=reward64, energy=b.energy_many, terminated=term.contiguous(),
             truncated=trunc.contiguous(), status=status.contiguous())
    if autoreset:
        w["final_obs"] = b.final_obs_many.contiguous()
    return w


def _check_step(g, want, layout, what, ok_slots=None):
    """Guards, written-ness and values of one step launch's outputs against the plain run `want` (see the module docstring).
    ok_slots (bool [n], id launches with bad ids): the slots whose final_obs may be written."""
    for k in ("obs", "reward", "reward_f64", "energy"):
        assert bool(torch.isfinite(want[k]).all()), (what, k)
    if layout == "records":
        rec = g["records"].check().view(U8)                               # every word of every record written; [ko, n, 56]
        assert bool((rec[..., 55] == 0).all()), (what, "byte 55 of a record is not 0")
        f = rec.view(F32)
        got = dict(obs=f[..., :12].transpose(1, 2), reward=f[..., 12], terminated=rec[..., 52], truncated=rec[..., 53])
        _same(rec[..., 54], want["status"], (what, "status byte of the records"))
    else:
        got = {k: g[k].check() for k in ("obs", "reward", "terminated", "truncated")}
    for k in ("reward_f64", "energy", "status"):
        if k in g:
            got[k] = g[k].check()
    for k, v in got.items():
        _same(v.contiguous(), want[k], (what, k))
    assert int(got["terminated"].max()) <= 1 and int(got["truncated"].max()) <= 1 and int(want["status"].max()) <= 4, what
    if "final_obs" in g:
        done = (want["terminated"] | want["truncated"]) != 0              # [ko, n]: final_obs is written for exactly these
        if ok_slots is not None:
            done = done & ok_slots
        mask = done[:, :, None] if layout == "records" else done[:, None, :]
        fo = g["final_obs"].check(written=mask)
        fo = fo.transpose(1, 2) if layout == "records" else fo
        sel = done[:, None, :].expand_as(fo)
        assert bool(torch.isfinite(want["final_obs"][sel]).all()), (what, "final_obs")
        _same(fo[sel], want["final_obs"][sel], (what, "final_obs"))
        return done
    return None


# ------------------------------------------------------------------------------------------------
# a. every launch form of one step
# ------------------------------------------------------------------------------------------------
def _P(**kw):
    return dict(dict(sort=0, pc=0, hybrid=0, refill=0, multi=0, by_kind=0, skip_done=0), **kw)


ONE = ((False, "records"),)
ALL4 = ((False, "records"), (True, "records"), (False, "soa"), (True, "soa"))
N_BIG = 65536 + 77
# (configuration, N, the plan it must take, (float64 actions, layout) variants)
STEP_ROWS = [
    # identity schedule: a single wavefront, or lane_sort = -1
    ("rk4-thermal", 1, _P(pc=1), ONE), ("rk4-thermal", 63, _P(pc=1), ONE), ("rk4-thermal", 64, _P(pc=1), ONE),
    ("rk4-thermal-identity", 130, _P(pc=1), ONE),
    # sorted schedule, one-wavefront workgroups
    ("rk4-T0", 65, _P(sort=1), ALL4), ("rk4-T0", 130, _P(sort=1), ALL4), ("rk4-T0", 4097, _P(sort=1), ALL4), ("rk4-T0", 4160, _P(sort=1), ALL4),
    ("euler-thermal-inline", 130, _P(sort=1), ONE),
    # producer / consumer pairs
    ("rk4-thermal", 65, _P(sort=1, pc=1), ALL4), ("rk4-thermal", 4160, _P(sort=1, pc=1), ALL4), ("rk45-thermal", 130, _P(sort=1, pc=1), ALL4),
    # RK45 with the normals inline
    ("rk45-thermal-inline", 130, _P(sort=1), ONE),
    # RK45 forced lane refill (with the thermal field the plan also says pc, which the refill launch overrides)
    ("rk45-T0-refill", 130, _P(sort=1, refill=2), ALL4), ("rk45-T0-refill", 4097, _P(sort=1, refill=2), ALL4),
    ("rk45-thermal-refill", 130, _P(sort=1, pc=1, refill=2), ALL4), ("rk45-thermal-refill", 4097, _P(sort=1, pc=1, refill=2), ALL4),
    # class table in LDS; device-physics torque model (by_kind + regroup); per-env parameter records
    ("rk4-T0-classes3", 130, _P(sort=1, multi=1), ONE),
    ("rk4-devphys-mixed", GUARD_TILE + 700, _P(sort=1, multi=1, by_kind=1), ONE), ("rk4-devphys-mixed", 300, _P(sort=1, multi=1, by_kind=1), ONE),
    ("rk4-thermal-per-env", 130, _P(sort=1, pc=1, multi=2), ONE),
    # skip_done: inactive lanes still write complete outputs
    ("rk4-thermal-skip-done", 130, _P(sort=1, pc=1, skip_done=1), ONE),
    # four-wavefront workgroups (no pairs, >= 65 536 envs) and the hybrid launch (2048 - 17 * 64 = 960 pairs)
    ("rk4-T0", N_BIG, _P(sort=1), ONE), ("rk4-thermal", N_BIG, _P(sort=1, pc=1, hybrid=961), ONE),
]
STEP_CASES = [(base, n, f64, layout) for base, n, _, variants in STEP_ROWS for f64, layout in variants]


def _case_id(c):
    base, n, f64, layout = c
    return f"{base}-{n}-{'f64' if f64 else 'f32'}-{layout}"


def _plan_input(base, n):
    """The arguments of plan_step for a full step of configuration `base` at n envs, as EnvConfig.to_abi and HipBackend hand them over."""
    kw = BASES[base]
    tri = {None: 0, True: 1, False: -1}
    mode = kw.get("mode")
    return dict(PLAN_DEFAULTS, solver=kw["solver"], thermal=int(kw.get("include_thermal_fluctuations", True)), temperature=300.0,
                torque_model=int(kw.get("torque_model") == "device"), lane_sort=tri[kw.get("lane_sort")], wave_spec=tri[kw.get("wave_spec")],
                lane_refill=kw.get("lane_refill") or 0, skip_done=int(kw.get("skip_done", False)), n=n, K=1, autoreset=0, ids=0,
                per_env=int(mode == "per-env"), ncls=0 if mode == "per-env" else (3 if mode else 1), has_cls=int(mode in ("classes", "classes-uneven")))


def test_table_covers_what_it_claims(tmp_path):
    """Every row of STEP_ROWS takes the launch form it is there for: plan_step (csrc/stg_launch_plan.hpp, built with the host compiler
    as tests/test_launch_plan.py builds it) returns the intended sort / pc / hybrid / refill / multi / by_kind (/ skip_done), and the
    rows together cover every form of the step launch."""
    src, exe = str(tmp_path / "plan_driver.cpp"), str(tmp_path / "plan_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    lines = [" ".join(str(_plan_input(base, n)[k]) for k in FIELDS) for base, n, _, _ in STEP_ROWS]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(STEP_ROWS), out
    forms = set()
    for (base, n, want, variants), line in zip(STEP_ROWS, out):
        words = line.split()
        assert words[0] == "plan", (base, n, line)
        got = dict(zip(PLAN, map(int, words[1:])))
        assert {k: got[k] for k in want} == want, (base, n, got)
        wg4 = int(n >= 65536 and not got["pc"])                           # (stg_kernels.hpp: STG_WG4_MIN_ENVS, decided in dispatch_step)
        for f64, layout in variants:
            forms.add((got["sort"], got["pc"] and not got["refill"], int(got["hybrid"] > 0), int(got["refill"] > 0), got["multi"], got["by_kind"],
                       got["skip_done"], wg4, f64, layout))
    def covered(**kw):
        keys = ("sort", "pc", "hybrid", "refill", "multi", "by_kind", "skip_done", "wg4", "f64", "layout")
        return any(all(f[keys.index(k)] == v for k, v in kw.items()) for f in forms)
    assert covered(sort=0, pc=1) and covered(sort=1, pc=0, refill=0, wg4=0) and covered(sort=1, pc=1, hybrid=0)
    assert covered(hybrid=1) and covered(wg4=1) and covered(multi=1, by_kind=0) and covered(multi=1, by_kind=1) and covered(multi=2)
    assert covered(skip_done=1)
    for f64 in (False, True):                                            # the three forms that read act_sorted in either dtype, in both layouts
        for layout in ("records", "soa"):
            assert covered(sort=1, pc=0, refill=0, f64=f64, layout=layout) and covered(sort=1, pc=1, f64=f64, layout=layout)
            assert covered(refill=1, f64=f64, layout=layout)


@gpu
@pytest.mark.parametrize("case", STEP_CASES, ids=_case_id)
def test_step_writes_every_output_and_nothing_else(stg, case):
    """One stg_step_many call with K = 1 in the launch form of the case: all of obs[12][N], reward, reward_f64, energy, terminated,
    truncated and status (or all 56 bytes of every record, byte 55 = 0) written, equal to the plain run, flags <= 1, status <= 4,
    every guard intact; the state afterwards equals the plain run's."""
    base, n, f64, layout = case
    plain, env = _make(stg, base, n, layout), _make(stg, base, n, layout)
    _start(plain, base, n); _start(env, base, n)
    a = _actions(n, 1, n, BASES[base]["solver"], f64)
    want = _plain_step_many(plain, a, 1, 0)
    g = _guarded_step_many(env, a, 1, 0, layout)
    _check_step(g, want, layout, case)
    _same_state(_state(env.backend), _state(plain.backend), case)
    if BASES[base].get("skip_done"):
        fin = (torch.arange(n, device="cuda") % 3 == 0)
        assert bool((want["status"][0][fin] == 3).all()) and not bool((want["status"][0][~fin] == 3).any())
    plain.close(); env.close()


@gpu
@pytest.mark.parametrize("layout", ("records", "soa"))
def test_stg_step_entry_point(stg, layout):
    """stg_step itself (stg_step_many with K = 1, out_every = 1, no auto-reset, no final_obs) with the same guards."""
    base, n = "rk4-thermal", 130
    plain, env = _make(stg, base, n, layout), _make(stg, base, n, layout)
    _start(plain, base, n); _start(env, base, n)
    a = _actions(n, 1, n, "rk4")
    want = _plain_step_many(plain, a, 1, 0)
    b = env.backend
    g = _step_guards(1, n, layout, False)
    obs, _, reward, reward_f64, energy, term, trunc, status = _out_args(g)
    _check(b.lib.stg_step(b._ctx, _ptr(a), 0, obs, reward, reward_f64, energy, term, trunc, status, b._stream()), b)
    _check_step(g, want, layout, layout)
    _same_state(_state(b), _state(plain.backend), layout)
    plain.close(); env.close()


# ------------------------------------------------------------------------------------------------
# b. fused steps and auto-reset
# ------------------------------------------------------------------------------------------------
K_FUSED = 3
FUSED = [(base, n, layout) for base in ("rk4-T0", "rk4-thermal") for n in (130, 4097) for layout in ("records", "soa")]


def _fused_pair(stg, base, n, layout, **extra):
    plain, env = _make(stg, base, n, layout, max_steps=2, **extra), _make(stg, base, n, layout, max_steps=2, **extra)
    _start(plain, base, n); _start(env, base, n)
    return plain, env, _actions(1000 + n, K_FUSED, n, "rk4")


@gpu
@pytest.mark.parametrize("case", FUSED, ids=lambda c: "-".join(map(str, c)))
def test_fused_steps_write_all_k_blocks(stg, case):
    """K = 3, out_every = 1, autoreset = 0, max_steps = 2 (every env is truncated at step 2 of the launch and stepped on)."""
    base, n, layout = case
    plain, env, a = _fused_pair(stg, base, n, layout)
    want = _plain_step_many(plain, a, 1, 0)
    assert bool((want["truncated"][1:] == 1).all()) and not bool((want["truncated"][0] == 1).any())
    _check_step(_guarded_step_many(env, a, 1, 0, layout), want, layout, case)
    _same_state(_state(env.backend), _state(plain.backend), case)
    plain.close(); env.close()


@gpu
@pytest.mark.parametrize("autoreset", (0, 1))
@pytest.mark.parametrize("case", FUSED, ids=lambda c: "-".join(map(str, c)))
def test_fused_last_step_only_writes_one_block(stg, case, autoreset):
    """out_every = 0: a leading dimension of 1 -- exactly one block is written, it equals the last step of the plain out_every = 1 run,
    and the K - 1 blocks behind it (inside the back guard) are untouched.  With autoreset (threshold 0: about half of the envs finish at
    the last step) final_obs is one block too."""
    base, n, layout = case
    plain, env, a = _fused_pair(stg, base, n, layout, success_threshold=0.0)
    want = {k: v[K_FUSED - 1:] for k, v in _plain_step_many(plain, a, 1, autoreset).items()}
    g = _guarded_step_many(env, a, 0, autoreset, layout)
    for name, gd in g.items():
        assert gd.shape[0] == 1 and gd.raw.numel() - gd.front - gd.numel >= (K_FUSED - 1) * gd.numel, name
    done = _check_step(g, want, layout, (case, autoreset))
    if autoreset:
        assert 0 < int(done.sum()) < n
    _same_state(_state(env.backend), _state(plain.backend), case)
    plain.close(); env.close()


@gpu
@pytest.mark.parametrize("threshold", (2.0, 0.0), ids=("all-at-step-2", "some-at-every-step"))
@pytest.mark.parametrize("case", FUSED, ids=lambda c: "-".join(map(str, c)))
def test_fused_autoreset_final_obs_exactly_where_an_episode_ended(stg, case, threshold):
    """autoreset = 1 with final_obs [K][12][N] ([K][N][12] in the records layout) guarded: block k holds the terminal observation of
    the envs whose episode ended at step k and the sentinel everywhere else.  With a threshold no alignment reaches, max_steps = 2
    ends every episode at step 2 of the launch and none at steps 1 and 3; with the threshold at 0 some episodes end at every step,
    so that each block mixes written and untouched entries."""
    base, n, layout = case
    plain, env, a = _fused_pair(stg, base, n, layout, success_threshold=threshold)
    want = _plain_step_many(plain, a, 1, 1)
    done = _check_step(_guarded_step_many(env, a, 1, 1, layout), want, layout, (case, threshold))
    if threshold == 0.0:
        assert all(0 < int(done[k].sum()) < n for k in range(K_FUSED))
    else:
        assert bool(done[1].all()) and not bool(done[0].any()) and not bool(done[2].any())
    _same_state(_state(env.backend), _state(plain.backend), case)
    plain.close(); env.close()


@gpu
@pytest.mark.parametrize("layout", ("records", "soa"))
def test_optional_step_outputs_may_be_null_in_any_combination(stg, layout):
    """reward_f64, energy and status NULL in all 2^3 combinations (final_obs NULL throughout, autoreset on): what remains is bit-identical
    to the run with every output present."""
    base, n = "rk4-thermal", 130
    plain = _make(stg, base, n, layout, max_steps=2)
    _start(plain, base, n)
    a = _actions(1000 + n, K_FUSED, n, "rk4")
    want = _plain_step_many(plain, a, 1, 1)
    del want["final_obs"]
    st = _state(plain.backend)
    plain.close()
    for combo in range(8):
        nulls = tuple(name for j, name in enumerate(("reward_f64", "energy", "status")) if combo >> j & 1)
        env = _make(stg, base, n, layout, max_steps=2)
        _start(env, base, n)
        g = _guarded_step_many(env, a, 1, 1, layout, final=False, nulls=nulls)
        assert set(g) & set(nulls) == set() and "final_obs" not in g
        _check_step(g, want, layout, (layout, nulls))
        _same_state(_state(env.backend), st, (layout, nulls))
        env.close()


# ------------------------------------------------------------------------------------------------
# c. stg_step_ids
# ------------------------------------------------------------------------------------------------
N_IDS = 5000
IDS_CFG = {   # configuration, layout, autoreset, extra keyword arguments
    "rk4-thermal-records-autoreset": ("rk4-thermal", "records", 1, dict(success_threshold=0.0)),
    "rk45-T0-refill-soa": ("rk45-T0-refill", "soa", 0, {}),
    "rk4-devphys-mixed-records-autoreset": ("rk4-devphys-mixed", "records", 1, dict(success_threshold=0.0)),
}


def _ids_pair(stg, name):
    base, layout, ar, extra = IDS_CFG[name]
    plain, env = _make(stg, base, N_IDS, layout, **extra), _make(stg, base, N_IDS, layout, **extra)
    _start(plain, base, N_IDS); _start(env, base, N_IDS)
    return plain, env, base, layout, ar


def _plain_ids(plain, a, ids, ar):
    """HipBackend.step_ids as the plain run: the same dict as _plain_step_many with a leading dimension of 1."""
    out = plain.backend.step_ids(a, ids, autoreset=bool(ar))
    torch.cuda.synchronize()
    w = {k: out[s].contiguous()[None] for k, s in (("obs", "obs"), ("reward", "reward"), ("reward_f64", "reward64"), ("energy", "energy"),
                                                   ("terminated", "terminated"), ("truncated", "truncated"), ("status", "status"))}
    if ar:
        w["final_obs"] = out["final_obs"].contiguous()[None]
    return w


def _guarded_ids(env, a, ids32, ar, layout, ws_for=None):
    """stg_step_ids with guarded outputs and a workspace of exactly stg_step_ids_workspace_bytes(ctx, ws_for or M) bytes between guards."""
    b = env.backend
    M = int(ids32.numel())
    nb = int(b.lib.stg_step_ids_workspace_bytes(b._ctx, int(ws_for or M)))
    assert nb > 0
    ws = Guarded("workspace", (nb,), U8)
    assert ws.interior.numel() == nb and ws.interior.data_ptr() % 16 == 0
    g = _step_guards(1, M, layout, bool(ar))
    _check(b.lib.stg_step_ids(b._ctx, M, _ptr(ids32), _ptr(a), int(a.dtype == F64), int(ar), _ptr(ws.interior), *_out_args(g), b._stream()), b)
    ws.check_guards()
    return g


@gpu
@pytest.mark.parametrize("M", (1, 63, 65, 130, 4097))
@pytest.mark.parametrize("name", list(IDS_CFG))
def test_step_ids_outputs_are_compact_and_the_workspace_is_enough(stg, name, M):
    """Random unsorted distinct ids out of 5000 envs: outputs with stride M (not N) fully written between intact guards, final_obs
    only for the listed envs whose episode ended, the workspace's two guards intact, results and state equal to HipBackend.step_ids."""
    plain, env, base, layout, ar = _ids_pair(stg, name)
    rng = np.random.default_rng(100 + M)
    ids = torch.tensor(rng.permutation(N_IDS)[:M].astype(np.int32), device="cuda")
    a = _actions(M, 1, M, BASES[base]["solver"])[0]
    want = _plain_ids(plain, a, ids, ar)
    done = _check_step(_guarded_ids(env, a, ids, ar, layout), want, layout, (name, M))
    if ar and M >= 63:
        assert 0 < int(done.sum()) < M
    _same_state(_state(env.backend), _state(plain.backend), (name, M))
    plain.close(); env.close()


@gpu
@pytest.mark.parametrize("name", list(IDS_CFG))
def test_step_ids_workspace_sized_for_a_longer_list(stg, name):
    """A workspace sized for 4097 ids serves a list of 65 with identical results."""
    plain, env, base, layout, ar = _ids_pair(stg, name)
    M = 65
    ids = torch.tensor(np.random.default_rng(3).permutation(N_IDS)[:M].astype(np.int32), device="cuda")
    a = _actions(M, 1, M, BASES[base]["solver"])[0]
    want = _plain_ids(plain, a, ids, ar)
    _check_step(_guarded_ids(env, a, ids, ar, layout, ws_for=4097), want, layout, name)
    _same_state(_state(env.backend), _state(plain.backend), name)
    plain.close(); env.close()


@gpu
@pytest.mark.parametrize("M", (130, 4097))
@pytest.mark.parametrize("name", list(IDS_CFG))
def test_step_ids_bad_ids_are_reported_and_nothing_else_moves(stg, name, M):
    """About a tenth of the list is >= N (N itself, 2^31 + 5, 0xFFFFFFFF, ...): those slots report status 4 with a zero observation,
    reward and flags and an untouched final_obs; every other slot equals the launch without them; guards and workspace intact."""
    plain, env, base, layout, ar = _ids_pair(stg, name)
    rng = np.random.default_rng(200 + M)
    ids = rng.permutation(N_IDS)[:M].astype(np.uint32)
    bad = rng.random(M) < 0.1
    bad[[0, M // 2, M - 1]] = True
    pool = np.array([N_IDS, N_IDS + 1, (1 << 31) + 5, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    ids[bad] = pool[np.arange(int(bad.sum())) % len(pool)]
    ids[M - 1] = 0xFFFFFFFF
    a = _actions(M, 1, M, BASES[base]["solver"])[0]
    good = torch.tensor(~bad, device="cuda")
    sub = _plain_ids(plain, a[:, good].contiguous(), torch.tensor(ids[~bad].astype(np.int32), device="cuda"), ar)
    want = {}
    for k, v in sub.items():                                             # the plain run's slots scattered into the full list, zeros elsewhere
        full = torch.zeros((*v.shape[:-1], M), dtype=v.dtype, device="cuda")
        full[..., good] = v
        want[k] = full
    want["status"][0, ~good] = 4
    _check_step(_guarded_ids(env, a, torch.tensor(ids.view(np.int32), device="cuda"), ar, layout), want, layout, (name, M), ok_slots=good[None])
    _same_state(_state(env.backend), _state(plain.backend), (name, M))
    plain.close(); env.close()


# ------------------------------------------------------------------------------------------------
# d. stg_reset
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("given", (False, True), ids=("device-draws", "given-rows"))
@pytest.mark.parametrize("masked", (False, True), ids=("all", "every-third"))
@pytest.mark.parametrize("layout", ("records", "soa"))
@pytest.mark.parametrize("n", (1, 65, 130))
def test_reset_footprint(stg, n, layout, masked, given):
    """stg_reset after one step.  SoA: every obs element written.  Records, pre-filled with the sentinel: a reset env's record is
    written whole with zero reward and flag bytes; an env the mask leaves alone gets bytes 0-47 rewritten with its current observation
    while bytes 48-55 stay untouched, and its state is bit for bit what it was.  obs_out = NULL is accepted and changes no state."""
    base = "rk4-thermal"
    envs = [_make(stg, base, n, layout) for _ in range(3)]               # plain, guarded, obs_out = NULL
    a = _actions(n, 1, n, "rk4")[0]
    for e in envs:
        _start(e, base, n)
        e.backend.step(a)
    rng = np.random.default_rng(40 + n)
    mask = ((torch.arange(n) + 1) % 3 == 0).to(U8).cuda() if masked else None      # (n = 1: the one env is left alone)
    init = torch.tensor((_unit_rows(rng, n) * rng.uniform(0.5, 3.0, (n, 1))).T.copy(), device="cuda") if given else None
    tgt = torch.tensor((_unit_rows(rng, n) * rng.uniform(0.5, 3.0, (n, 1))).T.copy(), device="cuda") if given else None
    seed = 77
    plain, env, quiet = (e.backend for e in envs)
    pre = _state(env)
    want = plain.reset(mask, init, tgt, seed).contiguous()               # [12, n]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all())
    g = Guarded("records", (n, 14), I32, n_axis=0) if layout == "records" else Guarded("obs", (12, n), F32)
    _check(env.lib.stg_reset(env._ctx, _ptr(mask), _ptr(init), _ptr(tgt), C.c_uint64(seed), _ptr(g.interior), env._stream()), env)
    _check(quiet.lib.stg_reset(quiet._ctx, _ptr(mask), _ptr(init), _ptr(tgt), C.c_uint64(seed), None, quiet._stream()), quiet)
    is_reset = torch.ones(n, dtype=torch.bool, device="cuda") if mask is None else mask != 0
    if layout == "records":
        written = torch.ones((n, 14), dtype=torch.bool, device="cuda")
        written[:, 12:] = is_reset[:, None]                               # reward and flag words: the reset envs' only
        rec = g.check(written=written)
        _same(rec.view(F32)[:, :12].t().contiguous(), want, "obs fields of the records")
        assert bool((rec[is_reset][:, 12:] == 0).all()), "reward and flag bytes of a reset env"
    else:
        _same(g.check(), want, "obs")
    post = _state(env)
    _same_state(post, _state(plain), (n, layout, masked, given))
    _same_state(_state(quiet), post, "obs_out = NULL")
    for k in STATE_KEYS:
        _same(post[k][..., ~is_reset], pre[k][..., ~is_reset], ("env left alone", k))
    if not masked:
        assert bool((post["step_count"] == 0).all()) and bool((post["total_energy"] == 0).all())
    for e in envs:
        e.close()


# ------------------------------------------------------------------------------------------------
# e. stg_get_state / stg_set_state
# ------------------------------------------------------------------------------------------------
N_STATE = 130
STATE_SHAPES = dict(m=(3, N_STATE), target=(3, N_STATE), total_energy=(N_STATE,), step_count=(N_STATE,), rng_step=(N_STATE,), done=(N_STATE,))


def _varied_env(stg):
    """Three steps with the thermal field: auto-reset on, one of them on half of the envs only (stream positions differ), the last one
    without auto-reset (done flags differ); threshold 0, so that step counts and total energies differ from env to env too."""
    env = _make(stg, "rk4-thermal", N_STATE, "records", success_threshold=0.0, max_steps=3)
    _start(env, "rk4-thermal", N_STATE)
    a = _actions(7, 3, N_STATE, "rk4")
    b = env.backend
    b.step(a[0], autoreset=True)
    half = torch.arange(0, N_STATE, 2, device="cuda", dtype=torch.int32)
    b.step_ids(a[1][:, ::2].contiguous(), half, autoreset=True)
    b.step(a[2], autoreset=False)
    st = _state(b)
    for k in ("step_count", "rng_step", "done", "total_energy"):
        assert len(torch.unique(st[k])) > 1, k
    return env, st


def _state_args(named):
    return [_ptr(named.get(k)) for k in STATE_KEYS]


@gpu
def test_get_state_single_pointers(stg):
    """stg_get_state with each single pointer non-NULL and the rest NULL writes that array fully, equal to the all-pointers call,
    between intact guards; and all six together."""
    env, st = _varied_env(stg)
    b = env.backend
    for k in STATE_KEYS:
        g = Guarded(k, STATE_SHAPES[k], STATE_DTYPES[k])
        _check(b.lib.stg_get_state(b._ctx, *_state_args({k: g.interior}), b._stream()), b)
        _same(g.check(), st[k], k)
    gs = {k: Guarded(k, STATE_SHAPES[k], STATE_DTYPES[k]) for k in STATE_KEYS}
    _check(b.lib.stg_get_state(b._ctx, *_state_args({k: g.interior for k, g in gs.items()}), b._stream()), b)
    for k in STATE_KEYS:
        _same(gs[k].check(), st[k], k)
    env.close()


@gpu
@pytest.mark.parametrize("field", STATE_KEYS)
def test_set_state_of_one_field_changes_only_that_field(stg, field):
    """step_count, the done bit and rng_step share one 8-byte word of the state record (and total_energy its 16-byte store): a partial
    set must merge, not overwrite."""
    env, st = _varied_env(stg)
    b = env.backend
    rng = np.random.default_rng(9)
    n = N_STATE
    new = dict(m=lambda: torch.tensor(_unit_rows(rng, n).T.copy()), target=lambda: torch.tensor(_unit_rows(rng, n).T.copy()),
               total_energy=lambda: torch.tensor(rng.uniform(0, 1e-12, n)),
               step_count=lambda: torch.tensor(np.r_[0x7FFFFFFF, 0, rng.integers(0, 1 << 31, n - 2)].astype(np.int32)),
               rng_step=lambda: torch.tensor(np.r_[0xFFFFFFFF, 0x80000000, rng.integers(0, 1 << 32, n - 2)].astype(np.uint32).view(np.int32)),
               done=lambda: (1 - st["done"].cpu()).to(U8))[field]().cuda()
    _check(b.lib.stg_set_state(b._ctx, *_state_args({field: new}), b._stream()), b)
    post = _state(b)
    for k in STATE_KEYS:
        _same(post[k], new if k == field else st[k], (field, "->", k))
    env.close()


@gpu
def test_state_round_trip_through_a_fresh_context(stg):
    """stg_set_state of all six fields into a context that was never reset, then one step: bit for bit the original's next step."""
    env, st = _varied_env(stg)
    fresh = _make(stg, "rk4-thermal", N_STATE, "records", success_threshold=0.0, max_steps=3)
    fb = fresh.backend
    _check(fb.lib.stg_set_state(fb._ctx, *_state_args(st), fb._stream()), fb)
    _same_state(_state(fb), st, "after set_state")
    a = _actions(8, 1, N_STATE, "rk4")
    wa, wb = _plain_step_many(env, a, 1, 1), _plain_step_many(fresh, a, 1, 1)
    for k in wa:
        _same(wa[k], wb[k], k)
    _same_state(_state(env.backend), _state(fb), "after the step")
    env.close(); fresh.close()


# ------------------------------------------------------------------------------------------------
# f. solver level
# ------------------------------------------------------------------------------------------------
def _solve_inputs(n, solver, seed=31, fail_lane=False):
    """Lanes with different pulse lengths, so that trajectories inside one wavefront differ in their row counts.  RK4 (max_step 1 ps):
    every other lane T = 1e-10 s = 100 sub-steps = 101 rows, the others up to 140.  fail_lane: lane 2 gets T = 0, which the fixed-step
    solvers' input validation rejects."""
    rng = np.random.default_rng(seed)
    m0, J = _unit_rows(rng, n).T.copy(), rng.uniform(-2e6, 2e6, n)
    if solver == "rk45":
        T = rng.uniform(1.5e-11, T_RK45, n)
    else:
        T = np.where(np.arange(n) % 2 == 0, 1e-10, rng.uniform(1e-10, 1.4e-10, n))
        if fail_lane and n > 2:
            T[2] = 0.0
    return torch.tensor(m0, device="cuda"), torch.tensor(J, device="cuda"), torch.tensor(T, device="cuda")


@gpu
@pytest.mark.parametrize("base", ("rk4-thermal", "rk45-T0"))
@pytest.mark.parametrize("n", (1, 65, 130))
def test_solve_footprint(stg, n, base):
    """stg_solve: m_final [3][N], n_points and success fully written between intact guards; n_points and success may be NULL."""
    env = _make(stg, base, n, "soa")
    b = env.backend
    m0, J, T = _solve_inputs(n, BASES[base]["solver"], fail_lane=True)
    want = b.solve(m0, J, T, env_step=3)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want["m_final"]).all())
    for nulls in ((), ("n_points",), ("success",), ("n_points", "success")):
        g = {k: Guarded(k, s, d) for k, s, d in (("m_final", (3, n), F64), ("n_points", (n,), I32), ("success", (n,), U8)) if k not in nulls}
        _check(b.lib.stg_solve(b._ctx, _ptr(m0), _ptr(J), _ptr(T), 3, _gptr(g, "m_final"), _gptr(g, "n_points"), _gptr(g, "success"), b._stream()), b)
        for k in g:
            _same(g[k].check(), want[k], (k, nulls))
    if BASES[base]["solver"] == "rk4" and n > 2:
        assert int(want["success"][2]) == 0 and int(want["success"].sum()) == n - 1
    env.close()


def _traj_guards(cap, n, names, rows_max):
    """t [cap][N], m [cap][3][N], energy / torques [cap][N] with back guards that hold a whole uncapped trajectory of rows_max rows."""
    shapes = dict(t=(cap, n), m=(cap, 3, n), energy=(cap, n), torques=(cap, n))
    g = {k: Guarded(k, shapes[k], F64, min_back=rows_max * n * (3 if k == "m" else 1)) for k in names}
    for k, gd in g.items():                    # (what makes a missing `row < cap` test a failed assertion and not a fault)
        assert gd.raw.numel() - gd.front >= rows_max * n * (3 if k == "m" else 1), k
    g.update(m_final=Guarded("m_final", (3, n), F64), n_points=Guarded("n_points", (n,), I32), success=Guarded("success", (n,), U8))
    return g


def _solve_traj(b, m0, J, T, cap, g):
    _check(b.lib.stg_solve_traj(b._ctx, _ptr(m0), _ptr(J), _ptr(T), 3, int(cap), _gptr(g, "t"), _gptr(g, "m"), _gptr(g, "energy"),
                                _gptr(g, "torques"), _gptr(g, "m_final"), _gptr(g, "n_points"), _gptr(g, "success"), b._stream()), b)


def _check_traj(g, want, rec_rows, cap, what):
    """rec_rows [rows, n] bool: the rows a lane records.  Rows [0, cap) of it are written -- equal to the plain run's -- and nothing else."""
    for k in ("m_final", "n_points", "success"):
        _same(g[k].check(), want[k], (what, k))
    for k in ("t", "m", "energy", "torques"):
        if k not in g:
            continue
        wr = rec_rows[:cap]
        wr = wr[:, None, :] if k == "m" else wr
        got = g[k].check(written=wr)
        ref = want[k][:cap]
        sel = wr.expand_as(got)
        assert bool(torch.isfinite(ref[sel]).all()), (what, k)
        _same(got[sel], ref[sel], (what, k))


TRAJ = {   # configuration -> (trajectory arrays it records, extra keyword arguments)
    "rk4-thermal": (("t", "m"), {}),
    "rk45-T0": (("t", "m", "energy", "torques"), {}),
    # an attempt budget of 6: every solve but the shortest pulses' fails (success = 0) after six recorded points
    "rk45-T0-budget": (("t", "m", "energy", "torques"), dict(max_attempts=6)),
}


@gpu
@pytest.mark.parametrize("name", list(TRAJ))
@pytest.mark.parametrize("n", (1, 65, 130))
def test_solve_traj_footprint(stg, oracle_mod, n, name):
    """stg_solve_traj at traj_cap 1, 7 and beyond every lane's row count.  Lane i records rows 0 ... n_points[i] (row 0 is t0) and
    leaves the rows behind them untouched; with a small cap exactly rows [0, cap) of those are written, equal to the large-cap run's,
    nothing behind row cap - 1 is touched, and m_final, n_points and success do not change.  What a failed solve (success = 0)
    records, as the header states it: a fixed-step solve whose inputs are rejected (T = 0) records no row at all, n_points = 0; an
    RK45 solve that runs out of attempts keeps the rows of the points it accepted, n_points counts them; m_final = m0 in both."""
    names, extra = TRAJ[name]
    base = name.replace("-budget", "")
    solver = BASES[base]["solver"]
    env = _make(stg, base, n, "soa", **extra)
    b = env.backend
    m0, J, T = _solve_inputs(n, solver, fail_lane=True)
    if "budget" in name:
        T[::5] = 1e-13                                                       # (these still arrive within six attempts)
    if solver == "rk45" and "budget" not in name:
        # on the CPU: every lane has at least 8 accepted points, so that a cap of 7 cuts every trajectory
        p = oracle_mod.make_params(stt_default_params(volume=VOL_RK45))
        c = oracle_mod.make_config(solver="rk45", thermal=False)
        pts = [oracle_mod.llgs_solve(m0[:, i].cpu().numpy(), float(T[i]), p, c, float(J[i]), i, 3)["n_points"] - 1 for i in range(n)]
        assert min(pts) >= 8, min(pts)
    cap_big = 160 if solver == "rk4" else 80
    want = b.solve(m0, J, T, env_step=3, traj_cap=cap_big, want_energy="energy" in names)
    torch.cuda.synchronize()
    npts, succ = want["n_points"], want["success"]
    assert int(npts.max()) + 1 < cap_big
    recorded = (succ != 0) | (npts > 0)
    rec_rows = (torch.arange(cap_big, device="cuda")[:, None] <= npts[None, :]) & recorded[None, :]
    if solver == "rk4":
        assert bool((npts[::2][npts[::2] > 0] == 100).all()) and (n < 3 or (int(npts.max()) > 100 and int(succ[2]) == 0 and int(npts[2]) == 0))
        if n > 2:
            assert not bool(rec_rows[:, 2].any())
    elif "budget" in name:
        failed = npts[succ == 0]
        assert bool((succ[::5] == 1).all()) and (n < 2 or (failed.numel() > 0 and int(failed.min()) > 0 and int(failed.max()) <= 6))
        _same(want["m_final"][:, succ == 0], m0[:, succ == 0], "m_final of a failed solve is m0")
    else:
        assert bool((succ == 1).all()) and (n < 3 or len(torch.unique(npts)) > 2)
    for cap in (1, 7, cap_big):
        g = _traj_guards(cap, n, names, cap_big)
        _solve_traj(b, m0, J, T, cap, g)
        _check_traj(g, want, rec_rows, cap, (name, n, cap))
    if solver == "rk45":
        for part in (("energy", "torques"), ("t", "m")):                     # the other pair NULL
            g = _traj_guards(7, n, part, cap_big)
            _solve_traj(b, m0, J, T, 7, g)
            _check_traj(g, want, rec_rows, 7, (name, n, part))
    env.close()


@gpu
@pytest.mark.parametrize("n", (1, 65, 130))
def test_thermal_normals_footprint_and_call0(stg, oracle_mod, n):
    """stg_thermal_normals: [n_calls][3][N] fully written between intact guards, and a dump that starts at call0 = 3 (odd) or 4 (even)
    equals those rows of the dump from call 0: the stream is replayed from its start with the even / odd draws alternating."""
    env = _make(stg, "rk4-thermal", n, "soa")
    b = env.backend

    def dump(call0, n_calls):
        g = Guarded("z", (n_calls, 3, n), F64)
        _check(b.lib.stg_thermal_normals(b._ctx, 5, call0, n_calls, _ptr(g.interior), b._stream()), b)
        return g.check()
    z8 = dump(0, 8)
    assert bool(torch.isfinite(z8).all())
    _same(z8, b.thermal_normals(env_step=5, call0=0, n_calls=8), "dump(0, 8)")
    assert torch.unique(z8.reshape(8, -1), dim=0).shape[0] == 8               # (no two rows alike: a repeated or shifted row shows)
    z35 = dump(3, 5)
    _same(z35, z8[3:8], "dump(3, 5)")
    for i in sorted({0, n // 2, n - 1}):                                      # ... and they are the oracle's calls 3 ... 7 (its fp32-normal tolerance)
        for c in range(5):
            ref = oracle_mod.thermal_normals(env.cfg.seed, i, 5, 3 + c)
            assert np.abs(z35[c, :, i].cpu().numpy() - ref).max() < 2e-5, (i, c)
    _same(dump(4, 4), z8[4:8], "dump(4, 4)")
    _same(dump(7, 1), z8[7:8], "dump(7, 1)")
    env.close()


@gpu
@pytest.mark.parametrize("n", (1, 65, 130))
def test_device_terms_footprint(stg, n):
    """stg_device_terms on a mixed STT / SOT / VCMA table: each output alone (the others NULL) is fully written between intact guards
    and equals the all-outputs call."""
    env = _make(stg, "rk4-devphys-mixed", n, "soa")
    b = env.backend
    rng = np.random.default_rng(12)
    m = torch.tensor(_unit_rows(rng, n).T.copy(), device="cuda")
    J, volt = torch.tensor(rng.uniform(-2e6, 2e6, n), device="cuda"), torch.tensor(rng.uniform(-1.0, 1.0, n), device="cuda")
    want = dict(zip(("tau_dl", "tau_fl", "k_eff"), b.device_terms(m, J, volt)))
    torch.cuda.synchronize()
    shapes = dict(tau_dl=(3, n), tau_fl=(3, n), k_eff=(n,))
    for names in (("tau_dl",), ("tau_fl",), ("k_eff",), ("tau_dl", "tau_fl", "k_eff")):
        g = {k: Guarded(k, shapes[k], F64) for k in names}
        _check(b.lib.stg_device_terms(b._ctx, _ptr(m), _ptr(J), _ptr(volt), _gptr(g, "tau_dl"), _gptr(g, "tau_fl"), _gptr(g, "k_eff"),
                                      b._stream()), b)
        for k in names:
            assert bool(torch.isfinite(want[k]).all())
            _same(g[k].check(), want[k], (k, names))
    env.close()

"""Step launches across a SEQUENCE of launches: hipGraph replay, mixed entry points, alternating streams, several contexts
(`pytest -m gpu`).

Everything else in the suite checks what ONE launch computes.  What a launch needs from the launches before it -- scratch of the
context, cursors of the refill queue, anything the host counts and bakes into kernel arguments -- shows only when launches follow
one another in a way the host code did not count on: a captured launch replays with the arguments of the capture, whatever the host
has counted since.

Replay matrix (test_replay_equals_eager).  Per case two backends with the same configuration, parameters, start rows and R = 4
distinct action sets, copied into one static action buffer before each launch: (i) R eager calls; (ii) w warm-up launches on a side
stream, ONE captured launch, the pristine state put back with set_state, the counters reset, R replays.  w = 1 and 2: the capture
lands on either parity of anything the host alternates.  After every launch every output array is compared bit for bit (final_obs
where an episode ended: other rows keep what earlier launches left), at the end every get_state array and the counters, and
env_steps == R * n * K exactly -- the assertion that catches a launch that silently does nothing.  max_steps = 2 with auto-reset
(wherever the entry point has it) puts resets inside the four launches.

Independent anchors: the eager run against tests/helpers.py: OracleBackend on three 64-env slices (first, last, one random), flags and
m after every launch, with the tolerances of tests/test_gpu_parity.py and tests/test_gpu_fullsize.py for the solver and field of the
case (named below); and, for every case whose plan is not the plain one-env-per-lane identity launch, bit for bit against a third
backend with lane_refill, wave_spec and lane_sort all forced off.  Each case asserts the launch form it is there for through
plan_step built with the host compiler (tests/test_launch_plan.py), so a moved threshold cannot empty a case; the refill cases also
assert refill_nw * 64 < n / 2: most envs go through the queue, not through the blocks every wavefront takes statically.

The launch-order tests below the matrix are eager (except the last): mixed entry points on one refill context, steps alternating
between two ordered streams, two contexts stepped alternately while a third is created, stepped and destroyed, and replays
interleaved with eager launches.  stg_step_ids and the array env have replay tests of their own (tests/test_gpu_step_ids.py,
tests/test_gpu_array_rollout.py)."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from conftest import sot_default_params, stt_default_params, vcma_default_params
from test_launch_plan import CSRC, DEFAULTS as PLAN_DEFAULTS, DRIVER, FIELDS, PLAN

pytestmark = pytest.mark.gpu

R = 4
SLICE = 64
VOL_RK4, VOL_RK45 = 8.75e-11, 9.7e-6          # the regimes in which the current drives switching (bench.py: volume_for)
# |m_hip - m_oracle| after a step, from the tests that compare the same solver and field with the oracle:
TOL_RK4 = 1e-10            # tests/test_gpu_parity.py, tests/test_gpu_fullsize.py: the fixed-step solvers at T = 0 K
TOL_RK4_THERMAL = 1e-9     # test_thermal_on_same_philox_stream_vs_oracle, test_cfg3_rk4_thermal_65536_vs_oracle_slices (V = 8.75e-11)
TOL_RK45 = 1e-8            # tests/test_gpu_fullsize.py: RK45 with and without the thermal field (V = 9.7e-6)
TOL_OU = 1e-8              # test_ornstein_uhlenbeck_noise_model_vs_oracle (V = 1e-27, J = 0)
# tests/test_gpu_fullsize.py: _cmp_slice -- an env that auto-reset carries a row redrawn from fp32 device normals
TOL_REDRAWN, TOL_REDRAWN_STEPPED = 2e-6, 1e-3
STATE_KEYS = ("m", "target", "total_energy", "step_count", "rng_step", "done")
NO_TABLES = {"current": None, "field": None}
PLAIN = dict(lane_refill=False, wave_spec=False, lane_sort=False)


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


@pytest.fixture(scope="module")
def plan_of(tmp_path_factory):
    """cfg (EnvConfig), n, K, autoreset, per_env, ncls -> the StepPlan of a full step as a dict (csrc/stg_launch_plan.hpp on the host)"""
    d = tmp_path_factory.mktemp("launch_replay_plan")
    src, exe = str(d / "plan_driver.cpp"), str(d / "plan_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])

    def plan(cfg, n, K, autoreset, per_env, ncls):
        abi = cfg.to_abi()
        c = dict(PLAN_DEFAULTS, solver=cfg.solver, thermal=abi.thermal, temperature=abi.temperature, torque_model=abi.torque_model,
                 lane_sort=abi.lane_sort, wave_spec=abi.wave_spec, lane_refill=abi.lane_refill, skip_done=abi.skip_done, n=n, K=K,
                 autoreset=int(autoreset), ids=0, per_env=int(per_env), ncls=ncls, has_cls=int(ncls > 1))
        out = subprocess.run([exe], input=" ".join(str(c[k]) for k in FIELDS) + "\n", capture_output=True, text=True, check=True).stdout.split()
        assert out[0] == "plan", out
        return dict(zip(PLAN, map(int, out[1:])))
    return plan


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def _case(solver, n, entry="many", K=1, out_every=True, tmax=3e-10, params="one", tol=None, form=(), zero_j=False, tables=False, **cfg):
    """entry: 'many' (stg_step_many, auto-reset), 'step' (stg_step: no auto-reset), 'wave' (stg_step_wave, auto-reset).
    form: (plan field, 'set' | 'zero') pairs the case's plan must show.  cfg: EnvConfig keyword arguments."""
    return dict(solver=solver, n=n, entry=entry, K=K, out_every=out_every, tmax=tmax, params=params, tol=tol, form=tuple(form), zero_j=zero_j,
                tables=tables, cfg=dict(solver=solver, **cfg))


T0 = dict(include_thermal_fluctuations=False)
REFILL_FORM = (("refill", "set"),)
CASES = {
    "rk45-T0-refill": _case("rk45", 4226, tol=TOL_RK45, form=REFILL_FORM, lane_refill=4, **T0),
    "rk45-thermal-refill": _case("rk45", 4226, params="stt3", tol=TOL_RK45, form=REFILL_FORM + (("multi", "set"),), lane_refill=4, out_layout="records"),
    "rk45-T0-auto-refill": _case("rk45", 131073 + 130, entry="step", tmax=2e-11, tol=TOL_RK45, form=REFILL_FORM, **T0),
    "rk45-thermal-pairs": _case("rk45", 4226, tol=TOL_RK45, form=(("pc", "set"), ("hybrid", "zero"), ("refill", "zero")), wave_spec=True, lane_refill=False),
    "rk45-thermal-hybrid": _case("rk45", 65536 + 4096 + 130, tmax=6e-11, tol=TOL_RK45, form=(("hybrid", "set"),)),
    "rk4-thermal-hybrid": _case("rk4", 65536 + 4096 + 130, tmax=6e-11, tol=TOL_RK4_THERMAL, form=(("hybrid", "set"),)),
    "rk45-T0-identity": _case("rk45", 130, tol=TOL_RK45, form=(("sort", "zero"), ("pc", "zero"), ("refill", "zero")), lane_sort=False, **T0),
    "rk4-ou-classes": _case("rk4", 4226, params="ou3", tol=TOL_OU, form=(("multi", "set"),), zero_j=True, noise_model="ou", correlation_time=3e-12),
    "rk4-devphys-regroup": _case("rk4", 4226, params="dev3", tol=TOL_RK4, form=(("regroup", "set"), ("by_kind", "set"), ("multi", "set")),
                                 torque_model="device", **T0),
    "euler-per-env": _case("euler", 130, params="per-env", tol=TOL_RK4, form=(("multi", "set"),), **T0),
    "rk45-thermal-fused-every": _case("rk45", 4226, K=3, tol=TOL_RK45, form=(("pc", "set"), ("refill", "zero"))),
    "rk45-thermal-fused-last": _case("rk45", 4226, K=3, out_every=False, tol=TOL_RK45, form=(("pc", "set"), ("refill", "zero"))),
    "wave-rk45": _case("rk45", 130, entry="wave", tables=True, tol=TOL_RK45, **T0),
    "wave-rk4-thermal": _case("rk4", 130, entry="wave", tables=True, tol=TOL_RK4_THERMAL),
    "wave-none": _case("rk4", 130, entry="wave", tol=TOL_RK4, **T0),
}


def _flat(stg, d, dev="stt_mram"):
    return stg.flatten_params(stg.DeviceFactory().create_device(dev, d))


def _params(stg, kind, solver, n):
    """-> (apply(backend, s0, m): sets the parameters of envs [s0, s0 + m) on a backend of m envs, per_env, ncls)"""
    vol = VOL_RK45 if solver == "rk45" else VOL_RK4
    if kind == "per-env":
        from spin_torque_gym_amd.devices import per_env_param_block
        rng = np.random.default_rng(23)
        ov = {"damping": rng.uniform(0.005, 0.03, n), "polarization": rng.uniform(0.5, 0.8, n)}

        def apply(b, s0, m):
            if hasattr(b, "set_params_per_env"):
                assert (s0, m) == (0, n)
                b.set_params_per_env(*per_env_param_block(_flat(stg, stt_default_params(volume=vol)), n, ov))
            else:                   # the oracle: one class per env (tests/test_gpu_fullsize.py does the same)
                b.set_params([_flat(stg, stt_default_params(volume=vol, damping=float(ov["damping"][i]), polarization=float(ov["polarization"][i])))
                              for i in range(s0, s0 + m)], np.arange(m, dtype=np.uint8))
        return apply, True, 0
    if kind == "one":
        table = [_flat(stg, stt_default_params(volume=vol))]
    elif kind == "stt3":
        table = [_flat(stg, stt_default_params(volume=vol)), _flat(stg, stt_default_params(volume=vol, damping=0.02)),
                 _flat(stg, stt_default_params(volume=vol, polarization=0.6))]
    elif kind == "ou3":             # strong field: the noise is most of the dynamics (test_ornstein_uhlenbeck_noise_model_vs_oracle)
        v = 1e-27
        table = [_flat(stg, stt_default_params(volume=v)), _flat(stg, sot_default_params(polarization=0.7, volume=0.9 * v), "sot_mram"),
                 _flat(stg, vcma_default_params(polarization=0.6, volume=0.8 * v), "vcma_mram")]
    elif kind == "dev3":            # bench.py's cfg4 classes (tests/test_gpu_fullsize.py: _cfg4_kwargs)
        table = [_flat(stg, stt_default_params(volume=vol)), _flat(stg, sot_default_params(polarization=0.7, volume=vol), "sot_mram"),
                 _flat(stg, vcma_default_params(polarization=0.7, volume=vol), "vcma_mram")]
    else:
        raise ValueError(kind)
    cls = np.random.default_rng(29).integers(0, len(table), n).astype(np.uint8) if len(table) > 1 else None

    def apply(b, s0, m):
        b.set_params(table, None if cls is None else torch.as_tensor(cls[s0:s0 + m].copy()))
    return apply, False, len(table)


def _problem(case, seed, sets=R):
    """start rows [3, n], targets [3, n] and `sets` action sets [K, 2, n] (float32, on the host)"""
    n, K = case["n"], case["K"]
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (3, n))
    m0 = v / np.linalg.norm(v, axis=0, keepdims=True)
    tgt = np.zeros((3, n))
    tgt[2] = np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0)
    acts = np.empty((sets, K, 2, n), dtype=np.float32)
    acts[:, :, 0] = 0.0 if case["zero_j"] else rng.uniform(-2e6, 2e6, (sets, K, n))
    acts[:, :, 1] = rng.uniform(1e-11, case["tmax"], (sets, K, n))
    return m0, tgt, acts


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(t):
    t = t.contiguous()
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def _same(x, y, what):
    """bit for bit (floats compared as integers: -0.0 is not 0.0, and a NaN would not equal itself otherwise)"""
    assert x.shape == y.shape and x.dtype == y.dtype, (what, x.shape, y.shape, x.dtype, y.dtype)
    bad = (_bits(x) != _bits(y)).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} of {x.numel()} elements differ, first at {bad[:4].tolist()}"


def _same_outputs(x, y, what):
    """two snapshots of one launch's outputs; final_obs where an episode ended at that step (the other rows are not written)"""
    assert set(x) == set(y), (what, sorted(x), sorted(y))
    for k in x:
        if k == "final_obs":
            done = ((x["terminated"] | x["truncated"]) != 0).unsqueeze(-2).expand_as(x[k])
            _same(x[k][done], y[k][done], (what, k))
        else:
            _same(x[k], y[k], (what, k))


def _snap(out):
    torch.cuda.synchronize()
    return {k: v.contiguous().clone() for k, v in out.items() if v is not None}


def _state(b):
    torch.cuda.synchronize()
    st = {k: v.clone() for k, v in b.get_state().items()}
    torch.cuda.synchronize()                      # (a launch on another stream may follow)
    return st


def _same_end(sa, ca, sb, cb, what):
    for k in STATE_KEYS:
        _same(sa[k], sb[k], (what, "state", k))
    assert ca == cb, (what, "counters", ca, cb)


def _step_outputs(b, autoreset):
    """the arrays HipBackend.step / step_wave write (the backend's own: static, so a captured launch writes the same ones)"""
    out = dict(obs=b.obs, reward=b.reward, reward_f64=b.reward64, energy=b.energy, terminated=b.terminated, truncated=b.truncated, status=b.status)
    if autoreset:
        out["final_obs"] = b.final_obs
    return out


class _Run:
    """One backend of a case with its static input buffers: load(r) copies action set r (and its tables) into them, launch() makes the
    case's library call on the current stream and returns the arrays it writes (not copies)."""

    def __init__(self, stg, case, problem, **over):
        from spin_torque_gym_amd.backend import EnvConfig, HipBackend
        self.case, (m0, tgt, acts) = case, problem
        n, K = case["n"], case["K"]
        self.cfg = EnvConfig(**{**case["cfg"], "diagnostics": True, "max_steps": 2, "seed": 1234, **over})
        self.b = b = HipBackend(n, self.cfg)
        apply, self.per_env, self.ncls = _params(stg, case["params"], case["solver"], n)
        apply(b, 0, n)
        b.reset(None, torch.as_tensor(m0), torch.as_tensor(tgt), 5)
        self.acts = torch.as_tensor(acts, device="cuda")                     # [sets, K, 2, n]
        self.a = torch.zeros((K, 2, n), dtype=torch.float32, device="cuda")
        self.autoreset = case["entry"] != "step"
        self.wave = NO_TABLES
        if case["tables"]:
            # the rectangular pulse as a table, zero field: j(t) = the parsed J of the action up to t = T and 0 from the next double on
            # (the reference's `J if t <= T else 0`, which the last stage of an RK4 sub-step can land behind) -- the drive of stg_step
            # through the table path of the kernel, so that the oracle's rectangular step can anchor it
            self.tj, self.jk = (torch.zeros((4, n), dtype=torch.float64, device="cuda") for _ in range(2))
            th = torch.tensor([0.0, 5e-9], dtype=torch.float64, device="cuda")[:, None].expand(2, n).contiguous()
            self.wave = {"current": (self.tj, self.jk), "field": (th, torch.zeros((2, 3, n), dtype=torch.float64, device="cuda"))}
        torch.cuda.synchronize()

    def load(self, r):
        self.a.copy_(self.acts[r])
        if self.case["tables"]:
            J, T = self.a[0, 0].double(), self.a[0, 1].double()             # (inside the clips of the action parse: |J| <= 2e6, 1e-12 <= T <= 5e-9)
            self.tj.copy_(torch.stack([torch.zeros_like(T), T, torch.nextafter(T, 2 * T), 2 * T]))
            self.jk.copy_(torch.stack([J, J, torch.zeros_like(J), torch.zeros_like(J)]))

    def launch(self):
        from spin_torque_gym_amd import _lib
        b, case = self.b, self.case
        if case["entry"] == "many":
            obs, reward, reward64, term, trunc, status = b.step_many(self.a, out_every=case["out_every"], autoreset=True)
            return dict(obs=obs, reward=reward, reward_f64=reward64, energy=b.energy_many, terminated=term, truncated=trunc, status=status,
                        final_obs=b.final_obs_many)
        if case["entry"] == "wave":
            b.step_wave(self.a[0], self.wave, autoreset=True)
            return _step_outputs(b, True)
        assert not b.records_layout
        _lib.check(b.lib.stg_step(b._ctx, _ptr(self.a), 0, _ptr(b.obs), _ptr(b.reward), _ptr(b.reward64), _ptr(b.energy), _ptr(b.terminated),
                                  _ptr(b.truncated), _ptr(b.status), b._stream()))
        return _step_outputs(b, False)

    def close(self):
        self.b.close()


def _eager(run, keep=None):
    """R eager launches: (snapshots, state, counters, per-launch (m, flags) of the envs `keep` on the host for the oracle anchor)"""
    seen, rec = [], []
    for r in range(R):
        run.load(r)
        seen.append(_snap(run.launch()))
        if keep is not None:
            s = seen[-1]
            rec.append(dict(m=run.b.get_state()["m"][:, keep].cpu().numpy(),
                            **{k: s[k][..., keep].reshape(-1, keep.numel()).cpu().numpy() for k in ("terminated", "truncated", "status")}))
    return seen, _state(run.b), run.b.counters(), rec


def _graphed(run, warmups):
    st0 = _state(run.b)
    run.load(0)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(warmups):
            run.launch()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = run.launch()
    run.b.set_state(st0)
    torch.cuda.synchronize()
    run.b.counters(reset=True)
    seen = []
    for r in range(R):
        run.load(r)
        g.replay()
        seen.append(_snap(out))
    return seen, _state(run.b), run.b.counters(), (g, out)


def _oracle_slice(stg, run, problem, s0):
    """the case's R launches of envs [s0, s0 + 64) on the oracle: one dict(m [3, 64], terminated / truncated / status [K, 64]) per launch"""
    from helpers import OracleBackend
    case, (m0, tgt, acts) = run.case, problem
    sl = slice(s0, s0 + SLICE)
    o = OracleBackend(SLICE, run.cfg, env_id0=s0)
    _params(stg, case["params"], case["solver"], case["n"])[0](o, s0, SLICE)
    o.reset(None, torch.as_tensor(m0[:, sl].copy()), torch.as_tensor(tgt[:, sl].copy()), 5)
    rec = []
    for r in range(R):
        _, _, _, term, trunc, status = o.step_many(torch.as_tensor(acts[r][:, :, sl].copy()), out_every=True, autoreset=run.autoreset)
        rec.append(dict(m=o.get_state()["m"].numpy().copy(), terminated=term.numpy().copy(), truncated=trunc.numpy().copy(), status=status.numpy().copy()))
    return rec


def _anchor(run, hip, ora, cols, what):
    """tests/test_gpu_fullsize.py: _cmp_slice restricted to m and the flags, over fused launches: flags exact and m within the case's
    tolerance while an env has not been auto-reset; the launch in which it is redrawn (and not stepped again) to TOL_REDRAWN; later
    launches of an env whose row was redrawn to TOL_REDRAWN_STEPPED, its flags not at all."""
    case = run.case
    K, every = case["K"], case["out_every"]
    redrawn = np.zeros(SLICE, dtype=bool)
    worst = 0.0
    for r, (h, o) in enumerate(zip(hip, ora)):
        fresh = np.zeros(SLICE, dtype=bool)              # redrawn at the launch's LAST step: the row is the redraw itself
        for k in range(K):
            clean = ~redrawn
            if every or k == K - 1:
                j = k if every else 0
                for key in ("status", "terminated", "truncated"):
                    assert np.array_equal(h[key][j][cols][clean], o[key][k][clean]), (what, "launch", r, "step", k, key)
            done = (o["terminated"][k] | o["truncated"][k]).astype(bool)
            ended = done & clean if run.autoreset else np.zeros(SLICE, dtype=bool)
            redrawn |= ended
            fresh = ended if k == K - 1 else np.zeros(SLICE, dtype=bool)
        dm = np.abs(h["m"][:, cols] - o["m"])
        tight = ~redrawn
        worst = max(worst, dm[:, tight].max(initial=0.0))
        assert dm[:, tight].max(initial=0.0) <= case["tol"], (what, "launch", r, dm[:, tight].max())
        assert dm[:, fresh].max(initial=0.0) < TOL_REDRAWN, (what, "launch", r, dm[:, fresh].max())
        done_last = (o["terminated"][K - 1] | o["truncated"][K - 1]).astype(bool)
        loose = redrawn & ~fresh & ~(done_last & run.autoreset)
        assert dm[:, loose].max(initial=0.0) < TOL_REDRAWN_STEPPED, (what, "launch", r, dm[:, loose].max())
    return worst


def _check_form(case, run, plan_of):
    n = case["n"]
    p = plan_of(run.cfg, n, case["K"], run.autoreset, run.per_env, run.ncls)
    for field, want in case["form"]:
        assert (p[field] != 0) == (want == "set"), (field, want, p)
    if p["refill"]:
        assert p["refill_nw"] * 64 < n / 2, ("most envs must come from the refill queue, not from the static blocks", p, n)
    return p


EAGER = {}


def _eager_of(stg, name):
    """the eager run of a case, its oracle anchor and its comparison with the plain launch: computed once, shared by w = 1 and 2"""
    if name not in EAGER:
        case = CASES[name]
        n = case["n"]
        problem = _problem(case, seed=sum(map(ord, name)))
        starts = [0, int(np.random.default_rng(n).integers(1, n - SLICE)), n - SLICE]      # (at n = 130 the slices overlap)
        keep = torch.cat([torch.arange(s, s + SLICE) for s in starts]).cuda()
        run = _Run(stg, case, problem)
        seen, state, counters, rec = _eager(run, keep)
        worst = 0.0
        for j, s0 in enumerate(starts):
            worst = max(worst, _anchor(run, rec, _oracle_slice(stg, run, problem, s0), slice(j * SLICE, (j + 1) * SLICE), (name, "oracle", s0)))
        print(f"{name}: eager run against the oracle on slices {starts}: worst |dm| before a redraw = {worst:.3g}")
        EAGER[name] = (problem, run.cfg, run.autoreset, run.per_env, run.ncls, seen, state, counters)
        run.close()
    return EAGER[name]


@pytest.mark.parametrize("name", list(CASES))
def test_case_form_and_eager_run(stg, plan_of, name):
    """The launch form the case is there for (plan_step on the host); the eager run against the oracle on three slices; env_steps; and,
    unless the case IS the plain launch, the eager run bit for bit against lane_refill / wave_spec / lane_sort all forced off."""
    case = CASES[name]
    problem, cfg, autoreset, per_env, ncls, seen, state, counters = _eager_of(stg, name)
    assert counters["env_steps"] == R * case["n"] * case["K"], counters
    if case["entry"] == "wave":                                   # one kernel, identity order: no plan
        return
    from types import SimpleNamespace
    p = _check_form(case, SimpleNamespace(cfg=cfg, autoreset=autoreset, per_env=per_env, ncls=ncls), plan_of)
    if p["sort"] == 0 and p["pc"] == 0 and p["hybrid"] == 0 and p["refill"] == 0:
        return
    plain = _Run(stg, case, problem, **PLAIN)
    q = plan_of(plain.cfg, case["n"], case["K"], plain.autoreset, plain.per_env, plain.ncls)
    assert q["sort"] == 0 and q["pc"] == 0 and q["hybrid"] == 0 and q["refill"] == 0, q
    seen_p, state_p, counters_p, _ = _eager(plain)
    plain.close()
    for r in range(R):
        _same_outputs(seen[r], seen_p[r], (name, "against the plain launch", r))
    _same_end(state, counters, state_p, counters_p, (name, "against the plain launch"))


@pytest.mark.parametrize("warmups", (1, 2))
@pytest.mark.parametrize("name", list(CASES))
def test_replay_equals_eager(stg, name, warmups):
    """One captured launch replayed R times == R eager launches: every output after every launch, the state, the counters."""
    case = CASES[name]
    problem, _, _, _, _, seen, state, counters = _eager_of(stg, name)
    run = _Run(stg, case, problem)
    seen_g, state_g, counters_g, graph = _graphed(run, warmups)
    try:
        assert counters_g["env_steps"] == R * case["n"] * case["K"], (name, counters_g, "a replayed launch did not step every env")
        for r in range(R):
            _same_outputs(seen_g[r], seen[r], (name, "replay", r))
        _same_end(state_g, counters_g, state, counters, (name, "after the replays"))
    finally:
        del graph
        run.close()


# ------------------------------------------------------------------------------------------------
# launch order
# ------------------------------------------------------------------------------------------------
def _ids_inputs(n, m, seed):
    """m ids of [0, n) forming a pair-closed set (envs 2k and 2k + 1: both or neither) in random order, and their actions [2, m]"""
    rng = np.random.default_rng(seed)
    pairs = rng.permutation(n // 2)[:m // 2]
    ids = rng.permutation(np.stack([2 * pairs, 2 * pairs + 1], axis=1).reshape(-1)).astype(np.int32)
    a = np.empty((2, m), dtype=np.float32)
    a[0], a[1] = rng.uniform(-2e6, 2e6, m), rng.uniform(1e-11, 3e-10, m)
    return torch.as_tensor(ids, device="cuda"), torch.as_tensor(a, device="cuda")


def _snap_ids(out):
    return _snap({k: out[k] for k in ("obs", "reward", "reward64", "energy", "terminated", "truncated", "status")})


def test_mixed_entry_points_on_a_refill_context(stg, plan_of):
    """step, step_ids, step_many(K = 2), step, step_wave without tables, step on ONE RK45 context with forced lane refill (the full
    steps take the refill launch and its context-owned cursors; the id launch has its own in its workspace; K = 2 and the wave step take
    other kernels in between) == the same sequence on a context with lane refill and lane sort off."""
    case = CASES["rk45-T0-refill"]
    n, m = case["n"], 1500
    problem = _problem(case, seed=41, sets=6)
    ids, a_ids = _ids_inputs(n, m, 43)
    res = []
    for over in (dict(max_steps=100), dict(max_steps=100, lane_refill=False, lane_sort=False)):
        run = _Run(stg, case, problem, **over)
        b, acts = run.b, run.acts
        if not res:
            _check_form(case, run, plan_of)
        ws, out = b.ids_workspace(m), b.alloc_ids_outputs(m)
        seen = []
        b.step(acts[0, 0]); seen.append(_snap(_step_outputs(b, False)))
        b.step_ids(a_ids, ids, workspace=ws, out=out); seen.append(_snap_ids(out))
        o = b.step_many(acts[1:3, 0].contiguous(), out_every=True)
        seen.append(_snap(dict(zip(("obs", "reward", "reward_f64", "terminated", "truncated", "status"), o), energy=b.energy_many)))
        b.step(acts[3, 0]); seen.append(_snap(_step_outputs(b, False)))
        b.step_wave(acts[4, 0], NO_TABLES); seen.append(_snap(_step_outputs(b, False)))
        b.step(acts[5, 0]); seen.append(_snap(_step_outputs(b, False)))
        res.append((seen, _state(b), b.counters()))
        run.close()
    (seen, state, counters), (seen_p, state_p, counters_p) = res
    assert counters["env_steps"] == 6 * n + m
    for k, (x, y) in enumerate(zip(seen, seen_p)):
        _same_outputs(x, y, ("mixed entry points, call", k))
    _same_end(state, counters, state_p, counters_p, "mixed entry points")


STREAM_CASES = {"rk45-T0-refill": CASES["rk45-T0-refill"], "rk4-thermal-pairs": _case("rk4", 4226, wave_spec=True)}


@pytest.mark.parametrize("name", list(STREAM_CASES))
def test_steps_on_alternating_ordered_streams(stg, name):
    """Six steps that alternate between two streams, each ordered after the one before (wait_stream: the documented contract for the
    launches of one context) == six steps on one stream."""
    case = STREAM_CASES[name]
    problem = _problem(case, seed=47, sets=6)
    res = []
    for two in (False, True):
        run = _Run(stg, case, problem)
        b = run.b
        streams = [torch.cuda.Stream(), torch.cuda.Stream()] if two else [torch.cuda.current_stream()] * 2
        prev = torch.cuda.current_stream()
        seen = []
        for r in range(6):
            s = streams[r % 2]
            s.wait_stream(prev)
            with torch.cuda.stream(s):
                b.step(run.acts[r, 0], autoreset=True)
                seen.append({k: v.contiguous().clone() for k, v in _step_outputs(b, True).items()})
            prev = s
        torch.cuda.current_stream().wait_stream(prev)
        res.append((seen, _state(b), b.counters()))
        run.close()
    (seen_1, state_1, counters_1), (seen_2, state_2, counters_2) = res
    assert counters_2["env_steps"] == 6 * case["n"]
    for r in range(6):
        _same_outputs(seen_2[r], seen_1[r], (name, "two streams, step", r))
    _same_end(state_2, counters_2, state_1, counters_1, (name, "two streams"))


def test_contexts_do_not_share_launch_state(stg):
    """include/spintorque_hip.h: "Contexts are independent (no global state)".  A (RK45, lane refill) and B (RK4, thermal, wave-specialised,
    another seed and size) stepped alternately on one stream, a third refill context created, stepped and destroyed in between: A and B
    each equal their solo run."""
    case_a = CASES["rk45-T0-refill"]
    case_b = _case("rk4", 1330, wave_spec=True)
    prob_a, prob_b = _problem(case_a, seed=53), _problem(case_b, seed=59)

    def step(run, r):
        run.b.step(run.acts[r, 0], autoreset=True)
        return _snap(_step_outputs(run.b, True))

    solo = {}
    for key, case, prob, over in (("a", case_a, prob_a, {}), ("b", case_b, prob_b, dict(seed=99))):
        run = _Run(stg, case, prob, **over)
        solo[key] = ([step(run, r) for r in range(R)], _state(run.b), run.b.counters())
        run.close()
    a, b = _Run(stg, case_a, prob_a), _Run(stg, case_b, prob_b, seed=99)
    seen = {"a": [], "b": []}
    for r in range(R):
        seen["a"].append(step(a, r))
        if r == 1:
            c = _Run(stg, case_a, _problem(case_a, seed=61), seed=7)
            step(c, 0); step(c, 1)
        seen["b"].append(step(b, r))
        if r == 2:
            step(c, 2)
            c.close()
    for key, run in (("a", a), ("b", b)):
        for r in range(R):
            _same_outputs(seen[key][r], solo[key][0][r], ("context", key, "step", r))
        _same_end(_state(run.b), run.b.counters(), solo[key][1], solo[key][2], ("context", key))
        assert solo[key][2]["env_steps"] == R * run.case["n"]
        run.close()


def test_replay_interleaved_with_eager_launches(stg):
    """replay, eager step, replay, eager step_ids, replay on a refill context == the five eager calls."""
    case = CASES["rk45-T0-refill"]
    n, m = case["n"], 1500
    problem = _problem(case, seed=67, sets=5)
    ids, a_ids = _ids_inputs(n, m, 71)
    res = []
    for use_graph in (False, True):
        run = _Run(stg, case, problem)
        b = run.b
        ws, out = b.ids_workspace(m), b.alloc_ids_outputs(m, autoreset=True)
        a_static = run.acts[0, 0].clone()
        launch = lambda: b.step(a_static, autoreset=True)            # noqa: E731
        replay = launch
        if use_graph:
            st0 = _state(b)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                launch()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    launch()
            b.set_state(st0)
            torch.cuda.synchronize()
            b.counters(reset=True)
            replay = g.replay
        seen, steps = [], []                                         # (steps: env_steps after every call)
        for k, how in enumerate(("replay", "eager", "replay", "ids", "replay")):
            if how == "ids":
                b.step_ids(a_ids, ids, autoreset=True, workspace=ws, out=out)
                s_ = _snap_ids(out)
                s_["final_obs"] = out["final_obs"].contiguous().clone()
                seen.append(s_)
            else:
                a_static.copy_(run.acts[k, 0])
                (replay if how == "replay" else launch)()
                seen.append(_snap(_step_outputs(b, True)))
            steps.append(b.counters()["env_steps"])
        res.append((seen, _state(b), b.counters(), steps))
        run.close()
    (seen_e, state_e, counters_e, steps_e), (seen_g, state_g, counters_g, steps_g) = res
    assert steps_e == steps_g == [n, 2 * n, 3 * n, 3 * n + m, 4 * n + m], (steps_e, steps_g)
    for k in range(5):
        _same_outputs(seen_g[k], seen_e[k], ("interleaved, call", k))
    _same_end(state_g, counters_g, state_e, counters_e, "interleaved")

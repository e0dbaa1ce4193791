"""The RK45 attempt loop after its non-arithmetic slots were cut (`pytest -m gpu`; csrc/stg_physics.hpp: llgs_lane_gate, llgs_lane_attempt,
attempt_loop_next, batch_ready, SharedNormalsT::chunk_end_go).

Three things the shorter loop does differently, each on the smallest batch that reaches it, in all forms of the loop (producer/consumer
pairs, normals inline with four wavefronts per workgroup, lane refill) and against the oracle:

 1. min_step = 10 ulp(t) is formed only in a wavefront one of whose lanes has a step size below min_step(T) -- a wave-uniform branch that a
    healthy batch never takes.  Start rows with NaN, infinite or overflowing components poison their solve: every attempt is rejected with
    factor 0.2 until the step falls below min_step(0), about 450 attempts of which the last 430 take the branch.
 2. The pairs fetch the six thermal fields of an attempt from the LDS ring as three batches with one wait each: solves of one chunk, of two
    or three, and of many.
 3. The loop's continue condition is one scalar compare of the attempt counter against a bound: budgets of 1, 2 and 7 attempts.

Tolerances are the project's (test_gpu_fullsize.py: TOL_RK45); status and the work counters -- env steps, attempts, failed solves -- are
exact against the oracle.  The oracle's env step reports accepted points as its work, so its attempts are taken from its solver
(oracle.llgs_solve: n_attempts), run per env on the env step's own state, action and noise stream.  The per-env count of accepted points,
which env.step does not return, is compared through the solve API, which runs the same loop."""
import numpy as np
import pytest
import torch

from conftest import stt_default_params
from test_gpu_fullsize import TOL_RK45, _inputs

pytestmark = pytest.mark.gpu

KW = dict(device_params=stt_default_params(volume=9.7e-6), include_thermal_fluctuations=True, temperature=300.0, solver="rk45", seed=77,
          autoreset=False)
FORMS = {"pairs": dict(wave_spec=True, lane_refill=False), "inline": dict(wave_spec=False, lane_refill=False),
         "refill": dict(wave_spec=False, lane_refill=2)}       # (forced: lane refill takes envs per lane, 2 at the least)
# Rows no solve can integrate.  reset() refuses rows that are not finite, so those are written into the state (set_state).  The overflowing
# row is finite and goes through reset(), which divides it by its infinite norm: the env starts from the zero row, whose normalisation in
# the solver's prologue is 0 / 0 -- a NaN state like the others.  Every one of them fails (status 1) once its step is below min_step(0).
BAD_ROWS = np.array([[np.nan, 0.0, 1.0], [np.inf, 0.0, 0.0], [0.0, np.nan, np.nan], [-np.inf, np.inf, 1.0]])
OVERFLOWING = np.array([1e200, 0.0, 0.0])


@pytest.fixture(scope="module")
def stg():
    import spin_torque_gym_amd as s
    assert torch.cuda.is_available(), "these tests need the GPU"
    return s


def _run(stg, n, m0, tgt, acts, rows=None, backend=None, **kw):
    """Steps an env (the HIP backend, or the oracle) through `acts`; `rows` = (mask, [k,3]) overwrites the state rows of the masked envs
    after the reset.  Returns what each step left (cloned) and the work counters."""
    env = stg.SpinTorqueVecEnv(n, diagnostics=True, **({} if backend is None else dict(backend=backend)), **kw)
    env.reset(options={"initial_state": m0, "target_state": tgt})
    if rows is not None:
        st = env.get_state()
        mask, r = rows
        st["m"][:, torch.from_numpy(mask).to(st["m"].device)] = torch.from_numpy(r.T.copy()).to(st["m"].device)
        env.backend.set_state(st)
    rec = []
    attempts = 0
    for a in acts:
        if backend is not None:
            attempts += _oracle_attempts(env.backend, a)
        o, r, te, tr, info = env.step(torch.from_numpy(a))
        st = env.get_state()
        rec.append(dict(obs=o.t().clone(), reward=info["reward_f64"].clone(), energy=info["energy"].clone(), term=te.clone(), trunc=tr.clone(),
                        status=info["status"].clone(), m=st["m"].clone(), step_count=st["step_count"].clone()))
    counters = env.backend.counters()
    if backend is not None:
        counters["work_units"] = attempts        # (the oracle backend sums accepted points there)
    env.close()
    return rec, counters


def _oracle_attempts(b, a):
    """Attempts of the oracle's RK45 solver over the envs of oracle backend `b` for the step it is about to take with actions `a` [n,2]:
    each env's own state row, parsed action (float32 in the kernels' range, clamped to the env's limits) and stream position."""
    import oracle
    total = 0
    for i in range(b.n):
        s = b.states[i]
        J = min(max(float(np.float32(a[i, 0])), -b.cfg.max_current), b.cfg.max_current)
        T = min(max(float(np.float32(a[i, 1])), 1e-12), b.cfg.max_duration)
        r = oracle.llgs_solve(np.array([s.m[0], s.m[1], s.m[2]]), T, b.params[0], b.ocfg, J, env_id=b.env_id0 + i, env_step=int(s.rng_step),
                              cap=4)          # (cap only sizes the trajectory buffers, which are not read here)
        total += int(r["n_attempts"])
    return total


def _assert_same_bits(a, b, tag):
    """Byte for byte (a failed solve leaves its NaN row, which compares unequal to itself as a number)."""
    for k, (x, y) in enumerate(zip(a, b)):
        for key in x:
            assert torch.equal(x[key].contiguous().view(torch.uint8), y[key].contiguous().view(torch.uint8)), (tag, k, key)


def _run_hip(stg, n, m0, tgt, acts, rows=None, **kw):
    return _run(stg, n, m0, tgt, acts, rows=rows, **kw)


def _run_oracle(stg, n, m0, tgt, acts, rows=None, **kw):
    from helpers import OracleBackend
    return _run(stg, n, m0, tgt, acts, rows=rows, backend=OracleBackend, **kw)


def _cmp_oracle(hip_rec, hip_counters, ora, tag):
    """Status, flags and step counts exactly; the state within TOL_RK45 (a failed solve leaves its row, NaN included); the work counters
    -- env steps, attempts, failed solves -- exactly."""
    ora_rec, ora_counters = ora
    worst = 0.0
    for k, (h, o) in enumerate(zip(hip_rec, ora_rec)):
        for key in ("status", "term", "trunc", "step_count"):
            assert np.array_equal(h[key].cpu().numpy(), o[key].cpu().numpy()), (tag, k, key)
        hm, om = h["m"].cpu().numpy(), o["m"].cpu().numpy()
        assert np.array_equal(np.isnan(hm), np.isnan(om)), (tag, k)
        d = np.nanmax(np.abs(hm - om), initial=0.0)
        worst = max(worst, d)
        assert d <= TOL_RK45, (tag, k, d)
    print(tag, "worst |dm| vs oracle =", worst, "counters", hip_counters)
    assert hip_counters == ora_counters, (tag, hip_counters, ora_counters)


def _slow_path_inputs(n):
    """Block 1 (envs 64 ... 127): every other env starts from a row no solve can integrate, the others and the neighbouring blocks are
    ordinary.  One bad env in five keeps the state reset() made of the overflowing row; the others get a BAD_ROWS row written over it.
    Returns the inputs, the same with ordinary rows in place of the bad ones, the mask of the bad envs, and (mask, rows) for set_state."""
    healthy, tgt, acts = _inputs(n, seed=2025, steps=2, thi=3e-10)
    bad = np.zeros(n, dtype=bool)
    bad[64:128:2] = True
    m0 = healthy.copy()
    m0[bad] = OVERFLOWING
    written = bad.copy()
    written[np.flatnonzero(bad)[4::5]] = False
    rows = BAD_ROWS[np.arange(int(written.sum())) % len(BAD_ROWS)]
    return m0, healthy, tgt, acts, bad, (written, rows)


def test_min_step_branch_same_bits_in_all_forms_and_oracle(stg):
    n = 192
    m0, healthy, tgt, acts, bad, rows = _slow_path_inputs(n)
    runs = {name: _run_hip(stg, n, m0, tgt, acts, rows=rows, **KW, **form) for name, form in FORMS.items()}
    pairs, c_pairs = runs["pairs"]
    for name in ("inline", "refill"):
        _assert_same_bits(pairs, runs[name][0], ("min_step branch: pairs / " + name))
        assert runs[name][1] == c_pairs, (name, runs[name][1], c_pairs)
    # the bad envs fail (status 1, a no-op step) after several hundred attempts each, the others do not
    for rec in pairs:
        st = rec["status"].cpu().numpy()
        assert (st[bad] == 1).all() and (st[~bad] == 0).all()
    assert c_pairs["noop_steps"] == 2 * int(bad.sum()) and c_pairs["work_units"] > 2 * int(bad.sum()) * 300
    _cmp_oracle(pairs, c_pairs, _run_oracle(stg, n, m0, tgt, acts, rows=rows, **KW), "min_step branch (192 envs)")
    # lanes that share a wavefront with a failing lane: the same bits as in a batch in which no wavefront takes the branch
    clean, c_clean = _run_hip(stg, n, healthy, tgt, acts, **KW, **FORMS["pairs"])
    assert c_clean["noop_steps"] == 0
    keep = torch.from_numpy(~bad).cuda()
    for k in range(len(acts)):
        for key in pairs[k]:
            assert torch.equal(pairs[k][key][..., keep], clean[k][key][..., keep]), ("healthy lanes next to failing ones", k, key)


def test_min_step_branch_forced_refill_256(stg):
    """The lane-refill form once more with 64 ordinary envs behind the three blocks (a fourth block in the queue)."""
    n = 256
    m0, healthy, tgt, acts, bad, rows = _slow_path_inputs(n)
    refill, c_refill = _run_hip(stg, n, m0, tgt, acts, rows=rows, **KW, **FORMS["refill"])
    inline, c_inline = _run_hip(stg, n, m0, tgt, acts, rows=rows, **KW, **FORMS["inline"])
    _assert_same_bits(refill, inline, "min_step branch, 256 envs: refill / inline")
    assert c_refill == c_inline and c_refill["noop_steps"] == 2 * int(bad.sum())
    _cmp_oracle(refill, c_refill, _run_oracle(stg, n, m0, tgt, acts, rows=rows, **KW), "min_step branch (256 envs, refill)")


def test_min_step_branch_accepted_points_per_env_vs_oracle(stg):
    """Accepted points per env (and success, and the returned row) through the solve API: bad and ordinary rows side by side in one
    wavefront, thermal field on."""
    from helpers import OracleBackend
    from spin_torque_gym_amd.backend import EnvConfig, HipBackend
    n = 64
    rng = np.random.default_rng(3)
    v = rng.normal(0, 1, (n, 3))
    m0 = v / np.linalg.norm(v, axis=1, keepdims=True)
    bad = np.arange(n) % 4 == 1
    m0[bad] = BAD_ROWS[np.arange(int(bad.sum())) % len(BAD_ROWS)]
    J = rng.uniform(-2e6, 2e6, n)
    T = rng.uniform(1e-11, 6e-11, n)
    table = [stg.flatten_params(stg.DeviceFactory().create_device("stt_mram", stt_default_params(volume=9.7e-6)))]
    res = []
    for B in (HipBackend, OracleBackend):
        b = B(n, EnvConfig(diagnostics=True, solver="rk45", include_thermal_fluctuations=True, temperature=300.0, seed=5))
        b.set_params(table, None)
        out = b.solve(torch.tensor(m0.T.copy()), torch.tensor(J), torch.tensor(T))
        res.append({key: torch.as_tensor(out[key]).cpu().numpy().copy() for key in ("m_final", "n_points", "success")})
        b.close()
    h, o = res
    assert np.array_equal(h["success"], o["success"])
    assert not h["success"][bad].any() and h["success"][~bad].all()
    assert np.array_equal(h["n_points"], o["n_points"])
    assert np.allclose(h["m_final"], o["m_final"], rtol=0, atol=TOL_RK45, equal_nan=True)


def test_batched_draws_one_chunk_few_chunks_many(stg):
    """128 thermal envs, pulses of 1 ps (one attempt: one chunk behind the prologue's), 3 ps (two or three) and 1 ns (many), mixed."""
    n = 128
    m0, tgt, acts = _inputs(n, seed=808, steps=2)
    acts[..., 1] = np.array([1e-12, 3e-12, 1e-9], dtype=np.float32)[np.arange(n) % 3]
    pairs, c_pairs = _run_hip(stg, n, m0, tgt, acts, **KW, **FORMS["pairs"])
    inline, c_inline = _run_hip(stg, n, m0, tgt, acts, **KW, **FORMS["inline"])
    _assert_same_bits(pairs, inline, "batched draws: pairs / inline")
    assert c_pairs == c_inline and c_pairs["noop_steps"] == 0
    _cmp_oracle(pairs, c_pairs, _run_oracle(stg, n, m0, tgt, acts, **KW), "batched draws (128 envs, 1 ps / 3 ps / 1 ns)")


@pytest.mark.parametrize("thermal", [True, False])
@pytest.mark.parametrize("budget", [1, 2, 7])
def test_budget_exhaustion_counters_and_flags_vs_oracle(stg, thermal, budget):
    n = 64
    m0, tgt, acts = _inputs(n, seed=11 + budget, steps=2, tlo=1e-12, thi=2e-11)
    kw = dict(KW, include_thermal_fluctuations=thermal, max_attempts=budget)
    ora = _run_oracle(stg, n, m0, tgt, acts, **kw)
    forms = FORMS if thermal else {k: dict(v) for k, v in FORMS.items() if k != "pairs"}
    for name, form in forms.items():
        hip, c = _run_hip(stg, n, m0, tgt, acts, **kw, **form)
        assert c["noop_steps"] > 0              # (the budget runs out in some envs; with 7 attempts others arrive before it does)
        _cmp_oracle(hip, c, ora, f"budget {budget}, thermal {thermal}, {name}")

"""A rounding property of the RK45 step and the pairs' flag protocol, checked on the host (no GPU; csrc/stg_physics.hpp: llgs_fun, llgs_lane_attempt,
SharedNormalsT, produce_normals, llgs_solve; csrc/stg_kernels.hpp: stg_step_kernel).

1. The step that is clamped to the pulse's end.  An attempt forms t_new = fmin(fl(t + h_abs), T), h = fl(t_new - t), and tests the pulse
   gate for the one stage time that can pass T, fl(t + h) <= T.  Property: if fl(t + h_abs) < T, then the minimum is the identity and
   fl(t + fl(t_new - t)) <= T -- the gate is open.  So the clamp and the gate matter only on a solve's last step and that step's rejected
   retries.  No kernel leans on this beyond the comment above llgs_fun, which argues it (an attempt body without the clamp was built
   on it and did not fit the register file: profiles/EXPERIMENTS.md round 9); here it is tried on 1.6e7 triples in float64, random ones
   and families built to land fl(t + h_abs) within +-4 ulp of T: t = 0, h_abs = max_step, T = k * 1e-12 among them.

2. The continue flag of a producer/consumer pair.  One s_barrier per attempt, two flag copies; the integrating wavefront sets both
   copies to 1 once per solve between the env-step's H1 and H2, writes nothing inside the loop, and after a solve of n attempts writes 0
   to copy n & 1 in front of the closing barrier; the producer's round k reads copy (k - 1) & 1 behind rendezvous k and returns on 0.
   The two wavefronts and the barrier are modelled as a small state machine: both sides must pass the same number of rendezvous
   (otherwise the GPU hangs), no flag copy may be written by one side and touched by the other between the same two barriers, and the
   producer must read 1 in rounds 1 ... n and the solve's own 0 in round n + 1 -- for n = 0 ... 5, K = 1 ... 3 fused env-steps, env-steps
   in which the wavefront does not integrate (skip_done) and attempt budgets that end the loop early."""
import itertools

import numpy as np
import pytest

MAX_STEP = 1e-12          # the env default the bench rows run with is of this order; the property does not depend on it


def _gate_open_where_unclamped(t, h_abs, T):
    """Returns (number of triples with fl(t + h_abs) < T, number of those that violate the property)."""
    s = t + h_abs
    un = s < T
    t_new = np.fmin(s, T)
    h = t_new - t
    on_end = (t + h) <= T
    bad = un & ~((t_new == s) & on_end)
    return int(un.sum()), int(bad.sum())


def _near_boundary(rng, n, t, T):
    """h_abs such that fl(t + h_abs) lands within +-4 ulp of T (and a little further out through the rounding of T - t)."""
    k = rng.integers(-4, 5, n)
    target = T.copy()
    for step in range(1, 5):
        target = np.where(k >= step, np.nextafter(target, np.inf), target)
        target = np.where(k <= -step, np.nextafter(target, -np.inf), target)
    h = target - t
    j = rng.integers(-2, 3, n)               # ... and h_abs itself a few ulp around that difference
    for step in range(1, 3):
        h = np.where(j >= step, np.nextafter(h, np.inf), h)
        h = np.where(j <= -step, np.nextafter(h, -np.inf), h)
    return np.abs(h)


def test_unclamped_step_keeps_the_pulse_gate_open():
    rng = np.random.default_rng(20240)
    seen = 0
    n = 2_000_000
    # random triples: pulses of 1 ps ... 1 us, t anywhere in [0, T), steps from far below to far above what is left
    T = 10.0 ** rng.uniform(-12, -6, n)
    t = T * rng.uniform(0, 1, n)
    h = (T - t) * 10.0 ** rng.uniform(-6, 1, n)
    fam = [(t, h, T)]
    # near the boundary, T as the env makes it (a float32 widened) and T = k * 1e-12
    T32 = rng.uniform(1e-12, 1e-6, n).astype(np.float32).astype(np.float64)
    Tk = rng.integers(1, 1_000_001, n) * 1e-12
    for TT in (T32, Tk):
        tt = TT * rng.uniform(0, 1, n)
        fam.append((tt, _near_boundary(rng, n, tt, TT), TT))
        # t = 0: the first step of a solve (a one-step pulse is all clamped; just short of T it is not)
        z = np.zeros(n)
        fam.append((z, _near_boundary(rng, n, z, TT), TT))
    # h_abs = max_step, t a whole number of steps (and a few ulp off) short of T
    Tm = rng.integers(1, 1_000_001, n) * 1e-12
    tm = Tm - MAX_STEP * rng.integers(1, 4, n)
    tm = np.where(tm < 0, 0.0, tm)
    for d in range(3):
        fam.append((tm, np.full(n, MAX_STEP), Tm))
        tm = np.nextafter(tm, np.inf)
    assert len(fam) == 8
    for k, (t, h, T) in enumerate(fam):
        un, bad = _gate_open_where_unclamped(t, h, T)
        assert bad == 0, (k, bad)
        assert un > n // 20, (k, un)             # (every family has both kinds of triples)
        assert un < n, (k, un)
        seen += n
    assert seen >= 10_000_000


# ---- the flag protocol -------------------------------------------------------------------------------------------------------------

BARRIER = "barrier"


def _attempts_made(needed, budget):
    """llgs_solve: no loop if nobody is active; otherwise at least one attempt whatever the budget, and the loop goes on while
    it < (somebody active ? budget : 0)."""
    if needed == 0:
        return 0
    it = 0
    while True:
        it += 1
        active = it < needed
        if not (it < (budget if active else 0)):
            return it


def _integrator(steps, budget, log):
    """The integrating wavefront: yields BARRIER at every rendezvous and ("w", copy, value, solve) for a flag write."""
    for k, needed in enumerate(steps):
        yield BARRIER                                  # H1 (s_go / s_rng published)
        if needed is None:                             # nobody in the wavefront integrates in this env-step
            continue
        yield ("w", 0, 1, k)                           # open: both copies say 1 (one ds_write_b32, lane l writes copy l & 1)
        yield ("w", 1, 1, k)
        yield BARRIER                                  # H2
        n = _attempts_made(needed, budget)
        for _ in range(n):
            yield BARRIER                              # chunk_meet, inside the attempt; the loop writes nothing
        yield ("w", n & 1, 0, k)                       # close
        yield BARRIER                                  # the closing rendezvous
        log.append(n)


def _producer(steps, reads):
    """The producing wavefront: ("r", copy) yields come back with the value read."""
    for k, needed in enumerate(steps):
        yield BARRIER                                  # H1
        if needed is None:
            continue
        yield BARRIER                                  # H2 (chunk 0 filled)
        r = 1
        while True:
            yield BARRIER                              # rendezvous r (chunk r filled)
            v = yield ("r", (r - 1) & 1)
            reads.append((k, r, v))
            if v[0] == 0:
                break
            r += 1
            assert r < 100, "the producer never saw a 0"


def _run_pair(steps, budget, integrator=None):
    """Runs both sides interval by interval (an interval = what a side does between two of its barriers).  Returns the integrator's
    attempts per solve, the producer's reads (env-step, round, (value, solve that wrote it)) and both sides' barrier counts."""
    flags = {0: (None, None), 1: (None, None)}
    attempts, reads = [], []
    gi, gp = (integrator or _integrator)(steps, budget, attempts), _producer(steps, reads)
    bars = [0, 0]
    live = [True, True]

    def interval(gen, side, touched, pending):
        """advances `gen` to its next barrier; flag writes are buffered in `pending` (applied at the barrier, a read of the producer sees
        memory as the last barrier left it: with no copy touched by both sides in one interval that IS what it sees)"""
        send = None
        while True:
            try:
                op = gen.send(send)
            except StopIteration:
                live[side] = False
                return
            send = None
            if op == BARRIER:
                bars[side] += 1
                return
            if op[0] == "w":
                touched.add(("w", op[1]))
                pending[op[1]] = (op[2], op[3])
            else:
                touched.add(("r", op[1]))
                send = flags[op[1]]

    while live[0] or live[1]:
        ti, tp, pend = set(), set(), {}
        if live[0]:
            interval(gi, 0, ti, pend)
        if live[1]:
            interval(gp, 1, tp, {})
        # one side finished while the other still waits at a barrier: a hang on the GPU
        assert live[0] == live[1], ("one wavefront waits at a barrier the other never reaches", steps, budget, bars)
        written = {c for kind, c in ti if kind == "w"}
        assert not (written & {c for _, c in tp}), ("a flag copy is written and read between the same two barriers", steps, budget)
        flags.update(pend)
    return attempts, reads, bars


def _check(steps, budget, integrator=None):
    attempts, reads, bars = _run_pair(steps, budget, integrator)
    assert bars[0] == bars[1], (steps, budget, bars)
    solves = [(k, needed) for k, needed in enumerate(steps) if needed is not None]
    assert len(attempts) == len(solves)
    # rendezvous: H1 per env-step, and H2 + n + 1 per solve, on both sides
    assert bars[0] == len(steps) + sum(1 + n + 1 for n in attempts), (steps, budget, bars, attempts)
    for (k, needed), n in zip(solves, attempts):
        assert n == _attempts_made(needed, budget)
        mine = [(r, v) for kk, r, v in reads if kk == k]
        assert [r for r, _ in mine] == list(range(1, n + 2)), (steps, budget, k, mine)
        # rounds 1 ... n read 1, round n + 1 reads 0, and every value read was written by THIS solve
        assert [v[0] for _, v in mine] == [1] * n + [0], (steps, budget, k, mine)
        assert all(v[1] == k for _, v in mine), (steps, budget, k, mine)


def test_pair_flag_protocol_every_solve_length_and_fusion():
    """n = 0 ... 5 attempts, K = 1 ... 3 fused env-steps, env-steps in which the wavefront does not integrate, every combination."""
    lengths = [None, 0, 1, 2, 3, 4, 5]
    cases = 0
    for K in (1, 2, 3):
        for steps in itertools.product(lengths, repeat=K):
            _check(steps, budget=1 << 20)
            cases += 1
    assert cases == 7 + 49 + 343


def test_pair_flag_protocol_exhausted_attempt_budget():
    """The budget ends the loop with lanes still active (budgets 0 ... 5 against solves that would need up to 7 attempts): the loop has
    made max(1, min(needed, budget)) attempts, and the protocol only ever sees that number."""
    for budget in range(0, 6):
        for K in (1, 2, 3):
            for steps in itertools.product([None, 0, 1, 3, 7], repeat=K):
                _check(steps, budget=budget)
    assert _attempts_made(7, 0) == 1 and _attempts_made(7, 1) == 1 and _attempts_made(7, 5) == 5 and _attempts_made(3, 5) == 3


def test_the_model_catches_a_missing_close():
    """(the checker itself: without the closing 0 the producer would never leave its loop)"""
    def broken_integrator(steps, budget, log):
        for op in _integrator(steps, budget, log):
            if op != BARRIER and op[2] == 0:
                continue
            yield op

    with pytest.raises(AssertionError):
        _check((2,), 1 << 20, integrator=broken_integrator)

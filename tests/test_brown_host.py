"""noise_model='brown' (the Brown field with its 1/sqrt(dt) factor), host side (no GPU):

  * the physics of the NumPy restatement (tests/brown_ref.py) with NumPy's own generator: relaxation from a uniform start reaches
    Boltzmann's <m_z^2> within the restatement's measured discretisation bias and four standard errors, and the same schedule at the
    reference's strength (no 1/sqrt(dt)) moves nothing -- the reason the model exists;
  * plumbing: EnvConfig -> C-ABI value, refusals, the solver classes' keywords through a recording backend seam, the checkpoint's
    configuration check, switching_probability's replication and counts against a fake backend."""
import numpy as np
import pytest
import torch

import brown_ref as br
from conftest import stt_default_params

T_RELAX = 1.5e-9
N_SAMPLES = 4096


# ------------------------------------------------------------------------------------------------
# physics of the restatement
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def relaxed(oracle_mod):
    """delta -> m_z [4096] after 1.5 ns at J = 0 from a uniform start (RK4, alpha = 0.1), computed once"""
    out = {}
    for delta, (max_step, _, _) in br.EQUILIBRIUM_BIAS.items():
        p = br.physics_params(br.volume_for(delta), 0.1)
        rng = np.random.default_rng(1000 + int(delta))
        n, _ = br.substeps([T_RELAX], max_step)
        r = br.solve(br.sphere(rng, N_SAMPLES), np.full(N_SAMPLES, T_RELAX), p, br.strength(oracle_mod, p),
                     rng.standard_normal((N_SAMPLES, int(n[0]), 3)), "rk4", J=np.zeros(N_SAMPLES), max_step=max_step)
        assert r["success"].all()
        out[delta] = r["m_final"][:, 2]
    return out


def test_volumes_of_the_issue():
    assert abs(br.volume_for(2.0) - 1.386e-26) < 5e-30 and abs(br.volume_for(4.0) - 2.771e-26) < 5e-30
    assert abs(br.volume_for(20.0) - br.SWITCH["volume"]) < 5e-29


@pytest.mark.parametrize("delta", [2.0, 4.0])
def test_relaxation_reaches_boltzmann(relaxed, delta):
    max_step, b, n_bias = br.EQUILIBRIUM_BIAS[delta]
    assert abs(b) <= 0.02 and n_bias >= 65536
    mz = relaxed[delta]
    exact = br.boltzmann_mz2(delta)
    mz2, se2 = float((mz * mz).mean()), float((mz * mz).std() / np.sqrt(len(mz)))
    mz1, se1 = float(mz.mean()), float(mz.std() / np.sqrt(len(mz)))
    print(f"Delta = {delta}: <m_z^2> = {mz2:.4f} +- {se2:.4f} against {exact:.4f} (bias {b:+.4f}); <m_z> = {mz1:+.4f} +- {se1:.4f}")
    assert abs(mz2 - exact) <= abs(b) + 4 * se2
    assert abs(mz1) <= 4 * se1


def test_boltzmann_quadrature():
    """the exact value against its series at small Delta and the limits"""
    assert abs(br.boltzmann_mz2(0.0) - 1.0 / 3.0) < 1e-12
    assert abs(br.boltzmann_mz2(1e-3) - (1.0 / 3.0 + 4e-3 / 45.0)) < 1e-8              # <x^2> = 1/3 + 4 Delta / 45 + O(Delta^2)
    assert abs(br.boltzmann_mz2(4.0) - 0.7046) < 1e-4 and abs(br.boltzmann_mz2(2.0) - 0.5313) < 1e-4


def test_reference_strength_moves_nothing(oracle_mod):
    """the same schedule with the reference's strength (no 1/sqrt(dt)) from m0 = +z: every m_z stays above 0.999999"""
    p = br.physics_params(br.volume_for(4.0), 0.1)
    rng = np.random.default_rng(7)
    m0 = np.tile([0.0, 0.0, 1.0], (N_SAMPLES, 1))
    r = br.solve(m0, np.full(N_SAMPLES, T_RELAX), p, br.strength(oracle_mod, p), rng.standard_normal((N_SAMPLES, 1500, 3)), "rk4",
                 J=np.zeros(N_SAMPLES), physical=False)
    assert r["success"].all() and r["m_final"][:, 2].min() > 0.999999


def test_restatement_is_the_ou_branch_with_zero_decay(oracle_mod):
    """brown_ref.solve against a plain loop that forms (s / sqrt(dt)) xi per sub-step, on a handful of problems: bit for bit"""
    p = br.physics_params(br.volume_for(4.0), 0.1)
    s = br.strength(oracle_mod, p)
    rng = np.random.default_rng(3)
    N = 5
    T = rng.uniform(2e-11, 4e-11, N)
    n, dt = br.substeps(T)
    z = rng.standard_normal((N, int(n.max()), 3))
    m0 = br.sphere(rng, N)
    for method in ("rk4", "euler"):
        a = br.solve(m0, T, p, s, z, method, J=np.full(N, 1e-9))
        import waveform_ref
        for j in range(N):
            # the white branch with the normals repeated per stage and the strength scaled is the same field
            stages = 4 if method == "rk4" else 1
            zz = np.repeat(z[j:j + 1, :n[j]], stages, axis=1)
            b = waveform_ref.solve(m0[j:j + 1], T[j:j + 1], p, method, J=[1e-9],
                                   thermal=dict(noise="white", strength=s / np.sqrt(dt[j]), normals=zz))
            assert np.array_equal(a["m_final"][j], b["m_final"][0]) and a["n_steps"][j] == n[j]


# ------------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------------
def test_env_config_maps_brown_to_2():
    from spin_torque_gym_amd.backend import EnvConfig
    assert [EnvConfig(noise_model=m).to_abi().noise_model for m in ("white", "ou", "brown")] == [0, 1, 2]
    assert EnvConfig(solver="euler", noise_model="brown").to_abi().noise_model == 2
    with pytest.raises(ValueError, match="noise_model"):
        EnvConfig(noise_model="pink").to_abi()
    with pytest.raises(ValueError, match="fixed-step"):
        EnvConfig(solver="rk45", noise_model="brown").to_abi()


class _FakeBackend:
    """HipBackend's constructor signature and the three methods the solver classes call; solve() hands back m_final = m0 with the sign
    of m_z flipped for the problems whose index is in `flip`, and fails those in `fail`."""
    made = []
    flip, fail = (), ()

    def __init__(self, n, cfg, device_index=0, env_id0=0):
        self.n, self.cfg, self.closed, self.calls = n, cfg, False, []
        _FakeBackend.made.append(self)

    def set_params(self, table, cls=None):
        self.table = table

    def solve(self, m0, J, T, env_step=0, traj_cap=0, want_energy=False, wave=None):
        self.calls.append(dict(m0=m0.clone(), J=J.clone(), T=T.clone(), env_step=env_step, wave=wave))
        mf = m0.clone()
        succ = torch.ones(self.n, dtype=torch.uint8)
        for i in self.flip:
            mf[2, i] = -mf[2, i]
        for i in self.fail:
            succ[i] = 0
        return dict(m_final=mf, n_points=torch.zeros(self.n, dtype=torch.int32), success=succ)

    def close(self):
        self.closed = True


@pytest.fixture()
def fake():
    _FakeBackend.made, _FakeBackend.flip, _FakeBackend.fail = [], (), ()
    return _FakeBackend


def test_solver_keywords_reach_the_backend_config(fake):
    from spin_torque_gym_amd import physics as stg
    p = stt_default_params()
    for cls, kw, want in ((stg.SimpleLLGSSolver, dict(method="rk4", noise_model="brown"), ("rk4", "brown", 1e-12)),
                          (stg.RobustLLGSSolver, dict(method="euler", noise_model="ou", correlation_time=3e-12), ("euler", "ou", 3e-12)),
                          (stg.SimpleLLGSSolver, dict(method="rk4"), ("rk4", "white", 1e-12))):
        s = cls(backend=fake, **kw)
        s.solve_batch(np.array([[0.0, 0.0, 1.0]]), [0.0], [1e-10], p, thermal_noise=True)
        cfg = fake.made[-1].cfg
        assert (cfg.solver, cfg.noise_model, cfg.correlation_time) == want and cfg.include_thermal_fluctuations
        assert cfg.to_abi().noise_model == {"white": 0, "ou": 1, "brown": 2}[want[1]]
    with pytest.raises(ValueError, match="white"):
        stg.LLGSSolver(noise_model="brown", backend=fake)
    with pytest.raises(ValueError, match="white"):
        stg.LLGSSolver(noise_model="ou", backend=fake)
    stg.LLGSSolver(noise_model="white", backend=fake)


def test_switching_probability_replicates_and_counts(fake):
    from spin_torque_gym_amd import physics as stg
    G, R = 3, 5
    fake.flip = (0, 1, 2, 3, 4, 7, 14)          # condition 0: all five; condition 1: one; condition 2: one
    fake.fail = (6, 14)
    m0 = np.array([[0.0, 0.0, 1.0], [0.0, 0.6, 0.8], [1.0, 0.0, 0.0]])
    m0[2] = [0.0, 0.8, 0.6]
    J, T = np.array([1e-9, 2e-9, 3e-9]), np.array([1e-10, 2e-10, 3e-10])
    s = stg.SimpleLLGSSolver(method="rk4", noise_model="brown", backend=fake)
    out = s.switching_probability(m0, J, T, stt_default_params(), R, env_step=4)
    b = fake.made[-1]
    assert len(fake.made) == 1 and len(b.calls) == 1 and b.closed and b.n == G * R            # one launch over G R problems
    assert b.cfg.noise_model == "brown" and b.cfg.include_thermal_fluctuations
    c = b.calls[0]
    assert c["env_step"] == 4 and c["wave"] is None
    assert np.array_equal(c["m0"].numpy(), np.repeat(m0, R, axis=0).T)                       # problem g R + r is condition g
    assert np.array_equal(c["J"].numpy(), np.repeat(J, R)) and np.array_equal(c["T"].numpy(), np.repeat(T, R))
    assert set(out) == {"p_switch", "n_switched", "n_failed", "stderr"} and all(np.shape(v) == (G,) for v in out.values())
    assert out["n_switched"].tolist() == [5, 1, 1] and out["n_failed"].tolist() == [0, 1, 1]
    assert np.array_equal(out["p_switch"], np.array([1.0, 0.2, 0.2]))
    assert np.allclose(out["stderr"], np.sqrt(out["p_switch"] * (1 - out["p_switch"]) / R), rtol=0, atol=1e-16)
    assert s.solve_count == G * R
    # another target and threshold: m . (0, 1, 0) > 0.7 holds for condition 2 only (m_y = 0.8 is untouched by the flip)
    out = s.switching_probability(m0, J, T, stt_default_params(), R, target=(0.0, 1.0, 0.0), threshold=0.7)
    assert out["n_switched"].tolist() == [0, 0, 5]
    # knots: one table for all conditions and one per condition, replicated per trial along the last axis
    tk = np.array([0.0, 1e-10])
    out = s.switching_probability(m0, None, T, stt_default_params(), R, current_knots=(tk, np.array([1e-9, 0.0])),
                                  field_knots=(np.tile(tk[:, None], (1, G)), np.arange(2 * G * 3, dtype=float).reshape(2, G, 3)))
    w = fake.made[-1].calls[0]["wave"]
    assert tuple(w["current"][0].shape) == (2, G * R) and tuple(w["current"][1].shape) == (2, G * R)
    assert tuple(w["field"][0].shape) == (2, G * R) and tuple(w["field"][1].shape) == (2, 3, G * R)
    assert np.array_equal(w["field"][1][1, :, R].numpy(), np.array([12.0, 13.0, 14.0]))       # knot 1 of condition 1, trial 0
    with pytest.raises(ValueError):
        s.switching_probability(m0, J, T, stt_default_params(), 0)


def test_checkpoint_configuration_names_the_noise_model(oracle_mod):
    import spin_torque_gym_amd as stg
    from helpers import OracleBackend
    kw = dict(device_params=stt_default_params(volume=8.75e-11), include_thermal_fluctuations=True, solver="rk4", seed=3,
              backend=OracleBackend)
    env = stg.SpinTorqueVecEnv(4, noise_model="brown", **kw)
    env.reset(seed=0)
    assert env.cfg.to_abi().noise_model == 2 and env.result_config()["noise_model"] == "brown"
    st = dict(env.state_dict(), config=env.result_config())
    same = stg.SpinTorqueVecEnv(4, noise_model="brown", **kw)
    same.load_state_dict(st)
    assert torch.equal(same.state_dict()["m"], st["m"])
    for other in ("white", "ou"):
        e = stg.SpinTorqueVecEnv(4, noise_model=other, **kw)
        with pytest.raises(ValueError, match="noise_model"):
            e.load_state_dict(st)
        e.close()
    env.close(); same.close()

"""The RK45 controller's minimum step, 10 * ulp(t): the exponent form the kernels use (frexp / ldexp, csrc/stg_minstep.hpp)
against its definition through nextafter, bit for bit, on the host: t = 0, subnormals, powers of two and their neighbours, random t."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_min_step_exponent_form_equals_definition(tmp_path):
    exe = str(tmp_path / "min_step_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "spin-torque-rl-gym_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "min_step_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert int(r.stdout.strip().split()[-1]) > 4_000_000


def test_numpy_agrees_with_the_definition():
    # the definition itself against NumPy's nextafter (what SciPy evaluates, rk.py:119)
    import numpy as np
    t = np.concatenate([[0.0, 5e-324, 2.2250738585072014e-308, 1.0, 1e-9], np.random.default_rng(0).uniform(0, 5e-9, 1000)])
    ref = 10 * np.abs(np.nextafter(t, np.inf) - t)
    m, e = np.frexp(t)
    got = np.where(t == 0, np.ldexp(10 * 2.0 ** -53, -1021), np.ldexp(10 * 2.0 ** -53, np.maximum(e, -1021)))
    assert np.array_equal(ref.view(np.uint64), got.view(np.uint64))

"""Which launch form a step takes, pinned on the CPU.

Results never depend on the schedule (every bit-for-bit test passes whatever the plan is), so a threshold that moves shows up only as
speed.  csrc/stg_launch_plan.hpp is plain C++: a small driver built with the host compiler evaluates `plan_step` for the cases below.
The expected values are written out here from the documented thresholds (65 536 envs = one wavefront per SIMD; hybrid launch with
2048 - nblk pairs down to 512 (RK45) / 640 (RK4); automatic lane refill from 98 305 envs with the thermal field, 131 073 without,
1024 wavefronts up to 8 envs per lane and 2048 beyond, a refill point every 32 / 16 attempts), with nblk = ceil(n / 4096) * 64.
"""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "spin-torque-rl-gym_amd", "csrc")
FIELDS = ("solver", "thermal", "temperature", "torque_model", "lane_sort", "wave_spec", "lane_refill", "skip_done",
          "n", "K", "autoreset", "ids", "per_env", "ncls", "has_cls")
DEFAULTS = dict(solver="rk45", thermal=1, temperature=300.0, torque_model=0, lane_sort=0, wave_spec=0, lane_refill=0, skip_done=0,
                n=4096, K=1, autoreset=0, ids=0, per_env=0, ncls=1, has_cls=0)
PLAN = ("sort", "by_kind", "regroup", "skip_done", "thermal", "multi", "devphys", "pc", "hybrid", "refill", "refill_check", "refill_nw")

DRIVER = r"""
#include "stg_launch_plan.hpp"
#include <cstdio>
#include <cstring>
int main() {
    char solver[16];
    stg_config c;
    long long n;
    int K, autoreset, ids, per_env, ncls, has_cls;
    for (;;) {
        std::memset(&c, 0, sizeof c);
        if (std::scanf("%15s %d %lf %d %d %d %d %d %lld %d %d %d %d %d %d", solver, &c.thermal, &c.temperature, &c.torque_model, &c.lane_sort,
                       &c.wave_spec, &c.lane_refill, &c.skip_done, &n, &K, &autoreset, &ids, &per_env, &ncls, &has_cls) != 15) break;
        c.solver = !std::strcmp(solver, "rk4") ? STG_SOLVER_RK4 : (!std::strcmp(solver, "euler") ? STG_SOLVER_EULER : STG_SOLVER_RK45);
        StepPlan p{};
        const char* err = "";
        const int rc = plan_step(c, n, K, autoreset != 0, ids != 0, per_env != 0, ncls, has_cls != 0, &p, &err);
        if (rc != STG_OK) std::printf("error %d %s\n", rc == STG_E_INVALID ? 1 : 0, err);
        else std::printf("plan %d %d %d %d %d %d %d %d %d %d %d %d\n", p.sort, p.by_kind, p.regroup, p.skip_done, p.thermal, p.multi, p.devphys, p.pc,
                         p.hybrid, p.refill, p.refill_check, p.refill_nw);
    }
    return 0;
}
"""

NO_REFILL = dict(refill=0, refill_check=32, refill_nw=0)
RK4 = dict(solver="rk4")
DEV3 = dict(solver="rk4", torque_model=1, ncls=3)

# (case, expected subset of the plan) -- or (case, error message)
CASES = [
    # one wavefront: nothing to sort, whatever the solver
    (dict(n=64), dict(sort=0, pc=1, hybrid=0, **NO_REFILL)),
    (dict(RK4, n=64), dict(sort=0)),
    (dict(solver="euler", n=64), dict(sort=0)),
    (dict(n=65), dict(sort=1)),
    # RK45 + thermal: wave-specialised up to 65 536 envs, hybrid to 98 304 (nblk 1088 -> 960 pairs, 1536 -> 512), then lane refill
    (dict(n=65536), dict(sort=1, thermal=1, multi=0, devphys=0, pc=1, hybrid=0, **NO_REFILL)),
    (dict(n=65537), dict(sort=1, pc=1, hybrid=960 + 1, **NO_REFILL)),
    (dict(n=98304), dict(sort=1, pc=1, hybrid=512 + 1, **NO_REFILL)),
    (dict(n=98305), dict(sort=1, pc=0, hybrid=0, refill=2, refill_nw=1024, refill_check=32)),
    (dict(n=524288), dict(pc=0, hybrid=0, refill=8, refill_nw=1024, refill_check=32)),
    (dict(n=524289), dict(pc=0, hybrid=0, refill=5, refill_nw=2048, refill_check=16)),
    # RK45 at T = 0 K (cfg.thermal = 0): no producer kernel, refill from 131 073 envs (nblk 2112 -> 3 per lane)
    (dict(thermal=0, n=65536), dict(sort=1, thermal=0, pc=0, hybrid=0, **NO_REFILL)),
    (dict(thermal=0, n=131072), dict(sort=1, thermal=0, pc=0, hybrid=0, **NO_REFILL)),
    (dict(thermal=0, n=131073), dict(thermal=0, pc=0, hybrid=0, refill=3, refill_nw=1024, refill_check=32)),
    # RK45 draws its field whenever cfg.thermal is set, the fixed-step solvers only at temperature > 0
    (dict(temperature=0.0, n=4096), dict(thermal=1, pc=1)),
    (dict(RK4, temperature=0.0, n=4096), dict(thermal=0, pc=0)),
    (dict(RK4, n=4096), dict(thermal=1, pc=1, hybrid=0, **NO_REFILL)),
    # RK4 + thermal: hybrid down to 640 pairs (90 112 envs: nblk 1408), never a refill launch
    (dict(RK4, n=90112), dict(pc=1, hybrid=640 + 1, **NO_REFILL)),
    (dict(RK4, n=90113), dict(pc=0, hybrid=0, **NO_REFILL)),
    (dict(RK4, n=200000), dict(pc=0, hybrid=0, **NO_REFILL)),
    (dict(solver="euler", n=80000), dict(pc=0, hybrid=0, **NO_REFILL)),
    (dict(RK4, torque_model=1, n=80000), dict(devphys=1, pc=0, hybrid=0)),
    (dict(RK4, torque_model=1, n=4096), dict(devphys=1, thermal=1, pc=0)),
    # what switches the refill launch off: fused steps, a forced wave_spec, lane_refill = -1; and the forced form
    (dict(n=200000), dict(pc=0, hybrid=0, refill=4, refill_nw=1024, refill_check=32)),
    (dict(n=200000, K=2), dict(pc=0, hybrid=0, **NO_REFILL)),
    (dict(n=200000, wave_spec=1), dict(pc=1, hybrid=0, **NO_REFILL)),
    (dict(n=200000, wave_spec=-1), dict(pc=0, refill=4, refill_nw=1024, refill_check=32)),
    (dict(n=200000, lane_refill=-1), dict(pc=0, hybrid=0, **NO_REFILL)),
    (dict(n=200000, lane_refill=4), dict(refill=4, refill_nw=784, refill_check=32)),       # ceil(3136 / 4)
    # the hybrid launch needs the sorted schedule and the automatic wave_spec; the refill launch does not need the sort
    (dict(n=70000), dict(sort=1, pc=1, hybrid=896 + 1, **NO_REFILL)),
    (dict(n=70000, lane_sort=-1), dict(sort=0, pc=0, hybrid=0, **NO_REFILL)),
    (dict(n=70000, wave_spec=-1), dict(pc=0, hybrid=0)),
    (dict(n=200000, lane_sort=-1), dict(sort=0, refill=4, refill_nw=1024, refill_check=32)),
    # id launches: no hybrid launch, everything else as the full step
    (dict(n=70000, ids=1), dict(sort=1, pc=0, hybrid=0, **NO_REFILL)),
    (dict(n=65536, ids=1), dict(sort=1, pc=1, hybrid=0, **NO_REFILL)),
    (dict(n=200000, ids=1), dict(sort=1, pc=0, hybrid=0, refill=4, refill_nw=1024, refill_check=32)),
    (dict(RK4, n=80000, ids=1), dict(pc=0, hybrid=0)),
    # per-env parameter records: neither hybrid nor refill
    (dict(n=200000, per_env=1, ncls=0), dict(multi=2, pc=0, hybrid=0, **NO_REFILL)),
    (dict(n=70000, per_env=1, ncls=0), dict(multi=2, pc=0, hybrid=0, **NO_REFILL)),
    (dict(n=4096, per_env=1, ncls=0), dict(multi=2, pc=1)),
    # the plan kernel's grouping by device kind (device-physics model only)
    (dict(DEV3, has_cls=1), dict(sort=1, multi=1, by_kind=1, regroup=1)),
    (dict(DEV3, ncls=0, per_env=1), dict(sort=1, multi=2, by_kind=1, regroup=0)),
    (dict(RK4, ncls=3, has_cls=1), dict(multi=1, by_kind=0, regroup=0)),
    (dict(RK4, torque_model=1), dict(multi=0, by_kind=0, regroup=0)),
    # finished envs sort last only when the launch does not reset them
    (dict(skip_done=1, autoreset=0), dict(sort=1, skip_done=1)),
    (dict(skip_done=1, autoreset=1), dict(sort=1, skip_done=0)),
    (dict(skip_done=0, autoreset=0), dict(skip_done=0)),
    # the two errors that belong to the decision
    (dict(n=1 << 32), "lane sort supports up to 2^32 envs per context"),
    (dict(n=(1 << 32) - 1), dict(sort=1)),
    (dict(n=1 << 39, lane_sort=-1, lane_refill=2), "lane refill: too many wavefronts"),
]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_plan")
    src, exe = str(d / "plan_driver.cpp"), str(d / "plan_driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe])
    lines = []
    for case, _ in CASES:
        assert set(case) <= set(FIELDS), case
        c = dict(DEFAULTS, **case)
        lines.append(" ".join(str(c[k]) for k in FIELDS))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(CASES), out
    return out


@pytest.mark.parametrize("k", range(len(CASES)), ids=lambda k: "-".join(f"{a}={b}" for a, b in CASES[k][0].items()))
def test_plan(plans, k):
    case, want = CASES[k]
    words = plans[k].split(" ", 2)
    if isinstance(want, str):
        assert words[0] == "error" and words[1] == "1" and words[2] == want, (case, plans[k])   # STG_E_INVALID with the message
        return
    assert words[0] == "plan", (case, plans[k])
    got = dict(zip(PLAN, map(int, plans[k].split()[1:])))
    assert set(want) <= set(PLAN)
    assert {f: got[f] for f in want} == want, (case, got)


def test_header_is_plain_cpp():
    """stg_launch_plan.hpp depends on the public header and <cstdint> only, and no schedule constant is defined anywhere else."""
    import re
    text = open(os.path.join(CSRC, "stg_launch_plan.hpp")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["../../include/spintorque_hip.h", "cstdint"]
    for name in ("STG_WAVE_SPEC_MAX_ENVS", "STG_REFILL_AUTO_ENVS", "STG_REFILL_AUTO_ENVS_THERMAL", "STG_REFILL_CHECK_DEFAULT", "TILE_ENVS", "TILE_WAVES"):
        defs = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp"))
                and re.search(r"constexpr\s+\w+\s+(?:\w+\s*=[^;]*,\s*)*" + name + r"\s*=", open(os.path.join(CSRC, f)).read())]
        assert defs == ["stg_launch_plan.hpp"], (name, defs)

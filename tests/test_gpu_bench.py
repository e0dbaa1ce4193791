"""bench.py's plain run on the GPU (`pytest -m gpu`): ONE block of exactly --steps timed steps, the headline keys of the result
line, and --dump-outputs writing the last timed step's outputs -- the same bits from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}


@pytest.mark.timeout(600)
def test_plain_run_times_steps_and_dumps_the_same_outputs_twice(tmp_path):
    n, steps = 4096, 3
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                            "--envs-per-gpu", str(n), "--dump-outputs", str(d)], cwd=ROOT, env=CLEAN, capture_output=True, text=True,
                           timeout=280)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["metric"] == "env_steps_per_sec" and line["unit"] == "env-steps/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f64" and line["steps"] == steps and line["warmup"] == 1
        assert line["blocks_timed"] == 1 and len(line["block_walls_ms"]) == 1
        assert line["ms_per_step"] == pytest.approx(line["block_walls_ms"][0] / steps, rel=1e-3)
        assert line["value"] == pytest.approx(n * 1e3 / line["ms_per_step"], rel=1e-3)
        assert line["cpu_baseline"] is None and line["api_ms_per_step"] is None and "also" not in line
        files = sorted(os.listdir(d))
        assert files == ["final_obs.npy", "obs.npy", "reward.npy", "status.npy", "terminated.npy", "truncated.npy"], files
        out = {f[:-4]: np.load(d / f) for f in files}
        assert all(a.dtype == np.float32 and a.shape[0] == n for a in out.values())
        assert out["obs"].shape == (n, 12) and out["final_obs"].shape == (n, 12)
        assert np.all(np.isfinite(out["obs"])) and np.all(np.isfinite(out["reward"]))
        assert np.abs(np.linalg.norm(out["obs"][:, :3].astype(np.float64), axis=1) - 1).max() < 1e-5      # obs[0:3] = m, a unit vector
        assert set(np.unique(out["terminated"])) <= {0.0, 1.0} and set(np.unique(out["truncated"])) <= {0.0, 1.0}
        runs.append(out)
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k

"""bench.py on the device: a plain run times exactly --steps steps and reports only the headline figure (the measurements
beside it are behind --full); --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_bench_plain_run_dumps_the_last_timed_step(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--batch", "4", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(out)], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["unit"] == "images/s"
    assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    assert "cpu_baseline" not in d and "fp32_mfma_only" not in d and "families" not in d["roofline"]
    names = sorted(os.listdir(out))
    assert names == ["loss.npy"] + [f"output_{k}.npy" for k in range(5)] + ["state.npy"]
    a = {n: np.load(out / n) for n in names}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert float(a["loss.npy"]) == d["config"]["final_loss"]
    assert all(a[f"output_{k}.npy"].shape[:2] == (4, 2) for k in range(5))
    assert sum(os.path.getsize(out / n) for n in names) <= 64 << 20

"""GPU: bench.py's command line.  A plain run measures the headline window only; --full adds the runs that moved behind
it; --dump-outputs writes what the last timed step computed, identically from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_and_full_runs_dump_the_same_outputs(dev, tmp_path):
    plain = _bench("--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / "plain"))
    assert plain["steps"] == 3 and plain["warmup"] == 2 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["higher_is_better"] is True and plain["unit"] == "rays/s" and plain["dtype"]
    assert plain["value_fp32_arithmetic"] is None and plain["breakdown_ms"] == {}
    assert plain["quality"] is None and plain["secondary"] is None and plain["cpu_baseline"] is None
    full = _bench("--steps", "3", "--warmup", "2", "--full", "--no-quality", "--no-cpu-baseline",
                  "--dump-outputs", str(tmp_path / "full"))
    assert full["value_fp32_arithmetic"] > 0 and full["breakdown_ms"]
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full"))
    assert {"rgb_loss.npy", "semantics_loss.npy", "interlevel_loss.npy", "parameters_sample.npy"} <= set(names)
    assert sum(os.path.getsize(tmp_path / "plain" / f) for f in names) <= 64 << 20
    for f in names:
        a, b = np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)
        assert a.dtype == np.float32 and np.all(np.isfinite(a)), f
        assert np.array_equal(a, b), f"{f} differs between two runs with the same inputs"

"""bench.py's single-GPU line end to end: a plain run prints the headline line only and times
exactly --steps steps, --dump-outputs writes the last step's [D] direction, the same from run to
run, and --full adds the roofline block to the same line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 8, 100_003
SHAPE = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--clients", str(N), "--dim", str(D)]
PLAIN_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus",
              "config", "build_id"}


def _bench(args, timeout=200):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), p.stderr


def test_plain_run_is_lean_and_its_dump_repeats(tmp_path):
    outs = []
    for run in ("a", "b"):
        line, err = _bench(SHAPE + ["--step-times", "--dump-outputs", str(tmp_path / run)])
        assert PLAIN_KEYS <= set(line) and line["steps"] == 2 and line["ms_per_step"] > 0
        assert not {"roofline", "cpu_baseline", "strong_c4", "multi_gpu"} & set(line)
        # --steps sets the number of timed steps: one HIP-event interval per step
        steps = [json.loads(l) for l in err.splitlines() if l.startswith('{"step_ms"')]
        assert len(steps) == 1 and len(steps[0]["step_ms"]) == 2
        assert os.listdir(tmp_path / run) == ["direction.npy"]
        outs.append(np.load(tmp_path / run / "direction.npy"))
    assert outs[0].dtype == np.float32 and outs[0].shape == (D,)
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    # topk:1% of N rows: at most N K coordinates are nonzero, and some are
    k = line["config"]["K"]
    assert 0 < np.count_nonzero(outs[0]) <= N * k


def test_full_run_adds_the_roofline_block():
    line, _ = _bench(SHAPE + ["--full", "--no-cpu-baseline"])
    assert PLAIN_KEYS <= set(line)
    roof = line["roofline"]
    assert roof["kernel"] and roof["launches"] > 0 and roof["read_ceiling"]["rows"] == N
    assert "cpu_baseline" in line and line["cpu_baseline"] is None

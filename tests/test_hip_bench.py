"""bench.py as a plain run and with --full, end to end on the GPU (small batch and resolution)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"roofline", "families", "loop", "validation", "yv5m", "cpu_baseline"}


def _bench(*args, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--batch", "8", "--size", "320", *args], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_only(tmp_path):
    """Without --full the run sets up, warms up, times the steps, dumps the outputs and prints the line: the headline
    fields are there, nothing that needs runs of its own (family table, roofline, loop / validation / yv5m legs, CPU
    baseline) is."""
    d = _bench("--dump-outputs", str(tmp_path))
    assert HEADLINE <= set(d) and not FULL_ONLY & set(d), sorted(d)
    assert d["metric"] == "images/sec YOLOv5s 320px train" and d["unit"] == "images/sec" and d["dtype"] == "bf16"
    assert d["higher_is_better"] is True and d["config"]["launch"] == "hipGraph replay"
    assert abs(d["value"] - 8 * 3 / (3 * d["ms_per_step"] * 1e-3)) < 0.02 * d["value"]
    assert np.isfinite(d["final_loss"]) and d["step_roofline"]["frac"] > 0
    got = {f[:-4] for f in os.listdir(tmp_path)}
    assert got == {"loss_total", "loss_parts", "bn_buffers", "params", "grads"}, got
    assert np.load(tmp_path / "loss_total.npy").tolist() == [d["final_loss"]]


def test_full_run_adds_the_family_table_and_legs():
    """--full keeps the headline and adds the per-family table with its roofline and the training-loop leg (the
    validation / yv5m legs and the CPU baseline left out here: --no-extra, --no-cpu-baseline)."""
    d = _bench("--full", "--no-extra", "--no-cpu-baseline", "--loop-steps", "3")
    assert HEADLINE <= set(d) and {"roofline", "families", "loop"} <= set(d), sorted(d)
    assert not {"validation", "yv5m", "cpu_baseline"} & set(d), sorted(d)
    assert abs(sum(f["share_of_step"] for f in d["families"]) - 1.0) < 0.02
    assert d["roofline"]["family"] == d["families"][0]["family"]
    assert d["loop"]["value"] > 0, d["loop"]

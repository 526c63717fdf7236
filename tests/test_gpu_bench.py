"""bench.py as a plain run: the headline line alone; what --full adds stays out of it."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(*args):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], cwd=REPO, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _headline(line, steps, warmup):
    assert line["steps"] == steps and line["warmup"] == warmup and line["full"] is False
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and line["ms_per_step"] > 0


def test_plain_run_prints_the_headline_alone():
    line = _line("--gpus", "1", "--steps", "20", "--warmup", "5")
    _headline(line, 20, 5)
    assert line["unit"] == "edge-messages/s"
    assert line["value"] == pytest.approx(4.0 * line["config"]["edges_per_gpu"] / (line["ms_per_step"] * 1e-3))
    for k in ("roofline", "roofline_other", "rollout", "train", "cpu_baseline", "ms_per_step_repeats"):
        assert line[k] is None, k
    assert line["kernels"] == {} and "other_configs" not in line


def test_plain_seq2seq_run_prints_the_headline_alone():
    line = _line("--seq2seq", "--steps", "10", "--warmup", "2")
    _headline(line, 10, 2)
    assert line["unit"] == "edge-steps/s"
    for k in ("roofline", "four_entry_points_ms_per_step", "cpu_baseline"):
        assert line[k] is None, k

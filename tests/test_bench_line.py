"""bench.py's two lines: a plain run prints the headline figure alone (set-up, warm-up, the timed steps, --dump-outputs, the
line); --full adds the oracle's checks, the CPU baseline and the legs that take launches of their own -- after the same timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _line(*extra, env=None):
    cmd = [sys.executable, BENCH, "--sources", "16", "--frames", "65536", "--steps", "3", "--warmup", "1", *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines  # ONE JSON line on stdout
    return json.loads(lines[0])


def test_full_is_an_option():
    r = subprocess.run([sys.executable, BENCH, "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout, r.stderr[-2000:]


@pytest.mark.gpu
def test_plain_line_is_the_headline_alone(tmp_path):
    d = _line("--dump-outputs", str(tmp_path))
    assert all(k in d for k in HEADLINE), d.keys()
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert not {"cpu_baseline", "parity", "multi_gpu"} & d.keys(), d.keys()
    rf = d["roofline"]
    assert rf["kernel_ms"] > 0 and rf["traffic"] is None and not {"per_source", "per_class", "side"} & rf.keys(), rf.keys()
    assert d["config"]["geometry"].get("autotuned") is True
    mix = np.load(tmp_path / "mix.npy")
    assert mix.size == d["config"]["out_frames"] * 2 and np.isfinite(mix).all()


@pytest.mark.gpu
def test_full_line_adds_the_checks_after_the_same_steps(tmp_path):
    plain, full = tmp_path / "plain", tmp_path / "full"
    # (the cost model's geometry in both: the same launches, so the same bits whatever an autotune would pick on the day)
    p = _line("--no-autotune", "--dump-outputs", str(plain))
    f = _line("--no-autotune", "--full", "--no-side", "--dump-outputs", str(full), env={"RH_BENCH_NO_PMC": "1"})
    assert all(k in f for k in HEADLINE) and f["metric"] == p["metric"] and f["unit"] == p["unit"] and f["dtype"] == p["dtype"]
    assert np.array_equal(np.load(plain / "mix.npy").view(np.uint32), np.load(full / "mix.npy").view(np.uint32))
    assert f["parity"]["ok"] and f["parity"]["frames_compared"] == f["config"]["out_frames"] and "unscaled" in f["parity"]
    assert f["cpu_baseline"]["kind"] == "port" and f["cpu_baseline"]["value"] > 0
    rf = f["roofline"]
    assert "disabled" in str(rf["traffic_detail"])  # the counter passes are --full's (switched off here)
    assert rf["per_source"]["parity"]["ok"] and rf["per_class"]["parity"]["ok"]

"""bench.py as a command: a plain run prints the headline line and does nothing reported next to it (c2, c5); --full adds those
figures (here: the frame checksums against tests/golden, the rest switched off to keep the test short)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _line(*args):
    out = subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0]), out.stderr


def test_bench_offers_full():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--full" in out.stdout, out.stderr


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone(gpu, tmp_path):
    d, err = _line("--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert d["unit"] == "iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(d["config"]["counted_iterations_per_step"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert d["roofline"]["launches_timed"] == 2 and d["roofline"]["traffic"] is None
    assert d["parity"] is None and d["sustained"] is None
    assert "cpu_baseline" not in d and "pipelined" not in d
    assert "[parity]" not in err and "PMC" not in err
    assert sorted(d["dumped_outputs"]["arrays"]) == ["count", "max", "pixel_index", "rgba16", "steps", "zbuf"]
    assert all((tmp_path / f"{name}.npy").exists() for name in d["dumped_outputs"]["arrays"])


@pytest.mark.gpu
def test_plain_c5_run_is_the_read_back_sweep_alone(gpu):
    d, _ = _line("--config", "c5", "--steps", "16", "--warmup", "16")
    assert d["steps"] == 16 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["rgba16_in_hbm"] is None and d["cold_sweep"] is None and d["parity"] is None
    json.loads(json.dumps(d), parse_constant=lambda c: pytest.fail(f"{c} in the line"))   # strict JSON: no NaN anywhere


@pytest.mark.gpu
def test_full_run_checks_the_frame_against_the_golden(gpu):
    d, _ = _line("--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-traffic",
                 "--no-pipeline", "--sustained-seconds", "0")
    assert d["parity"]["result"] == "equal", d["parity"]
    assert d["steps"] == 2 and d["value"] > 0

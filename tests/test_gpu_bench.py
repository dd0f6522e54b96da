"""bench.py without --full: the headline line alone, its outputs, and little time outside the timed steps."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

# what only --full measures or checks
FULL_ONLY_KEYS = ("c4", "value_host_to_host", "precision_ladder", "reg_sweep", "exact_emd", "c5_cellw2", "e2e_tl_s", "prepass",
                  "cpu_baseline", "cpu_baseline_equal_updates", "cpu_baseline_all_cores", "equal_work_note", "parity")


def test_plain_run_prints_the_headline_alone(tmp_path):
    steps, warmup = 5, 2
    t = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[:500]
    line = json.loads(lines[0])
    assert line["metric"] == "W2 patient-pairs/sec (full NxN EMD matrix)" and line["unit"] == "pairs/s"
    assert line["higher_is_better"] is True and line["steps"] == steps and line["warmup"] == warmup
    assert line["value"] == pytest.approx(600 * 600 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert line["roofline"]["kernel_ms"] > 0 and line["dtype"]
    assert not set(FULL_ONLY_KEYS) & set(line), sorted(set(FULL_ONLY_KEYS) & set(line))
    E = np.load(tmp_path / "emd.npy")
    assert E.shape == (600, 600) and np.isfinite(E).all()
    assert wall - (steps + warmup) * line["ms_per_step"] * 1e-3 < 30.0

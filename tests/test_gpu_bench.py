"""bench.py's plain run (no --full) and --dump-outputs: the result line's contract fields, and the dumped keys equal the
oracle's sort of the last timed step's input (batch W + K - 1: splitmix64 seed W + K)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_steps_output(tmp_path):
    K, W, log2n = 3, 1, 20
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
                          "--log2n", str(log2n), "--dump-outputs", str(tmp_path / "dump")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == K and line["warmup"] == W and line["unit"] == "Gkeys/s" and line["dtype"] == "u32"
    assert line["higher_is_better"] is True and line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - (1 << log2n) / (line["ms_per_step"] * 1e-3) / 1e9) < 1e-6 * line["value"]
    assert "cpu_baseline" not in line and line["kernels"]["lsd_only_ms_per_step"] is None      # (--full only)
    assert os.listdir(str(tmp_path / "dump")) == ["sorted_keys.npy"]
    got = np.load(str(tmp_path / "dump" / "sorted_keys.npy"))
    assert got.dtype == np.float64 and got.shape == (1 << log2n,)
    want = np.sort(ol.splitmix_fill(1 << log2n, ol.U32, 1 + (W + K - 1))).astype(np.float64)
    assert np.array_equal(got, want)

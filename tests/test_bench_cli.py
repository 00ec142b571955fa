"""bench.py command line: the result line and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_the_dataset(tmp_path):
    out_dir = tmp_path / "dump"
    proc = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1", "--path", "client",
         "--files", "3", "--file-size", str((1 << 20) + 4097),
         "--block-size", str(1 << 20), "--read-chunk", str(256 << 10),
         "--threads", "2", "--hbm-gb", "1",
         "--dump-outputs", str(out_dir)],
        capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert proc.returncode == 0, proc.stderr[-2000:]
    result = json.loads(proc.stdout.strip().splitlines()[-1])
    assert result["steps"] == 2 and result["warmup"] == 1
    assert result["ms_per_step"] > 0
    for key in ("metric", "value", "unit", "higher_is_better", "dtype"):
        assert key in result

    assert os.listdir(out_dir) == ["seqread_r0.npy"]
    rows = np.load(out_dir / "seqread_r0.npy")
    assert rows.dtype == np.float32 and rows.shape == (12, 64 << 10)
    # rank 0's files repeat one seeded 8 MiB pattern from offset 0, so every
    # sampled extent is a contiguous slice of that pattern
    base = np.random.default_rng(1234).integers(
        0, 256, size=8 << 20, dtype=np.uint8).tobytes()
    for row in rows:
        assert base.find(row.astype(np.uint8).tobytes()) >= 0

"""GPU: what a plain `bench.py` run does - the headline workload's timed steps, its outputs and the result line, nothing
that only `--full` measures or checks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_headline_steps_only(gpu, tmp_path):
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    stdout_lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(stdout_lines) == 1 and len(stdout_lines[0]) < 4096
    short = json.loads(stdout_lines[0])
    assert short["metric"] == "dcrt_ring_ops_per_s" and short["unit"] == "ring-ops/s" and short["higher_is_better"] is True
    assert short["dtype"] == "u32" and short["steps"] == 3 and short["warmup"] == 1
    assert short["value"] > 0 and short["ms_per_step"] > 0
    assert short["value"] == pytest.approx(3600 / (short["ms_per_step"] * 1e-3), rel=1e-4)
    assert short["configs"] == {} and short["cpu_baseline"] is None
    full = json.loads([l for l in out.stderr.splitlines() if l.startswith("bench.py detail: ")][-1][len("bench.py detail: "):])
    for key in ("preimage", "kernels", "m2b", "preimage_m3b", "chain_m4", "sustained", "exchange", "independent_units"):
        assert key not in full, key
    assert full["repeats"]["count"] == 1 and full["other_gather"] is None
    # --dump-outputs: the product of the last timed step (sampled: the whole matrix exceeds the dump limit)
    rec = full["dump_outputs"]["files"]["product.npy"]
    got = np.load(out_dir / "product.npy")
    assert list(got.shape) == rec["shape"] and got.dtype == np.float32 and rec["rows"] == 1 and rec["cols"] == 120

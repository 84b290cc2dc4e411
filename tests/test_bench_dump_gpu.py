"""bench.py --dump-outputs on the real steps (tests/test_bench_cpu.py covers the stub): a small training step, run twice,
writes the same loss / parameters / gradients bit for bit; a forward step writes its outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--clips", "1", "--frames", "2", "--actors", "4", "--points", "1024", "--height", "64", "--width", "96",
         "--steps", "2", "--warmup", "1"]


def _bench(argv, out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + argv + ["--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.strip()][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    return {f: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_train_step_dump_is_reproducible(tmp_path):
    a = _bench([], tmp_path / "a")
    b = _bench([], tmp_path / "b")
    assert sorted(a) == ["grads.npy", "loss.npy", "params.npy"]
    assert a["loss.npy"].shape == (1,)
    assert a["params.npy"].shape == a["grads.npy"].shape and a["params.npy"].size > 1000
    for f in a:
        assert a[f].dtype == np.float32 and np.isfinite(a[f]).all(), f
        assert a[f].tobytes() == b[f].tobytes(), "%s differs between two runs with the same arguments" % f
    assert np.abs(a["grads.npy"]).max() > 0


def test_forward_step_dump(tmp_path):
    a = _bench(["--mode", "forward"], tmp_path / "f")
    assert a and all(f.startswith("out") for f in a)
    for f, v in a.items():
        assert v.dtype in (np.float32, np.float64) and v.size > 0, f

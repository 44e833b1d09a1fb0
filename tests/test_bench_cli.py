"""bench.py's command line (no GPU): the options of a plain and a --full run, and the files that
--dump-outputs writes."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_help_lists_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs", "--no-extras", "--no-cpu"):
        assert opt in out.stdout, opt


def test_bench_rejects_zero_steps():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 2 and "--steps" in out.stderr


def test_dump_outputs_writes_float64_npy(tmp_path):
    import bench
    arrays = {"npivot": np.array([3.0]), "pivoterrors": np.array([1.0, 0.5, 0.25, 0.125])}
    d = tmp_path / "sub" / "dump"
    bench.dump_outputs(str(d), 0, 1, arrays)
    assert sorted(os.listdir(d)) == ["npivot.npy", "pivoterrors.npy"]
    for name, arr in arrays.items():
        got = np.load(d / f"{name}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, arr)
    # ranks above 0 of a multi-GPU run factorise their own matrices: their files carry the rank
    bench.dump_outputs(str(d), 1, 2, arrays)
    assert "npivot_rank1.npy" in os.listdir(d)

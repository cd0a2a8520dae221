"""The driver's bench contract: torchrun multi-rank launch emits ONE JSON
line from rank 0 with the whole-job aggregate (weak scaling, MAX-over-ranks
timing). Runs the real bench.py exactly as the driver does (gloo on CPU)."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(420)
def test_torchrun_world2_bench_json():
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29741", "bench.py", "--gpus", "2", "--steps",
         "2", "--warmup", "1", "--cpu"],
        cwd=REPO, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line from rank 0"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak"
    assert d["config"]["parallelism"] == "local_sgd_dp2"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    for key in ("metric", "unit", "steps", "warmup", "higher_is_better",
                "vs_baseline", "dtype", "data"):
        assert key in d


def test_single_process_bench_json():
    r = subprocess.run(
        [sys.executable, "bench.py", "--cpu", "--steps", "2", "--warmup",
         "1"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines()
                    if ln.startswith("{")][0])
    assert d["n_gpus"] == 1


def test_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes one replayed step's loss, parameters and AdamW
    first moment as float32 .npy; the same arguments give the same inputs,
    hence (on the deterministic CPU path) the same files, and --full is
    accepted."""
    import numpy as np
    runs = []
    for name, extra in (("a", []), ("b", ["--full"])):
        out = tmp_path / name
        r = subprocess.run(
            [sys.executable, "bench.py", "--cpu", "--steps", "2",
             "--warmup", "1", "--dump-outputs", str(out)] + extra,
            cwd=REPO, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([ln for ln in r.stdout.splitlines()
                        if ln.startswith("{")][0])
        assert d["steps"] == 2 and d["ms_per_step"] > 0
        arrs = {f.stem: np.load(f) for f in sorted(out.iterdir())}
        assert set(arrs) == {"loss", "params", "adam_m"}
        for a in arrs.values():
            assert a.dtype == np.float32 and np.isfinite(a).all()
        assert arrs["loss"].shape == (1,) and arrs["params"].ndim == 1
        assert arrs["adam_m"].shape == arrs["params"].shape
        assert np.abs(arrs["adam_m"]).max() > 0
        assert sum(a.nbytes for a in arrs.values()) <= 64 * 2**20
        runs.append(arrs)
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k])

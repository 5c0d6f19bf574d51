"""bench.py's multi-rank path (E1), rehearsed on one GPU.

The driver runs `torch.distributed.run --nproc-per-node N ... bench.py --gpus N`
on an 8-GPU node with RCCL, one GPU per rank.  Here two ranks share the one GPU
and talk over gloo (BB_BENCH_BACKEND=gloo): the same env sharding (global env
ids, per-env terrain generators), barriers, max-over-ranks timing and rank-0
JSON line, with the weak-scaling bookkeeping the driver reads.
"""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_plain_run_is_lean_and_dumps_the_last_timed_step(tmp_path):
    """A plain run times --steps steps and prints the line without the CPU leg or the per-step
    comparison run (--full's); --dump-outputs writes the last timed step's five outputs, one row
    per env, float32, and the same arguments give the same arrays."""
    import numpy as np

    dumps = []
    for d in ("a", "b"):
        cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3",
               "--burn-in", "10", "--envs", "300", "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["steps"] == 7 and line["status"] == "ok" and line["dtype"] == "f64"
        assert line["value"] == pytest.approx(300 * 7 / (line["ms_per_step"] * 7 / 1e3), rel=1e-6)
        assert not {"cpu_baseline", "cpu_baseline_multicore", "parity", "per_step"} & set(line)
        assert line["roofline"]["flops"]["source"] == "profiles/flops.json"  # no live count either
        dumps.append({p.stem: np.load(p) for p in sorted((tmp_path / d).glob("*.npy"))})
    shapes = {"obs": (300, 15), "reward": (300,), "done": (300,), "terminal_obs": (300, 15), "pos2d": (300, 2)}
    assert {k: v.shape for k, v in dumps[0].items()} == shapes
    for k, a in dumps[0].items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), k
        assert np.array_equal(a, dumps[1][k]), k
    assert np.abs(dumps[0]["obs"]).max() > 0


@pytest.mark.parametrize("terrain", ["flat", "perlin"])
def test_bench_two_ranks_over_gloo(terrain):
    env = dict(os.environ, BB_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), str(ROOT / "bench.py"), "--gpus", "2",
           "--steps", "20", "--warmup", "5", "--burn-in", "20", "--envs", "512", "--terrain", terrain,
           "--full", "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 prints ONE JSON line
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak"
    assert line["config"]["total_envs"] == 1024 and line["config"]["envs_per_gpu"] == 512
    assert line["value"] > 0 and line["steps"] == 20
    assert line["value"] == pytest.approx(1024 * 20 / (line["ms_per_step"] * 20 / 1e3), rel=1e-6)
    assert "env-sharded x2" in line["config"]["parallelism"]
    # two ranks share the chip: each rank's persistent relief pair (perlin) must still have
    # finished every launch without its budget firing (bench.py would have exited non-zero)
    assert line["stats"]["pair_budget"] == 0 and line["status"] == "ok"

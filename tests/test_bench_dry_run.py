"""bench.py's control flow for N = 1 and N = 2 without a GPU (tests/bench_dry_run.py: stub + gloo; numbers meaningless)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import host_profile as HP  # noqa: E402

KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
        "data", "config", "roofline", "cpu_baseline", "time_to_converged_s", "time_to_converged_setup_s"}


def _run_ranks(world, mode, bench_args):
    """bench.py under the dry-run wrapper on `world` ranks; -> rank 0's JSON line (the other ranks must print none)."""
    if not os.path.exists(os.path.join(ROOT, "gtsam_amd", "lib", "libgtsam_amd.so")):
        pytest.skip("libgtsam_amd.so not built")
    stub = HP.build_stub()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(world):
        env = dict(os.environ, LD_PRELOAD=stub, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   BENCH_PARALLELISM=mode, BENCH_ARGS=bench_args)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "bench_dry_run.py")], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    lines = [line for line in outs[0][0].splitlines() if line.startswith("{")]
    assert len(lines) == 1                                              # rank 0 prints ONE JSON line
    assert all(not any(line.startswith("{") for line in so.splitlines()) for so, _ in outs[1:])   # the other ranks print none
    return json.loads(lines[0])


@pytest.mark.parametrize("world,mode", [(1, "shard"), (2, "shard"), (2, "speculative")])
def test_bench_contract_and_multi_rank_flow(world, mode):
    rec = _run_ranks(world, mode, "--full")
    assert KEYS <= set(rec) and rec["n_gpus"] == world and rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["metric"] == "LM iterations/sec" and rec["unit"] == "iterations/s" and rec["higher_is_better"] is True
    assert rec["scaling"] == "strong" and rec["dtype"] == "f64" and rec["data"] == "synthetic" and rec["vs_baseline"] is None
    assert "workload" in rec["config"] and "model" not in rec["config"]
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(rec["roofline"])
    if world > 1:     # the other modes ride along in the same line (bench.py --extra-modes auto)
        other = "speculative" if mode == "shard" else "shard"
        assert set(rec["extra_modes"]) == {other, "pcg_shard"}, rec["extra_modes"]
        for k, v in rec["extra_modes"].items():
            assert "failed" not in v and v["steps"] >= 2 and v["value"] > 0, (k, v)
    else:
        assert rec["extra_modes"] is None
    assert {"lambda_tries", "tries_per_iteration", "device_phase_ms_per_iteration"} <= set(rec)
    assert rec["config"]["parallelism"].startswith("single GPU" if world == 1 else ("speculative-lambda x2" if mode == "speculative" else "landmark-shard x2"))


@pytest.mark.parametrize("world,mode", [(1, "shard"), (2, "shard")])
def test_plain_bench_run_prints_the_headline_only_and_dumps_the_last_step(world, mode, tmp_path):
    """Without --full: the headline keys, nothing of the --full legs, and --dump-outputs writes the last timed step's arrays."""
    out = tmp_path / "outputs"
    rec = _run_ranks(world, mode, f"--dump-outputs {out}")
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup"} <= set(rec)
    assert rec["metric"] == "LM iterations/sec" and rec["unit"] == "iterations/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["n_gpus"] == world and rec["steps"] == 2 and rec["warmup"] == 1
    assert abs(rec["ms_per_step"] - 1e3 / rec["value"]) <= 1e-9 * rec["ms_per_step"]
    assert not {"roofline", "cpu_baseline", "cpp_host", "python_mirror", "time_to_converged_s", "extra_modes", "workloads"} & set(rec)
    files = sorted(os.listdir(out))
    assert files == ["delta.npy", "error.npy", "lambda.npy", "values.npy"]
    total = 0
    for f in files:
        a = np.load(out / f)
        assert a.dtype in (np.float32, np.float64) and a.size > 0
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(out / "error.npy").shape == (1,) and np.load(out / "lambda.npy").shape == (1,)

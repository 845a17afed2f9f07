"""bench.py end to end on the small workload: a plain run does what its headline needs and nothing else, and --full adds
the legs, the rooflines and the checks on the same answer."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("alt_sharding", "pcie_inclusive_users_per_sec", "roofline", "c4", "streaming", "api", "structured", "cpu_baseline")
FULL_ONLY_FIT = ("tolerance_modes", "roofline", "all_features", "cpu_baseline")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "small", "--steps", "2", "--warmup", "1",
                        *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]          # one JSON line
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_only_and_full_adds_the_rest(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "out"))
    assert all(k in plain for k in HEADLINE) and plain["unit"] == "users/s" and plain["higher_is_better"] is True
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["fit"]["interactions_per_sec"] > 0 and plain["fit"]["W_nnz"] > 0
    assert not set(FULL_ONLY) & set(plain) and not set(FULL_ONLY_FIT) & set(plain["fit"])
    ids = np.load(tmp_path / "out" / "topk_ids.npy")           # the last timed step's ids, as exact float64
    assert ids.shape == (plain["config"]["n_users"], 10)
    assert zlib.crc32(ids.astype(np.int32).tobytes()) == plain["topk_ids_crc32"]

    full = _bench("--full", "--no-cpu-baseline", "--no-api", "--stream-batches", "0")
    assert all(full[k] == plain[k] for k in ("metric", "unit", "higher_is_better", "dtype"))
    assert full["topk_ids_crc32"] == plain["topk_ids_crc32"] and full["fit"]["W_nnz"] == plain["fit"]["W_nnz"]
    assert full["roofline"]["kernel_ms_avg"] > 0 and full["roofline"]["launches"] >= 2
    assert full["pcie_inclusive_users_per_sec"] > 0 and full["alt_sharding"] is None and full["c4"] is None
    assert set(full["fit"]["tolerance_modes"]) >= {"shuffle", "gram"} and full["fit"]["roofline"]["algorithmic_bytes"] > 0
    assert full["fit"]["all_features"]["W_nnz"] > 0          # the K=None fit of the small workloads

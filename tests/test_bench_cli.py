"""bench.py command line: a plain run reports only the headline figure,
--steps sets the number of timed steps, and --dump-outputs writes what the
last timed step returned — checked here against the CPU oracle's compaction
of the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

KEYS, PARTS, RUNS, NOW = 40_000, 2, 4, 1_000_000  # bench.py's epoch_now
STAT_FIELDS = ("input_records", "output_records", "expired", "filtered",
               "tombstones", "shadowed", "output_bytes")


@pytest.mark.gpu
def test_plain_run_and_dump_outputs(oracle_lib, tmp_path):
    out_dir = tmp_path / "dump"
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3",
         "--warmup", "1", "--keys", str(KEYS), "--partitions", str(PARTS),
         "--runs", str(RUNS), "--dump-outputs", str(out_dir)],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["metric"] == "compaction keys/sec per node"
    assert res["unit"] == "keys/s" and res["higher_is_better"] is True
    assert res["dtype"] == "u8"
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["ms_per_step"] > 0 and res["value"] > 0
    # value and ms_per_step describe the same timed region; ms_per_step is
    # rounded to 0.01 ms, value to 0.1 keys/s
    ms_from_value = res["config"]["keys_per_gpu"] / res["value"] * 1e3
    assert abs(res["ms_per_step"] - ms_from_value) <= 0.005 + 1e-6
    # the side measurements stay behind --full
    for k in ("roofline", "cpu_baseline", "extra"):
        assert k not in res

    assert sorted(os.listdir(out_dir)) == ["compact_stats.npy"]
    got = np.load(out_dir / "compact_stats.npy")
    assert got.dtype == np.float64 and got.shape == (PARTS, 1 + len(STAT_FIELDS))

    sys.path.insert(0, REPO)
    import bench

    want = []
    for p in range(PARTS):
        op = oracle_lib.open(1, p, -1)
        try:
            for run in bench.build_partition_data(KEYS // PARTS, RUNS, 0, p):
                op.ingest_run_arrays(np.ascontiguousarray(run["keys"]), run["koff"],
                                     np.ascontiguousarray(run["vals"]), run["voff"], run["sk"])
            err, st = op.manual_compact(NOW, keep_inputs=True)
        finally:
            op.close()
        want.append([err] + [getattr(st, f) for f in STAT_FIELDS])
    assert np.array_equal(got, np.array(want, dtype=np.float64))

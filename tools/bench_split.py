#!/usr/bin/env python3
"""Cost of the on-device partition split next to the route it replaces.

Builds ONE partition of the headline shape (bench.py defaults: 50M keys / 16
partitions, --runs 8 => ~3.5M fixed-stride records in 9 runs, see
tools/bench_minor_compact.py) and times, with one warm-up and --reps timed
repeats each on a freshly ingested handle:

  split : rrdb_split(parent, child, 2) — wall time of the call and the
          engine's own timers rrdb_phase_ms split_classify / split_emit /
          split_total; once with the crc64 table staged in LDS and once read
          from global memory (env engine.split_crc);
  copy  : what the parent commit could do: rrdb_checkpoint the parent,
          rrdb_restore into a fresh handle, rrdb_set_partition_version on both,
          rrdb_manual_compact on both with
          replica.split.validate_partition_hash on.

The generator does not place keys by hash, so the partition is split 1 -> 2
(pidx 0 -> 0 and 1): half the records move, exactly the work of splitting
partition p of 16 into p and p + 16.

Reported per route: wall ms (median), bytes moved per second counted as 2 x
the resident key+value bytes, and peak device memory above the level before
the route started (hipMemGetInfo, sampled from a second thread while the calls
run).  Not wired into bench.py.

    python tools/bench_split.py [--reps 5]
"""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("split_classify", "split_emit", "split_total")
EPOCH_NOW = 1_000_000


class MemWatch:
    """peak device-memory use (total - free) while a block runs"""

    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipMemGetInfo.argtypes = [ctypes.POINTER(ctypes.c_size_t)] * 2

    def used(self):
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert self.hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return total.value - free.value

    def __enter__(self):
        self.base = self.peak = self.used()
        self._stop = False
        self._t = threading.Thread(target=self._poll)
        self._t.start()
        return self

    def _poll(self):
        self.hip.hipSetDevice(0)
        while not self._stop:
            self.peak = max(self.peak, self.used())
            time.sleep(0.0002)

    def __exit__(self, *exc):
        self._stop = True
        self._t.join()
        self.end = self.used()
        self.peak = max(self.peak, self.end)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=50_000_000 // 16)
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--copy-reps", type=int, default=2)
    args = ap.parse_args()

    import incubator_pegasus_amd as pa
    from incubator_pegasus_amd import data as D

    hip = pa.hip_lib()
    runs = D.build_point_table_runs(args.keys, args.runs, seed=D.DEFAULT_SEED,
                                    value_len=100, dup_fraction=0.10, delete_fraction=0.02)
    resident = sum(int(r["koff"][-1]) + int(r["voff"][-1]) for r in runs)
    watch = MemWatch()

    def fresh(envs=None):
        parent, child = hip.open(1, 0, 0), hip.open(1, 1, 0)
        for h in (parent, child):
            h.set_envs({"replica.split.validate_partition_hash": "true", **(envs or {})})
        for r in runs:
            parent.ingest_run_arrays(np.ascontiguousarray(r["keys"]), r["koff"],
                                     np.ascontiguousarray(r["vals"]), r["voff"], r["sk"])
        return parent, child

    def split_route(crc):
        rows, stats = [], None
        for i in range(args.reps + 1):  # first pass warms up
            parent, child = fresh({"engine.split_crc": crc})
            with watch:
                t0 = time.perf_counter()
                err, stats = parent.split(child, 2)
                wall = (time.perf_counter() - t0) * 1e3
            assert err == 0 and stats.parent_unpruned_runs == 0
            if i:
                rows.append(dict(wall_ms=wall, peak_over_start=watch.peak - watch.base,
                                 end_over_start=watch.end - watch.base,
                                 **{ph: parent.phase_ms(ph) for ph in PHASES}))
            parent.close()
            child.close()
        return rows, stats

    def copy_route():
        rows, recs = [], None
        for i in range(args.copy_reps + 1):
            parent, child = fresh()
            d = tempfile.mkdtemp(prefix="bench-split-")
            try:
                with watch:
                    t0 = time.perf_counter()
                    assert parent.checkpoint(d, 1) == 0
                    assert child.restore(d, 1) == 0
                    t1 = time.perf_counter()
                    for h in (parent, child):
                        h.set_partition_version(1)
                        err, _ = h.manual_compact(EPOCH_NOW)
                        assert err == 0
                    t2 = time.perf_counter()
                recs = (int(parent.num_records()), int(child.num_records()))
                if i:
                    rows.append(dict(wall_ms=(t2 - t0) * 1e3, copy_ms=(t1 - t0) * 1e3,
                                     compact_ms=(t2 - t1) * 1e3,
                                     peak_over_start=watch.peak - watch.base,
                                     end_over_start=watch.end - watch.base))
            finally:
                shutil.rmtree(d, ignore_errors=True)
                parent.close()
                child.close()
        return rows, recs

    def med(rows):
        out = {k: round(statistics.median(r[k] for r in rows), 3) for k in rows[0]}
        out["spread_wall_ms"] = [round(min(r["wall_ms"] for r in rows), 3),
                                 round(max(r["wall_ms"] for r in rows), 3)]
        out["moved_GBps"] = round(2 * resident / (out["wall_ms"] * 1e-3) / 1e9, 2)
        for k in ("peak_over_start", "end_over_start"):
            out[k + "_MiB"] = round(out.pop(k) / 2**20, 1)
        return out

    out = {"records": int(sum(len(r["sk"]) for r in runs)), "runs": len(runs),
           "resident_key_value_MiB": round(resident / 2**20, 1), "reps": args.reps}
    for crc in ("lds", "global"):
        rows, st = split_route(crc)
        out["split_" + crc] = med(rows)
        # the emit reads and writes every byte that changes place
        moved = st.child_bytes + st.parent_bytes
        out["split_" + crc]["split_emit_GBps"] = round(
            2 * moved / (out["split_" + crc]["split_emit"] * 1e-3) / 1e9, 1)
    out["split_stats"] = {f: getattr(st, f) for f in st.__dataclass_fields__}
    rows, recs = copy_route()
    out["copy_then_filter"] = med(rows)
    out["copy_then_filter"]["records_parent_child_after"] = recs
    print(json.dumps(out))


if __name__ == "__main__":
    main()

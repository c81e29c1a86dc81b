#!/usr/bin/env python3
"""Rate of rrdb_incr_batch next to the loop a host shim composes today.

A resident partition of tools/bench_write_batch.py's shape (18-byte keys,
100 user bytes: a decimal counter right-aligned behind blanks, which the
reference's parse accepts) is built first and not timed.  For every batch size
and key distribution (uniform, and zipfian theta 0.99 over the resident keys,
so that a few hot counters collect long chains), on a fresh handle each time:

  batch : one rrdb_incr_batch call, increments of 1 (wall time of the C call,
          arrays prepared beforehand), with the engine's five device timers;
  loop  : per op rrdb_get + rrdb_ttl + rrdb_put, then one rrdb_flush.  Every
          read flushes the memtable, so the loop leaves a run per op and each
          read searches all of them; it is measured up to --loop-max ops only.

--lane-max sweeps env "engine.incr_lane_max" (the longest chain one lane
walks; longer ones get a wave) on the zipfian batches and reports incr_apply.
Median of --reps after one warm-up.  One JSON line per measurement.  Not wired
into bench.py.

    python tools/bench_incr_batch.py [--reps 3] [--sizes 1000,65536,1048576]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("incr_sort", "incr_lookup", "incr_apply", "incr_emit", "incr_total")
NOW = 100_000


_RESIDENT = {}


def resident(eng, n_res):
    """n_res counters, values 1000 + id % 9000, as two batch-written runs"""
    from incubator_pegasus_amd import data as D

    if n_res not in _RESIDENT:
        ids = np.arange(n_res, dtype=np.uint64)
        keys = np.ascontiguousarray(D.make_raw_keys(ids))
        vals = np.full((n_res, 100), 32, dtype=np.uint8)
        v = np.uint64(1000) + ids % np.uint64(9000)
        for j in range(4):
            vals[:, 99 - j] = (48 + (v // np.uint64(10 ** j)) % np.uint64(10)).astype(np.uint8)
        _RESIDENT[n_res] = (keys, vals)
    keys, vals = _RESIDENT[n_res]
    half = n_res // 2
    for lo, hi in ((0, half), (half, n_res)):
        m = hi - lo
        err, _ = eng.write_batch_arrays(
            keys[lo:hi].reshape(-1), D.fixed_offsets(m, 18), vals[lo:hi].reshape(-1),
            D.fixed_offsets(m, 100), np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint8), 0)
        assert err == 0


def op_keys(n, n_res, dist, seed):
    from incubator_pegasus_amd import data as D

    if dist == "zipfian":
        ids = D.zipfian_ids(n, n_res, seed=seed)
    else:
        ids = np.random.default_rng(seed).integers(0, n_res, n).astype(np.uint64)
    return np.ascontiguousarray(D.make_raw_keys(ids)), ids


def med(xs):
    return round(statistics.median(xs), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,65536,1048576")
    ap.add_argument("--resident", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-max", type=int, default=1000)
    ap.add_argument("--lane-max", default="4,32,256,4096")
    args = ap.parse_args()

    import incubator_pegasus_amd as pa
    from incubator_pegasus_amd import data as D

    hip = pa.hip_lib()
    sizes = [int(s) for s in args.sizes.split(",")]

    def run_batch(n, dist, lane_max=None):
        keys, ids = op_keys(n, args.resident, dist, 77 + n)
        koff = D.fixed_offsets(n, 18)
        inc = np.ones(n, dtype=np.int64)
        wall, phases, st = [], [], None
        for i in range(args.reps + 1):  # the first pass warms up
            eng = hip.open(1, 0, 0)
            if lane_max is not None:
                eng.set_envs({"engine.incr_lane_max": str(lane_max)})
            resident(eng, args.resident)
            t0 = time.perf_counter()
            err, nv, er, st = eng.incr_batch_arrays(keys.reshape(-1), koff, inc, None, NOW)
            dt = (time.perf_counter() - t0) * 1e3
            assert err == 0 and st.applied == n and eng.num_runs() == 3
            if i:
                wall.append(dt)
                phases.append({ph: eng.phase_ms(ph) for ph in PHASES})
            eng.close()
        _, counts = np.unique(ids, return_counts=True)
        row = {"ops": n, "dist": dist, "distinct_keys": int(st.output_records),
               "longest_chain": int(counts.max()), "batch_wall_ms": med(wall),
               "batch_ops_per_s": round(n / statistics.median(wall) * 1e3)}
        if lane_max is not None:
            row["lane_max"] = lane_max
        for ph in PHASES:
            row[ph + "_ms"] = med([p[ph] for p in phases])
        return row

    for n in sizes:
        for dist in ("uniform", "zipfian"):
            row = run_batch(n, dist)
            if n <= args.loop_max:
                keys, _ = op_keys(n, args.resident, dist, 77 + n)
                raw = [bytes(k) for k in keys]
                loop = []
                for i in range(args.reps + 1):
                    eng = hip.open(1, 0, 0)
                    resident(eng, args.resident)
                    t0 = time.perf_counter()
                    for k in raw:
                        err, val = eng.get(k, NOW)
                        _, ttl = eng.ttl(k, NOW)
                        new = int(val) + 1
                        assert eng.put(k[2:18], b"", b"%d" % new,
                                       NOW + ttl if ttl > 0 else 0, NOW) == 0
                    assert eng.flush() == 0
                    dt = (time.perf_counter() - t0) * 1e3
                    if i:
                        loop.append(dt)
                    row["loop_runs_left"] = int(eng.num_runs())
                    eng.close()
                row["loop_wall_ms"] = med(loop)
                row["loop_ops_per_s"] = round(n / statistics.median(loop) * 1e3)
                row["batch_speedup"] = round(statistics.median(loop) / row["batch_wall_ms"], 1)
            print(json.dumps(row), flush=True)

    for lm in [int(s) for s in args.lane_max.split(",") if s]:
        for n in sizes[1:]:
            row = run_batch(n, "zipfian", lm)
            print(json.dumps({k: row[k] for k in ("ops", "dist", "lane_max", "longest_chain",
                                                  "incr_apply_ms", "incr_total_ms",
                                                  "batch_wall_ms")}), flush=True)


if __name__ == "__main__":
    main()

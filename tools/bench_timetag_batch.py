#!/usr/bin/env python3
"""Rate of rrdb_write_batch_timetag next to rrdb_write_batch on the same batch.

A resident partition of tools/bench_write_batch.py's shape (18-byte keys, 100
user bytes) is built first, through rrdb_write_batch_timetag itself so that
every resident record carries a non-zero timetag (1000 + id % 1000), and is
not timed.  For every batch size and key distribution, on a fresh handle each
time:

  timetag : one rrdb_write_batch_timetag call of verified PUTs whose timetags
            are drawn from [500, 2500), so that a good part of them is stale
            (wall time of the C call, arrays prepared beforehand), with the
            engine's five device timers and two host timers;
  plain   : one rrdb_write_batch call on the same keys and values.  The
            difference is the price of the lookup and the walk.

Key distributions: uniform and zipfian (theta 0.99) over the resident keys,
and "hot": one key whose chain is the whole batch, which a single wave scans.
--lane-max sweeps env "engine.wbt_lane_max" (the longest chain one lane walks;
longer ones get a wave) on the zipfian batches and reports wbt_apply (a hot
batch is one chain on one wave at every setting below its length).
Median of --reps after one warm-up, with min and max.  One JSON line per
measurement.  Not wired into bench.py.

    python tools/bench_timetag_batch.py [--reps 3] [--sizes 1000,65536,1048576]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("wbt_sort", "wbt_lookup", "wbt_apply", "wbt_emit", "wbt_total", "wbt_stage",
          "wbt_upload")
NOW = 100_000

_RESIDENT = {}


def resident(eng, n_res):
    """n_res records with timetag 1000 + id % 1000, as two batch-written runs"""
    from incubator_pegasus_amd import data as D

    if n_res not in _RESIDENT:
        ids = np.arange(n_res, dtype=np.uint64)
        keys = np.ascontiguousarray(D.make_raw_keys(ids))
        vals = np.ascontiguousarray(D.make_values(ids, 100, version=1)[:, 12:])
        _RESIDENT[n_res] = (keys, vals, np.uint64(1000) + ids % np.uint64(1000))
    keys, vals, tts = _RESIDENT[n_res]
    half = n_res // 2
    for lo, hi in ((0, half), (half, n_res)):
        m = hi - lo
        err, _, st = eng.write_batch_timetag_arrays(
            keys[lo:hi].reshape(-1), D.fixed_offsets(m, 18), vals[lo:hi].reshape(-1),
            D.fixed_offsets(m, 100), np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint8),
            np.ascontiguousarray(tts[lo:hi]), None, NOW)
        assert err == 0 and st.applied == m


def op_ids(n, n_res, dist, seed):
    from incubator_pegasus_amd import data as D

    if dist == "zipfian":
        return D.zipfian_ids(n, n_res, seed=seed)
    if dist == "hot":
        return np.full(n, n_res // 3, dtype=np.uint64)
    return np.random.default_rng(seed).integers(0, n_res, n).astype(np.uint64)


def med(xs):
    return round(statistics.median(xs), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,65536,1048576")
    ap.add_argument("--resident", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lane-max", default="4,32,256,4096")
    args = ap.parse_args()

    import incubator_pegasus_amd as pa
    from incubator_pegasus_amd import data as D

    hip = pa.hip_lib()
    sizes = [int(s) for s in args.sizes.split(",")]

    def run_batch(n, dist, lane_max=None, plain=True):
        ids = op_ids(n, args.resident, dist, 77 + n)
        keys = np.ascontiguousarray(D.make_raw_keys(ids)).reshape(-1)
        koff, voff = D.fixed_offsets(n, 18), D.fixed_offsets(n, 100)
        vals = np.ascontiguousarray(
            D.make_values(np.arange(n, dtype=np.uint64), 100, version=1, salt=5)[:, 12:]
        ).reshape(-1)
        expire, kinds = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
        tts = np.random.default_rng(99 + n).integers(500, 2500, n).astype(np.uint64)
        verify = np.ones(n, dtype=np.uint8)
        wall, wall_plain, phases, st = [], [], [], None
        for i in range(args.reps + 1):  # the first pass warms up
            eng = hip.open(1, 0, 0)
            if lane_max is not None:
                eng.set_envs({"engine.wbt_lane_max": str(lane_max)})
            resident(eng, args.resident)
            t0 = time.perf_counter()
            err, ap_, st = eng.write_batch_timetag_arrays(keys, koff, vals, voff, expire, kinds,
                                                          tts, verify, NOW)
            dt = (time.perf_counter() - t0) * 1e3
            assert err == 0 and st.applied + st.ignored == n
            if i:
                wall.append(dt)
                phases.append({ph: eng.phase_ms(ph) for ph in PHASES})
            eng.close()
            if not plain:
                continue
            eng = hip.open(1, 0, 0)
            resident(eng, args.resident)
            t0 = time.perf_counter()
            err, _ = eng.write_batch_arrays(keys, koff, vals, voff, expire, kinds, NOW)
            dt = (time.perf_counter() - t0) * 1e3
            assert err == 0
            if i:
                wall_plain.append(dt)
            eng.close()
        _, counts = np.unique(ids, return_counts=True)
        row = {"ops": n, "dist": dist, "applied": int(st.applied), "ignored": int(st.ignored),
               "output_records": int(st.output_records), "longest_chain": int(counts.max()),
               "timetag_wall_ms": med(wall), "timetag_wall_min_max": [round(min(wall), 3),
                                                                      round(max(wall), 3)],
               "timetag_ops_per_s": round(n / statistics.median(wall) * 1e3)}
        if plain:
            row["plain_wall_ms"] = med(wall_plain)
            row["plain_wall_min_max"] = [round(min(wall_plain), 3), round(max(wall_plain), 3)]
            row["timetag_over_plain_ms"] = round(row["timetag_wall_ms"] - row["plain_wall_ms"], 3)
        if lane_max is not None:
            row["lane_max"] = lane_max
        for ph in PHASES:
            xs = [p[ph] for p in phases]
            row[ph + "_ms"] = med(xs)
            row[ph + "_min_max"] = [round(min(xs), 3), round(max(xs), 3)]
        return row

    for n in sizes:
        for dist in ("uniform", "zipfian", "hot"):
            print(json.dumps(run_batch(n, dist)), flush=True)

    for lm in [int(s) for s in args.lane_max.split(",") if s]:
        for n in sizes[1:]:
            for dist in ("zipfian",):
                row = run_batch(n, dist, lm, plain=False)
                print(json.dumps({k: row[k] for k in (
                    "ops", "dist", "lane_max", "longest_chain", "wbt_apply_ms",
                    "wbt_apply_min_max", "wbt_total_ms", "timetag_wall_ms")}), flush=True)


if __name__ == "__main__":
    main()

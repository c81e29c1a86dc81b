#!/usr/bin/env python3
"""Rate of rrdb_check_and_mutate_batch next to the loop a host shim composes
today.

A resident partition of tools/bench_write_batch.py's shape (18-byte keys, each
its own hashkey; 100 user bytes) is built first and not timed.  Every op is a
check_and_set on its check key: CT_VALUE_BYTES_EQUAL against a 100-byte
operand that equals the stored value for about half the ops, and one PUT of
the same 100 bytes (so that the share of passing checks does not drift along a
chain).  For every batch size and hashkey distribution (uniform, and zipfian
theta 0.99 over the resident keys, so that a few hot hashkeys collect long
segments), on a fresh handle each time:

  batch : one rrdb_check_and_mutate_batch call (wall time of the C call,
          arrays prepared beforehand), with the engine's five device timers;
  loop  : per op rrdb_get, the compare on the host, rrdb_put when it passes,
          then one rrdb_flush.  Every read flushes the memtable, so the loop
          leaves a run per passed op and each read searches all of them; it is
          measured up to --loop-max ops only.

The last row puts as many ops as the longest zipfian segment of the largest
size on ONE hashkey: the serial walk of one lane, the cost a hot hashkey adds.
Median of --reps after one warm-up.  One JSON line per measurement.  Not wired
into bench.py.

    python tools/bench_cas_batch.py [--reps 3] [--sizes 1000,65536,1048576]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("cas_sort", "cas_lookup", "cas_apply", "cas_emit", "cas_total")
NOW = 100_000
CT_VALUE_BYTES_EQUAL = 10

_RESIDENT = {}


def resident_arrays(n_res):
    """n_res records: 92 x 'v' and the id in eight digits"""
    from incubator_pegasus_amd import data as D

    if n_res not in _RESIDENT:
        ids = np.arange(n_res, dtype=np.uint64)
        keys = np.ascontiguousarray(D.make_raw_keys(ids))
        vals = np.full((n_res, 100), ord("v"), dtype=np.uint8)
        for j in range(8):
            vals[:, 99 - j] = (48 + (ids // np.uint64(10 ** j)) % np.uint64(10)).astype(np.uint8)
        _RESIDENT[n_res] = (keys, vals)
    return _RESIDENT[n_res]


def resident(eng, n_res):
    from incubator_pegasus_amd import data as D

    keys, vals = resident_arrays(n_res)
    half = n_res // 2
    for lo, hi in ((0, half), (half, n_res)):
        m = hi - lo
        err, _ = eng.write_batch_arrays(
            keys[lo:hi].reshape(-1), D.fixed_offsets(m, 18), vals[lo:hi].reshape(-1),
            D.fixed_offsets(m, 100), np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint8), 0)
        assert err == 0


def op_ids(n, n_res, dist, seed):
    from incubator_pegasus_amd import data as D

    if dist == "zipfian":
        return D.zipfian_ids(n, n_res, seed=seed)
    if dist == "hot":
        return np.full(n, 12345 % n_res, dtype=np.uint64)
    return np.random.default_rng(seed).integers(0, n_res, n).astype(np.uint64)


def med(xs):
    return round(statistics.median(xs), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,65536,1048576")
    ap.add_argument("--resident", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-max", type=int, default=1000)
    args = ap.parse_args()

    import incubator_pegasus_amd as pa
    from incubator_pegasus_amd import data as D

    hip = pa.hip_lib()
    sizes = [int(s) for s in args.sizes.split(",")]
    rkeys, rvals = resident_arrays(args.resident)

    def arrays(n, dist):
        ids = op_ids(n, args.resident, dist, 77 + n)
        keys = np.ascontiguousarray(rkeys[ids])
        vals = np.ascontiguousarray(rvals[ids])
        operands = vals.copy()
        miss = np.random.default_rng(99 + n).random(n) < 0.5
        operands[miss, 0] = ord("x")
        return ids, keys, vals, operands, miss

    def run_batch(n, dist):
        ids, keys, vals, operands, miss = arrays(n, dist)
        k18, v100 = D.fixed_offsets(n, 18), D.fixed_offsets(n, 100)
        types = np.full(n, CT_VALUE_BYTES_EQUAL, dtype=np.int32)
        moff = np.arange(n + 1, dtype=np.uint64)
        kinds = np.zeros(n, dtype=np.uint8)
        wall, phases, st = [], [], None
        for i in range(args.reps + 1):  # the first pass warms up
            eng = hip.open(1, 0, 0)
            resident(eng, args.resident)
            t0 = time.perf_counter()
            err, er, ex, _, st = eng.check_and_mutate_batch_arrays(
                keys.reshape(-1), k18, types, operands.reshape(-1), v100, moff, keys.reshape(-1),
                k18, vals.reshape(-1), v100, None, kinds, None, NOW, want_values=False)
            dt = (time.perf_counter() - t0) * 1e3
            assert err == 0 and st.passed == int((~miss).sum()) and st.failed_check == int(miss.sum())
            assert eng.num_runs() == 3
            if i:
                wall.append(dt)
                phases.append({ph: eng.phase_ms(ph) for ph in PHASES})
            eng.close()
        _, counts = np.unique(ids, return_counts=True)
        row = {"ops": n, "dist": dist, "distinct_hashkeys": int(len(counts)),
               "longest_segment": int(counts.max()), "passed": int(st.passed),
               "batch_wall_ms": med(wall),
               "batch_ops_per_s": round(n / statistics.median(wall) * 1e3)}
        for ph in PHASES:
            row[ph + "_ms"] = med([p[ph] for p in phases])
        return row

    longest = 1
    for n in sizes:
        for dist in ("uniform", "zipfian"):
            row = run_batch(n, dist)
            if dist == "zipfian":
                longest = row["longest_segment"]
            if n <= args.loop_max:
                _, keys, vals, operands, _ = arrays(n, dist)
                raw = [bytes(k) for k in keys]
                want = [bytes(o) for o in operands]
                new = [bytes(v) for v in vals]
                loop = []
                for i in range(args.reps + 1):
                    eng = hip.open(1, 0, 0)
                    resident(eng, args.resident)
                    t0 = time.perf_counter()
                    for k, o, v in zip(raw, want, new):
                        err, val = eng.get(k, NOW)
                        if err == 0 and val == o:
                            assert eng.put(k[2:18], b"", v, 0, NOW) == 0
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
    print(json.dumps(run_batch(max(2, longest), "hot")), flush=True)


if __name__ == "__main__":
    main()

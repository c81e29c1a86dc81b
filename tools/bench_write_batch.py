#!/usr/bin/env python3
"""Write rate of rrdb_write_batch next to the one-record write path.

Headline-shape records (18-byte keys, 100 user bytes = 112-byte encoded
values) in random order, a tenth of the ops overwriting earlier ones.  For
every batch size, on a fresh handle of the same library each time:

  batch  : one rrdb_write_batch call (wall time of the C call, arrays
           prepared beforehand), with the engine's own timers: wb_stage /
           wb_upload (host) and wb_sort / wb_emit / wb_total (device);
  single : rrdb_put x N + rrdb_flush, the existing path, called through a
           bare ctypes binding so that the Python wrapper is not in the loop.
           Its cost per op does not depend much on N, so sizes above
           --single-max are skipped unless --single-all is given.

Median of --reps after one warm-up, with min and max.  Prints one JSON line
per size and a final {"crossover_ops": ...} line: the smallest measured size
at which the batch is faster.  Not wired into bench.py.

    python tools/bench_write_batch.py [--reps 5] [--sizes 1000,10000,...]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("wb_stage", "wb_upload", "wb_sort", "wb_emit", "wb_total")


def make_batch(n, seed):
    """(keys (n,18) u8, values (n,100) u8): op i < 0.9n writes a fresh key,
    the rest overwrite earlier ones; then one shuffle of the key ids"""
    from incubator_pegasus_amd import data as D

    rng = np.random.default_rng(seed)
    fresh = max(1, n - n // 10)
    ids = rng.permutation(np.arange(fresh, dtype=np.uint64) * np.uint64(7) + np.uint64(3))
    ids = np.concatenate([ids, rng.choice(ids, n - fresh)]) if n > fresh else ids
    keys = np.ascontiguousarray(D.make_raw_keys(ids))
    vals = rng.integers(0, 256, size=(n, 100), dtype=np.uint8)
    return keys, vals


def summary(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3),
            "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000,100000,1000000,4000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single-max", type=int, default=1_000_000)
    ap.add_argument("--single-all", action="store_true")
    args = ap.parse_args()

    import incubator_pegasus_amd as pa
    from incubator_pegasus_amd import data as D

    hip = pa.hip_lib()
    L = hip._lib
    put = L.rrdb_put
    put.restype = C.c_int32
    put.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                    C.c_uint64, C.c_uint32, C.c_uint32]
    crossover = None
    for n in [int(s) for s in args.sizes.split(",")]:
        keys, vals = make_batch(n, 1234 + n)
        koff, voff = D.fixed_offsets(n, 18), D.fixed_offsets(n, 100)
        expire = np.zeros(n, dtype=np.uint32)
        kinds = np.zeros(n, dtype=np.uint8)
        kflat, vflat = keys.reshape(-1), vals.reshape(-1)
        kbase, vbase = keys.ctypes.data, vals.ctypes.data

        batch_ms, phases, stats = [], [], None
        for i in range(args.reps + 1):  # the first pass warms up
            eng = hip.open(1, 0, 0)
            t0 = time.perf_counter()
            err, stats = eng.write_batch_arrays(kflat, koff, vflat, voff, expire, kinds, 0)
            dt = (time.perf_counter() - t0) * 1e3
            assert err == 0 and eng.num_runs() == 1
            if i:
                batch_ms.append(dt)
                phases.append({ph: eng.phase_ms(ph) for ph in PHASES})
            eng.close()

        single_ms, call_ms = [], None
        if args.single_all or n <= args.single_max:
            # what n foreign-function calls cost by themselves (a getter that
            # takes no lock), to be read next to single_wall_ms
            eng = hip.open(1, 0, 0)
            nop, h = L.rrdb_memtable_entries, eng._h
            t0 = time.perf_counter()
            for j in range(n):
                nop(h)
            call_ms = (time.perf_counter() - t0) * 1e3
            eng.close()
            for i in range(args.reps + 1):
                eng = hip.open(1, 0, 0)
                h = eng._h
                t0 = time.perf_counter()
                # key = [00 10][16-byte hashkey], no sortkey
                for j in range(n):
                    put(h, kbase + 18 * j + 2, 16, None, 0, vbase + 100 * j, 100, 0, 0)
                assert eng.flush() == 0
                dt = (time.perf_counter() - t0) * 1e3
                assert eng.num_records() == stats.output_records
                if i:
                    single_ms.append(dt)
                eng.close()

        row = {"ops": n, "output_records": stats.output_records,
               "batch_wall_ms": summary(batch_ms),
               "batch_ops_per_s": round(n / statistics.median(batch_ms) * 1e3)}
        for ph in PHASES:
            row[ph + "_ms"] = summary([p[ph] for p in phases])
        med = {ph: statistics.median(p[ph] for p in phases) for ph in PHASES}
        row["host_staging_share"] = round(med["wb_stage"] / statistics.median(batch_ms), 3)
        row["wb_sort_ns_per_op"] = round(med["wb_sort"] * 1e6 / n, 3)
        if single_ms:
            row["single_wall_ms"] = summary(single_ms)
            row["single_ops_per_s"] = round(n / statistics.median(single_ms) * 1e3)
            row["single_call_overhead_ms"] = round(call_ms, 3)
            if crossover is None and statistics.median(batch_ms) < statistics.median(single_ms):
                crossover = n
        print(json.dumps(row), flush=True)
    print(json.dumps({"crossover_ops": crossover, "reps": args.reps}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of a window (minor) compaction next to the full pass.

Builds ONE partition of the headline shape (bench.py defaults: 50M keys / 16
partitions, --runs 8 => ~3.5M records: 8 base runs of ~390K plus the
generator's overlay run of ~375K newer versions and tombstones, 9 runs in
all) and reports the engine's own phase timers — rrdb_phase_ms compact_rank /
compact_emit / compact_total — for

  full   : rrdb_manual_compact over all runs (keep_inputs, so repeatable on
           the same handle), the all-fixed-stride emit;
  window : rrdb_compact_runs(4, R-4), the newer half [4, R) including the
           overlay run — non-bottommost, so it takes the per-row-size emit
           and keeps its tombstones.

keep_inputs has no meaning for a window pass (its point is to replace the
window in the run list), so the partition is re-ingested from the same host
arrays before every timed window pass.  Not wired into bench.py.

    python tools/bench_minor_compact.py [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("compact_rank", "compact_emit", "compact_total")
EPOCH_NOW = 1_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=50_000_000 // 16)
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--first", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import incubator_pegasus_amd as pa
    from incubator_pegasus_amd import data as D

    hip = pa.hip_lib()
    runs = D.build_point_table_runs(args.keys, args.runs, seed=D.DEFAULT_SEED,
                                    value_len=100, dup_fraction=0.10, delete_fraction=0.02)

    def fresh():
        eng = hip.open(1, 0, 0)
        for r in runs:
            eng.ingest_run_arrays(np.ascontiguousarray(r["keys"]), r["koff"],
                                  np.ascontiguousarray(r["vals"]), r["voff"], r["sk"])
        return eng

    def phases(eng):
        return {ph: eng.phase_ms(ph) for ph in PHASES}

    full, window = [], []
    eng = fresh()
    n_all = int(eng.num_records())
    n_runs = int(eng.num_runs())
    for i in range(args.reps + 1):  # first pass warms up
        err, st_full = eng.manual_compact(EPOCH_NOW, keep_inputs=True)
        assert err == 0
        if i:
            full.append(phases(eng))
    eng.close()
    n_win = n_runs - args.first
    for i in range(args.reps + 1):
        eng = fresh()
        err, st_win = eng.compact_runs(args.first, n_win, EPOCH_NOW)
        assert err == 0 and eng.num_runs() == args.first + 1, (err, eng.num_runs())
        if i:
            window.append(phases(eng))
        eng.close()

    def med(rows):
        return {ph: round(statistics.median(r[ph] for r in rows), 3) for ph in PHASES}

    out = {
        "records_all_runs": n_all,
        "runs": n_runs,
        "full": {"input_records": st_full.input_records,
                 "output_records": st_full.output_records,
                 "output_bytes": st_full.output_bytes, "median_ms": med(full)},
        "window": {"first": args.first, "n": n_win,
                   "input_records": st_win.input_records,
                   "output_records": st_win.output_records,
                   "shadowed": st_win.shadowed,
                   "output_bytes": st_win.output_bytes, "median_ms": med(window)},
        "reps": args.reps,
    }
    for k in ("full", "window"):
        ms = out[k]["median_ms"]["compact_total"]
        out[k]["ns_per_input_record"] = round(ms * 1e6 / out[k]["input_records"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

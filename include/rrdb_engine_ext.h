/* rrdb_engine_ext.h — engine-only extensions to the rrdb C interface.
 *
 * rrdb_engine.h is the contract BOTH backends export (the MI355X engine and
 * the CPU oracle).  The entry points below exist in the engine only: they
 * change the physical run layout without changing what any read returns, so
 * the oracle — whose reads define correctness — has no use for them.  A
 * loader must look the symbols up and treat their absence as "not supported".
 *
 * Minor (window) compaction.  Every flush appends a sorted run, and every
 * read pays for the run count.  rrdb_manual_compact merges ALL runs and is
 * bottommost: tombstones and filter-removed records vanish.  A window pass
 * merges a contiguous age range of runs that need not include the oldest.
 * When an older run lies below the window nothing may simply disappear, or
 * the older version of the key would come back to life:
 *   - a shadowed version (a newer one of the same key is in the window) is
 *     dropped, as ever;
 *   - a tombstone is kept verbatim;
 *   - a PUT that the compaction filter removes (expired, user delete rule,
 *     stale split hash) is kept as a tombstone: same key, same seqno, empty
 *     value (rocksdb's CompactionIterator does the same with a filter's
 *     Decision::kRemove above the bottommost level);
 *   - a surviving PUT is kept, with default-TTL / update_ttl header rewrites
 *     applied as in the full pass.
 * A window that starts at run 0 is bottommost and behaves like the full pass
 * restricted to those runs.
 *
 * Stats are counted over the window.  When not bottommost: tombstones == 0
 * (none is dropped), expired/filtered count the conversions, output_records
 * counts every emitted record (tombstones included), and
 * input_records == output_records + shadowed.
 */
#ifndef RRDB_ENGINE_EXT_H
#define RRDB_ENGINE_EXT_H

#include "rrdb_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Merge runs [first_run, first_run+n_runs) (0 = oldest) into one run that
 * takes their place.  Bottommost iff first_run == 0.  The memtable is flushed
 * first, as in the manual pass.  n_runs == 1 rewrites one run through the
 * filter.  kInvalidArgument: n_runs == 0, a window outside the run list, a
 * split compaction pending, or manual_compact.disabled. */
int32_t rrdb_compact_runs(void *h, uint64_t first_run, uint64_t n_runs,
                          uint32_t epoch_now, rrdb_compact_stats *stats);

/* Background-compaction tick (the host shim calls it after a flush): if
 * num_runs >= the L0 trigger (env "engine.l0_compaction_trigger", default 4,
 * values below 2 mean 2), pick one window, compact it, and report it;
 * otherwise do nothing and set *n_runs_out = 0.  The pick is size-tiered,
 * with n[i] the records of run i and R the run count:
 *     s = R-2, acc = n[R-1] + n[R-2];
 *     while s > 0 and n[s-1] <= 2*acc:  s -= 1, acc += n[s];
 *     window = [s, R).
 * Env "rocksdb.usage_scenario" = "bulk_load" switches the tick off.  It is
 * not a manual compaction: manual_compact.disabled does not stop it.
 * kInvalidArgument while a split compaction is pending.  Unflushed writes do
 * not count towards the trigger; when the tick does compact, the memtable is
 * flushed first and the new run is part of the pick. */
int32_t rrdb_auto_compact(void *h, uint32_t epoch_now, uint64_t *first_run_out,
                          uint64_t *n_runs_out, rrdb_compact_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* RRDB_ENGINE_EXT_H */

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
 *
 * Partition split.  The table's partition count doubles from N to 2N; every
 * partition p gives rise to child p + N, and from then on a record belongs to
 * the handle whose index equals pegasus_key_hash(key) & (2N-1).  The reference
 * copies the parent's checkpoint into the child's directory
 * (replica_split_manager.cpp:278, copy_checkpoint_to_dir), sets
 * partition_version = 2N-1 on both replicas (set_partition_version, :884), and
 * leaves the foreign half to the compaction filter's stale-split-hash rule
 * (key_ttl_compaction_filter.h:114-121) at some later compaction.  With runs
 * resident in HBM that route holds the partition twice until both sides have
 * compacted.  rrdb_split does the data part on the device instead: each
 * record is classified by its hash and each run is cut, stably, into the part
 * the parent keeps and the part the child receives.
 *   - Ownership: with mask = new_partition_count - 1 and
 *     t = key_hash(key) & mask, the record goes to the parent if
 *     t == parent.pidx, to the child if t == child.pidx, nowhere otherwise
 *     (it was stale before the split).  The hash is the compaction filter's
 *     and the scan validation's: over the hashkey, or over the sortkey bytes
 *     when the hashkey is empty.  A key shorter than two bytes (the codec
 *     produces none) stays in the parent.
 *   - All versions of a key share a hash, so tombstones, shadowed versions
 *     and expired records travel with their key.  Nothing is merged,
 *     filtered, rewritten or expired: records move byte for byte with their
 *     seq_kind, and there is no epoch_now argument.
 *   - Every parent run is partitioned stably (key order kept) and run order
 *     is kept on both sides.  A run that contributes nothing to a side
 *     produces no run there.  The parent's memtable is flushed first.
 *   - Device memory, two phases.  A: all child runs are built with the
 *     parent untouched; a failed allocation frees them and returns kIOError
 *     with both handles as before.  B: the parent is pruned one run at a time
 *     (allocate the kept part, emit, free the source, swap); a failed
 *     allocation here leaves the remaining runs whole, counts those that
 *     still hold foreign records in parent_unpruned_runs and returns kOk: the
 *     child is complete and the leftovers are exactly the stale records the
 *     compaction filter drops.  Peak residency is about 1.5x the partition
 *     plus half the largest run, ending at 1x.  A run that is entirely the
 *     parent's is not rewritten.
 *   - After kOk both handles have partition_version = new_partition_count-1,
 *     the child's sequence floor equals the parent's (later writes to the
 *     child outrank everything it inherited), and the parent's parked scan
 *     contexts are reclaimed as after a compaction (scan_next: kNotFound).
 *   - rrdb_phase_ms(parent, ...) reports split_classify, split_emit and
 *     split_total.
 *
 * Batched writes.  rrdb_put / rrdb_remove insert one record at a time into a
 * host memtable; the reference applies a whole batch of mutations per decree
 * (on_batched_write_requests, multi_put, multi_remove).  rrdb_write_batch
 * takes such a batch unsorted, in commit order, duplicate keys allowed, and
 * sorts and dedups it on the device.  The result is exactly what this
 * sequence leaves behind, ending in one new run: flush the memtable; for
 * i = 0..n-1 rrdb_put / rrdb_remove op i; rrdb_flush.
 *   - Keys are full keys [u16 BE hklen][hashkey][sortkey], as rrdb_get takes
 *     them.  Op i gets seqno next_seq_floor + i; on success the floor advances
 *     by n_ops, superseded ops included.  Of several ops on one key the last
 *     one wins and is the only one stored.
 *   - A PUT value is encoded as rrdb_put encodes it: the header of the
 *     handle's pegasus.data_version with timetag 0, and expire_ts == 0 with a
 *     default_ttl env becomes epoch_now + default_ttl.  A remove is a
 *     tombstone with an empty value.
 *   - Pending memtable entries are older than the batch: they are flushed
 *     first into a run of their own, and a failure of that flush is returned.
 *   - Everything is validated before anything changes.  kInvalidArgument with
 *     the handle as before: offsets that do not start at 0 or decrease; a key
 *     shorter than 2 bytes; hklen > klen - 2 or hklen == 0xFFFF; a kind other
 *     than 0/1; n_ops > 2^31 - 1; a split compaction or a pipelined count
 *     scan pending.  n_ops == 0 is kOk and does nothing.
 *   - Every allocation proportional to the batch may fail cleanly: on a full
 *     device the call returns kIOError, no run is added, the floor is
 *     unchanged, and a memtable flush that already happened stays.
 *   - rrdb_phase_ms reports wb_sort, wb_emit and wb_total (device time), and
 *     wb_stage and wb_upload (host time of the staging and of the copies).
 *
 * Batched counter increments.  The write service's read-modify-write family
 * starts with incr (pegasus_write_service_impl.h:264-344): read the stored
 * counter, add, store the decimal text.  rrdb_incr_batch takes n such ops
 * unsorted, in commit order, duplicate keys allowed, and applies them on the
 * device.  The call leaves behind exactly what this sequence leaves behind,
 * ending in at most one new run: flush the memtable; for i = 0..n-1 apply
 * incr op i as the reference does (its own read, then its own rrdb_put when
 * it succeeds); rrdb_flush.
 *   - Per op, with `old` the newest version of the key at that moment,
 *     earlier ops of this batch included:
 *       absent, tombstone or expired (expire > 0 && expire <= epoch_now):
 *         new = increment, new_expire = directive > 0 ? directive : 0;
 *       present with empty user data: new = increment, TTL as for "present";
 *       present, user data not an integer: errors[i] = kInvalidArgument,
 *         new_values[i] = 0, nothing is written;
 *       present, integer, old + increment leaves int64: errors[i] =
 *         kInvalidArgument, new_values[i] = old, nothing is written;
 *       present, integer, the sum fits: new = old + increment.  TTL for
 *         "present": directive 0 keeps the stored expire, < 0 clears it to 0,
 *         > 0 sets it.
 *   - "An integer" is what dsn::buf2int64 accepts: strtoll(s, &end, 0) in the
 *     C locale over the whole span.  Optional leading isspace bytes, optional
 *     sign, 0x/0X hex, leading-0 octal, else decimal; the whole span consumed
 *     (an embedded NUL or a trailing byte fails); inside int64; at least one
 *     digit ("0x", "09", "+", " " fail); no 0b prefix.
 *   - A successful op stores rrdb_put(key, decimal(new), new_expire,
 *     epoch_now): decimal is std::to_string (a '-' for negatives, no '+', no
 *     padding), the header is that of the handle's pegasus.data_version with
 *     timetag 0, and new_expire == 0 with a default_ttl env becomes
 *     epoch_now + default_ttl.  errors[i] = kOk, new_values[i] = new.
 *   - Only successful ops consume sequence numbers, as only they call
 *     rrdb_put: the k-th successful op gets next_seq_floor + k and the floor
 *     advances by `applied`.  Per key only the last successful op is stored,
 *     as one PUT.  If no op succeeds no run is added and the floor is
 *     unchanged; the call still returns kOk.
 *   - Pending memtable entries are older than the batch: they are flushed
 *     first into a run of their own, and a failure of that flush is returned.
 *   - Everything is validated before anything changes.  kInvalidArgument with
 *     the handle as before: offsets that do not start at 0 or decrease; a key
 *     shorter than 2 bytes; hklen > klen - 2 or hklen == 0xFFFF;
 *     increments == NULL; n_ops > 2^31 - 1; a split compaction or a pipelined
 *     count scan pending.  n_ops == 0 is kOk and does nothing.
 *   - Every allocation proportional to the batch may fail cleanly: on a full
 *     device the call returns kIOError, no run is added, the floor is
 *     unchanged, new_values / errors are unspecified, and a memtable flush
 *     that already happened stays.
 *   - rrdb_phase_ms reports incr_sort (sort and segments), incr_lookup,
 *     incr_apply (chains and seqno ranks), incr_emit and incr_total (device
 *     time).  Env "engine.incr_lane_max" (default 32) is the longest chain one
 *     lane walks; a longer one is scanned by a whole wave.
 *
 * Batched check-and-mutate.  The read-modify-write family ends with the
 * compare-and-swap pair check_and_set / check_and_mutate
 * (pegasus_write_service_impl.h:436-530, :710-833); check_and_set is
 * check_and_mutate with a one-PUT mutate list, so one call covers both.
 * rrdb_check_and_mutate_batch takes n such ops unsorted, in commit order,
 * duplicate keys allowed, and checks and applies them on the device.  The call
 * leaves behind exactly what this sequence leaves behind, ending in at most
 * one new run: flush the memtable; for i = 0..n-1 apply op i as the reference
 * does (its own read of the check key and, when the check passes, its own
 * rrdb_put / rrdb_remove per mutation, in list order); rrdb_flush.
 *   - An op is a check key (a full key [u16 BE hklen][hashkey][sortkey], as
 *     rrdb_get takes it), a check_type (int32, numbered as cas_check_type in
 *     idl/rrdb.thrift: 0 = CT_NO_CHECK ... 17 = CT_VALUE_INT_GREATER), a check
 *     operand (a byte span) and a list of mutations.  The lists of all ops are
 *     stored together and the n + 1 offsets mut_offs mark where each op's list
 *     starts and ends.  A mutation is a full key, a kind (RRDB_KIND_PUT /
 *     RRDB_KIND_DELETE) and, for a PUT, user data and a uint32 expire_ts.
 *     check_and_set is one PUT mutation; set_diff_sort_key == false means the
 *     mutation key equals the check key.  Every mutation key of an op must
 *     carry the check key's hashkey (the reference builds them all from one
 *     hash_key); that is validated for the whole batch, and it is what makes
 *     hashkeys independent of each other on the device.
 *   - Per op, with `old` the newest version of the check key at that moment,
 *     earlier ops of this batch included:
 *       malformed (an empty mutation list, a kind other than 0/1, a check_type
 *         outside 0..17): errors[i] = kInvalidArgument, no read happens
 *         (check_exist[i] = 0, the returned check value is empty), nothing is
 *         written;
 *       value_exist = `old` is a PUT that is not expired (expire > 0 &&
 *         expire <= epoch_now is expired); the check value is its user data,
 *         header stripped.  A PUT that an earlier op of the batch stored with
 *         an expire_ts already past is "not exist", as rrdb_get reports it;
 *       the check is the reference's validate_check (:1144-1270): types 0-4
 *         are the existence checks; 5-7 match anywhere / prefix / postfix (the
 *         value must exist, an empty operand passes, an operand longer than
 *         the value fails); 8-12 compare bytes (the value must exist; memcmp
 *         over the common length, then the shorter one is smaller); 13-17
 *         compare integers (the value must exist; value and operand both go
 *         through dsn::buf2int64, the parse described under rrdb_incr_batch,
 *         and if either does not parse the check fails with invalid_argument);
 *       passed: every mutation of the list is applied in order, a PUT as
 *         rrdb_put(key, data, expire_ts, epoch_now) encodes it (the header of
 *         the handle's pegasus.data_version, timetag 0, and expire_ts == 0
 *         with a default_ttl env becomes epoch_now + default_ttl), a DELETE as
 *         rrdb_remove encodes it (a tombstone with an empty value);
 *         errors[i] = kOk;
 *       not passed: nothing is written; errors[i] = kInvalidArgument when
 *         invalid_argument is set, else kTryAgain (RRDB_TRY_AGAIN);
 *       check_exist[i] = value_exist; when return_check_value[i] is set and
 *         the value exists, the check value is returned.
 *   - Only applied mutations consume sequence numbers: the k-th applied
 *     mutation (op order, then list order) gets next_seq_floor + k and the
 *     floor advances by mutations_applied.  Per key only the last applied
 *     mutation is stored.  If nothing is applied no run is added and the floor
 *     stays; the call still returns kOk.
 *   - Pending memtable entries are older than the batch: they are flushed
 *     first into a run of their own, and a failure of that flush is returned.
 *   - Everything is validated before anything changes.  kInvalidArgument with
 *     the handle as before: any offsets array that does not start at 0 or
 *     decreases; mut_offs[n] != the mutation count M (the C call carries no
 *     separate count: the mutation arrays are read as mut_offs[n] entries,
 *     and the Python binding refuses arrays of another length); a key
 *     shorter than 2 bytes; hklen > klen - 2 or hklen == 0xFFFF; a mutation
 *     key whose [hklen][hashkey] prefix differs from its op's check key;
 *     n + M > 2^31 - 1 (n is bounded before any array is read, n + M once
 *     mut_offs is); a required array that is NULL; a split compaction or a
 *     pipelined count scan pending.  n_ops == 0 is kOk and does nothing.
 *   - Every allocation proportional to the batch may fail cleanly: on a full
 *     device the call returns kIOError, no run is added, the floor is
 *     unchanged, the outputs are unspecified, and a memtable flush that
 *     already happened stays.
 *   - rrdb_phase_ms reports cas_sort (sort, heads, hashkey groups),
 *     cas_lookup, cas_apply (walk and ranks), cas_emit (the run and the
 *     returned check values) and cas_total (device time).
 *
 * Batched writes with timetags.  Duplication replays another cluster's put,
 * remove, multi_put and multi_remove through pegasus_write_service::duplicate
 * (pegasus_write_service.cpp:509-586) into rocksdb_wrapper::write_batch_put_ctx
 * (rocksdb_wrapper.cpp:129-183): every write carries a timetag, and with
 * verify_timetag set the stored record is read first and the write is dropped
 * when that record is live and its timetag is not smaller.
 * rrdb_write_batch_timetag takes n such ops unsorted, in commit order,
 * duplicate keys allowed, and verifies and applies them on the device.  The
 * call leaves behind exactly what this sequence leaves behind, ending in at
 * most one new run: flush the memtable; for i = 0..n-1 apply op i as
 * write_batch_put_ctx / write_batch_delete do, each with its own read;
 * rrdb_flush.
 *   - Keys, values, expire_ts and kinds are rrdb_write_batch's.  timetags[i]
 *     is the finished 64-bit timetag, generate_timetag(timestamp, cluster_id,
 *     deleted) = timestamp << 8 | cluster_id << 1 | deleted
 *     (pegasus_value_schema.h:44-47).  The engine stores it and compares it as
 *     an unsigned integer and never takes it apart.  A local write passes its
 *     own timetag with verify[i] = 0; a duplicated write passes the remote
 *     timetag and the request's verify_timetag.
 *   - Per op, with `old` the newest version of the key at that moment,
 *     earlier ops of this batch included:
 *       DELETE: always applied (write_batch_delete makes no check, :221-239);
 *         the record is a tombstone with an empty value and no timetag;
 *       PUT with verify[i] != 0 on a handle whose pegasus.data_version >= 1:
 *         ignored when `old` is live and timetag(old) >= timetags[i]; live
 *         means a PUT whose stored expire is not (> 0 && <= epoch_now).
 *         Nothing is stored for an ignored op and applied[i] = 0.  Otherwise
 *         the op is applied;
 *       any other PUT: applied.  Data version 0 has no timetag: verify is
 *         without effect there and nothing is stored beyond the expire (the
 *         reference's verify_timetag_compatible_with_version_0);
 *       an applied PUT stores the header of the handle's data version with
 *         the expire as rrdb_put computes it (expire_ts == 0 with a
 *         default_ttl env becomes epoch_now + default_ttl), timetags[i]
 *         big-endian in the 8 timetag bytes, then the user bytes;
 *         applied[i] = 1.  A PUT that this batch stored with an expire already
 *         past counts as not live for the ops after it, as rrdb_get would
 *         report it.
 *   - For a stale PUT the reference writes an empty key with an empty value
 *     instead (:157-161), a record that lies before every key a read can
 *     name.  The engine does not store it.
 *   - Op i has seqno next_seq_floor + i and the floor advances by n_ops,
 *     ignored and superseded ops included (the reference's empty record
 *     consumes a sequence number too).  Per key only the last applied op is
 *     stored.  If nothing is applied no run is added; the floor still
 *     advances and the call returns kOk.
 *   - With timetags == NULL and verify == NULL the call is rrdb_write_batch:
 *     the run, the floor and the shared stat fields are the same.
 *   - rrdb_put, rrdb_write_batch, rrdb_incr_batch and
 *     rrdb_check_and_mutate_batch store timetag 0.  A verified PUT with a
 *     timetag above 0 therefore beats their records, and a verified PUT with
 *     timetag 0 loses against any live record.
 *   - Pending memtable entries are older than the batch: they are flushed
 *     first into a run of their own, and a failure of that flush is returned.
 *   - Everything is validated before anything changes, as in
 *     rrdb_write_batch and with the same list; timetags, verify and applied
 *     are not validated (any value is meaningful).  n_ops == 0 is kOk and
 *     does nothing.
 *   - Every allocation proportional to the batch may fail cleanly: on a full
 *     device the call returns kIOError, no run is added, the floor is
 *     unchanged, applied is unspecified, and a memtable flush that already
 *     happened stays.
 *   - rrdb_phase_ms reports wbt_sort (sort and segments), wbt_lookup,
 *     wbt_apply (the walk), wbt_emit and wbt_total (device time), and
 *     wbt_stage and wbt_upload (host time of the staging and of the copies).
 *     Env "engine.wbt_lane_max" (default 32) is the longest chain one lane
 *     walks; a longer one is scanned by a whole wave.
 *
 * Compaction route.  One compaction pass is a rank kernel followed by an emit
 * kernel, and which pair runs is decided per pass: from the envs
 * "engine.rank_mode" and "engine.emit_mode", the run count, the key shape of
 * the runs (the tail-word kernels need one shared key stride >= 8 and a shared
 * first stride-8 bytes) and whether the pass is a window.  Every pair produces
 * the same run, so no read can tell them apart; rrdb_last_compact_route
 * reports which pair the last pass took, so that a test or a benchmark that
 * means one kernel can tell it ran that kernel.
 *   - rank: RRDB_ROUTE_RANK_GLOBAL / _LDS / _LDST / _GRP, numbered as
 *     engine.rank_mode numbers them.  A mode that does not apply (lds with a
 *     non-chunked emit, a single run or more than 64 runs; ldst or grp on runs that are not
 *     tail-word eligible; grp with more than 32 runs or the input-major
 *     emit) falls to ldst when engine.rank_mode is ldst and the runs are
 *     eligible, else to global.
 *   - emit: RRDB_ROUTE_EMIT_RANK / _INPUT / _CHUNKED as engine.emit_mode
 *     numbers them, and _CHUNKED_FIXED for the chunked emit in its
 *     all-fixed-stride form (bottommost, one key stride and one PUT-value
 *     stride across the runs).  A window pass always emits chunked.
 *   - RRDB_ROUTE_NONE (-1): rank when the pass had no input record or no pass
 *     has started on the handle; emit when nothing was emitted (no output
 *     record), and between rrdb_manual_compact_begin and its finish.  Both
 *     modes are read once, at the begin: an env set before the finish
 *     applies to the next pass.
 *   - Manual, window and auto passes all report.  A call that is rejected
 *     before the pass starts leaves the previous report.  Recording costs no
 *     device work and changes no behaviour.
 *
 * Multi_get lane.  A range multi_get is served by one device function behind
 * several lanes, each with its own request and response plumbing, and which
 * lane runs is decided per call: from the envs "engine.mg_persist" and
 * "engine.mg_graph", the run count, the request size, and whether a lane came
 * up at all (a refused graph capture or a resident kernel that is slow to
 * start switches that lane off for the handle, silently).  Every lane returns
 * the same rows; rrdb_last_multi_get_lane reports which one the last call
 * took, so that a test or a benchmark that means one lane can tell it ran
 * that lane.
 *   - lane, for the last rrdb_multi_get: RRDB_MG_LANE_POINT_LIST (n_sort_keys
 *     > 0), _SERVER (the resident mailbox kernel), _GRAPH (the captured
 *     graph), _SMALL (the plain fused launch) or _GENERAL (the view path).
 *     RRDB_MG_LANE_NONE: no call yet, or the call returned before any lane
 *     (rejected arguments, a failed flush, an empty range).
 *   - fused_first: when lane is _GENERAL, the fused lane (_SERVER, _GRAPH or
 *     _SMALL) that ran first and handed the request back: more than 4096
 *     candidate rows, a sortkey or user data above 65535 bytes, or a response
 *     that does not fit the fused buffer.  _NONE when the general path was
 *     taken directly (no run, or more than 64 runs).
 *   - tail_read: 1 when the fused response was larger than the pinned prefix
 *     that comes back with the header, so that the host read the whole
 *     response from device memory in a second copy.
 *   - batch_fused / batch_fallback, for the last rrdb_multi_get_batch: the
 *     requests the batch kernel answered and those that went through the
 *     per-request path (their sum is n_req).  batch_device_out: 1 when the
 *     result was delivered in dev_vals / dev_val_offs.  All zero when the
 *     batch was rejected.
 *   - The two calls keep separate fields: a batch leaves lane, fused_first
 *     and tail_read as the last rrdb_multi_get set them (its per-request
 *     fallbacks do not report), and rrdb_multi_get leaves the batch fields.
 *     Recording costs no device work and changes no behaviour.
 *
 * View route.  Every read that is no point lookup (rrdb_scan_open,
 * rrdb_sortkey_count, the general lane of rrdb_multi_get) first builds a view:
 * the records of every run inside the range are ranked into one order, and the
 * newest versions that are no tombstone are gathered.  Which rank kernel runs
 * is decided per view: from the env "engine.rank_mode", the run count, the key
 * shape of the runs (as for the compaction route) and the number of records in
 * the range.  Every kernel produces the same view; rrdb_last_view_route reports
 * which one the last view took, so that a test that means one kernel can tell
 * it ran that kernel.
 *   - rank: RRDB_ROUTE_RANK_GRP (engine.rank_mode grp, at most 32 tail-word
 *     eligible runs, more than one), _LDST (engine.rank_mode ldst on eligible
 *     runs) or _GLOBAL (everything else: a single run, runs that are not
 *     eligible, engine.rank_mode global or lds, which has no view kernel).
 *     RRDB_ROUTE_NONE (-1): no view yet on the handle, no run, or no record of
 *     any run inside the range; the other fields are 0 then.
 *   - bound_levels: the _GLOBAL and _LDST kernels narrow their searches by a
 *     bound table when there is more than one run and the range holds more
 *     than 100000 records: 1, or 2 when the largest window of a run is long
 *     enough for the coarse level (at least 9 << (engine.bt_shift + 6)
 *     records).  0: no table; _LDST then searches global memory instead of
 *     staging.  Always 0 under _GRP.
 *   - n_groups: the anchor groups the _GRP kernel ranked, else 0.  Its grid is
 *     capped at 3584 workgroups whatever engine.grp_blocks says, so above that
 *     a workgroup ranks several groups.
 *   - window_records: the records of all runs inside the range, shadowed
 *     versions and tombstones included.  visible: the rows of the view.
 *   - A read that returns before it builds a view (rejected arguments, a
 *     failed flush, start beyond stop, a multi_get a fused lane answered, a
 *     scan_next) leaves the previous report.  Recording costs no device work
 *     and changes no behaviour.
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

/* Split-time counters.  On the normal path parent_records + child_records +
 * dropped_records == input_records; a run left whole (parent_unpruned_runs)
 * counts all its records and bytes on the parent side. */
typedef struct {
    uint64_t input_records;   /* records in the parent's runs before the split   */
    uint64_t parent_records;  /* records left in the parent                      */
    uint64_t child_records;   /* records moved to the child                      */
    uint64_t dropped_records; /* records owned by neither (already stale)        */
    uint64_t parent_bytes;    /* key+value bytes, parent side                    */
    uint64_t child_bytes;     /* key+value bytes, child side                     */
    uint64_t runs_in, parent_runs, child_runs;
    uint64_t parent_unpruned_runs; /* phase B ran out of memory; 0 normally      */
} rrdb_split_stats;

/* Split `parent` (partition p of N) into itself and `child` (p + N), with
 * new_partition_count = 2N; see the header comment.  The child must be an
 * empty handle on the same device.  kInvalidArgument, both handles unchanged:
 * new_partition_count not a power of two in [2, 2^30];
 * parent.pidx >= new_partition_count/2;
 * child.pidx != parent.pidx + new_partition_count/2; parent == child; app_id,
 * device or data_version differ; the child has runs, memtable entries or
 * parked scan contexts; a split compaction or a pipelined count scan is
 * pending on either handle.  manual_compact.disabled does not stop a split.
 * Both handles' locks are taken together (deadlock-free); all device work
 * runs on the parent's stream. */
int32_t rrdb_split(void *parent, void *child, int32_t new_partition_count,
                   rrdb_split_stats *stats);

typedef struct {
    uint64_t input_ops;       /* n_ops                                         */
    uint64_t output_records;  /* records in the new run (one per distinct key) */
    uint64_t superseded;      /* input_ops - output_records                    */
    uint64_t puts, removes;   /* among the output records                      */
    uint64_t key_bytes, value_bytes; /* of the new run (values encoded)        */
} rrdb_write_batch_stats;

/* Apply n_ops puts/removes, given unsorted in commit order with duplicate
 * keys allowed, as one new run built on the device; see the header comment.
 * keys / key_offs: full rocksdb keys, packed, n+1 offsets.  values /
 * val_offs: user data, packed, n+1 offsets (a remove's span is ignored).
 * expire_ts[n] is ignored for removes and may be null (all zero).  kinds[n]:
 * RRDB_KIND_PUT / RRDB_KIND_DELETE. */
int32_t rrdb_write_batch(void *h, uint64_t n_ops,
                         const uint8_t *keys, const uint64_t *key_offs,
                         const uint8_t *values, const uint64_t *val_offs,
                         const uint32_t *expire_ts, const uint8_t *kinds,
                         uint32_t epoch_now, rrdb_write_batch_stats *stats);

typedef struct {
    uint64_t input_ops;      /* n_ops                                              */
    uint64_t applied;        /* ops that wrote (errors[i] == kOk)                  */
    uint64_t failed_parse;   /* old value not an integer / out of range            */
    uint64_t failed_range;   /* old + increment leaves int64                       */
    uint64_t output_records; /* records in the new run = distinct keys with >= 1 applied op */
    uint64_t key_bytes, value_bytes; /* of the new run (values encoded)            */
} rrdb_incr_batch_stats;

/* Apply n_ops counter increments, given unsorted in commit order with
 * duplicate keys allowed, on the device; see the header comment.  keys /
 * key_offs: full rocksdb keys, packed, n+1 offsets.  increments[n].
 * expire_ts_seconds[n]: the TTL directive of each op, may be null (all 0).
 * new_values[n] / errors[n]: caller-owned, either may be null. */
int32_t rrdb_incr_batch(void *h, uint64_t n_ops,
                        const uint8_t *keys, const uint64_t *key_offs,
                        const int64_t *increments,
                        const int32_t *expire_ts_seconds,
                        uint32_t epoch_now,
                        int64_t *new_values, int32_t *errors,
                        rrdb_incr_batch_stats *stats);

enum { RRDB_TRY_AGAIN = 13 }; /* rocksdb::Status::kTryAgain: the check did not pass */

typedef struct {
    uint64_t input_ops;         /* n_ops                                          */
    uint64_t passed;            /* errors[i] == kOk                               */
    uint64_t failed_check;      /* errors[i] == kTryAgain                         */
    uint64_t failed_invalid;    /* an int check whose value or operand is no int  */
    uint64_t malformed;         /* empty list, bad kind or bad check_type         */
    uint64_t mutations_applied; /* sequence numbers consumed                      */
    uint64_t output_records;    /* records in the new run = distinct keys applied to */
    uint64_t puts, removes;     /* among the output records                       */
    uint64_t key_bytes, value_bytes; /* of the new run (values encoded)           */
} rrdb_cas_batch_stats;

/* Check and apply n_ops check-and-mutate ops, given unsorted in commit order
 * with duplicate keys allowed, on the device; see the header comment.
 * check_keys / check_key_offs: full rocksdb keys, packed, n+1 offsets.
 * check_types[n].  operands / operand_offs: packed, n+1 offsets.  mut_offs:
 * n+1 offsets into the mutation arrays, mut_offs[n] = M.  mut_keys /
 * mut_key_offs and mut_values / mut_val_offs: packed, M+1 offsets (a DELETE's
 * value span is ignored).  mut_expire_ts[M] may be null (all zero).
 * mut_kinds[M].  return_check_value[n] may be null (none).  errors[n] /
 * check_exist[n]: caller-owned, either may be null.  check_values may be null;
 * else count = n and values[i] is op i's check value (len 0 when not asked
 * for or not existing), freed with rrdb_free_result. */
int32_t rrdb_check_and_mutate_batch(
    void *h, uint64_t n_ops, const uint8_t *check_keys, const uint64_t *check_key_offs,
    const int32_t *check_types, const uint8_t *operands, const uint64_t *operand_offs,
    const uint64_t *mut_offs, const uint8_t *mut_keys, const uint64_t *mut_key_offs,
    const uint8_t *mut_values, const uint64_t *mut_val_offs, const uint32_t *mut_expire_ts,
    const uint8_t *mut_kinds, const uint8_t *return_check_value, uint32_t epoch_now,
    int32_t *errors, uint8_t *check_exist, rrdb_result *check_values,
    rrdb_cas_batch_stats *stats);

typedef struct {
    uint64_t input_ops;       /* n_ops                                            */
    uint64_t applied;         /* ops whose write took effect (applied[i] == 1)    */
    uint64_t ignored;         /* verified PUTs dropped as stale (applied[i] == 0) */
    uint64_t output_records;  /* records in the new run = keys with >= 1 applied op */
    uint64_t superseded;      /* applied ops that are not their key's last applied op */
    uint64_t puts, removes;   /* among the output records                         */
    uint64_t key_bytes, value_bytes; /* of the new run (values encoded)           */
} rrdb_timetag_batch_stats;   /* input_ops == ignored + superseded + output_records */

/* Apply n_ops puts/removes that carry timetags, given unsorted in commit
 * order with duplicate keys allowed, verified and applied on the device; see
 * the header comment.  The first eight arguments are rrdb_write_batch's.
 * timetags[n] may be null (all 0).  verify[n] may be null (none).
 * applied[n]: caller-owned, may be null. */
int32_t rrdb_write_batch_timetag(void *h, uint64_t n_ops,
                                 const uint8_t *keys, const uint64_t *key_offs,
                                 const uint8_t *values, const uint64_t *val_offs,
                                 const uint32_t *expire_ts, const uint8_t *kinds,
                                 const uint64_t *timetags, const uint8_t *verify,
                                 uint32_t epoch_now, uint8_t *applied,
                                 rrdb_timetag_batch_stats *stats);

enum {
    RRDB_ROUTE_NONE = -1,
    RRDB_ROUTE_RANK_GLOBAL = 0, /* global searches + bound-table narrowing   */
    RRDB_ROUTE_RANK_LDS = 1,    /* LDS-staged full-key block rank            */
    RRDB_ROUTE_RANK_LDST = 3,   /* windowed LDS-staged tail-word rank        */
    RRDB_ROUTE_RANK_GRP = 4,    /* group-streaming tail-word rank            */
    RRDB_ROUTE_EMIT_RANK = 0,   /* rank-major waves                          */
    RRDB_ROUTE_EMIT_INPUT = 1,  /* input-major waves                         */
    RRDB_ROUTE_EMIT_CHUNKED = 2,       /* chunked, per-row sizes             */
    RRDB_ROUTE_EMIT_CHUNKED_FIXED = 3  /* chunked, all-fixed-stride          */
};

typedef struct {
    int32_t rank; /* RRDB_ROUTE_RANK_* or RRDB_ROUTE_NONE */
    int32_t emit; /* RRDB_ROUTE_EMIT_* or RRDB_ROUTE_NONE */
} rrdb_compact_route;

/* The rank and emit kernels the handle's last compaction pass dispatched to;
 * see the header comment.  Read-only.  kInvalidArgument: out == NULL. */
int32_t rrdb_last_compact_route(void *h, rrdb_compact_route *out);

enum {
    RRDB_MG_LANE_NONE = 0,
    RRDB_MG_LANE_POINT_LIST = 1, /* n_sort_keys > 0: the batched-get core   */
    RRDB_MG_LANE_SERVER = 2,     /* resident mailbox kernel                 */
    RRDB_MG_LANE_GRAPH = 3,      /* captured graph                          */
    RRDB_MG_LANE_SMALL = 4,      /* plain fused launch                      */
    RRDB_MG_LANE_GENERAL = 5     /* view build + host limiter               */
};

typedef struct {
    int32_t lane;             /* RRDB_MG_LANE_*: what answered the last rrdb_multi_get */
    int32_t fused_first;      /* the fused lane that ran first and handed back, or _NONE */
    int32_t tail_read;        /* 1 = the response needed the second device read */
    int32_t batch_device_out; /* 1 = the last batch was delivered on the device */
    uint64_t batch_fused;     /* requests of the last batch the kernel answered */
    uint64_t batch_fallback;  /* requests of the last batch served one by one   */
} rrdb_multi_get_lane;

/* The lane the handle's last rrdb_multi_get took and the fused / fallback
 * split of its last rrdb_multi_get_batch; see the header comment.  Read-only.
 * kInvalidArgument: out == NULL. */
int32_t rrdb_last_multi_get_lane(void *h, rrdb_multi_get_lane *out);

typedef struct {
    int32_t rank;            /* RRDB_ROUTE_RANK_GLOBAL / _LDST / _GRP or RRDB_ROUTE_NONE */
    int32_t bound_levels;    /* bound-table levels the rank searched through: 0, 1 or 2 */
    uint64_t n_groups;       /* anchor groups of the group rank, else 0 */
    uint64_t window_records; /* records of all runs inside the range */
    uint64_t visible;        /* rows of the view: newest versions that are no tombstone */
} rrdb_view_route;

/* The rank kernel the handle's last read view was built with and the sizes it
 * saw; see the header comment.  Read-only.  kInvalidArgument: out == NULL. */
int32_t rrdb_last_view_route(void *h, rrdb_view_route *out);

#ifdef __cplusplus
}
#endif
#endif /* RRDB_ENGINE_EXT_H */

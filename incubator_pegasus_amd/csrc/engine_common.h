/* engine_common.h — shared host/device types for the MI355X rrdb engine.
 *
 * The engine holds each partition's sorted runs resident in HBM:
 *   keys blob + u64 offsets, values blob + u64 offsets, and
 *   seq_kind[i] = (seqno<<1)|kind per record (kind: 0=PUT, 1=DELETE).
 * Runs are ordered oldest -> newest (ingest order); every seqno in run r+1
 * is greater than every seqno in run r (enforced at ingest), which makes
 * "newest version wins" a run-index comparison for equal keys.
 *
 * Merge strategy (MI355X-native, no sequential merging iterator): fully
 * data-parallel rank merging with (key asc, run desc) ordering; a record is
 * shadowed iff its predecessor in rank order carries the same key.  The
 * round-2 production form is the group-streaming merge-path rank
 * (kernels.hip k_rank_grp): anchor keys cut the merged order into groups
 * whose per-run segments are disjoint, so each group's workgroup streams
 * its tail words through LDS exactly once and position-in-group IS local
 * rank.  Replaces rocksdb's merging-iterator heap.
 */
#pragma once
#include <stdint.h>

#define RRDB_MAX_RUNS 64
/* tail-word rank modes: max run count (the group rank's org word packs the
 * run in 16-GRP_ORG_SHIFT bits); group-streaming rank group budget */
#define LDST_MAXR 32
#define GRP_ORG_SHIFT 11
/* group-size sweep (r02, same box): target 512 -> 0.362ms rank, 1024 ->
 * 0.316ms (fewer barriers per element), 2048 -> 0.441ms (80KB LDS drops to
 * 2 workgroups/CU).  1024 is the sweet spot. */
#define GRP_CAP 2048
#define GRP_TARGET 1024
/* read view (build_view): the grid cap of the MODE 1 group rank (a workgroup
 * takes several groups only above it; engine.grp_blocks does not apply to
 * views), and the window size above which the global and ldst ranks build a
 * bound table first (at or below it k_rank_ldst searches global memory) */
#define GRP_VIEW_BLOCKS 3584
#define VIEW_BT_MIN_RECORDS 100000

/* write batch (rrdb_write_batch): (word, op index) pairs one workgroup sorts
 * in LDS, and the output slice one workgroup merges per pass.  2048 pairs are
 * 24 KiB (u64 words + u32 indices), so six workgroups fit a CU's 160 KiB. */
#define WB_TILE 2048

/* device view of a staged write batch: what the sort's comparator needs to
 * break a tie in the 8-byte word */
struct WbKeys {
    const uint8_t *keys;
    const uint64_t *koff; /* n+1; null when every key is `fk` bytes long */
    uint64_t fk;
    const uint32_t *lcp;  /* device: L, the prefix all keys share */
};

/* write-batch emit reduction (one block of u64 words, vector atomics).  Of
 * every batch path's block the words in *_MIN_MASK fold with min and start at
 * ~0, those in *_MAX_MASK with max, the rest are sums (kernels.hip red_init,
 * red_fold). */
enum {
    WBR_KMIN = 0, WBR_KMAX, WBR_VMIN, WBR_VMAX, WBR_PVMIN, WBR_PVMAX, WBR_PUTS, WBR_WORDS
};
#define WBR_MIN_MASK (1u << WBR_KMIN | 1u << WBR_VMIN | 1u << WBR_PVMIN)
#define WBR_MAX_MASK (1u << WBR_KMAX | 1u << WBR_VMAX | 1u << WBR_PVMAX)

struct DevRun;

/* incr batch (rrdb_incr_batch).  The ops of one key form a segment of the
 * sorted batch.  A segment of up to INCR_LANE_MAX ops is walked by one lane;
 * a longer one (a hot counter) gets a whole wave.  Env "engine.incr_lane_max"
 * overrides it per handle (tools/bench_incr_batch.py sweeps it). */
#define INCR_LANE_MAX 32

/* incr-batch reduction (one block of u64 words, vector atomics) */
enum {
    IR_NSEG = 0, IR_APPLIED, IR_FPARSE, IR_FRANGE, IR_NOUT, IR_KBYTES, IR_VBYTES,
    IR_KMIN, IR_KMAX, IR_VMIN, IR_VMAX, IR_WORDS
};
#define IR_MIN_MASK (1u << IR_KMIN | 1u << IR_VMIN)
#define IR_MAX_MASK (1u << IR_KMAX | 1u << IR_VMAX)

#define INCR_NO_OP 0xFFFFFFFFu
/* errors[i] of a failed op: RRDB_INVALID_ARGUMENT (engine.cpp asserts the two agree) */
#define INCR_ERR_INVALID 4

/* everything the chain and emit kernels of rrdb_incr_batch share, by value */
struct IncrArgs {
    WbKeys k;              /* the uploaded keys, op order                       */
    uint64_t n;            /* ops                                               */
    const uint32_t *ix;    /* [n] sorted position -> op (key asc, op desc)      */
    const uint64_t *seg_start; /* [n_seg + 1] sorted position of each segment  */
    const int64_t *inc;    /* [n] op order                                      */
    const int32_t *dir;    /* [n] expire directive, op order                    */
    /* the lookup of every op's key against the runs (launch_get), op order;
     * status null = the handle has no run, every base is absent */
    const int32_t *status;
    const uint64_t *hit;
    const uint32_t *expire;
    const DevRun *runs;
    uint32_t data_version, epoch_now, default_ttl, lane_max;
    /* per op, op order */
    int64_t *new_val;
    int32_t *err;
    uint64_t *ok;          /* 1 = the op wrote                                  */
    /* per segment */
    int64_t *seg_val;      /* value after the last successful op                */
    uint32_t *seg_exp;     /* its stored expire                                 */
    uint32_t *seg_last;    /* that op, INCR_NO_OP when none succeeded           */
    uint64_t *seg_has, *seg_ksz, *seg_vsz;
    unsigned long long *red; /* IR_* */
};

/* timetag batch (rrdb_write_batch_timetag).  Segments as in the incr batch; a
 * segment of up to WBT_LANE_MAX ops is walked by one lane, a longer one gets a
 * wave.  Env "engine.wbt_lane_max" overrides it per handle
 * (tools/bench_timetag_batch.py sweeps it). */
#define WBT_LANE_MAX 32

/* timetag-batch reduction (one block of u64 words, vector atomics).  TR_NSEG
 * is IR_NSEG: the segment kernel is the incr batch's. */
enum {
    TR_NSEG = 0, TR_APPLIED, TR_IGNORED, TR_NOUT, TR_PUTS, TR_KBYTES, TR_VBYTES,
    TR_KMIN, TR_KMAX, TR_VMIN, TR_VMAX, TR_PVMIN, TR_PVMAX, TR_WORDS
};
static_assert(TR_NSEG == IR_NSEG, "k_incr_segs writes the segment count of both paths");
#define TR_MIN_MASK (1u << TR_KMIN | 1u << TR_VMIN | 1u << TR_PVMIN)
#define TR_MAX_MASK (1u << TR_KMAX | 1u << TR_VMAX | 1u << TR_PVMAX)

#define WBT_NO_OP 0xFFFFFFFFu

/* everything the walk and scatter kernels of rrdb_write_batch_timetag share,
 * by value */
struct TtArgs {
    WbKeys k;              /* the uploaded keys, op order                       */
    uint64_t n;            /* ops                                               */
    const uint32_t *ix;    /* [n] sorted position -> op (key asc, op desc)      */
    const uint64_t *seg_start; /* [n_seg + 1] sorted position of each segment  */
    const uint8_t *flags;  /* [n] TT_OP_* (tt_verify.h), op order               */
    const uint64_t *tt;    /* [n] timetags, op order                            */
    const uint8_t *svals;  /* staged values (wb_stage.h), op order              */
    const uint64_t *svoff; /* [n+1]                                             */
    /* the lookup of every op's key against the runs (launch_get), op order;
     * status null = no lookup was made, every base is dead */
    const int32_t *status;
    const uint64_t *hit;
    const DevRun *runs;
    uint32_t data_version, lane_max;
    uint8_t *applied;      /* [n] op order, 1 = the op's write took effect      */
    /* per segment */
    uint32_t *seg_last;    /* the newest applied op, WBT_NO_OP when none        */
    uint64_t *seg_has, *seg_ksz, *seg_vsz;
    unsigned long long *red; /* TR_* */
};

/* cas batch (rrdb_check_and_mutate_batch) reduction (one block of u64 words,
 * vector atomics).  CR_NGRP is the number of hashkey groups; CR_PASSED ..
 * CR_RETBYTES come from the walk, the rest from the output rows. */
enum {
    CR_NGRP = 0, CR_PASSED, CR_FCHECK, CR_FINVALID, CR_MALFORMED, CR_APPLIED, CR_RETBYTES,
    CR_NOUT, CR_PUTS, CR_KBYTES, CR_VBYTES, CR_KMIN, CR_KMAX, CR_VMIN, CR_VMAX, CR_PVMIN,
    CR_PVMAX, CR_WORDS
};
#define CR_MIN_MASK (1u << CR_KMIN | 1u << CR_VMIN | 1u << CR_PVMIN)
#define CR_MAX_MASK (1u << CR_KMAX | 1u << CR_VMAX | 1u << CR_PVMAX)

#define CAS_NONE 0xFFFFFFFFu
/* errors[i]: RRDB_INVALID_ARGUMENT / RRDB_TRY_AGAIN (engine.cpp asserts they agree) */
#define CAS_ERR_INVALID 4
#define CAS_ERR_TRY_AGAIN 13

/* everything the walk, row and emit kernels of rrdb_check_and_mutate_batch
 * share, by value.  "entry order" is the staged ordinal (cas_stage.h), a
 * "position" is an index into the sorted entries (key asc, ordinal desc). */
struct CasArgs {
    WbKeys k;               /* the staged entry keys, entry order               */
    uint64_t n, E;          /* ops, entries                                      */
    const uint32_t *ix;     /* [E] position -> entry                             */
    const uint32_t *pos;    /* [E] entry -> position                             */
    const uint8_t *khead;   /* [E] 1 = the position starts a full key            */
    const uint8_t *svals;   /* staged values, entry order                        */
    const uint64_t *svoff;  /* [E+1]                                             */
    const uint8_t *kind;    /* [E] CAS_ENT_*                                     */
    const uint8_t *op_flags;  /* [n] CAS_OP_*                                    */
    const int32_t *ctype;   /* [n]                                               */
    const uint8_t *opd;     /* check operands                                    */
    const uint64_t *opoff;  /* [n+1]                                             */
    const uint64_t *moff;   /* [n+1] mut_offs                                    */
    const uint32_t *ops;    /* [n] ops by (hashkey group asc, op asc)            */
    const uint64_t *seg_start; /* [n_grp+1] into ops                             */
    /* the lookup of every check key against the runs (launch_get), op order;
     * status null = the handle has no run, every base is absent */
    const int32_t *status;
    const uint64_t *hit;
    const DevRun *runs;
    uint32_t data_version, epoch_now;
    /* eff[q]: position of the newest applied mutation at or older than q
     * within q's key group, CAS_NONE when there is none */
    uint32_t *eff;
    uint64_t *applied;      /* [E] entry order, 1 = an applied mutation          */
    /* per op, op order */
    int32_t *err;
    uint8_t *exist;
    uint64_t *cv_src, *cv_len; /* the returned check value (len 0 = none)        */
    unsigned long long *red;   /* CR_* */
};

/* device-visible descriptor of one sorted run */
struct DevRun {
    const uint8_t *keys;
    const uint64_t *koff; /* n+1 */
    const uint8_t *vals;
    const uint64_t *voff; /* n+1 */
    const uint64_t *sk;   /* (seq<<1)|kind */
    uint64_t n;
    /* blocked bloom filter over full keys (§8(f)3; the reference's 10-bit
     * FullFilter equivalent, pegasus_server_impl_init.cpp:816-841): 64B
     * blocks, 6 probe bits; null = no filter (search every run). */
    const uint64_t *bloom;
    uint64_t bloom_blocks;
    /* all keys in the run share this length (0 = variable): searches then
     * compute key addresses directly instead of loading offset pairs */
    uint32_t fixed_klen;
    /* every key in a sorted run shares the lcp of its first and last key;
     * searches skip these leading bytes (multiple of 8, <=16) after one
     * per-call check that the query shares them too */
    uint32_t pfx_skip;
    /* exact (unfloored) shared-prefix length, capped at 32.  When the run is
     * fixed-stride and lcp_exact >= fixed_klen-8, the varying suffix fits one
     * u64 and probes compare a single big-endian word at key[klen-8..klen) */
    uint32_t lcp_exact;
    /* packed big-endian tail words (key[klen-8..klen) bswapped), built at run
     * creation when the single-word probe mode is eligible: 8B-strided probe
     * loads instead of klen-strided ones (null when ineligible) */
    const uint64_t *tails;
    /* hashkey-PREFIX blocked bloom (the reference's prefix-extractor bloom,
     * pegasus_server_impl_init.cpp:816-841 + hashkey_transform.h:40-54):
     * hashed over key[0 .. 2+hklen); prefix-scoped reads (multi_get, prefix
     * scans, sortkey_count) skip runs that cannot contain the hashkey. */
    const uint64_t *pfx_bloom;
    uint64_t pfx_bloom_blocks;
    /* per-record disposition column, built at run creation:
     * (expire_ts << 32) | kind.  Compaction-filter / scan-state evaluation
     * reads ONE coalescable 8B word instead of the sk word + voff pair + the
     * dependent 12B value-header parse (that gather chain dominated the
     * fused rank kernel).  Null only for transient descriptors that never
     * reach disposition (e.g. bloom builds). */
    const uint64_t *meta;
    /* all values in the run share this encoded length (0 = variable) */
    uint32_t fixed_vlen;
};

/* flattened user compaction rules/ops (device-resident)
 * mirrors compaction_filter_rule.{h,cpp} / compaction_operation.{h,cpp} */
enum { DFR_HASHKEY = 0, DFR_SORTKEY = 1, DFR_TTL_RANGE = 2 };
enum { DSM_ANYWHERE = 0, DSM_PREFIX = 1, DSM_POSTFIX = 2, DSM_INVALID = 3 };
enum { DOP_UPDATE_TTL = 0, DOP_DELETE = 1 };
enum { DUT_FROM_NOW = 0, DUT_FROM_CURRENT = 1, DUT_TIMESTAMP = 2, DUT_INVALID = 3 };

struct DevRule {
    int32_t type;       /* DFR_* */
    int32_t match_type; /* DSM_* (pattern rules) */
    uint32_t start_ttl, stop_ttl;
    uint32_t pat_off, pat_len; /* into pattern blob */
};

struct DevOp {
    int32_t type;    /* DOP_* */
    int32_t ut_type; /* DUT_* */
    uint32_t ut_value;
    int32_t rule_off, n_rules;
};

/* per-record scan/merge states (match the reference's range_iteration_state,
 * pegasus_server_impl.h) */
enum {
    ST_NORMAL = 0,
    ST_EXPIRED = 1,
    ST_FILTERED = 2,
    ST_HASH_INVALID = 3,
};

/* scan/filter parameter block passed to kernels by value */
struct ScanParams {
    uint32_t epoch_now;
    uint32_t data_version; /* value header: v0=4B, v1=12B, v2=13B */
    int32_t pidx;
    int32_t partition_version;
    uint8_t validate_hash;      /* engine-level env && request flag */
    int32_t hk_ft, sk_ft;       /* filter types (0..3) */
    const uint8_t *hk_pat;      /* device */
    uint64_t hk_pat_len;
    const uint8_t *sk_pat;
    uint64_t sk_pat_len;
    uint8_t no_value;
    uint64_t hash_key_skip;     /* multi_get: bytes of [len][hashkey] prefix to
                                   strip from emitted keys (0 for scan) */
};

struct CompactParams {
    uint32_t epoch_now;
    uint32_t data_version;
    uint32_t default_ttl;
    int32_t pidx;
    int32_t partition_version;
    uint8_t validate_hash;
    const DevOp *ops;     /* device */
    int32_t n_ops;
    const DevRule *rules; /* device */
    const uint8_t *pats;  /* device pattern blob */
    /* 1 = no older run lies below the merged window (the full pass): dropped
     * records vanish.  0 = window (minor) pass over runs [first>0, ..): a
     * tombstone is kept verbatim and a PUT the filter removes is converted
     * into a tombstone (changed[] == CH_TOMBSTONE), so the older version in
     * a run outside the window stays hidden. */
    uint8_t bottommost;
};

/* changed[] values written by the compaction rank kernels */
enum { CH_NONE = 0, CH_REWRITE = 1, CH_TOMBSTONE = 2 };


/* fused small-multi_get argument block (one-launch YCSB-E path) */
#define MG_MAX_ROWS 4096
#define MG_SCRATCH_BYTES (1 << 20)
struct MgFusedArgs {
    const uint8_t *start; /* full rocksdb keys (device) */
    uint64_t start_len;
    const uint8_t *stop;
    uint64_t stop_len;
    uint8_t start_inclusive, stop_inclusive, reverse, no_value;
    uint32_t max_kv_count;
    uint32_t max_iteration_count;
    int64_t max_iteration_size;
    int32_t sk_ft;
    const uint8_t *sk_pat;
    uint64_t sk_pat_len;
    uint32_t epoch_now;
    uint32_t data_version;
    uint64_t hash_key_skip;
    /* outputs: [4] hdr = n_rows(-1 fallback), complete, kbytes, vbytes.
     * out_blob layout (one D2H): [koff (n+1)*8][voff (n+1)*8][keys][vals] */
    int64_t *out_hdr;
    uint8_t *out_blob; /* MG_BLOB_BYTES */
};
#define MG_BLOB_BYTES (2 * MG_SCRATCH_BYTES + 2 * (MG_MAX_ROWS + 1) * 8)

/* graph-captured serving lane: the per-call request is ONE pinned H2D of
 * [MgGraphHdr][start][stop][pattern]; the captured graph replays
 * H2D -> kernel -> D2H as a single launch (hipGraph), cutting the 3-4
 * submission round-trips of the small-op path */
#define MG_GRAPH_IN 4096
struct MgGraphHdr {
    uint32_t start_len, stop_len, sk_pat_len;
    uint8_t start_inclusive, stop_inclusive, reverse, no_value;
    uint32_t max_kv_count, max_iteration_count;
    int64_t max_iteration_size;
    int32_t sk_ft;
    uint32_t epoch_now, data_version;
    uint64_t hash_key_skip;
};

/* persistent serving kernel mailbox (pinned host memory).  Host writes the
 * request slice then release-stores req_seq; the resident 1-workgroup
 * kernel acquire-polls it, runs the fused multi_get and release-stores
 * done_seq after writing the response prefix.  The kernel ALWAYS exits
 * within MG_SRV_IDLE_MS of the last request (or on quit), so device-wide
 * synchronization can stall at most that long and can never hang. */
/* small: a resident kernel occupies one of the few HW queues, and
 * null-stream / device-wide syncs and co-scheduled streams can stall until
 * it exits — 2ms bounds that while call rates above ~1kHz keep it warm */
#define MG_SRV_IDLE_MS 2
struct MgMailbox {
    alignas(64) uint64_t req_seq;
    alignas(64) uint64_t done_seq;
    alignas(64) uint32_t quit;
    alignas(64) uint32_t alive; /* 1 while the kernel loop runs, 0 on exit */
    alignas(64) uint8_t req[MG_GRAPH_IN];
    alignas(64) uint8_t resp[32 + (16 << 10)];
};

/* compact per-record disposition written by the filter kernel */
struct CompactStatsDev {
    unsigned long long expired, filtered, tombstones, shadowed, output_records;
};

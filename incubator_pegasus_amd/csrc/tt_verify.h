/* tt_verify.h — the conflict rule of rrdb_write_batch_timetag: what the
 * reference's rocksdb_wrapper::write_batch_put_ctx (rocksdb_wrapper.cpp:129-183)
 * and write_batch_delete (:221-239) do to one key, op after op.  No HIP call
 * and no engine type in here.  TT_HD makes every function host code and device
 * code at once: kernels.hip calls tt_step from the walk kernels, engine.cpp
 * calls tt_op_flags while it stages the batch, and tools/tt_verify_check.cpp
 * runs the very same functions on the CPU against a std::map restatement under
 * the address and undefined-behaviour sanitizers.
 *
 * The state of a key is what a read of it would find: dead (absent, a
 * tombstone, or a PUT whose stored expire is past), or live with the timetag
 * of the stored record.  The timetag is an opaque unsigned 64-bit number
 * (generate_timetag: timestamp << 8 | cluster_id << 1 | deleted); it is only
 * ever compared.
 *   DELETE:           applied, the key is dead.
 *   PUT, verified:    ignored iff the key is live and its timetag >= the op's;
 *                     the state stays.  Verification exists from data version 1
 *                     on: version 0 stores no timetag and verifies nothing.
 *   any other PUT:    applied.
 *   an applied PUT:   the key is live with the op's timetag, unless the expire
 *                     the op stores is already past: then it is dead.
 */
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TT_HD __host__ __device__
#else
#define TT_HD
#endif

/* an op, folded to what the rule looks at */
enum {
    TT_OP_DELETE = 1, /* else a PUT                                        */
    TT_OP_VERIFY = 2, /* a PUT that is checked against the stored timetag  */
    TT_OP_PAST = 4    /* a PUT whose stored expire is > 0 && <= epoch_now  */
};

struct TtState {
    uint32_t live;
    uint64_t timetag; /* meaningful when live */
};

/* the expire a PUT stores: rrdb_put's write-time default_ttl */
TT_HD static inline uint32_t tt_stored_expire(uint32_t expire_ts, uint32_t default_ttl,
                                              uint32_t epoch_now)
{
    return (expire_ts == 0 && default_ttl != 0) ? epoch_now + default_ttl : expire_ts;
}

/* kind: 0 PUT / 1 DELETE.  stored_expire: tt_stored_expire() of a PUT. */
TT_HD static inline uint8_t tt_op_flags(uint8_t kind, bool verify, uint32_t stored_expire,
                                        uint32_t epoch_now, uint32_t data_version)
{
    if (kind != 0)
        return TT_OP_DELETE;
    uint8_t f = 0;
    if (verify && data_version >= 1)
        f |= TT_OP_VERIFY;
    if (stored_expire > 0 && stored_expire <= epoch_now)
        f |= TT_OP_PAST;
    return f;
}

/* one op on one key: returns whether it is applied and moves the state */
TT_HD static inline bool tt_step(TtState *s, uint8_t flags, uint64_t timetag)
{
    if (flags & TT_OP_DELETE) {
        s->live = 0;
        s->timetag = 0;
        return true;
    }
    if ((flags & TT_OP_VERIFY) && s->live && s->timetag >= timetag)
        return false;
    s->live = (flags & TT_OP_PAST) ? 0u : 1u;
    s->timetag = s->live ? timetag : 0;
    return true;
}

/* the wave form of the same rule, valid for a chain without a TT_OP_PAST op
 * (every applied PUT is then live).  An element is (reset, present, max): a
 * DELETE is (1, 0, 0), an unverified PUT (1, 1, t), a verified PUT (0, 1, t).
 * combine(a, b), a the older: b if b resets, else (a.reset, a.present |
 * b.present, max).  With the base state in front, the combination of
 * everything older than op j is the state in front of j: ignored PUTs never
 * exceed the maximum, so they may stand in it.  rp packs reset << 1 | present;
 * max is 0 when not present. */
struct TtScan {
    uint32_t rp;
    uint64_t max;
};

TT_HD static inline TtScan tt_scan_elem(uint8_t flags, uint64_t timetag)
{
    if (flags & TT_OP_DELETE)
        return TtScan{2u, 0};
    return TtScan{(flags & TT_OP_VERIFY) ? 1u : 3u, timetag};
}

TT_HD static inline TtScan tt_scan_combine(TtScan a, TtScan b)
{
    if (b.rp & 2u)
        return b;
    return TtScan{a.rp | b.rp, a.max > b.max ? a.max : b.max};
}

/* op (flags, timetag) with `before` = the combination of everything older */
TT_HD static inline bool tt_scan_applied(TtScan before, uint8_t flags, uint64_t timetag)
{
    if ((flags & TT_OP_DELETE) || !(flags & TT_OP_VERIFY))
        return true;
    return !(before.rp & 1u) || timetag > before.max;
}

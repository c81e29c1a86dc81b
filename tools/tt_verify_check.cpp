/* tt_verify_check.cpp — stand-alone CPU check of rrdb_write_batch_timetag's
 * rule and host half (incubator_pegasus_amd/csrc/tt_verify.h: the per-key
 * state machine and its scan form; wb_stage.h: wb_stage_values_tt).  The walk
 * kernels compile the same tt_verify.h, so what holds here holds there.  The
 * program checks
 *   - tt_step, op by op over seeded chains, against a std::map restatement of
 *     write_batch_put_ctx / write_batch_delete that keeps the stored record
 *     (expire, timetag) per key and reads it back before every verified PUT;
 *   - the scan form (tt_scan_elem / tt_scan_combine / tt_scan_applied) against
 *     tt_step on every chain without a past-expire PUT, folded left to right
 *     and also in blocks of 64 with a carried element, as the wave does it;
 *   - wb_stage_values_tt over valid batches from exact-size heap buffers: the
 *     header bytes, the flags, and null against non-null timetags,
 * and is meant to run under the address and undefined-behaviour sanitizers:
 *
 *   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       tools/tt_verify_check.cpp -o bin/tt_verify_check && bin/tt_verify_check
 *
 * No HIP, no GPU, nothing loaded into another process.  Exit status 0 and a
 * final "tt_verify_check OK" line mean every expectation held. */
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../incubator_pegasus_amd/csrc/wb_stage.h"

namespace {

int g_fail = 0;
#define EXPECT(cond)                                                                               \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                        \
            g_fail++;                                                                              \
        }                                                                                          \
    } while (0)

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd()
{
    g_rng += 0x9E3779B97F4A7C15ull;
    uint64_t z = g_rng;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Op {
    int key;
    uint8_t kind;
    bool verify;
    uint32_t expire;
    uint64_t timetag;
};

/* the stored record of a key, as the reference's db holds it */
struct Rec {
    bool tombstone;
    uint32_t expire;
    uint64_t timetag;
};

/* write_batch_put_ctx / write_batch_delete, one op, on the map */
bool ref_apply(std::map<int, Rec> &db, const Op &o, uint32_t now, uint32_t dv, uint32_t default_ttl)
{
    if (o.kind != 0) {
        db[o.key] = Rec{true, 0, 0};
        return true;
    }
    if (o.verify && dv >= 1) {
        auto it = db.find(o.key);
        const bool found = it != db.end() && !it->second.tombstone &&
                           !(it->second.expire > 0 && it->second.expire <= now);
        if (found && it->second.timetag >= o.timetag)
            return false;
    }
    uint32_t e = o.expire;
    if (e == 0 && default_ttl != 0)
        e = now + default_ttl;
    db[o.key] = Rec{false, e, dv >= 1 ? o.timetag : 0};
    return true;
}

void check_rule(uint32_t dv, uint32_t default_ttl, bool with_past)
{
    const uint32_t now = 100000;
    for (int round = 0; round < 300; round++) {
        const int n_keys = 1 + (int)(rnd() % 6);
        const int n_ops = 1 + (int)(rnd() % 400);
        std::map<int, Rec> db;
        std::map<int, TtState> st;
        /* bases: absent, tombstone, expired, live */
        for (int k = 0; k < n_keys; k++) {
            const int what = (int)(rnd() % 4);
            TtState s{0, 0};
            if (what == 1)
                db[k] = Rec{true, 0, 0};
            if (what == 2)
                db[k] = Rec{false, now - 5, rnd() % 50};
            if (what == 3) {
                const uint64_t t = dv >= 1 ? rnd() % 50 : 0;
                db[k] = Rec{false, (rnd() & 1) ? 0u : now + 50, t};
                s = TtState{1, t};
            }
            st[k] = s;
        }
        std::map<int, std::vector<Op>> chains;
        std::map<int, std::vector<bool>> got;
        std::map<int, TtState> base = st;
        for (int i = 0; i < n_ops; i++) {
            Op o;
            o.key = (int)(rnd() % n_keys);
            const int w = (int)(rnd() % 10);
            o.kind = w < 2 ? 1 : 0;
            o.verify = w >= 4;
            o.expire = 0;
            if (rnd() % 5 == 0)
                o.expire = now + 500;
            if (with_past && rnd() % 9 == 0)
                o.expire = now - (uint32_t)(rnd() % 3);
            o.timetag = (rnd() % 7 == 0) ? ~0ull - rnd() % 3 : rnd() % 60;
            const bool want = ref_apply(db, o, now, dv, default_ttl);
            const uint32_t se = o.kind ? 0 : tt_stored_expire(o.expire, default_ttl, now);
            const uint8_t f = tt_op_flags(o.kind, o.verify, se, now, dv);
            const bool ap = tt_step(&st[o.key], f, o.timetag);
            EXPECT(ap == want);
            /* the state is what a read of the map finds */
            auto it = db.find(o.key);
            const bool live = it != db.end() && !it->second.tombstone &&
                              !(it->second.expire > 0 && it->second.expire <= now);
            EXPECT((st[o.key].live != 0) == live);
            if (live && dv >= 1)
                EXPECT(st[o.key].timetag == it->second.timetag);
            chains[o.key].push_back(o);
            got[o.key].push_back(ap);
        }
        if (with_past || (default_ttl != 0 && now + default_ttl <= now))
            continue;
        /* the scan form: folded op by op, and in strides of 64 with a carry */
        for (auto &kv : chains) {
            const std::vector<Op> &c = kv.second;
            const TtState b = base[kv.first];
            TtScan acc{b.live ? 1u : 0u, b.live ? b.timetag : 0};
            std::vector<uint8_t> fl(c.size());
            for (size_t j = 0; j < c.size(); j++) {
                fl[j] = tt_op_flags(c[j].kind, c[j].verify,
                                    c[j].kind ? 0 : tt_stored_expire(c[j].expire, default_ttl, now),
                                    now, dv);
                EXPECT(!(fl[j] & TT_OP_PAST));
                EXPECT(tt_scan_applied(acc, fl[j], c[j].timetag) == got[kv.first][j]);
                acc = tt_scan_combine(acc, tt_scan_elem(fl[j], c[j].timetag));
            }
            TtScan carry{b.live ? 1u : 0u, b.live ? b.timetag : 0};
            for (size_t s0 = 0; s0 < c.size(); s0 += 64) {
                /* a Hillis-Steele inclusive scan over the stride, identity padded */
                TtScan v[64];
                for (size_t l = 0; l < 64; l++)
                    v[l] = s0 + l < c.size() ? tt_scan_elem(fl[s0 + l], c[s0 + l].timetag)
                                             : TtScan{0u, 0};
                for (size_t off = 1; off < 64; off <<= 1) {
                    TtScan nv[64];
                    for (size_t l = 0; l < 64; l++)
                        nv[l] = l >= off ? tt_scan_combine(v[l - off], v[l]) : v[l];
                    for (size_t l = 0; l < 64; l++)
                        v[l] = nv[l];
                }
                for (size_t l = 0; l < 64 && s0 + l < c.size(); l++) {
                    const TtScan ex = l ? v[l - 1] : TtScan{0u, 0};
                    const TtScan before = tt_scan_combine(carry, ex);
                    EXPECT(tt_scan_applied(before, fl[s0 + l], c[s0 + l].timetag) ==
                           got[kv.first][s0 + l]);
                }
                carry = tt_scan_combine(carry, v[63]);
            }
        }
    }
}

std::string full_key(const std::string &hk, const std::string &sk)
{
    std::string k;
    k.push_back((char)(hk.size() >> 8));
    k.push_back((char)(hk.size() & 0xFF));
    return k + hk + sk;
}

struct StageOp {
    std::string val;
    uint32_t expire;
    uint8_t kind;
    uint64_t timetag;
    uint8_t verify;
};

/* exact-size heap copies, so that one byte too many is a sanitizer report */
struct Staged {
    std::string vals;
    std::vector<uint64_t> offs;
    std::vector<uint8_t> flags;
};

Staged stage(const std::vector<StageOp> &ops, uint32_t dv, uint32_t default_ttl, uint32_t now,
             bool null_tt, bool null_verify, bool want_flags)
{
    const uint64_t n = ops.size();
    uint64_t vb = 0;
    for (auto &o : ops)
        vb += o.val.size();
    uint8_t *vals = vb ? (uint8_t *)malloc(vb) : nullptr;
    uint64_t *voff = (uint64_t *)malloc((n + 1) * 8);
    uint32_t *expire = (uint32_t *)malloc(n * 4);
    uint8_t *kinds = (uint8_t *)malloc(n), *verify = (uint8_t *)malloc(n);
    uint64_t *tt = (uint64_t *)malloc(n * 8);
    voff[0] = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (!ops[i].val.empty())
            memcpy(vals + voff[i], ops[i].val.data(), ops[i].val.size());
        voff[i + 1] = voff[i] + ops[i].val.size();
        expire[i] = ops[i].expire;
        kinds[i] = ops[i].kind;
        verify[i] = ops[i].verify;
        tt[i] = ops[i].timetag;
    }
    uint64_t bytes = ~0ull;
    EXPECT(wb_staged_bytes(n, voff, kinds, dv, &bytes));
    uint8_t *out = (uint8_t *)malloc(bytes ? bytes : 1);
    uint64_t *ooff = (uint64_t *)malloc((n + 1) * 8);
    uint8_t *oflags = (uint8_t *)malloc(n);
    wb_stage_values_tt(n, vals, voff, expire, kinds, null_tt ? nullptr : tt,
                       null_verify ? nullptr : verify, dv, default_ttl, now, out, ooff,
                       want_flags ? oflags : nullptr);
    EXPECT(ooff[n] == bytes);
    Staged s;
    s.vals.assign((const char *)out, bytes);
    s.offs.assign(ooff, ooff + n + 1);
    if (want_flags)
        s.flags.assign(oflags, oflags + n);
    /* the unchanged entry point writes the same bytes as a null timetags */
    if (null_tt) {
        uint8_t *out2 = (uint8_t *)malloc(bytes ? bytes : 1);
        uint64_t *ooff2 = (uint64_t *)malloc((n + 1) * 8);
        wb_stage_values(n, vals, voff, expire, kinds, dv, default_ttl, now, out2, ooff2);
        EXPECT(std::string((const char *)out2, bytes) == s.vals);
        EXPECT(std::vector<uint64_t>(ooff2, ooff2 + n + 1) == s.offs);
        free(out2);
        free(ooff2);
    }
    free(vals);
    free(voff);
    free(expire);
    free(kinds);
    free(verify);
    free(tt);
    free(out);
    free(ooff);
    free(oflags);
    return s;
}

std::string be(uint64_t v, int bytes)
{
    std::string s;
    for (int j = bytes - 1; j >= 0; j--)
        s.push_back((char)(v >> (8 * j)));
    return s;
}

void check_stage()
{
    const uint32_t now = 1000;
    const std::vector<StageOp> ops = {
        {"v0", 0, 0, 0x0102030405060708ull, 1},  {"", 7, 0, ~0ull, 0},
        {"ignored", 0, 1, 55, 1},                {"v0b", now, 0, 1, 1},
        {std::string(300, 'x'), now + 1, 0, 0, 0}};
    for (uint32_t dv = 0; dv <= 2; dv++) {
        for (uint32_t ttl : {0u, 50u}) {
            const Staged got = stage(ops, dv, ttl, now, false, false, true);
            std::string want;
            std::vector<uint64_t> woffs{0};
            for (auto &o : ops) {
                if (o.kind == 0) {
                    if (dv == 2)
                        want.push_back((char)0x82);
                    want += be(o.expire == 0 && ttl ? now + ttl : o.expire, 4);
                    if (dv >= 1)
                        want += be(o.timetag, 8);
                    want += o.val;
                }
                woffs.push_back(want.size());
            }
            EXPECT(got.vals == want);
            EXPECT(got.offs == woffs);
            const uint8_t v = dv >= 1 ? TT_OP_VERIFY : 0;
            /* expire 7 and expire `now` are past at `now`; now + 1 is not */
            const std::vector<uint8_t> wf = {v, TT_OP_PAST, TT_OP_DELETE,
                                             (uint8_t)(v | TT_OP_PAST), 0};
            EXPECT(got.flags == wf);
            /* null timetags: the timetag bytes are zero, all else the same */
            const Staged zero = stage(ops, dv, ttl, now, true, false, false);
            std::vector<StageOp> z = ops;
            for (auto &o : z)
                o.timetag = 0;
            EXPECT(zero.vals == stage(z, dv, ttl, now, false, false, false).vals);
            EXPECT(zero.offs == got.offs);
            if (dv == 0)
                EXPECT(zero.vals == got.vals);
            else
                EXPECT(zero.vals != got.vals);
            /* null verify: no op is verified */
            const Staged nv = stage(ops, dv, ttl, now, false, true, true);
            for (uint8_t f : nv.flags)
                EXPECT(!(f & TT_OP_VERIFY));
            EXPECT(nv.vals == got.vals);
        }
    }
    /* an all-remove batch stages nothing */
    const std::vector<StageOp> rm = {{"x", 0, 1, 9, 1}, {"y", 0, 1, 9, 0}};
    const Staged r = stage(rm, 1, 0, 0, false, false, true);
    EXPECT(r.vals.empty() && r.offs == std::vector<uint64_t>({0, 0, 0}));
    EXPECT(r.flags == std::vector<uint8_t>({TT_OP_DELETE, TT_OP_DELETE}));
    (void)full_key;
}

/* rocksdb_wrapper_test.cpp:131-205, put_verify_timetag, by hand */
void check_reference_vector()
{
    auto tag = [](uint64_t ts, uint64_t cluster) { return ts << 8 | cluster << 1; };
    TtState s{0, 0};
    EXPECT(tt_step(&s, 0, tag(10, 1)));             /* local write            */
    EXPECT(tt_step(&s, 0, tag(15, 1)));             /* local write, newer     */
    EXPECT(tt_step(&s, TT_OP_VERIFY, tag(15, 2)));  /* remote: cluster breaks the tie */
    EXPECT(!tt_step(&s, TT_OP_VERIFY, tag(15, 2))); /* the same again: ignored */
    EXPECT(s.live && s.timetag == tag(15, 2));
    EXPECT(tt_step(&s, 0, tag(16, 1)));             /* local write            */
    EXPECT(tt_step(&s, 0, tag(16, 1)));             /* again, unverified      */
    /* version 0: verify is folded away */
    EXPECT(tt_op_flags(0, true, 0, 5, 0) == 0);
    EXPECT(tt_op_flags(0, true, 0, 5, 1) == TT_OP_VERIFY);
    EXPECT(tt_op_flags(0, false, 5, 5, 1) == TT_OP_PAST);
    EXPECT(tt_op_flags(0, false, 6, 5, 1) == 0);
    EXPECT(tt_op_flags(1, true, 5, 5, 2) == TT_OP_DELETE);
}

} // namespace

int main()
{
    for (uint32_t dv = 0; dv <= 2; dv++)
        for (uint32_t ttl : {0u, 777u})
            for (bool past : {false, true})
                check_rule(dv, ttl, past);
    check_stage();
    check_reference_vector();
    if (g_fail) {
        fprintf(stderr, "tt_verify_check: %d expectation(s) failed\n", g_fail);
        return 1;
    }
    printf("tt_verify_check OK\n");
    return 0;
}

/* wb_stage_check.cpp — stand-alone CPU check of rrdb_write_batch's host half
 * (incubator_pegasus_amd/csrc/wb_stage.h: validation, stride detection, value
 * staging).  The offsets are untrusted input, so this program feeds the
 * functions every malformed case the entry point rejects plus a few valid
 * batches, from exact-size heap buffers, and is meant to run under the
 * address and undefined-behaviour sanitizers:
 *
 *   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       tools/wb_stage_check.cpp -o bin/wb_stage_check && bin/wb_stage_check
 *
 * No HIP, no GPU, nothing loaded into another process.  Exit status 0 and a
 * final "wb_stage_check OK" line mean every expectation held. */
#include <cstdio>
#include <cstdlib>
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

struct Op {
    std::string key, val;
    uint32_t expire;
    uint8_t kind;
};

/* exact-size heap copies, so that one byte too many is a sanitizer report */
struct Batch {
    uint64_t n = 0;
    uint8_t *keys = nullptr, *vals = nullptr, *kinds = nullptr;
    uint64_t *koff = nullptr, *voff = nullptr;
    uint32_t *expire = nullptr;
    explicit Batch(const std::vector<Op> &ops) : n(ops.size())
    {
        uint64_t kb = 0, vb = 0;
        for (auto &o : ops) {
            kb += o.key.size();
            vb += o.val.size();
        }
        keys = (uint8_t *)malloc(kb ? kb : 1);
        vals = vb ? (uint8_t *)malloc(vb) : nullptr;
        kinds = (uint8_t *)malloc(n ? n : 1);
        expire = (uint32_t *)malloc((n ? n : 1) * 4);
        koff = (uint64_t *)malloc((n + 1) * 8);
        voff = (uint64_t *)malloc((n + 1) * 8);
        koff[0] = voff[0] = 0;
        for (uint64_t i = 0; i < n; i++) {
            memcpy(keys + koff[i], ops[i].key.data(), ops[i].key.size());
            if (!ops[i].val.empty())
                memcpy(vals + voff[i], ops[i].val.data(), ops[i].val.size());
            koff[i + 1] = koff[i] + ops[i].key.size();
            voff[i + 1] = voff[i] + ops[i].val.size();
            kinds[i] = ops[i].kind;
            expire[i] = ops[i].expire;
        }
    }
    ~Batch()
    {
        free(keys);
        free(vals);
        free(kinds);
        free(expire);
        free(koff);
        free(voff);
    }
    bool valid() const { return wb_validate(n, keys, koff, vals, voff, kinds); }
};

std::string full_key(const std::string &hk, const std::string &sk)
{
    std::string k;
    k.push_back((char)(hk.size() >> 8));
    k.push_back((char)(hk.size() & 0xFF));
    return k + hk + sk;
}

std::vector<Op> good_ops()
{
    return {{full_key("hk0", "s"), "v0", 0, 0},        {full_key("hk1", ""), "", 7, 0},
            {full_key("", "sortonly"), "ignored", 0, 1}, {full_key("hk0", "s"), "v0b", 0, 0},
            {full_key("hk2", std::string("s\0\0", 3)), std::string(300, 'x'), 99, 0}};
}

std::string stage(const std::vector<Op> &ops, uint32_t dv, uint32_t default_ttl, uint32_t now,
                  std::vector<uint64_t> *offs, bool null_expire = false)
{
    Batch b(ops);
    EXPECT(b.valid());
    uint64_t bytes = ~0ull;
    EXPECT(wb_staged_bytes(b.n, b.voff, b.kinds, dv, &bytes));
    uint8_t *out = (uint8_t *)malloc(bytes ? bytes : 1);
    uint64_t *ooff = (uint64_t *)malloc((b.n + 1) * 8);
    wb_stage_values(b.n, b.vals, b.voff, null_expire ? nullptr : b.expire, b.kinds, dv,
                    default_ttl, now, out, ooff);
    EXPECT(ooff[b.n] == bytes);
    std::string s((const char *)out, bytes);
    offs->assign(ooff, ooff + b.n + 1);
    free(out);
    free(ooff);
    return s;
}

std::string be32(uint32_t v)
{
    const char c[4] = {(char)(v >> 24), (char)(v >> 16), (char)(v >> 8), (char)v};
    return std::string(c, 4);
}

void check_valid()
{
    const auto ops = good_ops();
    for (uint32_t dv = 0; dv <= 2; dv++) {
        std::vector<uint64_t> offs;
        const std::string got = stage(ops, dv, 0, 1000, &offs);
        std::string want;
        std::vector<uint64_t> woffs{0};
        for (auto &o : ops) {
            if (o.kind == 0) {
                if (dv == 2)
                    want.push_back((char)0x82);
                want += be32(o.expire);
                if (dv >= 1)
                    want += std::string(8, '\0');
                want += o.val;
            }
            woffs.push_back(want.size());
        }
        EXPECT(got == want);
        EXPECT(offs == woffs);
    }
    /* write-time default_ttl: only where expire_ts is 0, and a null expire
     * array means all zero */
    std::vector<uint64_t> offs;
    std::string got = stage(ops, 1, 50, 1000, &offs);
    EXPECT(got.substr(0, 4) == be32(1050));
    EXPECT(got.substr(offs[1], 4) == be32(7));
    got = stage(ops, 1, 0, 1000, &offs, true);
    EXPECT(got.substr(offs[1], 4) == be32(0));

    /* strides */
    std::vector<Op> fixed;
    for (int i = 0; i < 5; i++)
        fixed.push_back({full_key("hk" + std::to_string(i), "s"), "12345678", 0, 0});
    Batch f(fixed);
    EXPECT(f.valid());
    EXPECT(wb_fixed_stride(f.koff, f.n) == 6);
    EXPECT(wb_fixed_stride(f.voff, f.n) == 8);
    Batch g(good_ops());
    EXPECT(wb_fixed_stride(g.koff, g.n) == 0);
    EXPECT(wb_fixed_stride(g.koff, 0) == 0);
    /* an all-remove batch stages nothing and has no stride */
    std::vector<Op> rm = {{full_key("a", "1"), "x", 0, 1}, {full_key("a", "2"), "y", 0, 1}};
    got = stage(rm, 1, 0, 0, &offs);
    EXPECT(got.empty() && offs == std::vector<uint64_t>({0, 0, 0}));
    EXPECT(wb_fixed_stride(offs.data(), 2) == 0);
    /* the longest hashkey the length prefix can carry */
    std::vector<Op> longhk = {{full_key(std::string(0xFFFE, 'h'), "s"), "v", 0, 0}};
    EXPECT(Batch(longhk).valid());
    /* a key that is nothing but the length prefix (empty hashkey, no sortkey) */
    std::vector<Op> bare = {{full_key("", ""), "v", 0, 0}};
    EXPECT(Batch(bare).valid());
}

void check_malformed()
{
    {
        Batch b(good_ops());
        b.koff[0] = 1;
        EXPECT(!b.valid());
    }
    {
        Batch b(good_ops());
        b.koff[3] = b.koff[2] - 1;
        EXPECT(!b.valid());
    }
    {
        /* an offset far past the blob: rejected by the ordering check before
         * any key byte is read through it */
        Batch b(good_ops());
        b.koff[2] = ~0ull;
        EXPECT(!b.valid());
    }
    {
        Batch b(good_ops());
        b.voff[0] = 5;
        EXPECT(!b.valid());
    }
    {
        Batch b(good_ops());
        b.voff[4] = b.voff[3] - 1;
        EXPECT(!b.valid());
    }
    for (const std::string &k : {std::string(), std::string("\0", 1)}) {
        auto ops = good_ops();
        ops[2].key = k; /* shorter than the length prefix */
        EXPECT(!Batch(ops).valid());
        ops = good_ops();
        ops.back().key = k; /* and as the very last bytes of the blob */
        EXPECT(!Batch(ops).valid());
    }
    {
        auto ops = good_ops();
        ops[1].key = std::string("\0\5abc", 5); /* hklen 5 in a 3-byte body */
        EXPECT(!Batch(ops).valid());
    }
    {
        auto ops = good_ops();
        ops[1].key = std::string("\xff\xff", 2) + std::string(0xFFFF, 'h') + "s";
        EXPECT(!Batch(ops).valid()); /* hklen 0xFFFF fits the key, still refused */
    }
    {
        auto ops = good_ops();
        ops[3].kind = 2;
        EXPECT(!Batch(ops).valid());
    }
    {
        Batch b(good_ops());
        EXPECT(!wb_validate(0, b.keys, b.koff, b.vals, b.voff, b.kinds));
        /* too many ops: refused before an array is touched */
        EXPECT(!wb_validate(WB_MAX_OPS + 1, b.keys, b.koff, b.vals, b.voff, b.kinds));
        EXPECT(!wb_validate(b.n, nullptr, b.koff, b.vals, b.voff, b.kinds));
        EXPECT(!wb_validate(b.n, b.keys, nullptr, b.vals, b.voff, b.kinds));
        EXPECT(!wb_validate(b.n, b.keys, b.koff, b.vals, nullptr, b.kinds));
        EXPECT(!wb_validate(b.n, b.keys, b.koff, b.vals, b.voff, nullptr));
        /* PUT bytes announced, no value blob */
        EXPECT(!wb_validate(b.n, b.keys, b.koff, nullptr, b.voff, b.kinds));
    }
    {
        /* value spans whose sum wraps 64 bits */
        const uint64_t voff[3] = {0, ~0ull - 3, ~0ull - 2};
        const uint8_t kinds[2] = {0, 0};
        uint64_t bytes = 0;
        EXPECT(!wb_staged_bytes(2, voff, kinds, 1, &bytes));
    }
}

} // namespace

int main()
{
    check_valid();
    check_malformed();
    if (g_fail) {
        fprintf(stderr, "wb_stage_check: %d expectation(s) failed\n", g_fail);
        return 1;
    }
    printf("wb_stage_check OK\n");
    return 0;
}

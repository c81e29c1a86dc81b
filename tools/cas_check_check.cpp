/* cas_check_check.cpp — stand-alone CPU check of the host-visible halves of
 * rrdb_check_and_mutate_batch: the check function
 * (incubator_pegasus_amd/csrc/cas_check.h) and the validation and staging of
 * the input arrays (cas_stage.h).  The device kernels compile the same check
 * header, so what holds here holds there.
 *   - cas_check runs over every check type x a table of values and operands
 *     and over seeded random pairs, each from exact-size heap buffers, and is
 *     compared with a plain std::string restatement (find, compare, strtoll).
 *   - cas_validate / cas_stage run over valid and malformed batches whose
 *     arrays are exact-size heap copies; the staged columns are compared with
 *     a straightforward rebuild.
 * Meant to run under the address and undefined-behaviour sanitizers:
 *
 *   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       tools/cas_check_check.cpp -o bin/cas_check_check && bin/cas_check_check
 *
 * No HIP, no GPU, nothing loaded into another process.  Exit status 0 and a
 * final "cas_check_check OK" line mean every expectation held. */
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../incubator_pegasus_amd/csrc/cas_check.h"
#include "../incubator_pegasus_amd/csrc/cas_stage.h"

namespace {

int g_fail = 0;

#define EXPECT(c)                                                                                 \
    do {                                                                                          \
        if (!(c)) {                                                                               \
            fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c);                           \
            g_fail++;                                                                             \
        }                                                                                         \
    } while (0)

/* dsn::buf2int64: strtoll(s, &end, 0), whole span consumed, no range error,
 * no C23 binary prefix */
bool libc_parse(const std::string &s, int64_t *out)
{
    size_t i = 0;
    while (i < s.size() && incr_isspace((uint8_t)s[i]))
        i++;
    if (i < s.size() && (s[i] == '+' || s[i] == '-'))
        i++;
    if (s.empty() || (i + 1 < s.size() && s[i] == '0' && (s[i + 1] == 'b' || s[i + 1] == 'B')))
        return false;
    errno = 0;
    char *end = nullptr;
    long long v = strtoll(s.c_str(), &end, 0);
    if ((size_t)(end - s.c_str()) != s.size() || errno != 0)
        return false;
    *out = v;
    return true;
}

/* validate_check, restated over std::string */
bool model_check(int type, bool exist, const std::string &v, const std::string &o, bool *inv)
{
    *inv = false;
    if (type == 0)
        return true;
    if (type == 1)
        return !exist;
    if (type == 2)
        return !exist || v.empty();
    if (type == 3)
        return exist;
    if (type == 4)
        return exist && !v.empty();
    if (!exist)
        return false;
    if (type <= 7) {
        if (o.empty())
            return true;
        if (v.size() < o.size())
            return false;
        if (type == 5)
            return v.find(o) != std::string::npos;
        if (type == 6)
            return v.compare(0, o.size(), o) == 0;
        return v.compare(v.size() - o.size(), o.size(), o) == 0;
    }
    int c;
    if (type <= 12) {
        c = v.compare(o);
        type -= 8;
    } else {
        int64_t a = 0, b = 0;
        if (!libc_parse(v, &a) || !libc_parse(o, &b)) {
            *inv = true;
            return false;
        }
        c = a < b ? -1 : (a > b ? 1 : 0);
        type -= 13;
    }
    switch (type) {
    case 0:
        return c < 0;
    case 1:
        return c <= 0;
    case 2:
        return c == 0;
    case 3:
        return c >= 0;
    default:
        return c > 0;
    }
}

uint8_t *exact(const std::string &s)
{
    /* exact-size copy: one byte read past the span is a sanitizer report */
    uint8_t *p = (uint8_t *)malloc(s.size() ? s.size() : 1);
    memcpy(p, s.data(), s.size());
    return p;
}

void check_one(int type, bool exist, const std::string &v, const std::string &o)
{
    uint8_t *pv = exact(v), *po = exact(o);
    bool wi = false, gi = false;
    const bool w = model_check(type, exist, v, o, &wi);
    const bool g = cas_check(type, exist, exist ? pv : nullptr, exist ? v.size() : 0, po,
                             o.size(), &gi);
    if (w != g || wi != gi) {
        fprintf(stderr, "FAIL check type %d exist %d value %zu bytes operand %zu bytes: "
                        "model %d/%d, cas_check %d/%d\n",
                type, (int)exist, v.size(), o.size(), (int)w, (int)wi, (int)g, (int)gi);
        g_fail++;
    }
    free(pv);
    free(po);
}

template <typename T> T *exact_vec(const std::vector<T> &v)
{
    T *p = (T *)malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (!v.empty())
        memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

std::string full_key(const std::string &hk, const std::string &sk)
{
    std::string k;
    k.push_back((char)(hk.size() >> 8));
    k.push_back((char)hk.size());
    return k + hk + sk;
}

struct Batch {
    std::vector<uint8_t> ck, opd, mk, mv, kinds, ret;
    std::vector<uint64_t> ckoff{0}, opoff{0}, moff{0}, mkoff{0}, mvoff{0};
    std::vector<int32_t> ct;
    std::vector<uint32_t> exp;
    void op(const std::string &key, int type, const std::string &operand, bool r)
    {
        ck.insert(ck.end(), key.begin(), key.end());
        ckoff.push_back(ck.size());
        opd.insert(opd.end(), operand.begin(), operand.end());
        opoff.push_back(opd.size());
        ct.push_back(type);
        ret.push_back(r ? 1 : 0);
        moff.push_back(kinds.size());
    }
    void mut(const std::string &key, int kind, const std::string &val, uint32_t e)
    {
        mk.insert(mk.end(), key.begin(), key.end());
        mkoff.push_back(mk.size());
        mv.insert(mv.end(), val.begin(), val.end());
        mvoff.push_back(mv.size());
        kinds.push_back((uint8_t)kind);
        exp.push_back(e);
        moff.back() = kinds.size();
    }
};

/* validate (and, when valid, stage and compare) one batch from exact copies */
bool run_batch(const Batch &b, uint32_t ver, uint32_t default_ttl, uint32_t now, bool null_exp)
{
    const uint64_t n = b.ct.size();
    uint8_t *ck = exact_vec(b.ck), *opd = exact_vec(b.opd), *mk = exact_vec(b.mk),
            *mv = exact_vec(b.mv), *kinds = exact_vec(b.kinds), *ret = exact_vec(b.ret);
    uint64_t *ckoff = exact_vec(b.ckoff), *opoff = exact_vec(b.opoff), *moff = exact_vec(b.moff),
             *mkoff = exact_vec(b.mkoff), *mvoff = exact_vec(b.mvoff);
    int32_t *ct = exact_vec(b.ct);
    uint32_t *ex = exact_vec(b.exp);
    uint64_t M = ~0ull, sv = 0;
    const bool ok =
        cas_validate(n, ck, ckoff, ct, opd, opoff, moff, mk, mkoff, mv, mvoff, kinds, &M);
    if (ok) {
        EXPECT(M == b.kinds.size());
        EXPECT(wb_staged_bytes(M, mvoff, kinds, ver, &sv));
        const uint64_t E = n + M;
        uint8_t *ek = (uint8_t *)malloc(b.ck.size() + b.mk.size() + 1);
        uint8_t *evl = (uint8_t *)malloc(sv ? sv : 1);
        uint64_t *ekoff = (uint64_t *)malloc((E + 1) * 8), *evoff = (uint64_t *)malloc((E + 1) * 8);
        uint8_t *ekind = (uint8_t *)malloc(E), *fl = (uint8_t *)malloc(n);
        cas_stage(n, ck, ckoff, ct, moff, mk, mkoff, mv, mvoff, null_exp ? nullptr : ex, kinds,
                  ret, ver, default_ttl, now, ek, ekoff, evl, evoff, ekind, fl);
        /* the straightforward rebuild */
        const uint32_t hdr = wb_hdr_len(ver);
        uint64_t e = 0;
        for (uint64_t i = 0; i < n; i++) {
            EXPECT(e == i + b.moff[i]);
            std::string key((const char *)b.ck.data() + b.ckoff[i], b.ckoff[i + 1] - b.ckoff[i]);
            EXPECT(ekoff[e + 1] - ekoff[e] == key.size() &&
                   memcmp(ek + ekoff[e], key.data(), key.size()) == 0);
            EXPECT(ekind[e] == CAS_ENT_CHECK && evoff[e + 1] == evoff[e]);
            e++;
            bool bad = b.moff[i + 1] == b.moff[i] || b.ct[i] < 0 || b.ct[i] > 17;
            for (uint64_t j = b.moff[i]; j < b.moff[i + 1]; j++, e++) {
                std::string mkey((const char *)b.mk.data() + b.mkoff[j],
                                 b.mkoff[j + 1] - b.mkoff[j]);
                EXPECT(ekoff[e + 1] - ekoff[e] == mkey.size() &&
                       memcmp(ek + ekoff[e], mkey.data(), mkey.size()) == 0);
                if (b.kinds[j] > 1)
                    bad = true;
                if (b.kinds[j] != 0) {
                    EXPECT(ekind[e] == CAS_ENT_DELETE && evoff[e + 1] == evoff[e]);
                    continue;
                }
                uint32_t ts = null_exp ? 0 : b.exp[j];
                if (ts == 0 && default_ttl)
                    ts = now + default_ttl;
                std::string want(hdr, '\0');
                const uint32_t off = ver == 2 ? 1 : 0;
                if (ver == 2)
                    want[0] = (char)0x82;
                for (int s = 0; s < 4; s++)
                    want[off + s] = (char)(ts >> (24 - 8 * s));
                want.append((const char *)b.mv.data() + b.mvoff[j], b.mvoff[j + 1] - b.mvoff[j]);
                EXPECT(ekind[e] == CAS_ENT_PUT && evoff[e + 1] - evoff[e] == want.size() &&
                       memcmp(evl + evoff[e], want.data(), want.size()) == 0);
            }
            EXPECT(fl[i] == ((bad ? CAS_OP_MALFORMED : 0) | (b.ret[i] ? CAS_OP_RETURN : 0)));
        }
        EXPECT(e == E && ekoff[E] == b.ck.size() + b.mk.size() && evoff[E] == sv);
        free(ek);
        free(evl);
        free(ekoff);
        free(evoff);
        free(ekind);
        free(fl);
    }
    free(ck);
    free(opd);
    free(mk);
    free(mv);
    free(kinds);
    free(ret);
    free(ckoff);
    free(opoff);
    free(moff);
    free(mkoff);
    free(mvoff);
    free(ct);
    free(ex);
    return ok;
}

Batch good_batch(std::mt19937_64 &rng, int n)
{
    Batch b;
    for (int i = 0; i < n; i++) {
        const std::string hk = rng() % 5 ? "h" + std::to_string(rng() % 7) : "";
        b.op(full_key(hk, "s" + std::to_string(rng() % 4)), (int)(rng() % 20) - 1,
             std::string(rng() % 6, 'o'), rng() & 1);
        const int m = (int)(rng() % 4); /* 0 = a malformed op */
        for (int j = 0; j < m; j++)
            b.mut(full_key(hk, "s" + std::to_string(rng() % 4)), (int)(rng() % 7 == 0 ? 2 : rng() % 2),
                  std::string(rng() % 9, 'v'), rng() % 3 ? 0 : (uint32_t)(rng() % 2000));
    }
    return b;
}

} // namespace

int main()
{
    const std::vector<std::string> words = {
        "", "a", "ab", "abc", "bc", "b", "abd", "abcabc", std::string("a\0b", 3),
        std::string("\0", 1), "\xff", "\xff\x01", "0", "7", "-7", "+7", " 7", "7 ", "007", "0x10",
        "16", "9223372036854775807", "9223372036854775808", "-9223372036854775808", "1e3", "x",
        std::string(300, 'q'), std::string(299, 'q') + "r", "q",
    };
    for (int type = 0; type <= 17; type++)
        for (auto &v : words)
            for (auto &o : words) {
                check_one(type, true, v, o);
                check_one(type, false, v, o);
            }
    std::mt19937_64 rng(20241021);
    const std::string alphabet("ab0159 -+x\0", 11);
    for (int it = 0; it < 200000; it++) {
        std::string v, o;
        for (size_t j = rng() % 9; j > 0; j--)
            v.push_back(alphabet[rng() % alphabet.size()]);
        for (size_t j = rng() % 5; j > 0; j--)
            o.push_back(alphabet[rng() % alphabet.size()]);
        check_one((int)(rng() % 18), rng() % 8 != 0, v, o);
    }

    /* valid batches, malformed ops included, all data versions */
    for (int it = 0; it < 300; it++) {
        Batch b = good_batch(rng, 1 + (int)(rng() % 40));
        EXPECT(run_batch(b, (uint32_t)(it % 3), it % 2 ? 0 : 500, 1000, it % 5 == 0));
    }
    /* every rejection */
    {
        Batch g = good_batch(rng, 8);
        while (g.kinds.size() < 2)
            g = good_batch(rng, 8);
        EXPECT(run_batch(g, 1, 0, 1000, false));
        Batch b = g;
        b.ckoff[0] = 1;
        EXPECT(!run_batch(b, 1, 0, 1000, false));
        b = g;
        b.opoff[1] = b.opoff[2] + 1; /* decreasing */
        EXPECT(!run_batch(b, 1, 0, 1000, false));
        b = g;
        b.moff[0] = 1;
        EXPECT(!run_batch(b, 1, 0, 1000, false));
        b = g;
        b.mkoff[1] = b.mkoff[2] + 1; /* decreasing */
        EXPECT(!run_batch(b, 1, 0, 1000, false));
        b = g;
        b.mvoff[0] = 1;
        EXPECT(!run_batch(b, 1, 0, 1000, false));
        b = g;
        b.ck[0] = 0x7f; /* hklen past the key */
        EXPECT(!run_batch(b, 1, 0, 1000, false));
        b = g;
        b.ck[0] = (uint8_t)0xff;
        b.ck[1] = (uint8_t)0xff;
        EXPECT(!run_batch(b, 1, 0, 1000, false));
        /* a foreign hashkey in a mutation */
        Batch f;
        f.op(full_key("hk", "a"), 0, "", false);
        f.mut(full_key("hx", "a"), 0, "v", 0);
        EXPECT(!run_batch(f, 1, 0, 1000, false));
        Batch f2;
        f2.op(full_key("hk", "a"), 0, "", false);
        f2.mut(full_key("h", "ka"), 0, "v", 0); /* same bytes, another split */
        EXPECT(!run_batch(f2, 1, 0, 1000, false));
        Batch f3;
        f3.op(full_key("hk", "a"), 0, "", false);
        f3.mut(full_key("hk", ""), 1, "", 0);
        EXPECT(run_batch(f3, 2, 0, 1000, true));
        /* a one-byte key */
        Batch s;
        s.op(std::string("\0", 1), 0, "", false);
        EXPECT(!run_batch(s, 1, 0, 1000, false));
        /* the count bounds are refused before any array is read */
        uint64_t M = 0;
        EXPECT(!cas_validate(0x80000000ull, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                             nullptr, nullptr, nullptr, nullptr, nullptr, &M));
        const uint64_t huge[2] = {0, 0x7FFFFFFFull};
        const int32_t one_type[1] = {0};
        EXPECT(!cas_validate(1, nullptr, nullptr, one_type, nullptr, nullptr, huge, nullptr,
                             nullptr, nullptr, nullptr, nullptr, &M));
        /* required arrays */
        const uint64_t z2[2] = {0, 0};
        const uint8_t key3[3] = {0, 0, 'k'};
        const uint64_t k2[2] = {0, 3};
        EXPECT(cas_validate(1, key3, k2, one_type, nullptr, z2, z2, nullptr, z2, nullptr, z2,
                            nullptr, &M) && M == 0);
        EXPECT(!cas_validate(1, key3, k2, nullptr, nullptr, z2, z2, nullptr, z2, nullptr, z2,
                             nullptr, &M));
        EXPECT(!cas_validate(1, nullptr, k2, one_type, nullptr, z2, z2, nullptr, z2, nullptr, z2,
                             nullptr, &M));
        EXPECT(!cas_validate(1, key3, k2, one_type, nullptr, nullptr, z2, nullptr, z2, nullptr, z2,
                             nullptr, &M));
        EXPECT(!cas_validate(1, key3, k2, one_type, nullptr, z2, nullptr, nullptr, z2, nullptr, z2,
                             nullptr, &M));
        EXPECT(!cas_validate(1, key3, k2, one_type, nullptr, z2, z2, nullptr, nullptr, nullptr, z2,
                             nullptr, &M));
        EXPECT(!cas_validate(1, key3, k2, one_type, nullptr, z2, z2, nullptr, z2, nullptr, nullptr,
                             nullptr, &M));
    }

    if (g_fail) {
        fprintf(stderr, "cas_check_check: %d failure(s)\n", g_fail);
        return 1;
    }
    printf("cas_check_check OK\n");
    return 0;
}

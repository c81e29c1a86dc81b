/* engine.cpp — host side of the MI355X rrdb engine (C-ABI in
 * include/rrdb_engine.h).  One handle per partition; all record data lives in
 * HBM; every per-record data-path operation runs in the HIP kernels of
 * kernels.hip.  There is NO CPU fallback: rrdb_open fails without a GPU.
 *
 * Host responsibilities only: run registry, request parsing (incl. the
 * user_specified_compaction JSON of compaction_operation.cpp:160-190),
 * range-bound construction (pegasus_key_schema.h:41-122 byte logic), scan
 * contexts (pegasus_scan_context.h:33-140 equivalent), result marshalling.
 *
 * Reference semantics restated per handler: see the comment on each function
 * and include/rrdb_engine.h.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/rrdb_engine.h"
#include "../../include/rrdb_engine_ext.h"
#include "engine_common.h"
#include "launch.h"
#include "emit_tile.h"
#include "wb_stage.h"
#include "cas_stage.h"

#define HIP_OK(x)                                                                                \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "rrdb-hip fatal: %s at %s:%d\n", hipGetErrorString(e_), __FILE__,      \
                    __LINE__);                                                                     \
            abort();                                                                               \
        }                                                                                          \
    } while (0)

namespace {

/* ================ crc64 table (host build; same construction as
 * reference crc.cpp:236-295, restated) ================ */
uint64_t host_crc64_table[256];
void build_crc64_table()
{
    static const int bits[] = {63, 61, 59, 58, 56, 55, 52, 49, 48, 47, 46, 44, 41, 37, 36, 34,
                               32, 31, 28, 26, 23, 22, 19, 16, 13, 12, 10, 9,  6,  4,  3,  0};
    uint64_t poly = 0;
    for (int b : bits)
        poly |= 1ull << (63 - b);
    for (int i = 0; i < 256; i++) {
        uint64_t k = (uint64_t)i;
        for (int j = 0; j < 8; j++)
            k = (k & 1) ? ((k >> 1) ^ poly) : (k >> 1);
        host_crc64_table[i] = k;
    }
}

/* host crc64 over a buffer (same table); used for checkpoint-file integrity */
static uint64_t host_crc64(const void *p, uint64_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    uint64_t crc = ~0ull;
    for (uint64_t i = 0; i < n; i++)
        crc = host_crc64_table[(uint8_t)(crc ^ b[i])] ^ (crc >> 8);
    return ~crc;
}

/* ================ result arena ================ */
struct Arena {
    std::vector<void *> host_blocks;
    std::vector<void *> dev_ptrs;
    void *alloc(size_t n)
    {
        void *p = malloc(n ? n : 1);
        host_blocks.push_back(p);
        return p;
    }
    ~Arena()
    {
        for (void *p : host_blocks)
            free(p);
        for (void *p : dev_ptrs)
            (void)hipFree(p);
    }
};

Arena *result_init(rrdb_result *r)
{
    memset(r, 0, sizeof(*r));
    Arena *a = new Arena();
    r->_arena = a;
    return a;
}

/* ================ tiny JSON parser (independent of the oracle's) ======== */
struct Json {
    enum Type { NUL, BOOL, NUM, STR, ARR, OBJ } type = NUL;
    bool b = false;
    long long num = 0;
    std::string str;
    std::vector<Json> arr;
    std::vector<std::pair<std::string, Json>> obj;
    const Json *get(const std::string &k) const
    {
        for (auto &kv : obj)
            if (kv.first == k)
                return &kv.second;
        return nullptr;
    }
};

struct JParse {
    const char *s, *e;
    bool ok = true;
    void ws()
    {
        while (s < e && (*s == ' ' || *s == '\t' || *s == '\n' || *s == '\r'))
            s++;
    }
    bool lit(char c)
    {
        ws();
        if (s < e && *s == c) {
            s++;
            return true;
        }
        return false;
    }
    std::string pstr()
    {
        ws();
        std::string out;
        if (s >= e || *s != '"') {
            ok = false;
            return out;
        }
        s++;
        while (s < e && *s != '"') {
            char c = *s++;
            if (c == '\\' && s < e) {
                char esc = *s++;
                switch (esc) {
                case 'n': c = '\n'; break;
                case 't': c = '\t'; break;
                case 'r': c = '\r'; break;
                case 'b': c = '\b'; break;
                case 'f': c = '\f'; break;
                case 'u': {
                    if (e - s < 4) { ok = false; return out; }
                    unsigned v = 0;
                    for (int i = 0; i < 4; i++) {
                        char h = s[i];
                        v <<= 4;
                        if (h >= '0' && h <= '9') v |= h - '0';
                        else if (h >= 'a' && h <= 'f') v |= h - 'a' + 10;
                        else if (h >= 'A' && h <= 'F') v |= h - 'A' + 10;
                        else { ok = false; return out; }
                    }
                    s += 4;
                    c = (char)v;
                    break;
                }
                default: c = esc; break;
                }
            }
            out.push_back(c);
        }
        if (s >= e) {
            ok = false;
            return out;
        }
        s++;
        return out;
    }
    Json value()
    {
        Json j;
        ws();
        if (s >= e) {
            ok = false;
            return j;
        }
        char c = *s;
        if (c == '"') {
            j.type = Json::STR;
            j.str = pstr();
        } else if (c == '{') {
            s++;
            j.type = Json::OBJ;
            ws();
            if (lit('}'))
                return j;
            for (;;) {
                std::string k = pstr();
                if (!ok || !lit(':')) {
                    ok = false;
                    return j;
                }
                j.obj.emplace_back(std::move(k), value());
                if (!ok)
                    return j;
                if (lit('}'))
                    return j;
                if (!lit(',')) {
                    ok = false;
                    return j;
                }
            }
        } else if (c == '[') {
            s++;
            j.type = Json::ARR;
            ws();
            if (lit(']'))
                return j;
            for (;;) {
                j.arr.push_back(value());
                if (!ok)
                    return j;
                if (lit(']'))
                    return j;
                if (!lit(',')) {
                    ok = false;
                    return j;
                }
            }
        } else if (c == 't' && e - s >= 4 && !strncmp(s, "true", 4)) {
            j.type = Json::BOOL;
            j.b = true;
            s += 4;
        } else if (c == 'f' && e - s >= 5 && !strncmp(s, "false", 5)) {
            j.type = Json::BOOL;
            s += 5;
        } else if (c == 'n' && e - s >= 4 && !strncmp(s, "null", 4)) {
            s += 4;
        } else if (c == '-' || (c >= '0' && c <= '9')) {
            j.type = Json::NUM;
            bool neg = c == '-';
            if (neg)
                s++;
            if (s >= e || *s < '0' || *s > '9') {
                ok = false;
                return j;
            }
            long long v = 0;
            while (s < e && *s >= '0' && *s <= '9')
                v = v * 10 + (*s++ - '0');
            j.num = neg ? -v : v;
        } else {
            ok = false;
        }
        return j;
    }
};

bool json_parse(const std::string &text, Json &out)
{
    JParse p{text.c_str(), text.c_str() + text.size()};
    out = p.value();
    return p.ok;
}

/* host-side parsed rules/ops (mirrors compaction_operation.cpp:116-190) */
struct HostRule {
    int type = -1;       /* DFR_* */
    int match_type = DSM_INVALID;
    uint32_t start_ttl = 0, stop_ttl = 0;
    std::string pattern;
};
struct HostOp {
    int type = -1; /* DOP_* */
    int ut_type = DUT_INVALID;
    uint32_t ut_value = 0;
    std::vector<HostRule> rules;
};

int enum_smt(const std::string &s)
{
    if (s == "SMT_MATCH_ANYWHERE") return DSM_ANYWHERE;
    if (s == "SMT_MATCH_PREFIX") return DSM_PREFIX;
    if (s == "SMT_MATCH_POSTFIX") return DSM_POSTFIX;
    return DSM_INVALID;
}
int enum_frt(const std::string &s)
{
    if (s == "FRT_HASHKEY_PATTERN") return DFR_HASHKEY;
    if (s == "FRT_SORTKEY_PATTERN") return DFR_SORTKEY;
    if (s == "FRT_TTL_RANGE") return DFR_TTL_RANGE;
    return -1;
}
int enum_cot(const std::string &s)
{
    if (s == "COT_UPDATE_TTL") return DOP_UPDATE_TTL;
    if (s == "COT_DELETE") return DOP_DELETE;
    return -1;
}
int enum_utot(const std::string &s)
{
    if (s == "UTOT_FROM_NOW") return DUT_FROM_NOW;
    if (s == "UTOT_FROM_CURRENT") return DUT_FROM_CURRENT;
    if (s == "UTOT_TIMESTAMP") return DUT_TIMESTAMP;
    return DUT_INVALID;
}

/* invalid rules skipped; op kept only with >=1 valid rule and valid params
 * (compaction_operation.cpp:160-190; all DEFINE_JSON fields required) */
bool parse_user_ops(const std::string &text, std::vector<HostOp> &out)
{
    out.clear();
    Json root;
    if (!json_parse(text, root) || root.type != Json::OBJ)
        return false;
    const Json *ops = root.get("ops");
    if (!ops || ops->type != Json::ARR)
        return true; /* decodes, but no ops */
    for (const Json &jop : ops->arr) {
        if (jop.type != Json::OBJ)
            return false;
        const Json *jt = jop.get("type");
        const Json *jp = jop.get("params");
        const Json *jr = jop.get("rules");
        /* a missing "params" decodes as "" (json_helper.h:136-143
         * JSON_TRY_DECODE_ENTRY tolerates absent members): delete_key
         * ignores params, update_ttl's own params decode then fails and
         * drops the op */
        if (!jt || jt->type != Json::STR || (jp && jp->type != Json::STR) || !jr ||
            jr->type != Json::ARR)
            continue;
        std::string op_params = jp ? jp->str : std::string();
        HostOp op;
        op.type = enum_cot(jt->str);
        for (const Json &jrule : jr->arr) {
            if (jrule.type != Json::OBJ)
                continue;
            const Json *rt = jrule.get("type");
            const Json *rp = jrule.get("params");
            if (!rt || rt->type != Json::STR || !rp || rp->type != Json::STR)
                continue;
            HostRule rule;
            rule.type = enum_frt(rt->str);
            if (rule.type < 0)
                continue;
            Json rparams;
            if (!json_parse(rp->str, rparams) || rparams.type != Json::OBJ)
                continue;
            if (rule.type == DFR_TTL_RANGE) {
                const Json *a = rparams.get("start_ttl");
                const Json *b = rparams.get("stop_ttl");
                if (!a || a->type != Json::NUM || !b || b->type != Json::NUM)
                    continue;
                rule.start_ttl = (uint32_t)a->num;
                rule.stop_ttl = (uint32_t)b->num;
            } else {
                const Json *pat = rparams.get("pattern");
                const Json *mt = rparams.get("match_type");
                if (!pat || pat->type != Json::STR || !mt || mt->type != Json::STR)
                    continue;
                rule.pattern = pat->str;
                rule.match_type = enum_smt(mt->str);
            }
            op.rules.push_back(std::move(rule));
        }
        if (op.rules.empty() || op.type < 0)
            continue;
        if (op.type == DOP_UPDATE_TTL) {
            Json oparams;
            if (!json_parse(op_params, oparams) || oparams.type != Json::OBJ)
                continue;
            const Json *t = oparams.get("type");
            const Json *v = oparams.get("value");
            /* both fields required: the reference's tolerant decode would
             * accept one missing and read the uninitialized member
             * (compaction_operation.cpp:75 initializes neither) — UB with
             * no semantics to restate, so the op is dropped instead */
            if (!t || t->type != Json::STR || !v || v->type != Json::NUM)
                continue;
            op.ut_type = enum_utot(t->str);
            op.ut_value = (uint32_t)v->num;
        }
        out.push_back(std::move(op));
    }
    return true;
}

/* ================ key byte helpers (pegasus_key_schema.h) ================ */
/* the 2-byte length prefix caps hash keys at 64KiB-1; the reference
 * CHECK_LTs (pegasus_key_schema.h:43) — as a library we reject with
 * kInvalidArgument at the C-ABI boundary instead of aborting */
static inline bool hklen_ok(uint64_t hklen) { return hklen < 0xFFFFull; }
std::string make_key(const uint8_t *hk, uint64_t hklen, const uint8_t *sk, uint64_t sklen)
{
    std::string k;
    k.reserve(2 + hklen + sklen);
    k.push_back((char)(hklen >> 8));
    k.push_back((char)(hklen & 0xFF));
    k.append((const char *)hk, hklen);
    if (sk)
        k.append((const char *)sk, sklen);
    return k;
}
std::string next_blob(std::string k)
{
    size_t p = k.size() - 1;
    while ((uint8_t)k[p] == 0xFF)
        p--;
    k[p] = (char)((uint8_t)k[p] + 1);
    k.resize(p + 1);
    return k;
}
int key_cmp(const std::string &a, const std::string &b)
{
    int c = memcmp(a.data(), b.data(), std::min(a.size(), b.size()));
    if (c)
        return c;
    return a.size() < b.size() ? -1 : (a.size() > b.size() ? 1 : 0);
}

[[maybe_unused]] uint32_t hdr_len(uint32_t ver) { return ver == 0 ? 4u : (ver == 1 ? 12u : 13u); }

/* sorted order => every key in a run shares lcp(first key, last key); device
 * searches skip that many leading bytes (whole 8B words, capped at 16) */
static uint32_t lcp_exact32(const uint8_t *a, uint64_t al, const uint8_t *b, uint64_t bl)
{
    uint32_t m = (uint32_t)std::min<uint64_t>(std::min(al, bl), 32);
    uint32_t i = 0;
    while (i < m && a[i] == b[i])
        i++;
    return i;
}
static void set_pfx(uint32_t lcp, uint32_t *pfx_skip, uint32_t *lcp_exact)
{
    *lcp_exact = lcp;
    *pfx_skip = std::min(lcp, 16u) & ~7u;
}

/* constant key stride lets device searches skip the offset-pair loads */
/* constant encoded-value stride (0 = variable); mirrors detect_fixed_klen */
static uint32_t detect_fixed_vlen(const uint64_t *voff, uint64_t n)
{
    if (n == 0)
        return 0;
    uint64_t s = voff[1] - voff[0];
    if (s == 0 || s > UINT32_MAX)
        return 0;
    for (uint64_t i = 1; i < n; i++)
        if (voff[i + 1] - voff[i] != s)
            return 0;
    return (uint32_t)s;
}

/* constant encoded-value stride over PUT records only (tombstones carry
 * empty values and break the plain stride): the compaction OUTPUT contains
 * only surviving PUTs, so this is the output stride the fixed-emit mode
 * needs even when inputs hold tombstones */
static uint32_t detect_fixed_vlen_put(const uint64_t *voff, const uint64_t *sk, uint64_t n)
{
    uint64_t s = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (sk[i] & 1)
            continue;
        uint64_t d = voff[i + 1] - voff[i];
        if (d == 0 || d > UINT32_MAX)
            return 0;
        if (s == 0)
            s = d;
        else if (d != s)
            return 0;
    }
    return (uint32_t)s;
}

static uint32_t detect_fixed_klen(const uint64_t *koff, uint64_t n)
{
    if (n == 0)
        return 0;
    uint64_t s = koff[1] - koff[0];
    if (s == 0 || s > UINT32_MAX)
        return 0;
    for (uint64_t i = 1; i < n; i++)
        if (koff[i + 1] - koff[i] != s)
            return 0;
    return (uint32_t)s;
}

/* ================ engine ================ */
struct RunBuf {
    uint8_t *keys = nullptr;
    uint64_t *koff = nullptr;
    uint8_t *vals = nullptr;
    uint64_t *voff = nullptr;
    uint64_t *sk = nullptr;
    uint64_t n = 0;
    uint64_t *bloom = nullptr; /* blocked bloom over full keys (may be null) */
    uint64_t bloom_blocks = 0;
    uint32_t fixed_klen = 0; /* nonzero when every key in the run has this length */
    uint32_t pfx_skip = 0;   /* lcp(first,last) floored to 8B words, <=16 */
    uint32_t lcp_exact = 0;  /* exact lcp(first,last), capped at 32 */
    uint64_t *tails = nullptr; /* packed BE tail words (word-probe mode) */
    uint64_t *pfx_bloom = nullptr; /* hashkey-prefix blocked bloom */
    uint64_t pfx_bloom_blocks = 0;
    uint64_t *meta = nullptr;  /* (expire_ts<<32)|kind disposition column */
    uint32_t fixed_vlen = 0;   /* constant encoded-value stride (0=variable) */
    uint32_t fixed_vlen_put = 0; /* constant PUT-value stride (emit output) */
};
/* what a run's allocation does on a full device (HipEngine::col_alloc) */
enum class RunAlloc { Abort, Try, Arena };
/* first and last key of a run, cut to the 32 bytes lcp_exact32 looks at */
struct KeyEnds {
    uint8_t a[32], b[32];
    uint64_t al = 0, bl = 0;
};
/* the stride field `f` when every run of the window shares it, else 0:
 * outputs are verbatim-length copies of inputs, so a shared stride survives */
static uint32_t shared_stride(const RunBuf *wr, int R, uint32_t RunBuf::*f)
{
    for (int r = 1; r < R; r++)
        if (wr[r].*f != wr[0].*f)
            return 0;
    return R ? wr[0].*f : 0;
}

/* build_view's result, a range's visible record ids in key order: a plain device
 * allocation (a parked scan keeps it), move-only, freed on every way out */
struct DevView {
    uint64_t *d = nullptr;
    uint64_t n = 0;
    DevView() = default;
    DevView(uint64_t *d_, uint64_t n_) : d(d_), n(n_) {}
    DevView(DevView &&o) noexcept : d(o.d), n(o.n) { o.d = nullptr, o.n = 0; }
    DevView &operator=(DevView &&o) noexcept
    {
        std::swap(d, o.d), std::swap(n, o.n);
        return *this;
    }
    ~DevView() { if (d) (void)hipFree(d); }
};

/* the phase events of one call; destroyed on every way out of it */
template <int N> struct PhaseEvents {
    hipEvent_t ev[N];
    PhaseEvents()
    {
        for (auto &x : ev)
            HIP_OK(hipEventCreate(&x));
    }
    PhaseEvents(const PhaseEvents &) = delete;
    PhaseEvents &operator=(const PhaseEvents &) = delete;
    ~PhaseEvents()
    {
        for (auto &x : ev)
            (void)hipEventDestroy(x);
    }
    void record(int i, hipStream_t s) { HIP_OK(hipEventRecord(ev[i], s)); }
    /* false (and *out untouched) when either event has not completed */
    bool ms(int i, int j, float *out) const
    {
        return hipEventElapsedTime(out, ev[i], ev[j]) == hipSuccess;
    }
};

/* an exclusive scan's grand total is its last entry plus the last input: both
 * copies, into out[0] and out[1]; the caller adds them after its sync */
static void scan_tail_async(const uint64_t *d_scan, const uint64_t *d_in, uint64_t n,
                            uint64_t out[2], hipStream_t st)
{
    HIP_OK(hipMemcpyAsync(&out[0], d_scan + n - 1, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(&out[1], d_in + n - 1, 8, hipMemcpyDeviceToHost, st));
}

/* group-streaming rank: records of the anchor run per group, as a shift.  A
 * group stages about GRP_TARGET records over all R runs. */
static int grp_shift(int R)
{
    int gs = 4;
    while ((1ull << (gs + 1)) * (uint64_t)R <= GRP_TARGET && gs < 8)
        gs++;
    return gs;
}

struct HipScanCtx {
    int64_t id = 0;
    uint32_t parked_at = 0; /* epoch_now when (re-)parked; 5-min GC */
    DevView view;
    uint64_t cursor = 0;
    int32_t batch_size = -1;
    uint8_t no_value = 0, validate_hash_req = 1, return_expire_ts = 0, only_return_count = 0,
            on_device_out = 0;
    int32_t hk_ft = 0, sk_ft = 0;
    uint8_t *d_hk_pat = nullptr;
    uint64_t hk_pat_len = 0;
    uint8_t *d_sk_pat = nullptr;
    uint64_t sk_pat_len = 0;
    ~HipScanCtx()
    {
        if (d_hk_pat)
            (void)hipFree(d_hk_pat);
        if (d_sk_pat)
            (void)hipFree(d_sk_pat);
    }
};

struct HipEngine {
    int32_t app_id = 0, pidx = 0, partition_version = -1;
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t data_version = 1, default_ttl = 0;
    bool validate_hash = false, manual_compact_disabled = false;
    /* background-compaction tick (rrdb_auto_compact): run-count trigger (env
     * "engine.l0_compaction_trigger", the reference's
     * level0_file_num_compaction_trigger) and the bulk_load usage scenario,
     * which switches the tick off */
    uint32_t l0_trigger = 4;
    bool bulk_load = false;
    /* rrdb_incr_batch: longest segment one lane walks (env
     * "engine.incr_lane_max"); longer ones get a wave */
    uint32_t incr_lane_max = INCR_LANE_MAX;
    /* rrdb_write_batch_timetag: the same threshold for its walk (env
     * "engine.wbt_lane_max") */
    uint32_t wbt_lane_max = WBT_LANE_MAX;
    bool bloom_enabled = true; /* env "rocksdb.filter_type": common(default)|none */
    uint32_t max_iter_count = 1000, mg_max_iter_count = 3000;
    uint64_t mg_max_iter_size = 30ull << 20, iter_time_ms = 30000;
    std::vector<RunBuf> runs;
    DevRun *d_runs = nullptr;
    bool d_runs_dirty = true;
    int ldst_elig_cache = -1; /* -1 unknown; recomputed when the run set changes */
    /* ---- compaction: the pending pass and what outlives it ---- */
    /* One pass, built by compact_begin and consumed by compact_finish
     * (rrdb_manual_compact_begin / _finish split the two).  Device pointers
     * are arena memory under arena_pin until finish; none points into d_runs,
     * so a run appended between begin and finish cannot invalidate the plan. */
    struct CompactPlan {
        bool active = false, trivial = false, keep_inputs = false;
        /* the pass merges runs [first, first+R); bottommost iff first == 0 */
        size_t first = 0;
        int R = 0;
        uint64_t total = 0;
        bool bottommost = true;
        /* the emit the arrays below were built for: engine.emit_mode as begin
         * read it (chunked for a window), so that a set_envs between begin
         * and finish cannot send them to another emit kernel */
        int emit_mode = 2;
        uint32_t fk = 0, fv = 0; /* all-fixed-stride emit (ksz/vsz/kpos skipped) */
        bool no_rewrite = false;  /* changed/new_expire arrays skipped */
        /* the window's DevRun rows, the pass's own copy: run ids in order[]
         * index it */
        DevRun *dr = nullptr;
        uint64_t *d_lo = nullptr, *d_hi = nullptr, *d_wp = nullptr;
        uint64_t *d_order = nullptr, *d_keepw = nullptr;
        uint8_t *d_changed = nullptr;
        uint32_t *d_new_expire = nullptr;
        uint64_t *d_ksz = nullptr, *d_vsz = nullptr;
        uint64_t *d_kpos = nullptr, *d_koffs = nullptr, *d_voffs = nullptr;
        uint64_t *d_tile_base = nullptr; /* all-fixed-stride emit: first output row per tile */
        uint64_t *d_rank_of = nullptr;
        CompactStatsDev *d_stats = nullptr; /* 8 banks, summed by finish */
        rrdb_compact_stats st{};
    } pend;
    /* what outlives a pass: the pinned read-back targets, its events (resolved
     * lazily by phase_ms() so the keep_inputs finish can return without
     * draining the emit) and the kernels it dispatched to
     * (rrdb_last_compact_route: written in rank_pass / emit_pass only) */
    struct CompactKept {
        uint64_t *sizes = nullptr;        /* pinned [6]: output sizes d2h target */
        CompactStatsDev *stats = nullptr; /* pinned [8]: stats d2h target */
        hipEvent_t ev[6] = {};
        bool ev_live = false, have_emit = false;
        rrdb_compact_route route{RRDB_ROUTE_NONE, RRDB_ROUTE_NONE};
        void init()
        {
            if (sizes)
                return;
            HIP_OK(hipHostMalloc((void **)&sizes, 6 * 8));
            HIP_OK(hipHostMalloc((void **)&stats, 8 * sizeof(CompactStatsDev)));
            for (auto &x : ev)
                HIP_OK(hipEventCreate(&x));
        }
    } kept;
    void resolve_phase_events()
    {
        if (!kept.ev_live)
            return;
        kept.ev_live = false;
        float ms;
        HIP_OK(hipEventSynchronize(kept.ev[1]));
        HIP_OK(hipEventElapsedTime(&ms, kept.ev[0], kept.ev[1]));
        phase_ms["compact_rank"] = ms;
        phase_ms["compact_flags"] = 0.0;
        if (kept.have_emit) {
            HIP_OK(hipEventSynchronize(kept.ev[4]));
            HIP_OK(hipEventElapsedTime(&ms, kept.ev[3], kept.ev[4]));
            phase_ms["compact_emit"] = ms;
            HIP_OK(hipEventElapsedTime(&ms, kept.ev[0], kept.ev[4]));
            phase_ms["compact_total"] = ms;
        }
    }
    /* serving-lane staging for the fused multi_get: one pinned H2D of
     * [start|stop|pattern], one pinned D2H of hdr + blob prefix (small-op
     * latency; pageable copies + two syncs dominated the 77us/call path) */
    static constexpr uint64_t MG_IN_CAP = 64 << 10;
    static constexpr uint64_t MG_OUT_PREFIX = 16 << 10;
    uint8_t *mg_hin = nullptr, *mg_din = nullptr, *mg_hout = nullptr;
    uint8_t *mg_dout = nullptr; /* persistent output buffer (graph-stable) */
    hipGraphExec_t mg_graph = nullptr;
    hipStream_t mg_capture_stream = nullptr; /* idle stream used ONLY for
        capture: capturing e->stream while earlier async work (e.g. a pending
        compaction) is in flight aborts inside the ROCm runtime */
    uint64_t mg_graph_gen = ~0ull; /* runs_gen the graph was captured at */
    uint64_t runs_gen = 0;         /* bumped whenever d_runs is rebuilt */
    bool mg_graph_enabled = true;  /* env "engine.mg_graph" */
    void mg_lane_init()
    {
        if (mg_hin)
            return;
        HIP_OK(hipHostMalloc((void **)&mg_hin, MG_IN_CAP));
        HIP_OK(hipMalloc(&mg_din, MG_IN_CAP));
        HIP_OK(hipHostMalloc((void **)&mg_hout, 32 + MG_OUT_PREFIX));
        HIP_OK(hipMalloc(&mg_dout, 32 + MG_BLOB_BYTES));
    }
    /* (re)capture the serving graph: H2D request slice -> fused kernel ->
     * D2H hdr+prefix.  One hipGraphLaunch replaces 3 submissions. */
    bool mg_graph_ready()
    {
        if (!mg_graph_enabled)
            return false;
        /* refresh the device run table FIRST: it bumps runs_gen when the
         * run set changed, and a stale graph would replay against freed
         * run buffers (GPU aperture fault) */
        DevRun *dr = dev_runs();
        if (mg_graph && mg_graph_gen == runs_gen)
            return true;
        if (mg_graph) {
            (void)hipGraphExecDestroy(mg_graph);
            mg_graph = nullptr;
        }
        int R = (int)runs.size();
        if (!mg_capture_stream && hipStreamCreate(&mg_capture_stream) != hipSuccess) {
            mg_graph_enabled = false;
            return false;
        }
        hipStream_t cs = mg_capture_stream;
        hipGraph_t g = nullptr;
        if (hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) != hipSuccess)
            return false;
        bool ok = hipMemcpyAsync(mg_din, mg_hin, MG_GRAPH_IN, hipMemcpyHostToDevice,
                                 cs) == hipSuccess;
        launch_multi_get_graph(dr, R, mg_din, mg_dout, cs);
        ok = ok && hipMemcpyAsync(mg_hout, mg_dout, 32 + MG_OUT_PREFIX,
                                  hipMemcpyDeviceToHost, cs) == hipSuccess;
        if (hipStreamEndCapture(cs, &g) != hipSuccess || !ok || !g) {
            if (g)
                (void)hipGraphDestroy(g);
            mg_graph_enabled = false; /* capture unsupported: stay on the
                                         plain path */
            return false;
        }
        if (hipGraphInstantiate(&mg_graph, g, nullptr, nullptr, 0) != hipSuccess) {
            (void)hipGraphDestroy(g);
            mg_graph_enabled = false;
            return false;
        }
        (void)hipGraphDestroy(g);
        mg_graph_gen = runs_gen;
        return true;
    }

    /* ---- persistent serving kernel (env engine.mg_persist, default on):
     * a resident 1-workgroup kernel polls the pinned mailbox, removing the
     * per-call dispatch floor.  It self-exits within MG_SRV_IDLE_MS of the
     * last request, so device-wide syncs stall at most that long. ---- */
    MgMailbox *mg_mb = nullptr;
    hipStream_t mg_srv_stream = nullptr;
    uint64_t mg_srv_gen = ~0ull; /* runs_gen the resident kernel was launched at */
    uint64_t mg_srv_seq = 0;
    /* 0 = off, 1 = auto (default: engage only after a sustained burst on
     * THIS handle — a resident kernel helps a hot partition but its poll
     * windows tax handles that are merely visited round-robin), 2 = on */
    int mg_persist_mode = 1;
    bool mg_persist_enabled = true; /* false = runtime failure, stay off */
    std::chrono::steady_clock::time_point mg_last_call{};
    uint32_t mg_hot = 0;
    bool mg_persist_wanted()
    {
        if (!mg_persist_enabled || mg_persist_mode == 0)
            return false;
        if (mg_persist_mode == 2)
            return true;
        auto now = std::chrono::steady_clock::now();
        auto us = std::chrono::duration_cast<std::chrono::microseconds>(now - mg_last_call)
                      .count();
        mg_last_call = now;
        if (us < 1000) {
            if (mg_hot < 1000)
                mg_hot++;
        } else {
            mg_hot = 0;
        }
        return mg_hot >= 32;
    }
    void server_quit_sync()
    {
        if (!mg_mb || mg_srv_gen == ~0ull)
            return;
        __atomic_store_n(&mg_mb->quit, 1u, __ATOMIC_RELEASE);
        auto t0 = std::chrono::steady_clock::now();
        while (__atomic_load_n(&mg_mb->alive, __ATOMIC_ACQUIRE)) {
            if (std::chrono::duration_cast<std::chrono::milliseconds>(
                    std::chrono::steady_clock::now() - t0)
                    .count() > 200) {
                /* should be impossible (bounded loop); stop using it */
                mg_persist_enabled = false;
                break;
            }
        }
        (void)hipStreamSynchronize(mg_srv_stream); /* retire the kernel */
        __atomic_store_n(&mg_mb->quit, 0u, __ATOMIC_RELEASE);
        mg_srv_gen = ~0ull;
    }
    bool server_ready()
    {
        if (!mg_persist_enabled)
            return false;
        DevRun *dr = dev_runs(); /* bumps runs_gen when the run set changed */
        if (mg_srv_gen == runs_gen &&
            __atomic_load_n(&mg_mb->alive, __ATOMIC_ACQUIRE))
            return true;
        server_quit_sync();
        mg_lane_init();
        if (!mg_mb) {
            if (hipHostMalloc((void **)&mg_mb, sizeof(MgMailbox)) != hipSuccess) {
                mg_persist_enabled = false;
                return false;
            }
            memset((void *)mg_mb, 0, sizeof(MgMailbox));
        }
        if (!mg_srv_stream &&
            hipStreamCreateWithFlags(&mg_srv_stream, hipStreamNonBlocking) != hipSuccess) {
            mg_persist_enabled = false;
            return false;
        }
        mg_mb->quit = 0;
        mg_mb->alive = 0;
        mg_mb->req_seq = mg_srv_seq;
        mg_mb->done_seq = mg_srv_seq;
        launch_mg_server(dr, (int)runs.size(), mg_mb, mg_dout, mg_srv_stream);
        auto t0 = std::chrono::steady_clock::now();
        while (!__atomic_load_n(&mg_mb->alive, __ATOMIC_ACQUIRE)) {
            if (std::chrono::duration_cast<std::chrono::milliseconds>(
                    std::chrono::steady_clock::now() - t0)
                    .count() > 100) {
                __atomic_store_n(&mg_mb->quit, 1u, __ATOMIC_RELEASE);
                (void)hipStreamSynchronize(mg_srv_stream);
                mg_persist_enabled = false;
                return false;
            }
        }
        mg_srv_gen = runs_gen;
        return true;
    }
    /* pending fused count scan (rrdb_scan_count_begin/finish): buffers are
     * plain hipMallocs so interleaved reads/compactions cannot reclaim them */
    struct PendingScanCount {
        bool active = false, trivial = false;
        int64_t trivial_count = 0;
        CompactStatsDev *d_stats = nullptr;
        uint64_t *d_anch = nullptr, *d_lo = nullptr, *d_hi = nullptr;
        uint8_t *d_start = nullptr; /* pooled request-bytes slab */
        /* pooled capacities: buffers persist across calls, realloc only on
         * growth (8 hipMallocs per begin measurably taxed the 16-partition
         * fan-out on slow-host boxes) */
        uint64_t anch_cap = 0, lo_cap = 0, bytes_cap = 0;
    } pend_scan;
    uint64_t next_seq_floor = 0;
    /* user ops: host + device */
    std::vector<HostOp> host_ops;
    DevOp *d_ops = nullptr;
    DevRule *d_rules = nullptr;
    uint8_t *d_pats = nullptr;
    int n_ops = 0;
    /* write path (§8(f)1): host memtable, newest write per key wins */
    std::map<std::string, std::tuple<std::string /*encoded value*/, uint64_t /*seq*/,
                                     int /*kind*/>> memtable;
    std::unordered_map<int64_t, HipScanCtx *> ctxs;
    int64_t next_ctx_id = 0;
    std::mutex mu;
    std::unordered_map<std::string, double> phase_ms;
    int emit_mode = 2; /* 2 = chunked (default; 2.8 TB/s on the copy probe),
                          0 = rank-major waves, 1 = input-major waves
                          (env "engine.emit_mode": chunked|rank|input) */
    int rank_mode = 4; /* 4 = group-streaming rank (default; anchor-key
                          groups partition the runs disjointly, each staged
                          through LDS exactly once; falls back to mode 0 per
                          compact when runs are not word-probe eligible),
                          3 = r01 windowed LDS-staged tail-word rank,
                          0 = global searches + bound-table narrowing,
                          1 = LDS-staged full-key block rank
                          (env "engine.rank_mode": grp|ldst|global|lds) */
    /* which lane the last rrdb_multi_get took and how the last
       rrdb_multi_get_batch split (rrdb_last_multi_get_lane): written at the
       branches of multi_get_locked / rrdb_multi_get_batch, read by nothing
       else */
    rrdb_multi_get_lane last_mg_lane{};
    /* which rank kernel the last read view was built with
       (rrdb_last_view_route): written at the branches of build_view, read by
       nothing else */
    rrdb_view_route last_view{RRDB_ROUTE_NONE, 0, 0, 0, 0};
    int split_crc_lds = 1; /* rrdb_split classify: crc64 table staged in LDS
                              once per workgroup (1, default) or read from
                              global memory (0) (env "engine.split_crc":
                              lds|global; DESIGN.md §3c has the A/B) */
    int bt_shift = 5;  /* bound-table block = 1<<bt_shift records (env
                          "engine.bt_shift") */
    int grp_blocks = 3584; /* group-rank grid cap (env "engine.grp_blocks");
                              grid-stride beats one-block-per-group by ~24%
                              (workgroup setup/LDS churn) */

    void activate() { HIP_OK(hipSetDevice(device)); }

    /* tail-word rank eligibility (shared by the grp and ldst modes): every
     * run in single-word probe mode with one shared stride and one shared
     * cross-run first-(fk-8)-byte prefix, so tail-word compares decide
     * cross-run order exactly */
    bool word_eligible()
    {
        if (runs.size() < 2)
            return false;
        if (ldst_elig_cache >= 0)
            return ldst_elig_cache != 0;
        ldst_elig_cache = word_eligible_range(0, runs.size()) ? 1 : 0;
        return ldst_elig_cache != 0;
    }
    /* the same test over runs [first, first+n) only (a window compaction
     * ranks just those); never reads or writes the whole-set cache */
    bool word_eligible_range(size_t first, size_t n)
    {
        if (n < 2)
            return false;
        uint32_t fk = runs[first].fixed_klen;
        if (fk < 8)
            return false;
        for (size_t ri = first; ri < first + n; ri++)
            if (!runs[ri].tails || runs[ri].fixed_klen != fk || runs[ri].n == 0)
                return false;
        if (fk > 8) {
            uint8_t p0[32], pi[32];
            uint64_t pl = fk - 8 < 32 ? fk - 8 : 32;
            HIP_OK(hipMemcpy(p0, runs[first].keys, pl, hipMemcpyDeviceToHost));
            for (size_t ri = first + 1; ri < first + n; ri++) {
                HIP_OK(hipMemcpy(pi, runs[ri].keys, pl, hipMemcpyDeviceToHost));
                if (memcmp(p0, pi, pl) != 0)
                    return false;
            }
        }
        return true;
    }
    bool window_word_eligible(size_t first, size_t n)
    {
        return (first == 0 && n == runs.size()) ? word_eligible() : word_eligible_range(first, n);
    }
    bool ldst_eligible(size_t first, size_t n)
    {
        return rank_mode == 3 && window_word_eligible(first, n);
    }
    bool grp_eligible(size_t first, size_t n)
    {
        return rank_mode == 4 && n <= LDST_MAXR && window_word_eligible(first, n);
    }

    void free_run(RunBuf &r)
    {
        (void)hipFree(r.keys);
        (void)hipFree(r.koff);
        (void)hipFree(r.vals);
        (void)hipFree(r.voff);
        (void)hipFree(r.sk);
        if (r.bloom)
            (void)hipFree(r.bloom);
        if (r.tails)
            (void)hipFree(r.tails);
        if (r.pfx_bloom)
            (void)hipFree(r.pfx_bloom);
        if (r.meta)
            (void)hipFree(r.meta);
        r = RunBuf();
    }

    /* ---- run creation: every new run goes through alloc_base (or
     * upload_run, which wraps it), then finish_run, then the run list with
     * runs_changed(); whoever frees a run calls before_run_free() first ---- */

    /* one device buffer of a run.  Abort: a full device ends the process,
     * like every HIP_OK.  Try: false, with the sticky HIP error cleared.
     * Arena: scratch memory, for a run that is dropped with the operation. */
    template <typename T> bool col_alloc(T **p, uint64_t bytes, RunAlloc mode)
    {
        if (mode == RunAlloc::Arena) {
            *p = talloc<T>(bytes);
            return true;
        }
        hipError_t rc = hipMalloc(p, bytes ? bytes : 1);
        if (mode == RunAlloc::Abort)
            HIP_OK(rc);
        if (rc != hipSuccess)
            (void)hipGetLastError();
        return rc == hipSuccess;
    }
    /* the five base columns of an n-record run; false (Try only) leaves
     * nothing allocated */
    bool alloc_base(RunBuf &r, uint64_t n, uint64_t kbytes, uint64_t vbytes, RunAlloc mode)
    {
        r.n = n;
        if (col_alloc(&r.keys, kbytes, mode) && col_alloc(&r.koff, (n + 1) * 8, mode) &&
            col_alloc(&r.vals, vbytes, mode) && col_alloc(&r.voff, (n + 1) * 8, mode) &&
            col_alloc(&r.sk, n * 8, mode))
            return true;
        free_run(r);
        return false;
    }
    /* a validated sorted run arriving from the host: base columns, strides,
     * and its first/last key in *ends for finish_run.  false (Try only) = the
     * device is full and nothing is left allocated. */
    bool upload_run(RunBuf &r, const uint8_t *keys, const uint64_t *koff, const uint8_t *vals,
                    const uint64_t *voff, const uint64_t *sk, uint64_t n, RunAlloc mode,
                    KeyEnds *ends)
    {
        if (!alloc_base(r, n, koff[n], voff[n], mode))
            return false;
        const struct {
            void *dst;
            const void *src;
            uint64_t bytes;
        } cols[5] = {{r.keys, keys, koff[n]},
                     {r.koff, koff, (n + 1) * 8},
                     {r.vals, vals, voff[n]},
                     {r.voff, voff, (n + 1) * 8},
                     {r.sk, sk, n * 8}};
        for (auto &c : cols) {
            if (!c.bytes)
                continue;
            hipError_t rc = hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyHostToDevice);
            if (mode == RunAlloc::Abort)
                HIP_OK(rc);
            if (rc != hipSuccess) {
                (void)hipGetLastError();
                free_run(r);
                return false;
            }
        }
        r.fixed_klen = detect_fixed_klen(koff, n);
        r.fixed_vlen = detect_fixed_vlen(voff, n);
        r.fixed_vlen_put = detect_fixed_vlen_put(voff, sk, n);
        *ends = KeyEnds();
        if (n) {
            ends->al = std::min<uint64_t>(koff[1] - koff[0], 32);
            ends->bl = std::min<uint64_t>(koff[n] - koff[n - 1], 32);
            memcpy(ends->a, keys + koff[0], ends->al);
            memcpy(ends->b, keys + koff[n - 1], ends->bl);
        }
        return true;
    }
    /* first/last key of a run built on the device (n > 0, fixed_klen set by
     * the caller).  A fixed stride gives both addresses without the offsets. */
    KeyEnds read_key_ends(const RunBuf &r)
    {
        KeyEnds k;
        const uint64_t fk = r.fixed_klen;
        uint64_t fo[2] = {0, fk}, lo[2] = {(r.n - 1) * fk, r.n * fk};
        if (!fk) {
            HIP_OK(hipMemcpy(fo, r.koff, 16, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(lo, r.koff + (r.n - 1), 16, hipMemcpyDeviceToHost));
        }
        k.al = std::min<uint64_t>(fo[1] - fo[0], 32);
        k.bl = std::min<uint64_t>(lo[1] - lo[0], 32);
        HIP_OK(hipMemcpy(k.a, r.keys + fo[0], k.al ? k.al : 1, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(k.b, r.keys + lo[0], k.bl ? k.bl : 1, hipMemcpyDeviceToHost));
        return k;
    }

    /* the three column builders only enqueue on `stream`; finish_run drains.
     * false = a Try allocation failed (what was allocated stays in r). */
    /* packed 8B-strided probe words for the single-word search mode */
    bool build_tails(RunBuf &r, RunAlloc mode)
    {
        if (r.n == 0 || r.fixed_klen < 8 || r.lcp_exact + 8 < r.fixed_klen)
            return true;
        if (!col_alloc(&r.tails, r.n * 8, mode))
            return false;
        launch_build_tails(r.keys, r.fixed_klen, r.n, r.tails, stream);
        return true;
    }

    /* disposition column (expire<<32|kind): one 8B gather replaces the
     * sk + voff + value-header chain in filter/scan-state evaluation */
    bool build_meta(RunBuf &r, RunAlloc mode)
    {
        if (r.n == 0)
            return true;
        if (!col_alloc(&r.meta, r.n * 8, mode))
            return false;
        launch_build_meta(r.vals, r.voff, r.fixed_vlen, r.sk, r.n, data_version, r.meta,
                          stream);
        return true;
    }

    /* §8(f)3: ~10 bits/key blocked bloom, built once per run on device */
    bool build_bloom(RunBuf &r, RunAlloc mode)
    {
        if (r.n == 0)
            return true;
        uint64_t n_blocks = (r.n * 10 + 511) / 512;
        if (n_blocks == 0)
            n_blocks = 1;
        if (!col_alloc(&r.bloom, n_blocks * 64, mode) ||
            !col_alloc(&r.pfx_bloom, n_blocks * 64, mode))
            return false;
        DevRun dr = to_dev(r);
        HIP_OK(hipMemsetAsync(r.bloom, 0, n_blocks * 64, stream));
        launch_bloom_build(dr, r.bloom, n_blocks, stream);
        /* §8(f)3 second half: hashkey-prefix bloom (the reference's
         * prefix-extractor filter, _init.cpp:816-841, hashkey_transform.h) */
        HIP_OK(hipMemsetAsync(r.pfx_bloom, 0, n_blocks * 64, stream));
        launch_bloom_pfx_build(dr, r.pfx_bloom, n_blocks, stream);
        r.bloom_blocks = n_blocks;
        r.pfx_bloom_blocks = n_blocks;
        return true;
    }

    /* the derived half of run creation: shared-prefix fields from the run's
     * first/last key (`host_ends` from upload_run; null = the run was built
     * on the device, read them back), then the tails, meta and bloom
     * columns, one stream drain for all three.  `bloom` is the owning
     * handle's rocksdb.filter_type (the split passes the child's for the
     * child's runs).  false = a Try allocation failed; the stream is drained
     * first, because the caller frees buffers that enqueued builds may still
     * read. */
    bool finish_run(RunBuf &r, const KeyEnds *host_ends, RunAlloc mode, bool bloom)
    {
        const KeyEnds ends = host_ends ? *host_ends : read_key_ends(r);
        set_pfx(lcp_exact32(ends.a, ends.al, ends.b, ends.bl), &r.pfx_skip, &r.lcp_exact);
        bool ok = build_tails(r, mode) && build_meta(r, mode) && (!bloom || build_bloom(r, mode));
        HIP_OK(hipStreamSynchronize(stream));
        return ok;
    }

    /* the run list (or a column of one of its runs) changed */
    void runs_changed()
    {
        d_runs_dirty = true;
        ldst_elig_cache = -1;
    }
    /* must precede freeing any run: the resident serving kernel and every
     * parked scan view still reference it.  Appending a run needs neither. */
    void before_run_free()
    {
        server_quit_sync();
        invalidate_ctxs();
    }

    static DevRun to_dev(const RunBuf &r)
    {
        DevRun d{};
        d.keys = r.keys;
        d.koff = r.koff;
        d.vals = r.vals;
        d.voff = r.voff;
        d.sk = r.sk;
        d.n = r.n;
        d.bloom = r.bloom;
        d.bloom_blocks = r.bloom_blocks;
        d.fixed_klen = r.fixed_klen;
        d.pfx_skip = r.pfx_skip;
        d.lcp_exact = r.lcp_exact;
        d.tails = r.tails;
        d.pfx_bloom = r.pfx_bloom;
        d.pfx_bloom_blocks = r.pfx_bloom_blocks;
        d.meta = r.meta;
        d.fixed_vlen = r.fixed_vlen;
        return d;
    }
    DevRun *dev_runs()
    {
        if (d_runs_dirty) {
            server_quit_sync(); /* the resident kernel holds the old table */
            if (d_runs)
                (void)hipFree(d_runs);
            std::vector<DevRun> h(runs.size() ? runs.size() : 1);
            for (size_t i = 0; i < runs.size(); i++)
                h[i] = to_dev(runs[i]);
            HIP_OK(hipMalloc(&d_runs, h.size() * sizeof(DevRun)));
            HIP_OK(hipMemcpy(d_runs, h.data(), h.size() * sizeof(DevRun), hipMemcpyHostToDevice));
            d_runs_dirty = false;
            runs_gen++;
        }
        return d_runs;
    }

    void upload_ops()
    {
        if (d_ops)
            (void)hipFree(d_ops), d_ops = nullptr;
        if (d_rules)
            (void)hipFree(d_rules), d_rules = nullptr;
        if (d_pats)
            (void)hipFree(d_pats), d_pats = nullptr;
        n_ops = (int)host_ops.size();
        if (n_ops == 0)
            return;
        std::vector<DevOp> ops;
        std::vector<DevRule> rules;
        std::string pats;
        for (auto &op : host_ops) {
            DevOp d;
            d.type = op.type;
            d.ut_type = op.ut_type;
            d.ut_value = op.ut_value;
            d.rule_off = (int32_t)rules.size();
            d.n_rules = (int32_t)op.rules.size();
            for (auto &r : op.rules) {
                DevRule dr;
                dr.type = r.type;
                dr.match_type = r.match_type;
                dr.start_ttl = r.start_ttl;
                dr.stop_ttl = r.stop_ttl;
                dr.pat_off = (uint32_t)pats.size();
                dr.pat_len = (uint32_t)r.pattern.size();
                pats += r.pattern;
                rules.push_back(dr);
            }
            ops.push_back(d);
        }
        HIP_OK(hipMalloc(&d_ops, ops.size() * sizeof(DevOp)));
        HIP_OK(hipMemcpy(d_ops, ops.data(), ops.size() * sizeof(DevOp), hipMemcpyHostToDevice));
        HIP_OK(hipMalloc(&d_rules, rules.size() * sizeof(DevRule)));
        HIP_OK(hipMemcpy(d_rules, rules.data(), rules.size() * sizeof(DevRule),
                         hipMemcpyHostToDevice));
        HIP_OK(hipMalloc(&d_pats, pats.size() ? pats.size() : 1));
        if (!pats.empty())
            HIP_OK(hipMemcpy(d_pats, pats.data(), pats.size(), hipMemcpyHostToDevice));
    }

    uint8_t *upload_bytes(const void *p, uint64_t n)
    {
        uint8_t *d = nullptr;
        HIP_OK(hipMalloc(&d, n ? n : 1));
        if (n)
            HIP_OK(hipMemcpy(d, p, n, hipMemcpyHostToDevice));
        return d;
    }

    /* engine-owned persistent scratch arena for per-operation temporaries.
     * Bump-allocated; reset at the start of each C-ABI operation (no live
     * scratch crosses operations — persistent data uses plain hipMalloc).
     * Grows to the high-water mark once and then never allocates again —
     * per-op hipMalloc/hipFree (and mempool behavior variance across
     * driver configs) was a large, box-dependent share of step time. */
    std::vector<std::pair<uint8_t *, size_t>> sblocks;
    size_t sblock_i = 0, s_off = 0;
    /* while a split compaction is pending its phase-1 buffers live at the
     * arena head; reads between begin/finish reset only to this watermark
     * (unguarded resets let reads reuse the pending buffers) */
    bool arena_pinned = false;
    size_t pin_block = 0, pin_off = 0;
    void scratch_reset()
    {
        sblock_i = arena_pinned ? pin_block : 0;
        s_off = arena_pinned ? pin_off : 0;
    }
    void arena_pin()
    {
        arena_pinned = true;
        pin_block = sblock_i;
        pin_off = s_off;
    }
    void arena_unpin() { arena_pinned = false; }
    /* reclaim parked scanner contexts older than 5 minutes (the reference
     * drops unused contexts after std::chrono::minutes(5),
     * pegasus_server_impl.cpp:1381-1387; a used context re-parks under a
     * fresh handle with a fresh timer, as ours does).  Driven by the
     * caller-supplied epoch clock so tests are deterministic. */
    void gc_ctxs(uint32_t epoch_now)
    {
        for (auto it = ctxs.begin(); it != ctxs.end();) {
            if (epoch_now > it->second->parked_at &&
                epoch_now - it->second->parked_at > 300) {
                delete it->second;
                it = ctxs.erase(it);
            } else {
                ++it;
            }
        }
    }
    /* compaction rebuilt the run list: every parked view indexes freed runs.
     * Reclaim them all; a later scan_next returns kNotFound, the reference's
     * expired-context behavior (on_scan:1539-1541). */
    void invalidate_ctxs()
    {
        for (auto &p : ctxs)
            delete p.second;
        ctxs.clear();
    }
    template <typename T> T *talloc(uint64_t n_bytes)
    {
        uint64_t n = (n_bytes + 255) & ~255ull;
        if (n == 0)
            n = 256;
        for (;;) {
            if (sblock_i < sblocks.size()) {
                if (s_off + n <= sblocks[sblock_i].second)
                    break;
                sblock_i++; /* tail of this block is wasted until reset */
                s_off = 0;
                continue;
            }
            /* grow: blocks are kept forever (an op-time hipMalloc happens at
             * most a handful of times per engine lifetime; consolidation-
             * style free+realloc cost ~100ms per engine at 7M-record
             * partitions and poisoned the first timed step) */
            size_t tot = 0;
            for (auto &b : sblocks)
                tot += b.second;
            size_t want = std::max<size_t>({(size_t)n, tot, (size_t)(256ull << 20)});
            uint8_t *pb = nullptr;
            HIP_OK(hipMalloc(&pb, want));
            sblocks.push_back({pb, want});
            s_off = 0;
        }
        T *out = (T *)(sblocks[sblock_i].first + s_off);
        s_off += n;
        return out;
    }
    void tfree(void *) {} /* arena memory is reclaimed at scratch_reset */
    /* build the search bound table for windows lo/hi (BT_SHIFT=8 blocks);
     * returns device row-offset + table pointers (arena memory) */
    void build_bound_table_level(DevRun *dr, int R, const std::vector<uint64_t> &lo,
                                 const std::vector<uint64_t> &hi, const uint64_t *d_lo,
                                 const uint64_t *d_hi, int shift, const uint64_t *cbt_off,
                                 const uint64_t *cbt, int cbt_shift, uint64_t **out_bt_off,
                                 uint64_t **out_bt)
    {
        std::vector<uint64_t> bt_off(R + 1);
        uint64_t rows = 0;
        for (int r = 0; r < R; r++) {
            bt_off[r] = rows;
            uint64_t w = hi[r] - lo[r];
            rows += (w >> shift) + 2; /* P_r + sentinel */
        }
        bt_off[R] = rows;
        uint64_t *d_bt_off = (uint64_t *)upload_tmp(bt_off.data(), (R + 1) * 8);
        uint64_t *d_bt = talloc<uint64_t>(rows * (uint64_t)R * 8);
        launch_bound_table(dr, R, d_lo, d_hi, d_bt_off, rows, shift, d_bt, cbt_off, cbt,
                           cbt_shift, stream);
        *out_bt_off = d_bt_off;
        *out_bt = d_bt;
    }

    /* returns the number of table levels built (1, or 2 with the coarse one) */
    int build_bound_table(DevRun *dr, int R, const std::vector<uint64_t> &lo,
                          const std::vector<uint64_t> &hi, const uint64_t *d_lo,
                          const uint64_t *d_hi, uint64_t **out_bt_off, uint64_t **out_bt)
    {
        uint64_t wmax = 0;
        for (int r = 0; r < R; r++)
            wmax = std::max(wmax, hi[r] - lo[r]);
        uint64_t *c_off = nullptr, *c_bt = nullptr;
        int cshift = bt_shift + 6;
        if ((wmax >> cshift) > 8) /* coarse level pays only at scale */
            build_bound_table_level(dr, R, lo, hi, d_lo, d_hi, cshift, nullptr, nullptr, 0,
                                    &c_off, &c_bt);
        build_bound_table_level(dr, R, lo, hi, d_lo, d_hi, bt_shift, c_off, c_bt, cshift,
                                out_bt_off, out_bt);
        return c_bt ? 2 : 1;
    }

    uint64_t *psum_scratch(uint64_t n)
    {
        return talloc<uint64_t>(psum_scratch_elems(n) * 8);
    }
    uint8_t *upload_tmp(const void *p, uint64_t n)
    {
        uint8_t *d = talloc<uint8_t>(n);
        if (n)
            HIP_OK(hipMemcpyAsync(d, p, n, hipMemcpyHostToDevice, stream));
        return d;
    }

    /* pinned host staging (reused; grown to high-water) — unpinned D2H runs
     * at a fraction of PCIe rate, so big result copies stage through here */
    uint8_t *pinned = nullptr;
    size_t pinned_cap = 0;
    uint8_t *pinned_buf(size_t n)
    {
        if (n > pinned_cap) {
            if (pinned)
                (void)hipHostFree(pinned);
            pinned_cap = std::max<size_t>(n, pinned_cap * 2);
            HIP_OK(hipHostMalloc((void **)&pinned, pinned_cap));
        }
        return pinned;
    }
    /* D2H via pinned staging into an arbitrary host destination */
    void d2h(void *dst, const void *src, size_t n)
    {
        if (n == 0)
            return;
        if (n <= (64u << 10)) { /* small copies: direct */
            HIP_OK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            return;
        }
        uint8_t *pb = pinned_buf(n);
        HIP_OK(hipMemcpyAsync(pb, src, n, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        memcpy(dst, pb, n);
    }

    /* group-streaming rank: pick the anchor run (largest window) and stride,
     * build the anchor table (arena memory).  Returns n_groups. */
    uint64_t build_anchors(DevRun *dr, int R, const std::vector<uint64_t> &lo,
                           const std::vector<uint64_t> &hi, const uint64_t *d_lo,
                           const uint64_t *d_hi, uint64_t **out_anch)
    {
        int q0 = 0;
        uint64_t wmax = 0;
        for (int r = 0; r < R; r++)
            if (hi[r] - lo[r] > wmax) {
                wmax = hi[r] - lo[r];
                q0 = r;
            }
        const int gs = grp_shift(R);
        uint64_t n_groups = (wmax + (1ull << gs) - 1) >> gs;
        if (n_groups == 0)
            n_groups = 1;
        uint64_t *d_anch = talloc<uint64_t>((n_groups + 1) * R * 8);
        launch_anchor_rows(dr, R, q0, d_lo, d_hi, gs, n_groups, d_anch, stream);
        *out_anch = d_anch;
        return n_groups;
    }

    /* The rank route of runs [first, first+R) and the tables its kernel narrows
     * by: anchors for the group rank, else a one- or two-level bound table above
     * bt_min_records.  Compaction and views each launch their own kernel. */
    struct RankPrep {
        int32_t route = RRDB_ROUTE_RANK_GLOBAL;
        uint64_t *d_anch = nullptr, n_groups = 0;
        uint64_t *d_bt_off = nullptr, *d_bt = nullptr;
        int bound_levels = 0;
    };
    RankPrep prepare_rank(DevRun *dr, size_t first, int R, const std::vector<uint64_t> &lo,
                          const std::vector<uint64_t> &hi, const uint64_t *d_lo,
                          const uint64_t *d_hi, uint64_t total, uint64_t bt_min_records,
                          bool grp_allowed)
    {
        RankPrep p;
        if (R < 2)
            return p;
        if (grp_allowed && grp_eligible(first, (size_t)R)) {
            p.route = RRDB_ROUTE_RANK_GRP;
            p.n_groups = build_anchors(dr, R, lo, hi, d_lo, d_hi, &p.d_anch);
            return p;
        }
        if (total > bt_min_records)
            p.bound_levels = build_bound_table(dr, R, lo, hi, d_lo, d_hi, &p.d_bt_off, &p.d_bt);
        if (ldst_eligible(first, (size_t)R))
            p.route = RRDB_ROUTE_RANK_LDST;
        return p;
    }

    /* build the visible view for [start, stop_excl); a null bound is open */
    DevView build_view(const std::string *start, const std::string *stop_excl)
    {
        int R = (int)runs.size();
        last_view = rrdb_view_route{RRDB_ROUTE_NONE, 0, 0, 0, 0};
        if (R == 0)
            return {};
        DevRun *dr = dev_runs();
        uint64_t *d_lo = talloc<uint64_t>(R * 8);
        uint64_t *d_hi = talloc<uint64_t>(R * 8);
        uint8_t *d_start = start ? upload_tmp(start->data(), start->size()) : nullptr;
        uint8_t *d_stop = stop_excl ? upload_tmp(stop_excl->data(), stop_excl->size()) : nullptr;
        launch_bounds(dr, R, d_start, start ? start->size() : 0, d_lo, 0, stream);
        /* null stop = unbounded: upper flag makes the null-key case yield n */
        launch_bounds(dr, R, d_stop, stop_excl ? stop_excl->size() : 0, d_hi,
                      stop_excl ? 0 : 1, stream);
        std::vector<uint64_t> lo(R), hi(R), wprefix(R + 1);
        HIP_OK(hipMemcpyAsync(lo.data(), d_lo, R * 8, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipMemcpyAsync(hi.data(), d_hi, R * 8, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        uint64_t total = 0;
        for (int r = 0; r < R; r++) {
            if (hi[r] < lo[r])
                hi[r] = lo[r];
            wprefix[r] = total;
            total += hi[r] - lo[r];
        }
        wprefix[R] = total;
        tfree(d_start);
        tfree(d_stop);
        if (total == 0) {
            tfree(d_lo);
            tfree(d_hi);
            return {};
        }
        /* re-upload corrected hi + wprefix */
        HIP_OK(hipMemcpy(d_hi, hi.data(), R * 8, hipMemcpyHostToDevice));
        uint64_t *d_wp = (uint64_t *)upload_tmp(wprefix.data(), (R + 1) * 8);
        uint64_t *d_order = talloc<uint64_t>(total * 8);
        uint8_t *d_shadow = talloc<uint8_t>(total);
        uint64_t *d_flags = talloc<uint64_t>(total * 8);
        uint64_t *d_pos = talloc<uint64_t>(total * 8);
        last_view.window_records = total;
        const RankPrep rp = prepare_rank(dr, 0, R, lo, hi, d_lo, d_hi, total,
                                         VIEW_BT_MIN_RECORDS, true);
        last_view.rank = rp.route;
        last_view.n_groups = rp.n_groups;
        last_view.bound_levels = rp.bound_levels;
        if (rp.route == RRDB_ROUTE_RANK_GRP)
            launch_rank_grp_view(dr, R, d_lo, rp.d_anch, rp.n_groups, d_order, d_shadow, stream);
        else if (rp.route == RRDB_ROUTE_RANK_LDST)
            launch_rank_ldst(dr, R, d_lo, d_hi, d_wp, total, d_order, d_shadow, rp.d_bt_off,
                             rp.d_bt, bt_shift, stream);
        else
            launch_rank(dr, R, d_lo, d_hi, d_wp, total, d_order, d_shadow, rp.d_bt_off, rp.d_bt,
                        bt_shift, stream);
        launch_visible(dr, d_order, d_shadow, total, d_flags, stream);
        launch_psum(d_flags, d_pos, total, psum_scratch(total), stream);
        uint64_t last[2] = {0, 0};
        scan_tail_async(d_pos, d_flags, total, last, stream);
        HIP_OK(hipStreamSynchronize(stream));
        uint64_t nv = last[0] + last[1];
        last_view.visible = nv;
        uint64_t *d_view = nullptr;
        if (nv) {
            HIP_OK(hipMalloc(&d_view, nv * 8));
            launch_gather(d_order, d_flags, d_pos, total, d_view, stream);
            HIP_OK(hipStreamSynchronize(stream));
        }
        tfree(d_lo);
        tfree(d_hi);
        tfree(d_wp);
        tfree(d_order);
        tfree(d_shadow);
        tfree(d_flags);
        tfree(d_pos);
        HIP_OK(hipStreamSynchronize(stream));
        return DevView(d_view, nv);
    }
};

std::once_flag g_init_once;

} // namespace

static int32_t engine_flush(HipEngine *e); /* write path, defined below */

/* internal: upload a prepared sorted run (validation already established);
 * kIOError (with the partial run unwound) when the device is full */
static int32_t ingest_prepared(HipEngine *e, const uint8_t *keys, const uint64_t *koff,
                               const uint8_t *vals, const uint64_t *voff, const uint64_t *sk,
                               uint64_t n)
{
    RunBuf r;
    KeyEnds ends;
    if (!e->upload_run(r, keys, koff, vals, voff, sk, n, RunAlloc::Try, &ends))
        return RRDB_IO_ERROR;
    /* the derived columns abort on a full device, as they always have here */
    e->finish_run(r, &ends, RunAlloc::Abort, e->bloom_enabled);
    e->runs.push_back(r);
    e->runs_changed();
    return RRDB_OK;
}

extern "C" {

const char *rrdb_backend(void) { return "hip-gfx950"; }

double rrdb_phase_ms(void *h, const char *phase)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    e->activate();
    e->resolve_phase_events();
    auto it = e->phase_ms.find(phase);
    return it == e->phase_ms.end() ? -1.0 : it->second;
}

void *rrdb_open(int32_t app_id, int32_t pidx, int32_t gpu_id)
{
    if (gpu_id < 0)
        return nullptr; /* GPU engine requires a device */
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || gpu_id >= ndev) {
        fprintf(stderr, "rrdb-hip: no HIP device %d (count=%d) — the product engine has no CPU "
                        "fallback\n",
                gpu_id, ndev);
        return nullptr;
    }
    auto *e = new HipEngine();
    e->app_id = app_id;
    e->pidx = pidx;
    e->device = gpu_id;
    e->activate();
    /* spin completion: interrupt-driven stream waits cost ~10-20us each on
     * the small-op serving path (ignored if the runtime refuses) */
    (void)hipSetDeviceFlags(hipDeviceScheduleSpin);
    std::call_once(g_init_once, [] {
        build_crc64_table();
        launch_crc64_table_init(host_crc64_table);
    });
    HIP_OK(hipStreamCreate(&e->stream));
    {
        hipMemPool_t pool;
        if (hipDeviceGetDefaultMemPool(&pool, gpu_id) == hipSuccess) {
            uint64_t thr = UINT64_MAX;
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &thr);
        }
    }
    return e;
}

void rrdb_close(void *h)
{
    auto *e = (HipEngine *)h;
    if (!e)
        return;
    e->activate();
    e->server_quit_sync(); /* retire the resident serving kernel first */
    for (auto &kv : e->ctxs)
        delete kv.second;
    e->ctxs.clear();
    {
        auto &ps = e->pend_scan;
        for (void *p : {(void *)ps.d_stats, (void *)ps.d_anch, (void *)ps.d_lo,
                        (void *)ps.d_hi, (void *)ps.d_start})
            if (p)
                (void)hipFree(p);
    }
    for (auto &r : e->runs)
        e->free_run(r);
    if (e->d_runs)
        (void)hipFree(e->d_runs);
    for (auto &b : e->sblocks)
        (void)hipFree(b.first);
    if (e->pinned)
        (void)hipHostFree(e->pinned);
    if (e->kept.sizes) {
        (void)hipHostFree(e->kept.sizes);
        (void)hipHostFree(e->kept.stats);
        for (auto &x : e->kept.ev)
            (void)hipEventDestroy(x);
    }
    e->server_quit_sync();
    if (e->mg_mb)
        (void)hipHostFree((void *)e->mg_mb);
    if (e->mg_srv_stream)
        (void)hipStreamDestroy(e->mg_srv_stream);
    if (e->mg_graph)
        (void)hipGraphExecDestroy(e->mg_graph);
    if (e->mg_capture_stream)
        (void)hipStreamDestroy(e->mg_capture_stream);
    if (e->mg_hin) {
        (void)hipHostFree(e->mg_hin);
        (void)hipFree(e->mg_din);
        (void)hipHostFree(e->mg_hout);
        (void)hipFree(e->mg_dout);
    }
    if (e->d_ops)
        (void)hipFree(e->d_ops);
    if (e->d_rules)
        (void)hipFree(e->d_rules);
    if (e->d_pats)
        (void)hipFree(e->d_pats);
    (void)hipStreamDestroy(e->stream);
    delete e;
}

int32_t rrdb_set_partition_version(void *h, int32_t pv)
{
    ((HipEngine *)h)->partition_version = pv;
    return RRDB_OK;
}

int32_t rrdb_set_envs(void *h, const char *const *keys, const char *const *values, int32_t n)
{
    auto *e = (HipEngine *)h;
    e->activate();
    for (int32_t i = 0; i < n; i++) {
        std::string k = keys[i], v = values[i];
        if (k == "default_ttl") {
            long long t = atoll(v.c_str());
            e->default_ttl = t > 0 ? (uint32_t)t : 0;
        } else if (k == "user_specified_compaction") {
            std::vector<HostOp> ops;
            if (!parse_user_ops(v, ops))
                ops.clear(); /* invalid json -> no ops (cpp:165-169) */
            e->host_ops = std::move(ops);
            e->upload_ops();
        } else if (k == "replica.split.validate_partition_hash") {
            e->validate_hash = (v == "true");
        } else if (k == "manual_compact.disabled") {
            e->manual_compact_disabled = (v == "true");
        } else if (k == "pegasus.data_version") {
            uint32_t nv = (uint32_t)atoi(v.c_str());
            if (nv != e->data_version) {
                e->data_version = nv;
                /* the meta column bakes in the value-header layout */
                e->activate();
                for (auto &r : e->runs) {
                    if (r.meta) {
                        (void)hipFree(r.meta);
                        r.meta = nullptr;
                    }
                    e->build_meta(r, RunAlloc::Abort);
                }
                HIP_OK(hipStreamSynchronize(e->stream));
                e->runs_changed();
            }
        } else if (k == "replica.rocksdb_iteration_threshold_time_ms") {
            e->iter_time_ms = (uint64_t)atoll(v.c_str());
        } else if (k == "rocksdb.max_iteration_count") {
            e->max_iter_count = (uint32_t)atoll(v.c_str());
        } else if (k == "rocksdb.multi_get_max_iteration_count") {
            e->mg_max_iter_count = (uint32_t)atoll(v.c_str());
        } else if (k == "rocksdb.multi_get_max_iteration_size") {
            e->mg_max_iter_size = (uint64_t)atoll(v.c_str());
        } else if (k == "rocksdb.filter_type") {
            e->bloom_enabled = (v != "none"); /* common/prefix -> full-key bloom */
        } else if (k == "engine.rank_mode") {
            e->rank_mode =
                (v == "lds") ? 1 : (v == "ldst" ? 3 : (v == "global" ? 0 : 4));
        } else if (k == "engine.grp_blocks") {
            int b = atoi(v.c_str());
            if (b >= 256 && b <= 65535)
                e->grp_blocks = b;
        } else if (k == "engine.bt_shift") {
            int s_ = atoi(v.c_str());
            if (s_ >= 4 && s_ <= 16)
                e->bt_shift = s_;
        } else if (k == "engine.mg_persist") {
            if (v == "off") {
                e->activate();
                e->server_quit_sync();
                e->mg_persist_mode = 0;
            } else if (v == "on") {
                e->mg_persist_mode = 2;
                e->mg_persist_enabled = true;
            } else { /* "auto" */
                e->mg_persist_mode = 1;
                e->mg_persist_enabled = true;
            }
        } else if (k == "engine.mg_graph") {
            e->mg_graph_enabled = (v != "off");
            if (!e->mg_graph_enabled && e->mg_graph) {
                e->activate();
                (void)hipGraphExecDestroy(e->mg_graph);
                e->mg_graph = nullptr;
            }
        } else if (k == "engine.split_crc") {
            e->split_crc_lds = (v == "global") ? 0 : 1;
        } else if (k == "engine.emit_mode") {
            e->emit_mode = (v == "input") ? 1 : (v == "rank" ? 0 : 2);
        } else if (k == "engine.l0_compaction_trigger") {
            long long t = atoll(v.c_str());
            e->l0_trigger = t < 2 ? 2u : (uint32_t)std::min<long long>(t, UINT32_MAX);
        } else if (k == "engine.incr_lane_max") {
            long long t = atoll(v.c_str());
            e->incr_lane_max = t < 1 ? 1u : (uint32_t)std::min<long long>(t, 1 << 20);
        } else if (k == "engine.wbt_lane_max") {
            long long t = atoll(v.c_str());
            e->wbt_lane_max = t < 1 ? 1u : (uint32_t)std::min<long long>(t, 1 << 20);
        } else if (k == "rocksdb.usage_scenario") {
            /* bulk_load sets level0_file_num_compaction_trigger to -1, i.e.
             * no automatic compaction (set_usage_scenario); normal and
             * prefer_write leave it on */
            e->bulk_load = (v == "bulk_load");
        }
    }
    return RRDB_OK;
}

int32_t rrdb_ingest_run(void *h, const uint8_t *keys, const uint64_t *key_offs,
                        const uint8_t *values, const uint64_t *val_offs, const uint64_t *seq_kind,
                        uint64_t n)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    engine_flush(e); /* buffered writes are older than this run */
    if (n == 0)
        return RRDB_OK;
    /* validate on host (data arrives host-side anyway) */
    if (key_offs[0] != 0 || key_offs[1] == 0)
        return RRDB_INVALID_ARGUMENT; /* keys must be nonempty, offsets 0-based */
    for (uint64_t i = 0; i < n; i++) {
        if ((seq_kind[i] >> 1) < e->next_seq_floor)
            return RRDB_INVALID_ARGUMENT;
        if (i > 0) {
            uint64_t al = key_offs[i] - key_offs[i - 1], bl = key_offs[i + 1] - key_offs[i];
            const uint8_t *a = keys + key_offs[i - 1];
            const uint8_t *b = keys + key_offs[i];
            int c = memcmp(a, b, std::min(al, bl));
            if (c > 0 || (c == 0 && al >= bl))
                return RRDB_INVALID_ARGUMENT;
        }
    }
    e->activate();
    int32_t rc = ingest_prepared(e, keys, key_offs, values, val_offs, seq_kind, n);
    if (rc != RRDB_OK)
        return rc;
    uint64_t mx = 0;
    for (uint64_t i = 0; i < n; i++)
        mx = std::max(mx, seq_kind[i] >> 1);
    e->next_seq_floor = mx + 1;
    return RRDB_OK;
}

uint64_t rrdb_num_runs(void *h) { return ((HipEngine *)h)->runs.size(); }
uint64_t rrdb_num_records(void *h)
{
    auto *e = (HipEngine *)h;
    uint64_t t = 0;
    for (auto &r : e->runs)
        t += r.n;
    return t;
}

void rrdb_free_result(rrdb_result *r)
{
    if (r && r->_arena) {
        delete (Arena *)r->_arena;
        r->_arena = nullptr;
    }
}

/* ---- batched point lookup core (on_get / on_batch_get / DB::MultiGet) ---- */
static int32_t get_core(HipEngine *e, uint64_t nq, const uint8_t *keys, const uint64_t *key_offs,
                        uint32_t epoch_now, std::vector<int32_t> &status,
                        std::vector<std::pair<const uint8_t *, uint64_t>> &vals, Arena *a)
{
    e->activate();
    e->scratch_reset();
    int R = (int)e->runs.size();
    status.assign(nq, RRDB_NOT_FOUND);
    vals.assign(nq, {nullptr, 0});
    if (R == 0)
        return RRDB_OK;
    DevRun *dr = e->dev_runs();
    uint8_t *d_keys = e->upload_tmp(keys, key_offs[nq]);
    uint64_t *d_offs = (uint64_t *)e->upload_tmp(key_offs, (nq + 1) * 8);
    int32_t *d_status = e->talloc<int32_t>(nq * 4);
    uint64_t *d_hit = e->talloc<uint64_t>(nq * 8);
    uint64_t *d_ulen = e->talloc<uint64_t>(nq * 8);
    uint64_t *d_voffs = e->talloc<uint64_t>((nq + 1) * 8);
    uint64_t last[2] = {0, 0};
    PhaseEvents<2> gev;
    gev.record(0, e->stream);
    launch_get(dr, R, d_keys, d_offs, nq, epoch_now, e->data_version, d_status, d_hit, d_ulen,
               nullptr, e->stream);
    gev.record(1, e->stream);
    launch_psum(d_ulen, d_voffs, nq, e->psum_scratch(nq), e->stream);
    scan_tail_async(d_voffs, d_ulen, nq, last, e->stream);
    HIP_OK(hipMemcpyAsync(status.data(), d_status, nq * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    float ms;
    if (gev.ms(0, 1, &ms))
        e->phase_ms["get_search"] = ms;
    uint64_t total = last[0] + last[1];
    std::vector<uint64_t> voffs(nq + 1);
    HIP_OK(hipMemcpy(voffs.data(), d_voffs, nq * 8, hipMemcpyDeviceToHost));
    voffs[nq] = total;
    uint8_t *blob = (uint8_t *)a->alloc(total);
    if (total) {
        uint8_t *d_blob = e->talloc<uint8_t>(total);
        launch_emit_values(dr, d_hit, d_status, nq, e->data_version, d_voffs, d_blob, e->stream);
        e->d2h(blob, d_blob, total);
        e->tfree(d_blob);
    }
    for (uint64_t i = 0; i < nq; i++)
        if (status[i] == RRDB_OK)
            vals[i] = {blob + voffs[i], voffs[i + 1] - voffs[i]};
    e->tfree(d_keys);
    e->tfree(d_offs);
    e->tfree(d_status);
    e->tfree(d_hit);
    e->tfree(d_ulen);
    e->tfree(d_voffs);
    return RRDB_OK;
}

int32_t rrdb_get(void *h, const uint8_t *key, uint64_t key_len, uint32_t epoch_now,
                 rrdb_result *out)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(((HipEngine *)h)->mu);
    engine_flush((HipEngine *)h); /* memtable visible to reads */
    Arena *a = result_init(out);
    uint64_t offs[2] = {0, key_len};
    std::vector<int32_t> status;
    std::vector<std::pair<const uint8_t *, uint64_t>> vals;
    get_core(e, 1, key, offs, epoch_now, status, vals, a);
    if (status[0] != RRDB_OK) {
        out->error = status[0];
        return out->error;
    }
    out->count = 1;
    out->keys = (rrdb_slice *)a->alloc(sizeof(rrdb_slice));
    out->values = (rrdb_slice *)a->alloc(sizeof(rrdb_slice));
    out->keys[0] = {nullptr, 0};
    out->values[0] = {(uint8_t *)vals[0].first, vals[0].second};
    out->error = RRDB_OK;
    return RRDB_OK;
}

int32_t rrdb_batch_get(void *h, uint64_t n_keys, const uint8_t *keys, const uint64_t *key_offs,
                       uint32_t epoch_now, rrdb_result *out)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(((HipEngine *)h)->mu);
    engine_flush((HipEngine *)h); /* memtable visible to reads */
    Arena *a = result_init(out);
    if (n_keys == 0) {
        out->error = RRDB_INVALID_ARGUMENT; /* on_batch_get:922-928 */
        return out->error;
    }
    std::vector<int32_t> status;
    std::vector<std::pair<const uint8_t *, uint64_t>> vals;
    get_core(e, n_keys, keys, key_offs, epoch_now, status, vals, a);
    out->keys = (rrdb_slice *)a->alloc(n_keys * sizeof(rrdb_slice));
    out->values = (rrdb_slice *)a->alloc(n_keys * sizeof(rrdb_slice));
    /* one block for every returned key (a per-key arena alloc was ~30ms at
     * 1M-key batches) */
    uint8_t *kblock = (uint8_t *)a->alloc(key_offs[n_keys]);
    uint64_t m = 0, kb = 0;
    for (uint64_t i = 0; i < n_keys; i++) {
        if (status[i] != RRDB_OK)
            continue; /* NotFound/expired skipped (on_batch_get:952-965) */
        uint64_t kl = key_offs[i + 1] - key_offs[i];
        memcpy(kblock + kb, keys + key_offs[i], kl);
        out->keys[m] = {kblock + kb, kl};
        out->values[m] = {(uint8_t *)vals[i].first, vals[i].second};
        kb += kl;
        m++;
    }
    out->count = m;
    out->error = RRDB_OK;
    return RRDB_OK;
}

int32_t rrdb_ttl(void *h, const uint8_t *key, uint64_t key_len, uint32_t epoch_now,
                 rrdb_result *out)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(((HipEngine *)h)->mu);
    engine_flush((HipEngine *)h); /* memtable visible to reads */
    ((HipEngine *)h)->scratch_reset();
    Arena *a = result_init(out);
    e->activate();
    int R = (int)e->runs.size();
    if (R == 0) {
        out->error = RRDB_NOT_FOUND;
        return out->error;
    }
    DevRun *dr = e->dev_runs();
    uint64_t offs[2] = {0, key_len};
    uint8_t *d_key = e->upload_tmp(key, key_len);
    uint64_t *d_offs = (uint64_t *)e->upload_tmp(offs, 16);
    int32_t *d_status = e->talloc<int32_t>(4);
    uint64_t *d_hit = e->talloc<uint64_t>(8);
    uint64_t *d_ulen = e->talloc<uint64_t>(8);
    uint32_t *d_expire = e->talloc<uint32_t>(4);
    launch_get(dr, R, d_key, d_offs, 1, epoch_now, e->data_version, d_status, d_hit, d_ulen,
               d_expire, e->stream);
    int32_t st;
    uint32_t expire;
    HIP_OK(hipMemcpyAsync(&st, d_status, 4, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipMemcpyAsync(&expire, d_expire, 4, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    e->tfree(d_key);
    e->tfree(d_offs);
    e->tfree(d_status);
    e->tfree(d_hit);
    e->tfree(d_ulen);
    e->tfree(d_expire);
    (void)a;
    out->error = st;
    if (st == RRDB_OK)
        out->i64 = expire > 0 ? (int64_t)expire - (int64_t)epoch_now : -1; /* on_ttl:1135-1142 */
    return out->error;
}

} /* extern "C" */

/* ---- what the read entry points below share; what a path does differently
 * stays written out in its function.  DevView is up with HipScanCtx. ---- */
namespace {

/* flush, fresh scratch and result.  Null: the flush failed (device full; writes
 * retained), *out says kIOError.  activate() is the caller's: it may validate first. */
Arena *read_begin(HipEngine *e, rrdb_result *out)
{
    if (engine_flush(e) != RRDB_OK) {
        result_init(out);
        out->error = RRDB_IO_ERROR;
        return nullptr;
    }
    e->scratch_reset();
    return result_init(out);
}

/* a key range: a builder sets the ends and clamps them by a prefix filter,
 * close() finishes it; what an empty range returns is the caller's business */
struct KeyRange {
    std::string start, stop;
    std::string stop_excl; /* smallest key past the range: what the kernels take */
    bool start_inclusive = true, stop_inclusive = false;
    void clamp_start(const std::string &ps)
    {
        if (key_cmp(ps, start) > 0)
            start = ps, start_inclusive = true;
    }
    /* false: the range is empty (on_get_scanner:1227-1243, on_multi_get:580-607) */
    bool close()
    {
        int c = key_cmp(start, stop);
        if (c > 0 || (c == 0 && (!start_inclusive || !stop_inclusive)))
            return false;
        stop_excl = stop;
        if (stop_inclusive)
            stop_excl.push_back('\0');
        return true;
    }
};

/* scan: the request's keys; a hash-key prefix filter clamps start only
 * (on_get_scanner:1206-1224).  The caller has checked the pattern's length. */
KeyRange scan_range(const rrdb_scan_request *q)
{
    KeyRange kr;
    kr.start.assign((const char *)q->start_key.data, q->start_key.len);
    kr.stop.assign((const char *)q->stop_key.data, q->stop_key.len);
    kr.start_inclusive = q->start_inclusive;
    kr.stop_inclusive = q->stop_inclusive;
    if (q->hash_key_filter_type == RRDB_FT_MATCH_PREFIX && q->hash_key_filter_pattern.len > 0)
        kr.clamp_start(
            make_key(q->hash_key_filter_pattern.data, q->hash_key_filter_pattern.len, nullptr, 0));
    return kr;
}

/* all of one hash key: start=(hk,""), stop=next(hk) (on_sortkey_count:1030-1036) */
KeyRange hash_key_range(const uint8_t *hk, uint64_t hklen)
{
    KeyRange kr;
    kr.start = make_key(hk, hklen, nullptr, 0);
    kr.stop = next_blob(kr.start);
    return kr;
}

/* multi_get's range (on_multi_get:542-578): sort-key bounds in one hash key, an
 * empty stop being the hash key's end; a sort-key prefix filter clamps both ends */
KeyRange mg_range(const rrdb_multi_get_request *q)
{
    const uint8_t *hk = q->hash_key.data;
    const uint64_t hklen = q->hash_key.len;
    KeyRange kr = hash_key_range(hk, hklen);
    kr.start = make_key(hk, hklen, q->start_sortkey.data, q->start_sortkey.len);
    kr.start_inclusive = q->start_inclusive;
    if (q->stop_sortkey.len != 0) {
        kr.stop = make_key(hk, hklen, q->stop_sortkey.data, q->stop_sortkey.len);
        kr.stop_inclusive = q->stop_inclusive;
    }
    if (q->sort_key_filter_type == RRDB_FT_MATCH_PREFIX && q->sort_key_filter_pattern.len > 0) {
        std::string ps =
            make_key(hk, hklen, q->sort_key_filter_pattern.data, q->sort_key_filter_pattern.len);
        kr.clamp_start(ps);
        if (std::string pe = next_blob(ps); key_cmp(pe, kr.stop) <= 0)
            kr.stop = pe, kr.stop_inclusive = false;
    }
    return kr;
}

/* is the record at this view position exactly `bound`?  One launch, one host sync. */
bool key_at_equals(HipEngine *e, const uint64_t *d_view_pos, const std::string &bound)
{
    uint32_t *d_eq = e->talloc<uint32_t>(4);
    uint8_t *d_b = e->upload_tmp(bound.data(), bound.size());
    launch_first_eq(e->dev_runs(), d_view_pos, 1, d_b, bound.size(), d_eq, e->stream);
    uint32_t eq = 0;
    HIP_OK(hipMemcpyAsync(&eq, d_eq, 4, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    e->tfree(d_eq);
    e->tfree(d_b);
    return eq != 0;
}

/* the engine's part of a ScanParams; the rest starts zero */
ScanParams base_scan_params(const HipEngine *e, uint32_t epoch_now)
{
    ScanParams sp{};
    sp.epoch_now = epoch_now;
    sp.data_version = e->data_version;
    sp.pidx = e->pidx;
    sp.partition_version = e->partition_version;
    return sp;
}

/* multi_get's limits (on_multi_get:523-533): the request's, capped by the engine's */
struct MgLimits {
    uint32_t max_kv_count, max_iteration_count;
    int64_t max_kv_size, max_iter_size;
    MgLimits(const HipEngine *e, const rrdb_multi_get_request *q)
    {
        max_kv_count = max_iteration_count = e->mg_max_iter_count;
        if (q->max_kv_count > 0 && (uint32_t)q->max_kv_count < max_kv_count)
            max_kv_count = (uint32_t)q->max_kv_count;
        max_kv_size = q->max_kv_size > 0 ? q->max_kv_size : INT32_MAX;
        max_iter_size = std::min<int64_t>(
            max_kv_size, e->mg_max_iter_size > 0 ? (int64_t)e->mg_max_iter_size : INT32_MAX);
    }
};

} // namespace

extern "C" {

/* ---- scan machinery shared by scan/sortkey_count/multi_get-range ---- */

/* a zero-row batch returns allocated (empty) arrays: only the empty-RANGE early
 * return leaves them null (matches the oracle's scan_batch, observable via expire_ts) */
static void scan_empty_rows(const HipScanCtx *c, rrdb_result *out, Arena *a)
{
    out->keys = (rrdb_slice *)a->alloc(sizeof(rrdb_slice));
    out->values = (rrdb_slice *)a->alloc(sizeof(rrdb_slice));
    if (c->return_expire_ts)
        out->expire_ts = (int32_t *)a->alloc(4);
}

/* the filters and flags a scan context carries, as the kernels take them */
static ScanParams ctx_scan_params(const HipEngine *e, const HipScanCtx *c, uint32_t epoch_now)
{
    ScanParams sp = base_scan_params(e, epoch_now);
    sp.validate_hash = (uint8_t)(c->validate_hash_req && e->validate_hash);
    sp.hk_ft = c->hk_ft;
    sp.sk_ft = c->sk_ft;
    sp.hk_pat = c->d_hk_pat;
    sp.hk_pat_len = c->hk_pat_len;
    sp.sk_pat = c->d_sk_pat;
    sp.sk_pat_len = c->sk_pat_len;
    sp.no_value = c->no_value;
    return sp;
}

/* run one forward batch over ctx->view[cursor..]; emits into result */
static void scan_batch_gpu(HipEngine *e, HipScanCtx *c, uint32_t epoch_now, rrdb_result *out,
                           Arena *a)
{
    auto t_start = std::chrono::steady_clock::now();
    uint32_t batch_count = e->max_iter_count;
    if (c->batch_size > 0 && (uint32_t)c->batch_size < batch_count)
        batch_count = (uint32_t)c->batch_size;
    uint64_t remaining = c->view.n - c->cursor;
    uint64_t w = std::min<uint64_t>(remaining, e->max_iter_count);
    if (w == 0) {
        out->error = RRDB_OK;
        out->context_id = RRDB_SCAN_CONTEXT_ID_COMPLETED;
        if (c->only_return_count)
            out->i64 = 0;
        else
            scan_empty_rows(c, out, a);
        return;
    }
    DevRun *dr = e->dev_runs();
    const uint64_t *d_win = c->view.d + c->cursor;
    const ScanParams sp = ctx_scan_params(e, c, epoch_now);
    uint8_t *d_state = e->talloc<uint8_t>(w);
    uint64_t *d_ksz = e->talloc<uint64_t>(w * 8);
    uint64_t *d_vsz = e->talloc<uint64_t>(w * 8);
    uint64_t *d_flags = e->talloc<uint64_t>(w * 8);
    uint64_t *d_npos = e->talloc<uint64_t>(w * 8);
    uint64_t *d_cut = e->talloc<uint64_t>(16);
    PhaseEvents<4> sev;
    sev.record(0, e->stream);
    launch_scan_state(dr, d_win, w, sp, d_state, d_ksz, d_vsz, e->stream);
    sev.record(1, e->stream);
    launch_normal_flags(d_state, w, d_flags, e->stream);
    launch_psum(d_flags, d_npos, w, e->psum_scratch(w), e->stream);
    launch_cutoff(d_npos, d_flags, w, batch_count, d_cut, e->stream);
    uint64_t cut[2];
    HIP_OK(hipMemcpyAsync(cut, d_cut, 16, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    uint64_t consumed = cut[0], n_out = cut[1];

    if (c->only_return_count) {
        out->i64 = (int64_t)n_out;
        out->count = 0;
    } else if (n_out == 0) {
        out->count = 0;
        scan_empty_rows(c, out, a);
    } else {
        launch_cut_sizes(d_state, w, consumed, d_ksz, d_vsz, e->stream);
        uint64_t *d_koffs = e->talloc<uint64_t>(w * 8);
        uint64_t *d_voffs = e->talloc<uint64_t>(w * 8);
        launch_psum(d_ksz, d_koffs, w, e->psum_scratch(w), e->stream);
        launch_psum(d_vsz, d_voffs, w, e->psum_scratch(w), e->stream);
        uint64_t t[4] = {0, 0, 0, 0};
        scan_tail_async(d_koffs, d_ksz, w, &t[0], e->stream);
        scan_tail_async(d_voffs, d_vsz, w, &t[2], e->stream);
        HIP_OK(hipStreamSynchronize(e->stream));
        uint64_t kbytes = t[0] + t[1], vbytes = t[2] + t[3];
        uint8_t *d_kout, *d_vout;
        uint64_t *d_kooffs, *d_vooffs;
        int32_t *d_ets = nullptr;
        if (c->on_device_out) {
            /* handed to the caller: plain allocations, freed by rrdb_free_result */
            HIP_OK(hipMalloc(&d_kout, kbytes ? kbytes : 1));
            HIP_OK(hipMalloc(&d_vout, vbytes ? vbytes : 1));
            HIP_OK(hipMalloc(&d_kooffs, (n_out + 1) * 8));
            HIP_OK(hipMalloc(&d_vooffs, (n_out + 1) * 8));
        } else {
            d_kout = e->talloc<uint8_t>(kbytes);
            d_vout = e->talloc<uint8_t>(vbytes);
            d_kooffs = e->talloc<uint64_t>((n_out + 1) * 8);
            d_vooffs = e->talloc<uint64_t>((n_out + 1) * 8);
        }
        if (c->return_expire_ts)
            d_ets = e->talloc<int32_t>(n_out * 4);
        sev.record(2, e->stream);
        launch_emit_scan(dr, d_win, w, d_state, consumed, d_npos, d_koffs, d_voffs, sp, d_kout,
                         d_vout, d_kooffs, d_vooffs, d_ets, n_out, e->stream);
        sev.record(3, e->stream);
        if (c->on_device_out) {
            HIP_OK(hipStreamSynchronize(e->stream));
            out->dev_keys = d_kout;
            out->dev_key_offs = d_kooffs;
            out->dev_vals = d_vout;
            out->dev_val_offs = d_vooffs;
            a->dev_ptrs.insert(a->dev_ptrs.end(), {d_kout, d_vout, d_kooffs, d_vooffs});
        } else {
            uint8_t *kb = (uint8_t *)a->alloc(kbytes);
            uint8_t *vb = (uint8_t *)a->alloc(vbytes);
            std::vector<uint64_t> kooffs(n_out + 1), vooffs(n_out + 1);
            e->d2h(kb, d_kout, kbytes);
            e->d2h(vb, d_vout, vbytes);
            HIP_OK(hipMemcpyAsync(kooffs.data(), d_kooffs, (n_out + 1) * 8,
                                  hipMemcpyDeviceToHost, e->stream));
            HIP_OK(hipMemcpyAsync(vooffs.data(), d_vooffs, (n_out + 1) * 8,
                                  hipMemcpyDeviceToHost, e->stream));
            int32_t *ets = nullptr;
            if (d_ets) {
                ets = (int32_t *)a->alloc(n_out * 4);
                HIP_OK(hipMemcpyAsync(ets, d_ets, n_out * 4, hipMemcpyDeviceToHost, e->stream));
            }
            HIP_OK(hipStreamSynchronize(e->stream));
            out->keys = (rrdb_slice *)a->alloc(n_out * sizeof(rrdb_slice));
            out->values = (rrdb_slice *)a->alloc(n_out * sizeof(rrdb_slice));
            for (uint64_t i = 0; i < n_out; i++) {
                out->keys[i] = {kb + kooffs[i], kooffs[i + 1] - kooffs[i]};
                out->values[i] = {vb + vooffs[i], vooffs[i + 1] - vooffs[i]};
            }
            out->expire_ts = ets;
            e->tfree(d_kout);
            e->tfree(d_vout);
            e->tfree(d_kooffs);
            e->tfree(d_vooffs);
        }
        if (d_ets)
            e->tfree(d_ets); /* always pool-allocated; never handed out */
        out->count = n_out;
        e->tfree(d_koffs);
        e->tfree(d_voffs);
    }
    {
        float ms;
        HIP_OK(hipEventSynchronize(sev.ev[1]));
        HIP_OK(hipEventElapsedTime(&ms, sev.ev[0], sev.ev[1]));
        e->phase_ms["scan_state"] = ms;
        if (hipEventQuery(sev.ev[3]) == hipSuccess && sev.ms(2, 3, &ms))
            e->phase_ms["scan_emit"] = ms;
    }
    e->tfree(d_state);
    e->tfree(d_ksz);
    e->tfree(d_vsz);
    e->tfree(d_flags);
    e->tfree(d_npos);
    e->tfree(d_cut);
    c->cursor += consumed;
    out->error = RRDB_OK;
    out->context_id =
        (c->cursor >= c->view.n) ? RRDB_SCAN_CONTEXT_ID_COMPLETED : 0 /* caller parks */;
    /* time budget (range_read_limiter.h:56-79), batch granularity: an
     * over-budget incomplete batch returns kIncomplete, no re-park */
    if (out->context_id != RRDB_SCAN_CONTEXT_ID_COMPLETED && e->iter_time_ms > 0) {
        auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(
                      std::chrono::steady_clock::now() - t_start)
                      .count();
        if ((uint64_t)ms > e->iter_time_ms) {
            out->error = RRDB_INCOMPLETE;
            out->context_id = RRDB_SCAN_CONTEXT_ID_COMPLETED;
        }
    }
}

int32_t rrdb_scan_open(void *h, const rrdb_scan_request *q, uint32_t epoch_now, rrdb_result *out)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    Arena *a = read_begin(e, out);
    if (!a)
        return out->error;
    if (q->hash_key_filter_type < 0 || q->hash_key_filter_type > 3 ||
        q->sort_key_filter_type < 0 || q->sort_key_filter_type > 3 ||
        (q->hash_key_filter_type == RRDB_FT_MATCH_PREFIX &&
         !hklen_ok(q->hash_key_filter_pattern.len))) {
        out->error = RRDB_INVALID_ARGUMENT; /* on_get_scanner:1168-1186 */
        return out->error;
    }
    e->activate();
    KeyRange kr = scan_range(q);
    if (!kr.close()) {
        out->error = RRDB_OK; /* empty range: the arrays stay null */
        out->context_id = RRDB_SCAN_CONTEXT_ID_COMPLETED;
        return RRDB_OK;
    }
    auto *ctx = new HipScanCtx();
    ctx->view = e->build_view(&kr.start, &kr.stop_excl);
    /* first_exclusive: skip an exact start match (on_get_scanner:1277-1283) */
    if (!kr.start_inclusive && ctx->view.n > 0 && key_at_equals(e, ctx->view.d, kr.start))
        ctx->cursor = 1;
    ctx->batch_size = q->batch_size;
    ctx->no_value = q->no_value;
    ctx->validate_hash_req = q->validate_partition_hash;
    ctx->return_expire_ts = q->return_expire_ts;
    ctx->only_return_count = q->only_return_count;
    ctx->on_device_out = q->on_device_out;
    ctx->hk_ft = q->hash_key_filter_type;
    ctx->sk_ft = q->sort_key_filter_type;
    ctx->hk_pat_len = q->hash_key_filter_pattern.len;
    ctx->d_hk_pat = e->upload_bytes(q->hash_key_filter_pattern.data, ctx->hk_pat_len);
    ctx->sk_pat_len = q->sort_key_filter_pattern.len;
    ctx->d_sk_pat = e->upload_bytes(q->sort_key_filter_pattern.data, ctx->sk_pat_len);

    scan_batch_gpu(e, ctx, epoch_now, out, a);
    e->gc_ctxs(epoch_now);
    if (out->context_id == RRDB_SCAN_CONTEXT_ID_COMPLETED) {
        delete ctx;
    } else {
        ctx->id = ++e->next_ctx_id;
        ctx->parked_at = epoch_now;
        e->ctxs[ctx->id] = ctx;
        out->context_id = ctx->id;
    }
    return out->error;
}

int32_t rrdb_scan_next(void *h, int64_t context_id, uint32_t epoch_now, rrdb_result *out)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    Arena *a = result_init(out);
    e->activate();
    e->scratch_reset();
    e->gc_ctxs(epoch_now);
    HipScanCtx *c = nullptr;
    {
        auto it = e->ctxs.find(context_id);
        if (it != e->ctxs.end()) {
            c = it->second;
            e->ctxs.erase(it);
        }
    }
    if (!c) {
        out->error = RRDB_NOT_FOUND; /* on_scan:1539-1541; also the 5-min
                                        expired-context path (:1381-1387) */
        return out->error;
    }
    scan_batch_gpu(e, c, epoch_now, out, a);
    if (out->context_id == RRDB_SCAN_CONTEXT_ID_COMPLETED) {
        delete c;
    } else {
        c->id = ++e->next_ctx_id; /* re-park under a fresh handle (on_scan:1516-1526) */
        c->parked_at = epoch_now;
        e->ctxs[c->id] = c;
        out->context_id = c->id;
    }
    return out->error;
}

/* fused pipelined count scan (the count_data path,
 * src/shell/commands/data_operations.cpp:2305 fan-out): begin submits
 * bounds + anchor rows + the MODE=2 group-rank kernel with NO host sync, so
 * the caller can begin every partition and then finish each — partitions'
 * count kernels co-run on their per-engine streams exactly like the
 * split compaction.  Supports the full-count shape (only_return_count,
 * forward, start-inclusive, caps >= table size); other shapes return
 * kInvalidArgument and the caller falls back to rrdb_scan_open.  The 30s
 * time budget does not apply (single fused operation; documented
 * deviation like the batch-granular budget). */
int32_t rrdb_scan_count_begin(void *h, const rrdb_scan_request *q, uint32_t epoch_now)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    if (e->pend_scan.active)
        return RRDB_INVALID_ARGUMENT;
    if (engine_flush(e) != RRDB_OK)
        return RRDB_IO_ERROR;
    e->activate();
    if (!q->only_return_count || !q->start_inclusive || q->hash_key_filter_type < 0 ||
        q->hash_key_filter_type > 3 || q->sort_key_filter_type < 0 ||
        q->sort_key_filter_type > 3)
        return RRDB_INVALID_ARGUMENT;
    uint64_t total = 0;
    for (auto &r : e->runs)
        total += r.n;
    uint64_t batch_cap = q->batch_size > 0 ? (uint64_t)q->batch_size : (uint64_t)INT32_MAX;
    int R0 = (int)e->runs.size();
    bool single = R0 == 1; /* no merge/shadow needed: plain count kernel */
    if ((R0 > 1 && !e->grp_eligible(0, (size_t)R0)) || batch_cap < total ||
        e->max_iter_count < total)
        return RRDB_INVALID_ARGUMENT;
    if (R0 == 0) {
        e->pend_scan.active = true;
        e->pend_scan.trivial = true;
        e->pend_scan.trivial_count = 0;
        return RRDB_OK;
    }

    /* the pattern's length matters only where the prefix clamp uses it */
    if (q->hash_key_filter_type == RRDB_FT_MATCH_PREFIX && q->hash_key_filter_pattern.len > 0 &&
        !hklen_ok(q->hash_key_filter_pattern.len))
        return RRDB_INVALID_ARGUMENT;
    KeyRange kr = scan_range(q);
    kr.start_inclusive = true; /* the request's, required above */
    if (!kr.close()) {
        e->pend_scan.active = true;
        e->pend_scan.trivial = true;
        e->pend_scan.trivial_count = 0;
        return RRDB_OK; /* empty range */
    }
    e->pend_scan.trivial = false;
    const std::string &start = kr.start, &stop_excl = kr.stop_excl;

    int R = (int)e->runs.size();
    DevRun *dr = e->dev_runs();
    auto &ps = e->pend_scan;
    /* pooled allocations: grow-only, freed at close */
    if ((uint64_t)R * 8 > ps.lo_cap) {
        if (ps.d_lo)
            (void)hipFree(ps.d_lo);
        if (ps.d_hi)
            (void)hipFree(ps.d_hi);
        HIP_OK(hipMalloc(&ps.d_lo, R * 8));
        HIP_OK(hipMalloc(&ps.d_hi, R * 8));
        ps.lo_cap = (uint64_t)R * 8;
    }
    uint64_t need_bytes = start.size() + stop_excl.size() + q->hash_key_filter_pattern.len +
                          q->sort_key_filter_pattern.len + 4;
    if (need_bytes > ps.bytes_cap) {
        if (ps.d_start)
            (void)hipFree(ps.d_start);
        HIP_OK(hipMalloc(&ps.d_start, need_bytes));
        ps.bytes_cap = need_bytes;
    }
    uint64_t boff = 0;
    auto upl = [&](const uint8_t *p, uint64_t n) {
        uint8_t *d = ps.d_start + boff;
        if (n)
            HIP_OK(hipMemcpyAsync(d, p, n, hipMemcpyHostToDevice, e->stream));
        boff += n + 1;
        return d;
    };
    uint8_t *d_start_b = upl((const uint8_t *)start.data(), start.size());
    uint8_t *d_stop_b = upl((const uint8_t *)stop_excl.data(), stop_excl.size());
    launch_bounds(dr, R, d_start_b, start.size(), ps.d_lo, 0, e->stream);
    launch_bounds(dr, R, d_stop_b, stop_excl.size(), ps.d_hi, 0, e->stream);
    uint64_t n_groups = 0;
    if (!single) {
        /* anchors from the largest run's FULL size (the window is device-
         * side only); rows past the window collapse to sentinels in-kernel */
        int q0 = 0;
        uint64_t nmax = 0;
        for (int r = 0; r < R; r++)
            if (e->runs[r].n > nmax) {
                nmax = e->runs[r].n;
                q0 = r;
            }
        const int gs = grp_shift(R);
        n_groups = (nmax + (1ull << gs) - 1) >> gs;
        if (n_groups == 0)
            n_groups = 1;
        if ((n_groups + 1) * R * 8 > ps.anch_cap) {
            if (ps.d_anch)
                (void)hipFree(ps.d_anch);
            HIP_OK(hipMalloc(&ps.d_anch, (n_groups + 1) * R * 8));
            ps.anch_cap = (n_groups + 1) * R * 8;
        }
        launch_anchor_rows(dr, R, q0, ps.d_lo, ps.d_hi, gs, n_groups, ps.d_anch, e->stream);
    }

    ScanParams sp = base_scan_params(e, epoch_now);
    sp.validate_hash = (uint8_t)(q->validate_partition_hash && e->validate_hash);
    sp.hk_ft = q->hash_key_filter_type;
    sp.sk_ft = q->sort_key_filter_type;
    sp.hk_pat_len = q->hash_key_filter_pattern.len;
    sp.hk_pat = upl(q->hash_key_filter_pattern.data, q->hash_key_filter_pattern.len);
    sp.sk_pat_len = q->sort_key_filter_pattern.len;
    sp.sk_pat = upl(q->sort_key_filter_pattern.data, q->sort_key_filter_pattern.len);
    sp.no_value = 1;

    if (!ps.d_stats)
        HIP_OK(hipMalloc(&ps.d_stats, 8 * sizeof(CompactStatsDev)));
    HIP_OK(hipMemsetAsync(ps.d_stats, 0, 8 * sizeof(CompactStatsDev), e->stream));
    if (single)
        launch_count_single(dr, ps.d_lo, ps.d_hi, sp, ps.d_stats, e->runs[0].n, e->stream);
    else
        launch_rank_grp_count(dr, R, ps.d_lo, ps.d_anch, n_groups, sp, ps.d_stats, e->stream);
    ps.active = true;
    return RRDB_OK;
}

int32_t rrdb_scan_count_finish(void *h, rrdb_result *out)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    result_init(out);
    auto &ps = e->pend_scan;
    if (!ps.active) {
        out->error = RRDB_INVALID_ARGUMENT;
        return out->error;
    }
    ps.active = false;
    e->activate();
    if (ps.trivial) {
        out->i64 = ps.trivial_count;
        out->count = 0;
        out->error = RRDB_OK;
        out->context_id = RRDB_SCAN_CONTEXT_ID_COMPLETED;
        return RRDB_OK;
    }
    HIP_OK(hipStreamSynchronize(e->stream));
    CompactStatsDev hsb[8];
    HIP_OK(hipMemcpy(hsb, ps.d_stats, sizeof(hsb), hipMemcpyDeviceToHost));
    uint64_t count = 0;
    for (auto &b : hsb)
        count += b.output_records;
    /* pooled device buffers persist for the next count (freed at close) */
    ps.trivial = false;
    out->i64 = (int64_t)count;
    out->count = 0;
    out->error = RRDB_OK;
    out->context_id = RRDB_SCAN_CONTEXT_ID_COMPLETED;
    return RRDB_OK;
}

void rrdb_clear_scanner(void *h, int64_t context_id)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    auto it = e->ctxs.find(context_id);
    if (it != e->ctxs.end()) {
        e->activate();
        delete it->second;
        e->ctxs.erase(it);
    }
}

int32_t rrdb_sortkey_count(void *h, const uint8_t *hash_key, uint64_t hklen, uint32_t epoch_now,
                           rrdb_result *out)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    if (!read_begin(e, out))
        return out->error;
    e->activate();
    if (!hklen_ok(hklen)) {
        out->error = RRDB_INVALID_ARGUMENT;
        return out->error;
    }
    /* count all visible non-expired rows of the hash key — no count cap in
     * the reference's loop */
    KeyRange kr = hash_key_range(hash_key, hklen);
    (void)kr.close(); /* never empty (start < next(start)); called for stop_excl */
    DevView view = e->build_view(&kr.start, &kr.stop_excl);
    const uint64_t n = view.n;
    int64_t count = 0;
    if (n) {
        /* no hash validation, no filter */
        ScanParams sp = base_scan_params(e, epoch_now);
        uint8_t *d_state = e->talloc<uint8_t>(n);
        uint64_t *d_ksz = e->talloc<uint64_t>(n * 8);
        uint64_t *d_vsz = e->talloc<uint64_t>(n * 8);
        uint64_t *d_flags = e->talloc<uint64_t>(n * 8);
        uint64_t *d_npos = e->talloc<uint64_t>(n * 8);
        launch_scan_state(e->dev_runs(), view.d, n, sp, d_state, d_ksz, d_vsz, e->stream);
        launch_normal_flags(d_state, n, d_flags, e->stream);
        launch_psum(d_flags, d_npos, n, e->psum_scratch(n), e->stream);
        uint64_t last[2] = {0, 0};
        scan_tail_async(d_npos, d_flags, n, last, e->stream);
        HIP_OK(hipStreamSynchronize(e->stream));
        count = (int64_t)(last[0] + last[1]);
        e->tfree(d_state);
        e->tfree(d_ksz);
        e->tfree(d_vsz);
        e->tfree(d_flags);
        e->tfree(d_npos);
    }
    out->i64 = count;
    out->error = RRDB_OK;
    return RRDB_OK;
}

/* bounded busy-wait completion for the small-op serving path: the blocking
 * stream sync costs ~10-20us of wakeup latency per call */
static inline void spin_sync(hipStream_t st)
{
    hipError_t e;
    int spins = 0;
    while ((e = hipStreamQuery(st)) == hipErrorNotReady) {
        if (++spins > (1 << 22)) { /* ~seconds: fall back to blocking */
            HIP_OK(hipStreamSynchronize(st));
            return;
        }
    }
    HIP_OK(e);
}

/* it->Valid() after a limit exit (on_multi_get:777-788): does any
 * rocksdb-iterator-visible record exist beyond the range boundary?
 * forward: key >= bound; reverse: key < bound. */
static bool valid_beyond(HipEngine *e, const std::string &bound, bool reverse)
{
    if (e->runs.empty())
        return false;
    if ((int)e->runs.size() <= RRDB_MAX_RUNS) {
        uint32_t *d_out = e->talloc<uint32_t>(4);
        uint8_t *d_b = e->upload_tmp(bound.data(), bound.size());
        launch_valid_beyond(e->dev_runs(), (int)e->runs.size(), d_b, bound.size(),
                            reverse ? 1 : 0, d_out, e->stream);
        uint32_t v = 0;
        HIP_OK(hipMemcpyAsync(&v, d_out, 4, hipMemcpyDeviceToHost, e->stream));
        HIP_OK(hipStreamSynchronize(e->stream));
        e->tfree(d_out);
        e->tfree(d_b);
        return v != 0;
    }
    /* > RRDB_MAX_RUNS runs: fall back to a visible-view existence check */
    return (reverse ? e->build_view(nullptr, &bound) : e->build_view(&bound, nullptr)).n != 0;
}

/* the three bodies of multi_get, dispatched by multi_get_locked below them;
 * rep is the call's lane report, only ever written */

/* point-list variant (on_multi_get:779-860) over the batched-get core */
static int32_t mg_point_list(HipEngine *e, const rrdb_multi_get_request *q, const MgLimits &lim,
                             uint32_t epoch_now, rrdb_result *out, Arena *a)
{
    std::vector<uint64_t> offs(q->n_sort_keys + 1);
    std::string keys;
    for (uint64_t i = 0; i < q->n_sort_keys; i++) {
        offs[i] = keys.size();
        keys += make_key(q->hash_key.data, q->hash_key.len, q->sort_keys + q->sort_key_offs[i],
                         q->sort_key_offs[i + 1] - q->sort_key_offs[i]);
    }
    offs[q->n_sort_keys] = keys.size();
    std::vector<int32_t> status;
    std::vector<std::pair<const uint8_t *, uint64_t>> vals;
    get_core(e, q->n_sort_keys, (const uint8_t *)keys.data(), offs.data(), epoch_now, status,
             vals, a);
    out->keys = (rrdb_slice *)a->alloc(q->n_sort_keys * sizeof(rrdb_slice));
    out->values = (rrdb_slice *)a->alloc(q->n_sort_keys * sizeof(rrdb_slice));
    uint64_t m = 0;
    int64_t count = 0, size = 0;
    bool exceed = false;
    for (uint64_t i = 0; i < q->n_sort_keys; i++) {
        if (status[i] != RRDB_OK)
            continue;
        if (count >= (int64_t)lim.max_kv_count || size >= lim.max_kv_size) {
            exceed = true; /* :837-841 */
            break;
        }
        uint64_t sklen = q->sort_key_offs[i + 1] - q->sort_key_offs[i];
        uint8_t *kc = (uint8_t *)a->alloc(sklen);
        memcpy(kc, q->sort_keys + q->sort_key_offs[i], sklen);
        out->keys[m] = {kc, sklen};
        if (!q->no_value)
            out->values[m] = {(uint8_t *)vals[i].first, vals[i].second};
        else
            out->values[m] = {nullptr, 0};
        count++;
        size += (int64_t)out->keys[m].len + (int64_t)out->values[m].len;
        m++;
    }
    out->count = m;
    out->error = exceed ? RRDB_INCOMPLETE : RRDB_OK;
    return out->error;
}

/* ---- fused single-launch fast path (small ranges, the YCSB-E shape), at most
 * RRDB_MAX_RUNS runs: one pinned H2D of the request bytes, one launch, one
 * pinned D2H of hdr + blob prefix, one sync; or the same kernel body behind the
 * resident server or the captured graph.  False: range too large or a row
 * oversize, the general lane has to serve it. ---- */
static bool mg_fused(HipEngine *e, const rrdb_multi_get_request *q, const KeyRange &kr,
                     const MgLimits &lim, uint32_t epoch_now, rrdb_result *out, Arena *a,
                     rrdb_multi_get_lane *rep)
{
    const std::string &start = kr.start, &stop_excl = kr.stop_excl;
    e->mg_lane_init();
    MgFusedArgs fa{};
    uint64_t in_n = start.size() + stop_excl.size() + q->sort_key_filter_pattern.len;
    const uint8_t *d_blob = nullptr;
    const uint8_t *h_resp = e->mg_hout;
    bool served = false;
    int32_t fused_lane = RRDB_MG_LANE_SMALL;
    /* the request slice of the server and graph lanes: MgGraphHdr, then the bytes */
    auto fill_slice = [&](uint8_t *req) {
        MgGraphHdr *hh = (MgGraphHdr *)req;
        hh->start_len = (uint32_t)start.size();
        hh->stop_len = (uint32_t)stop_excl.size();
        hh->sk_pat_len = (uint32_t)q->sort_key_filter_pattern.len;
        hh->start_inclusive = kr.start_inclusive;
        hh->stop_inclusive = kr.stop_inclusive;
        hh->reverse = q->reverse;
        hh->no_value = q->no_value;
        hh->max_kv_count = lim.max_kv_count;
        hh->max_iteration_count = lim.max_iteration_count;
        hh->max_iteration_size = lim.max_iter_size;
        hh->sk_ft = q->sort_key_filter_type;
        hh->epoch_now = epoch_now;
        hh->data_version = e->data_version;
        hh->hash_key_skip = 2 + q->hash_key.len;
        uint8_t *pp = req + sizeof(MgGraphHdr);
        memcpy(pp, start.data(), start.size());
        pp += start.size();
        memcpy(pp, stop_excl.data(), stop_excl.size());
        pp += stop_excl.size();
        if (q->sort_key_filter_pattern.len)
            memcpy(pp, q->sort_key_filter_pattern.data, q->sort_key_filter_pattern.len);
    };
    if (sizeof(MgGraphHdr) + in_n <= MG_GRAPH_IN && e->mg_persist_wanted() &&
        e->server_ready()) {
        /* resident-kernel lane: write the request slice, bump the doorbell, spin for completion */
        fill_slice(e->mg_mb->req);
        uint64_t seq = ++e->mg_srv_seq;
        __atomic_store_n(&e->mg_mb->req_seq, seq, __ATOMIC_RELEASE);
        auto t0 = std::chrono::steady_clock::now();
        bool ok = true;
        while (__atomic_load_n(&e->mg_mb->done_seq, __ATOMIC_ACQUIRE) != seq) {
            auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(
                          std::chrono::steady_clock::now() - t0)
                          .count();
            if (ms > 2 && !__atomic_load_n(&e->mg_mb->alive, __ATOMIC_ACQUIRE)) {
                /* idle-expired between the readiness check and the doorbell: relaunch (seq
                 * rewound so the fresh kernel sees this request as new) and re-ring */
                e->mg_srv_gen = ~0ull;
                e->mg_srv_seq = seq - 1;
                bool up = e->server_ready();
                e->mg_srv_seq = seq;
                if (!up) {
                    ok = false;
                    break;
                }
                __atomic_store_n(&e->mg_mb->req_seq, seq, __ATOMIC_RELEASE);
                t0 = std::chrono::steady_clock::now();
                continue;
            }
            if (ms > 200) {
                ok = false; /* server died: fall to the graph lane */
                break;
            }
        }
        if (ok) {
            h_resp = e->mg_mb->resp;
            d_blob = e->mg_dout + 32;
            served = true;
            fused_lane = RRDB_MG_LANE_SERVER;
        }
    }
    if (!served && sizeof(MgGraphHdr) + in_n <= MG_GRAPH_IN && e->mg_graph_ready()) {
        /* captured-graph lane: fill the request slice, one graph launch */
        fill_slice(e->mg_hin);
        HIP_OK(hipGraphLaunch(e->mg_graph, e->stream));
        spin_sync(e->stream);
        d_blob = e->mg_dout + 32;
        served = true;
        fused_lane = RRDB_MG_LANE_GRAPH;
    }
    if (!served && in_n <= HipEngine::MG_IN_CAP) {
        uint64_t o = 0;
        memcpy(e->mg_hin + o, start.data(), start.size());
        fa.start = e->mg_din + o;
        o += start.size();
        memcpy(e->mg_hin + o, stop_excl.data(), stop_excl.size());
        fa.stop = e->mg_din + o;
        o += stop_excl.size();
        if (q->sort_key_filter_pattern.len)
            memcpy(e->mg_hin + o, q->sort_key_filter_pattern.data, q->sort_key_filter_pattern.len);
        fa.sk_pat = e->mg_din + o;
        HIP_OK(hipMemcpyAsync(e->mg_din, e->mg_hin, in_n ? in_n : 1,
                              hipMemcpyHostToDevice, e->stream));
    } else if (!served) { /* giant keys: pageable per-piece uploads */
        fa.start = e->upload_tmp(start.data(), start.size());
        fa.stop = e->upload_tmp(stop_excl.data(), stop_excl.size());
        fa.sk_pat = e->upload_tmp(q->sort_key_filter_pattern.data, q->sort_key_filter_pattern.len);
    }
    fa.start_len = start.size();
    fa.stop_len = stop_excl.size();
    fa.start_inclusive = kr.start_inclusive;
    fa.stop_inclusive = kr.stop_inclusive;
    fa.reverse = q->reverse;
    fa.no_value = q->no_value;
    fa.max_kv_count = lim.max_kv_count;
    fa.max_iteration_count = lim.max_iteration_count;
    fa.max_iteration_size = lim.max_iter_size;
    fa.sk_ft = q->sort_key_filter_type;
    fa.sk_pat_len = q->sort_key_filter_pattern.len;
    fa.epoch_now = epoch_now;
    fa.data_version = e->data_version;
    fa.hash_key_skip = 2 + q->hash_key.len;
    if (!served) {
        uint8_t *d_out = e->talloc<uint8_t>(32 + MG_BLOB_BYTES);
        fa.out_hdr = (int64_t *)d_out;
        fa.out_blob = d_out + 32;
        launch_multi_get_small(e->dev_runs(), (int)e->runs.size(), fa, e->stream);
        HIP_OK(hipMemcpyAsync(e->mg_hout, d_out, 32 + HipEngine::MG_OUT_PREFIX,
                              hipMemcpyDeviceToHost, e->stream));
        spin_sync(e->stream);
        d_blob = fa.out_blob;
    }
    const int64_t *hdr4 = (const int64_t *)h_resp;
    if (hdr4[0] >= 0) {
        rep->lane = fused_lane;
        uint64_t m = (uint64_t)hdr4[0];
        uint64_t kb = (uint64_t)hdr4[2], vb = (uint64_t)hdr4[3];
        int64_t complete_flag = hdr4[1];
        out->keys = (rrdb_slice *)a->alloc(m * sizeof(rrdb_slice));
        out->values = (rrdb_slice *)a->alloc(m * sizeof(rrdb_slice));
        if (m) {
            uint64_t blob_n = 2 * (m + 1) * 8 + kb + vb;
            uint8_t *hb = (uint8_t *)a->alloc(blob_n);
            if (blob_n <= HipEngine::MG_OUT_PREFIX) {
                memcpy(hb, h_resp + 32, blob_n); /* already on host */
            } else {
                rep->tail_read = 1;
                HIP_OK(hipMemcpyAsync(hb, d_blob, blob_n, hipMemcpyDeviceToHost, e->stream));
                HIP_OK(hipStreamSynchronize(e->stream));
            }
            const uint64_t *koffs = (const uint64_t *)hb;
            const uint64_t *voffs = koffs + (m + 1);
            uint8_t *hk = hb + 2 * (m + 1) * 8;
            uint8_t *hv = hk + kb;
            for (uint64_t j = 0; j < m; j++) {
                out->keys[j] = {hk + koffs[j], koffs[j + 1] - koffs[j]};
                out->values[j] = {hv + voffs[j], voffs[j + 1] - voffs[j]};
            }
        }
        out->count = m;
        out->error = complete_flag ? RRDB_OK : RRDB_INCOMPLETE;
        return true;
    }
    /* fallback: large range or oversize rows — the general lane */
    rep->fused_first = fused_lane;
    return false;
}

/* the general lane: the range's view, the per-record state of a window of it,
 * and the reference's limiter loop over that window on the host */
static int32_t mg_general(HipEngine *e, const rrdb_multi_get_request *q, const KeyRange &kr,
                          const MgLimits &lim, uint32_t epoch_now, rrdb_result *out, Arena *a)
{
    const std::string &start = kr.start, &stop = kr.stop;
    const bool start_inclusive = kr.start_inclusive, stop_inclusive = kr.stop_inclusive;
    const DevView view = e->build_view(&start, &kr.stop_excl);
    const uint64_t *d_view = view.d;
    const uint64_t n = view.n;
    if (n == 0) {
        out->error = RRDB_OK;
        return RRDB_OK;
    }
    /* window: the limiter consumes at most mg_max_iter_count iterations plus
     * one possible uncounted first/last-exclusive skip */
    uint64_t wcap = (uint64_t)lim.max_iteration_count + 1;
    uint64_t wstart = 0, w = std::min<uint64_t>(n, wcap);
    if (q->reverse)
        wstart = n - w;
    DevRun *dr = e->dev_runs();
    /* no hash validation, no hash-key filter */
    ScanParams sp = base_scan_params(e, epoch_now);
    sp.sk_ft = q->sort_key_filter_type;
    sp.sk_pat_len = q->sort_key_filter_pattern.len;
    uint8_t *d_skpat = e->upload_tmp(q->sort_key_filter_pattern.data, sp.sk_pat_len);
    sp.sk_pat = d_skpat;
    sp.no_value = q->no_value;
    sp.hash_key_skip = 2 + q->hash_key.len; /* emit sortkey only (:2496-2499) */

    uint8_t *d_state = e->talloc<uint8_t>(w);
    uint64_t *d_ksz = e->talloc<uint64_t>(w * 8);
    uint64_t *d_vsz = e->talloc<uint64_t>(w * 8);
    /* sortkey filter types: scan_state's sk filter operates on key minus
     * 2+hklen prefix — same as multi_get's sortkey check */
    launch_scan_state(dr, d_view + wstart, w, sp, d_state, d_ksz, d_vsz, e->stream);
    std::vector<uint8_t> state(w);
    std::vector<uint64_t> ksz(w), vsz(w);
    HIP_OK(hipMemcpyAsync(state.data(), d_state, w, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipMemcpyAsync(ksz.data(), d_ksz, w * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipMemcpyAsync(vsz.data(), d_vsz, w * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    e->tfree(d_state);
    e->tfree(d_ksz);
    e->tfree(d_vsz);

    /* host limiter loop, mirroring on_multi_get:616-778 exactly */
    int64_t count = 0, size = 0;
    uint64_t iteration_count = 0;
    std::vector<uint64_t> sel; /* view positions to emit, ascending */
    bool complete = false;
    bool skipped_first = false;
    /* reverse + start-exclusive: a record == start is OUT OF RANGE for the
     * reverse walk (on_multi_get:697-700) — excluded, and it keeps the
     * iterator Valid() on a limit exit */
    uint64_t lo_skip = 0;
    if (q->reverse && !start_inclusive && wstart == 0 && n > 0)
        lo_skip = key_at_equals(e, d_view, start) ? 1 : 0;
    uint64_t steps = w;
    for (uint64_t s = 0; s < steps; s++) {
        uint64_t wi = q->reverse ? (steps - 1 - s) : s;
        if (q->reverse && lo_skip && wi == 0)
            break; /* reached the excluded == start record: out of range */
        if (count >= (int64_t)lim.max_kv_count || iteration_count >= lim.max_iteration_count ||
            size >= lim.max_iter_size)
            break;
        /* first-exclusive skip of the exact boundary key: the host has the
         * sizes only, so a device compare */
        if (s == 0) {
            bool check = (!q->reverse && !start_inclusive) || (q->reverse && !stop_inclusive);
            if (check && key_at_equals(e, d_view + wstart + wi, q->reverse ? stop : start)) {
                skipped_first = true;
                continue;
            }
        }
        iteration_count++;
        if (state[wi] != ST_NORMAL)
            continue; /* kExpired / kFiltered */
        sel.push_back(wstart + wi);
        count++;
        size += (int64_t)ksz[wi] + (int64_t)vsz[wi];
    }
    /* completion (on_multi_get:777-788): kIncomplete iff the iterator is
     * still Valid() after a limit exit — even when the remaining records lie
     * past the range.  Exception: the post-append c==0 break
     * (:668-672/:739-744) completes when the LAST iterated record equals the
     * inclusive far boundary, regardless of limits. */
    {
        bool boundary_hit = false;
        uint64_t countable_chk = w - (skipped_first ? 1 : 0) - lo_skip;
        if (iteration_count >= countable_chk && iteration_count > 0 && w == n && w > 0 &&
            ((!q->reverse && stop_inclusive) || (q->reverse && start_inclusive))) {
            /* last iterated in-range record = the far end of the view */
            uint64_t vidx = q->reverse ? (lo_skip) : (n - 1);
            boundary_hit = key_at_equals(e, d_view + vidx, q->reverse ? start : stop);
        }
        bool limit_exit = !boundary_hit && (count >= (int64_t)lim.max_kv_count ||
                                            iteration_count >= lim.max_iteration_count ||
                                            size >= lim.max_iter_size);
        uint64_t countable = w - (skipped_first ? 1 : 0) - lo_skip;
        bool consumed_all = (iteration_count >= countable);
        if (w < n || !consumed_all)
            complete = false; /* in-range records remain: iterator valid */
        else if (!limit_exit)
            complete = true; /* walked past the range end */
        else if (q->reverse)
            complete = !(lo_skip || valid_beyond(e, start, true));
        else
            complete = !valid_beyond(e, kr.stop_excl, false);
    }
    uint64_t m = sel.size();
    if (q->reverse)
        std::reverse(sel.begin(), sel.end()); /* ascending output (:758-765) */
    out->keys = (rrdb_slice *)a->alloc(m * sizeof(rrdb_slice));
    out->values = (rrdb_slice *)a->alloc(m * sizeof(rrdb_slice));
    if (m > 0) {
        std::vector<uint64_t> koffs(m + 1), voffs(m + 1);
        uint64_t kb = 0, vb = 0;
        for (uint64_t j = 0; j < m; j++) {
            uint64_t wi = sel[j] - wstart;
            koffs[j] = kb;
            voffs[j] = vb;
            kb += ksz[wi];
            vb += vsz[wi];
        }
        koffs[m] = kb;
        voffs[m] = vb;
        uint64_t *d_rows = (uint64_t *)e->upload_tmp(sel.data(), m * 8);
        uint64_t *d_ko = (uint64_t *)e->upload_tmp(koffs.data(), (m + 1) * 8);
        uint64_t *d_vo = (uint64_t *)e->upload_tmp(voffs.data(), (m + 1) * 8);
        uint8_t *d_kout = e->talloc<uint8_t>(kb);
        uint8_t *d_vout = e->talloc<uint8_t>(vb);
        launch_emit_rows(dr, d_view, d_rows, m, d_ko, d_vo, sp, d_kout, d_vout, e->stream);
        uint8_t *hkb = (uint8_t *)a->alloc(kb);
        uint8_t *hvb = (uint8_t *)a->alloc(vb);
        HIP_OK(hipMemcpyAsync(hkb, d_kout, kb, hipMemcpyDeviceToHost, e->stream));
        HIP_OK(hipMemcpyAsync(hvb, d_vout, vb, hipMemcpyDeviceToHost, e->stream));
        HIP_OK(hipStreamSynchronize(e->stream));
        for (uint64_t j = 0; j < m; j++) {
            out->keys[j] = {hkb + koffs[j], koffs[j + 1] - koffs[j]};
            out->values[j] = {hvb + voffs[j], voffs[j + 1] - voffs[j]};
        }
        e->tfree(d_rows);
        e->tfree(d_ko);
        e->tfree(d_vo);
        e->tfree(d_kout);
        e->tfree(d_vout);
    }
    e->tfree(d_skpat);
    out->count = m;
    out->error = complete ? RRDB_OK : RRDB_INCOMPLETE; /* :789-799 */
    return out->error;
}

/* body of on_multi_get; caller holds the engine lock */
static int32_t multi_get_locked(void *h, const rrdb_multi_get_request *q, uint32_t epoch_now,
                                rrdb_result *out, rrdb_multi_get_lane *rep)
{
    auto *e = (HipEngine *)h;
    /* a batch's per-request fallbacks hand in a scratch report */
    rep->lane = RRDB_MG_LANE_NONE;
    rep->fused_first = RRDB_MG_LANE_NONE;
    rep->tail_read = 0;
    Arena *a = read_begin(e, out);
    if (!a)
        return out->error;
    e->activate();
    if (q->sort_key_filter_type < 0 || q->sort_key_filter_type > 3 ||
        !hklen_ok(q->hash_key.len)) {
        out->error = RRDB_INVALID_ARGUMENT; /* on_multi_get:508-517 */
        return out->error;
    }
    const MgLimits lim(e, q);
    if (q->n_sort_keys > 0) {
        rep->lane = RRDB_MG_LANE_POINT_LIST;
        return mg_point_list(e, q, lim, epoch_now, out, a);
    }
    /* range variant (on_multi_get:540-778) */
    KeyRange kr = mg_range(q);
    if (!kr.close()) {
        out->error = RRDB_OK; /* empty range: no lane */
        return RRDB_OK;
    }
    if (!e->runs.empty() && (int)e->runs.size() <= RRDB_MAX_RUNS &&
        mg_fused(e, q, kr, lim, epoch_now, out, a, rep))
        return out->error;
    rep->lane = RRDB_MG_LANE_GENERAL;
    return mg_general(e, q, kr, lim, epoch_now, out, a);
}

int32_t rrdb_multi_get(void *h, const rrdb_multi_get_request *q, uint32_t epoch_now,
                       rrdb_result *out)
{
    std::lock_guard<std::mutex> g(((HipEngine *)h)->mu);
    return multi_get_locked(h, q, epoch_now, out, &((HipEngine *)h)->last_mg_lane);
}

int32_t rrdb_last_multi_get_lane(void *h, rrdb_multi_get_lane *out)
{
    if (!out)
        return RRDB_INVALID_ARGUMENT;
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    *out = e->last_mg_lane;
    return RRDB_OK;
}

int32_t rrdb_last_view_route(void *h, rrdb_view_route *out)
{
    if (!out)
        return RRDB_INVALID_ARGUMENT;
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    *out = e->last_view;
    return RRDB_OK;
}

/* ---- the compaction pass ----
 * It merges the window [first, first+n) of e->runs (0 = oldest) into one run
 * that takes the window's place; it is bottommost iff first == 0.
 * win == nullptr is the manual pass: every run, honouring
 * manual_compact.disabled and engine.emit_mode.  A window pass (the caller
 * validated it after flushing) always takes the chunked emit, the only one
 * that knows converted tombstones.  compact_begin's four steps come first. */
struct CompactWindow {
    size_t first, n;
};
using CompactPlan = HipEngine::CompactPlan;
static constexpr uint64_t COMPACT_BT_MIN_RECORDS = 100000; /* bound table above this */

/* step 1, host decisions only: the window, the emit the pass is built for and
 * which arrays that emit can do without */
static CompactPlan plan_pass(const HipEngine *e, const rrdb_compact_options *opts,
                             const CompactWindow *win)
{
    CompactPlan p;
    p.active = true;
    p.keep_inputs = opts && opts->keep_inputs;
    p.first = win ? win->first : 0;
    p.R = (int)(win ? win->n : e->runs.size());
    p.bottommost = p.first == 0;
    p.emit_mode = win ? 2 : e->emit_mode;
    const RunBuf *wr = e->runs.data() + p.first; /* the window's runs */
    for (int r = 0; r < p.R; r++)
        p.total += wr[r].n;
    p.st.input_records = p.total;
    p.trivial = p.total == 0;
    if (p.trivial)
        return p;
    /* all-fixed-stride fast mode: every run shares one key and one value
     * stride (the hashkey-table schema), so output offsets derive from the
     * keep count — no ksz/vsz arrays, one prefix sum instead of three.  Not
     * when non-bottommost: tombstone rows (kept or converted) are not fv long.
     * The fused emit indexes inside a tile in 32 bits, hence the stride cap. */
    const uint32_t ffk = shared_stride(wr, p.R, &RunBuf::fixed_klen);
    const uint32_t ffv = shared_stride(wr, p.R, &RunBuf::fixed_vlen_put);
    if (ffk > 0 && ffv > 0 && p.emit_mode == 2 && p.bottommost && ffk <= EMIT_MAX_STRIDE &&
        ffv <= EMIT_MAX_STRIDE)
        p.fk = ffk, p.fv = ffv;
    /* no default-TTL and no user ops => the filter can never rewrite a
     * value: skip the changed/new_expire arrays and the patch pass.  Not so
     * when non-bottommost: an expired PUT is rewritten into a tombstone and
     * changed[] carries that marker. */
    p.no_rewrite = e->default_ttl == 0 && e->n_ops == 0 && p.emit_mode == 2 && p.bottommost;
    return p;
}

/* step 2: the pass's arena arrays, each only where step 1 left it needed */
static void alloc_pass_arrays(HipEngine *e, CompactPlan &p)
{
    const int R = p.R;
    const uint64_t total = p.total;
    const RunBuf *wr = e->runs.data() + p.first;
    /* rows | lo | hi | wprefix travel as one upload: [R DevRun] [R] [R] [R + 1].
     * The rows are the pass's own: e->d_runs may be rebuilt before finish. */
    static_assert(sizeof(DevRun) % 8 == 0, "DevRun rows precede 8-byte bounds");
    const size_t row_words = sizeof(DevRun) / 8;
    std::vector<uint64_t> up(R * row_words + 3 * (size_t)R + 1, 0);
    uint64_t *bounds = up.data() + R * row_words;
    uint64_t acc = 0;
    for (int r = 0; r < R; r++) {
        const DevRun row = HipEngine::to_dev(wr[r]);
        memcpy(up.data() + r * row_words, &row, sizeof(row));
        bounds[R + r] = wr[r].n;
        bounds[2 * R + r] = acc;
        acc += wr[r].n;
    }
    bounds[3 * R] = acc;
    p.dr = (DevRun *)e->upload_tmp(up.data(), up.size() * 8);
    p.d_lo = (uint64_t *)(p.dr + R);
    p.d_hi = p.d_lo + R;
    p.d_wp = p.d_hi + R;
    p.d_order = e->talloc<uint64_t>(total * 8);
    if (!p.no_rewrite) {
        p.d_changed = e->talloc<uint8_t>(total);
        p.d_new_expire = e->talloc<uint32_t>(total * 4);
    }
    p.d_keepw = e->talloc<uint64_t>(total * 8);
    if (!p.fk) {
        /* all-fixed-stride has none of these: its emit scans the keep flags by tile */
        p.d_ksz = e->talloc<uint64_t>(total * 8);
        p.d_vsz = e->talloc<uint64_t>(total * 8);
        p.d_kpos = e->talloc<uint64_t>(total * 8);
        p.d_koffs = e->talloc<uint64_t>(total * 8);
        p.d_voffs = e->talloc<uint64_t>(total * 8);
    } else {
        p.d_tile_base = e->talloc<uint64_t>(emit_n_tiles(total) * 8);
    }
    if (p.emit_mode == 1)
        p.d_rank_of = e->talloc<uint64_t>(total * 8);
    /* 8 stat banks: the group rank flushes per-block tallies to bank
     * blockIdx&7; legacy kernels add to bank 0; finish sums all banks */
    p.d_stats = e->talloc<CompactStatsDev>(8 * sizeof(CompactStatsDev));
    HIP_OK(hipMemsetAsync(p.d_stats, 0, 8 * sizeof(CompactStatsDev), e->stream));
}

/* step 3: one of four rank kernels between ev[0] and ev[1]; the tables it
 * narrows by are built in front of ev[0] */
static void rank_pass(HipEngine *e, const CompactPlan &p, uint32_t epoch_now)
{
    const int R = p.R;
    DevRun *dr = p.dr;
    std::vector<uint64_t> lo(R, 0), hi(R); /* full-range rank merge */
    for (int r = 0; r < R; r++)
        hi[r] = e->runs[p.first + r].n;
    CompactParams cp{};
    cp.epoch_now = epoch_now;
    cp.data_version = e->data_version;
    cp.default_ttl = e->default_ttl;
    cp.pidx = e->pidx;
    cp.partition_version = e->partition_version;
    cp.validate_hash = e->validate_hash ? 1 : 0;
    cp.ops = e->d_ops;
    cp.n_ops = e->n_ops;
    cp.rules = e->d_rules;
    cp.pats = e->d_pats;
    cp.bottommost = p.bottommost ? 1 : 0;
    hipEvent_t *ev = e->kept.ev;
    if (e->rank_mode == 1 && R > 1 && R <= RRDB_MAX_RUNS && p.emit_mode == 2) {
        /* LDS-staged block rank: shift-8 bound table + per-run block counts.
         * The kernel keeps per-run window tables of RRDB_MAX_RUNS entries in
         * LDS; more runs than that take the global rank below */
        e->kept.route.rank = RRDB_ROUTE_RANK_LDS;
        uint64_t *c_off = nullptr, *c_bt = nullptr, *d_bt8_off = nullptr, *d_bt8 = nullptr;
        uint64_t wmax = 0;
        for (int r = 0; r < R; r++)
            wmax = std::max(wmax, hi[r] - lo[r]);
        if ((wmax >> 14) > 8)
            e->build_bound_table_level(dr, R, lo, hi, p.d_lo, p.d_hi, 14, nullptr, nullptr, 0,
                                       &c_off, &c_bt);
        e->build_bound_table_level(dr, R, lo, hi, p.d_lo, p.d_hi, 8, c_off, c_bt, 14,
                                   &d_bt8_off, &d_bt8);
        std::vector<uint64_t> blkp(R + 1);
        uint64_t nb = 0;
        for (int r = 0; r < R; r++) {
            blkp[r] = nb;
            nb += (hi[r] - lo[r] + 255) >> 8;
        }
        blkp[R] = nb;
        uint64_t *d_blkp = (uint64_t *)e->upload_tmp(blkp.data(), (R + 1) * 8);
        HIP_OK(hipEventRecord(ev[0], e->stream));
        launch_rank_compact_lds(dr, R, p.d_lo, p.d_hi, d_blkp, nb, cp, d_bt8_off, d_bt8,
                                p.d_order, p.d_keepw, p.d_changed, p.d_new_expire, p.d_ksz,
                                p.d_vsz, p.d_stats, e->stream);
        HIP_OK(hipEventRecord(ev[1], e->stream));
        return;
    }
    /* the input-major emit needs rank_of[], which the group rank does not write */
    const HipEngine::RankPrep rp =
        e->prepare_rank(dr, p.first, R, lo, hi, p.d_lo, p.d_hi, p.total, COMPACT_BT_MIN_RECORDS,
                        p.emit_mode != 1);
    e->kept.route.rank = rp.route;
    HIP_OK(hipEventRecord(ev[0], e->stream));
    if (rp.route == RRDB_ROUTE_RANK_GRP)
        launch_rank_grp_compact(dr, R, p.d_lo, rp.d_anch, rp.n_groups, cp, p.d_order, p.d_keepw,
                                p.d_changed, p.d_new_expire, p.d_ksz, p.d_vsz, p.d_stats,
                                e->grp_blocks, e->stream);
    else if (rp.route == RRDB_ROUTE_RANK_LDST)
        launch_rank_compact_ldst(dr, R, p.d_lo, p.d_hi, p.d_wp, p.total, cp, p.d_order,
                                 p.d_keepw, p.d_changed, p.d_new_expire, p.d_ksz, p.d_vsz,
                                 p.d_rank_of, rp.d_bt_off, rp.d_bt, e->bt_shift, p.d_stats,
                                 e->stream);
    else
        launch_rank_compact(dr, R, p.d_lo, p.d_hi, p.d_wp, p.total, cp, p.d_order, p.d_keepw,
                            p.d_changed, p.d_new_expire, p.d_ksz, p.d_vsz, p.d_rank_of,
                            rp.d_bt_off, rp.d_bt, e->bt_shift, p.d_stats, e->stream);
    HIP_OK(hipEventRecord(ev[1], e->stream));
}

/* step 4: the size scans, and the stats and the six sizes (one when
 * all-fixed-stride) on their way to the pinned targets finish reads */
static void submit_sizes(HipEngine *e, const CompactPlan &p)
{
    const uint64_t total = p.total;
    HIP_OK(hipEventRecord(e->kept.ev[2], e->stream));
    HIP_OK(hipMemcpyAsync(e->kept.stats, p.d_stats, 8 * sizeof(CompactStatsDev),
                          hipMemcpyDeviceToHost, e->stream));
    uint64_t *t = e->kept.sizes;
    memset(t, 0, 6 * 8);
    if (p.fk) {
        /* only the per-tile keep counts are summed here; the scan's grand
         * total is the whole keep count: t[1] stays 0 */
        const uint64_t n_tiles = emit_n_tiles(total);
        uint32_t *d_tile_cnt = e->talloc<uint32_t>(n_tiles * 4);
        uint64_t *d_n_out = e->talloc<uint64_t>(8);
        launch_keep_tile_scan(p.d_keepw, total, d_tile_cnt, p.d_tile_base, d_n_out, e->stream);
        HIP_OK(hipMemcpyAsync(&t[0], d_n_out, 8, hipMemcpyDeviceToHost, e->stream));
        return;
    }
    launch_psum(p.d_keepw, p.d_kpos, total, e->psum_scratch(total), e->stream);
    launch_psum(p.d_ksz, p.d_koffs, total, e->psum_scratch(total), e->stream);
    launch_psum(p.d_vsz, p.d_voffs, total, e->psum_scratch(total), e->stream);
    scan_tail_async(p.d_kpos, p.d_keepw, total, &t[0], e->stream);
    scan_tail_async(p.d_koffs, p.d_ksz, total, &t[2], e->stream);
    scan_tail_async(p.d_voffs, p.d_vsz, total, &t[4], e->stream);
}

/* phase 1 (the pipelined-partitions seam; the reference runs per-replica
 * compactions concurrently on THREAD_POOL_COMPACT —
 * pegasus_server_impl.cpp:3373): submit rank + prefix sums + async size
 * reads, NO host-blocking sync.  Caller holds the handle lock. */
static int32_t compact_begin(HipEngine *e, const rrdb_compact_options *opts, uint32_t epoch_now,
                             const CompactWindow *win = nullptr)
{
    if (e->pend.active)
        return RRDB_INVALID_ARGUMENT;
    if (engine_flush(e) != RRDB_OK) /* memtable visible to reads */
        return RRDB_IO_ERROR;
    e->scratch_reset();
    if (!win && e->manual_compact_disabled)
        return RRDB_INVALID_ARGUMENT;
    e->activate();
    e->kept.route = {RRDB_ROUTE_NONE, RRDB_ROUTE_NONE};
    CompactPlan p = plan_pass(e, opts, win);
    if (!p.trivial) {
        e->kept.init();
        e->resolve_phase_events(); /* previous pass's timing, before reuse */
        e->kept.have_emit = false;
        alloc_pass_arrays(e, p);
        rank_pass(e, p, epoch_now);
        submit_sizes(e, p);
        e->arena_pin(); /* reads between begin/finish must not reuse the plan's arrays */
    }
    e->pend = p;
    return RRDB_OK;
}

/* finish, after its sync: output sizes, and the summed stat banks into p.st */
struct PassSizes {
    uint64_t n_out, kbytes, vbytes;
    bool tombstone_out; /* a tombstone was emitted (non-bottommost only) */
};
static PassSizes read_sizes_and_stats(const HipEngine *e, CompactPlan &p)
{
    const uint64_t *t = e->kept.sizes;
    PassSizes s;
    s.n_out = t[0] + t[1];
    s.kbytes = p.fk ? s.n_out * p.fk : t[2] + t[3];
    s.vbytes = p.fk ? s.n_out * p.fv : t[4] + t[5];
    CompactStatsDev hs{};
    for (int b = 0; b < 8; b++) {
        hs.shadowed += e->kept.stats[b].shadowed;
        hs.tombstones += e->kept.stats[b].tombstones;
        hs.expired += e->kept.stats[b].expired;
        hs.filtered += e->kept.stats[b].filtered;
    }
    p.st.output_records = s.n_out;
    p.st.expired = hs.expired;
    p.st.filtered = hs.filtered;
    /* non-bottommost: no tombstone is dropped (each is in output_records);
     * expired/filtered count the conversions */
    p.st.tombstones = p.bottommost ? hs.tombstones : 0;
    p.st.shadowed = hs.shadowed;
    p.st.output_bytes = s.kbytes + s.vbytes;
    s.tombstone_out = !p.bottommost && hs.tombstones + hs.expired + hs.filtered > 0;
    return s;
}

/* the merged run's strides: keys, values and PUT values come out as
 * verbatim-length copies, so a stride every input shares survives */
static void output_strides(const RunBuf *wr, int R, bool tombstone_out, RunBuf *nr)
{
    nr->fixed_klen = shared_stride(wr, R, &RunBuf::fixed_klen);
    nr->fixed_vlen = shared_stride(wr, R, &RunBuf::fixed_vlen);
    nr->fixed_vlen_put = shared_stride(wr, R, &RunBuf::fixed_vlen_put);
    if (tombstone_out)
        nr->fixed_vlen = 0; /* kept, or converted with an empty value: no plain stride */
    else if (!nr->fixed_vlen)
        nr->fixed_vlen = nr->fixed_vlen_put; /* only PUTs came out */
}

/* the emit the plan was built for, between ev[3] and ev[4].  fk and
 * no_rewrite imply the chunked emit (plan_pass). */
static void emit_pass(HipEngine *e, const CompactPlan &p, const PassSizes &s, const RunBuf &nr)
{
    HIP_OK(hipEventRecord(e->kept.ev[3], e->stream));
    if (p.fk) {
        /* all-fixed-stride: scan, row columns and both copies in one
         * kernel over the tiles submit_sizes counted */
        e->kept.route.emit = RRDB_ROUTE_EMIT_CHUNKED_FIXED;
        launch_emit_fixed_fused(p.dr, p.R, p.d_order, p.total, p.d_keepw, p.d_tile_base,
                                p.d_changed, p.d_new_expire, e->data_version, p.fk, p.fv, s.n_out,
                                nr.keys, nr.vals, nr.koff, nr.voff, nr.sk, e->stream);
    } else if (p.emit_mode == 2) {
        e->kept.route.emit = RRDB_ROUTE_EMIT_CHUNKED;
        uint64_t *d_row_ksrc = e->talloc<uint64_t>(s.n_out * 8);
        uint64_t *d_row_vsrc = e->talloc<uint64_t>(s.n_out * 8);
        uint32_t *d_row_patch = e->talloc<uint32_t>(s.n_out * 4);
        uint32_t *d_row_expire = e->talloc<uint32_t>(s.n_out * 4);
        uint64_t kanch = (((s.kbytes + 15) >> 4) >> 6) + 1;
        uint64_t vanch = (((s.vbytes + 15) >> 4) >> 6) + 1;
        uint64_t *d_kanchor = e->talloc<uint64_t>(kanch * 8);
        uint64_t *d_vanchor = e->talloc<uint64_t>(vanch * 8);
        launch_emit_compact_chunked(p.dr, p.d_order, p.total, p.d_keepw, p.d_changed,
                                    p.d_new_expire, p.d_kpos, p.d_koffs, p.d_voffs,
                                    e->data_version, s.n_out, s.kbytes, s.vbytes, d_row_ksrc,
                                    d_row_vsrc, d_row_patch, d_row_expire, nr.keys, nr.vals,
                                    nr.koff, nr.voff, nr.sk, d_kanchor, d_vanchor, e->stream);
    } else if (p.emit_mode == 1) {
        e->kept.route.emit = RRDB_ROUTE_EMIT_INPUT;
        launch_emit_compact_inmajor(p.dr, p.R, p.d_wp, p.total, p.d_rank_of, p.d_keepw,
                                    p.d_changed, p.d_new_expire, p.d_kpos, p.d_koffs, p.d_voffs,
                                    e->data_version, nr.keys, nr.vals, nr.koff, nr.voff, nr.sk,
                                    s.n_out, e->stream);
    } else {
        e->kept.route.emit = RRDB_ROUTE_EMIT_RANK;
        launch_emit_compact(p.dr, p.d_order, p.total, p.d_keepw, p.d_changed, p.d_new_expire,
                            p.d_kpos, p.d_koffs, p.d_voffs, e->data_version, nr.keys, nr.vals,
                            nr.koff, nr.voff, nr.sk, s.n_out, e->stream);
    }
    HIP_OK(hipEventRecord(e->kept.ev[4], e->stream));
    e->kept.have_emit = true;
}

/* only the window's runs go; the merged run (when it has a record) takes
 * their place at index `first`, older and newer runs stay where they are */
static void replace_window(HipEngine *e, const CompactPlan &p, RunBuf &nr)
{
    e->before_run_free();
    for (int r = 0; r < p.R; r++)
        e->free_run(e->runs[p.first + r]);
    e->runs.erase(e->runs.begin() + p.first, e->runs.begin() + p.first + p.R);
    if (nr.n > 0) {
        e->finish_run(nr, nullptr, RunAlloc::Abort, e->bloom_enabled);
        e->runs.insert(e->runs.begin() + p.first, nr);
    }
    e->runs_changed();
}

/* phase 2: wait for the submitted work, allocate + emit the output run,
 * collect stats.  Caller holds the handle lock. */
static int32_t compact_finish(HipEngine *e, rrdb_compact_stats *stats)
{
    CompactPlan &p = e->pend;
    if (!p.active)
        return RRDB_INVALID_ARGUMENT;
    e->activate();
    p.active = false;
    e->arena_unpin();
    if (!p.trivial) {
        /* wait for the submitted merge phase only (rank + prefix sums + the
         * async size/stats reads — all of this stream's pending work) */
        HIP_OK(hipStreamSynchronize(e->stream));
        const PassSizes s = read_sizes_and_stats(e, p);
        RunBuf nr;
        if (s.n_out > 0) {
            output_strides(e->runs.data() + p.first, p.R, s.tombstone_out, &nr);
            /* keep_inputs drops the output at the end of the pass: arena memory */
            e->alloc_base(nr, s.n_out, s.kbytes, s.vbytes,
                          p.keep_inputs ? RunAlloc::Arena : RunAlloc::Abort);
            emit_pass(e, p, s, nr);
            /* the swap below frees the input runs the emit reads: drain.
             * keep_inputs (repeatable-pass, benchmarking) drops the output
             * instead and returns with the emit in flight — later partitions'
             * finishes overlap it; stream order protects the arena reuse */
            if (!p.keep_inputs)
                HIP_OK(hipStreamSynchronize(e->stream));
        }
        e->kept.ev_live = true; /* timing is resolved lazily by phase_ms() */
        if (!p.keep_inputs)
            replace_window(e, p, nr);
    }
    if (stats)
        *stats = p.st;
    return RRDB_OK;
}

/* a whole pass; a refused begin leaves zeroed stats */
static int32_t compact_pass(HipEngine *e, const rrdb_compact_options *opts, uint32_t epoch_now,
                            const CompactWindow *win, rrdb_compact_stats *stats)
{
    int32_t rc = compact_begin(e, opts, epoch_now, win);
    if (rc != RRDB_OK) {
        if (stats)
            *stats = rrdb_compact_stats{};
        return rc;
    }
    return compact_finish(e, stats);
}

int32_t rrdb_manual_compact(void *h, const rrdb_compact_options *opts, uint32_t epoch_now,
                            rrdb_compact_stats *stats)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    return compact_pass(e, opts, epoch_now, nullptr, stats);
}

int32_t rrdb_manual_compact_begin(void *h, const rrdb_compact_options *opts, uint32_t epoch_now)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    return compact_begin(e, opts, epoch_now);
}

int32_t rrdb_manual_compact_finish(void *h, rrdb_compact_stats *stats)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    return compact_finish(e, stats);
}

/* ---- engine-only extensions (include/rrdb_engine_ext.h) ---- */

int32_t rrdb_last_compact_route(void *h, rrdb_compact_route *out)
{
    auto *e = (HipEngine *)h;
    if (!out)
        return RRDB_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> g(e->mu);
    *out = e->kept.route;
    return RRDB_OK;
}

int32_t rrdb_compact_runs(void *h, uint64_t first_run, uint64_t n_runs, uint32_t epoch_now,
                          rrdb_compact_stats *stats)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    if (stats)
        *stats = rrdb_compact_stats{};
    if (e->pend.active || e->manual_compact_disabled)
        return RRDB_INVALID_ARGUMENT;
    if (engine_flush(e) != RRDB_OK) /* as the manual pass: the memtable becomes a run */
        return RRDB_IO_ERROR;
    uint64_t R = e->runs.size();
    if (n_runs == 0 || first_run >= R || n_runs > R - first_run)
        return RRDB_INVALID_ARGUMENT;
    const CompactWindow w{(size_t)first_run, (size_t)n_runs};
    return compact_pass(e, nullptr, epoch_now, &w, stats);
}

/* Size-tiered pick over the age-ordered run list: start from the two newest
 * runs and extend the window towards older runs while the next older run is
 * no more than twice the records gathered so far — a big old run is left
 * alone until the young ones have grown to its tier. */
int32_t rrdb_auto_compact(void *h, uint32_t epoch_now, uint64_t *first_run_out,
                          uint64_t *n_runs_out, rrdb_compact_stats *stats)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    if (stats)
        *stats = rrdb_compact_stats{};
    if (first_run_out)
        *first_run_out = 0;
    if (n_runs_out)
        *n_runs_out = 0;
    if (e->pend.active)
        return RRDB_INVALID_ARGUMENT;
    if (e->bulk_load)
        return RRDB_OK;
    if (e->runs.size() < e->l0_trigger)
        return RRDB_OK;
    /* the pass flushes first, as every pass does; pick over the result so
     * the window still ends at the newest run */
    if (engine_flush(e) != RRDB_OK)
        return RRDB_IO_ERROR;
    size_t R = e->runs.size();
    size_t s = R - 2;
    uint64_t acc = e->runs[R - 1].n + e->runs[R - 2].n;
    while (s > 0 && e->runs[s - 1].n <= 2 * acc) {
        s--;
        acc += e->runs[s].n;
    }
    const CompactWindow w{s, R - s};
    int32_t rc = compact_pass(e, nullptr, epoch_now, &w, stats);
    if (rc == RRDB_OK) {
        if (first_run_out)
            *first_run_out = s;
        if (n_runs_out)
            *n_runs_out = R - s;
    }
    return rc;
}

/* ---- partition split (rrdb_split) ----
 * Per source run: one classify pass writes side[] and per-wave side counts,
 * one scan over the counts gives wave bases; a side is then emitted by
 * split_emit_side.  Temporaries are arena memory sized for the largest run
 * and reused run after run (everything is ordered on the parent's stream). */
struct SplitRunInfo {
    uint8_t *side = nullptr;   /* [n] SPLIT_* code per record */
    uint64_t *wbase = nullptr; /* scanned [parent waves | child waves] counts */
    uint64_t nw = 0;
    uint64_t cnt[2] = {0, 0};  /* records owned by parent / child */
    bool has_put[2] = {false, false};
};
struct SplitTmp {
    uint64_t *ksz = nullptr, *kpos = nullptr, *vsz = nullptr, *vpos = nullptr;
    uint64_t *row_ksrc = nullptr, *row_vsrc = nullptr, *kanch = nullptr, *vanch = nullptr;
    uint64_t *psc_k = nullptr, *psc_v = nullptr;
    PhaseEvents<2> ev;
    double emit_ms = 0.0;
};

/* Build side s (0 parent, 1 child) of `src` as a finished run in *out and
 * its key+value bytes in *bytes.  si.cnt[s] > 0.  `bloom` is the
 * rocksdb.filter_type of the handle that will own the run.  false = an
 * allocation failed; nothing is left allocated and src is untouched. */
static bool split_emit_side(HipEngine *e, const RunBuf &src, const SplitRunInfo &si, int s,
                            SplitTmp &t, bool bloom, RunBuf *out, uint64_t *bytes)
{
    const uint64_t ns = si.cnt[s], n = src.n;
    const uint64_t fk = src.fixed_klen, fv = src.fixed_vlen;
    uint64_t kbytes = ns * fk, vbytes = ns * fv;
    if (!fk || !fv) {
        /* variable-length column: scan this side's sizes for its offsets */
        uint64_t tot[4] = {0, 0, 0, 0};
        launch_split_sizes(si.side, (uint32_t)s, src.koff, src.voff, n, fk ? nullptr : t.ksz,
                           fv ? nullptr : t.vsz, e->stream);
        if (!fk) {
            launch_psum(t.ksz, t.kpos, n, t.psc_k, e->stream);
            scan_tail_async(t.kpos, t.ksz, n, &tot[0], e->stream);
        }
        if (!fv) {
            launch_psum(t.vsz, t.vpos, n, t.psc_v, e->stream);
            scan_tail_async(t.vpos, t.vsz, n, &tot[2], e->stream);
        }
        HIP_OK(hipStreamSynchronize(e->stream));
        if (!fk)
            kbytes = tot[0] + tot[1];
        if (!fv)
            vbytes = tot[2] + tot[3];
    }
    RunBuf r;
    if (!e->alloc_base(r, ns, kbytes, vbytes, RunAlloc::Try))
        return false;
    t.ev.record(0, e->stream);
    launch_split_scatter(src.keys, src.koff, src.vals, src.voff, src.sk, n, fk, fv, si.side,
                         (uint32_t)s, si.wbase + (s ? si.nw : 0), s ? si.cnt[0] : 0, t.kpos,
                         t.vpos, ns, kbytes, vbytes, r.koff, r.voff, r.sk, t.row_ksrc,
                         t.row_vsrc, e->stream);
    launch_split_copy(t.row_ksrc, r.koff, ns, fk, kbytes, t.kanch, r.keys, e->stream);
    launch_split_copy(t.row_vsrc, r.voff, ns, fv, vbytes, t.vanch, r.vals, e->stream);
    t.ev.record(1, e->stream);
    HIP_OK(hipStreamSynchronize(e->stream));
    float ms = 0;
    if (t.ev.ms(0, 1, &ms))
        t.emit_ms += ms;
    /* a subset of a fixed-stride run is fixed-stride.  The put-stride is
     * "the length every PUT shares" and is 0 for a run without PUTs
     * (detect_fixed_vlen_put), so it is inherited only when the side has one */
    r.fixed_klen = src.fixed_klen;
    r.fixed_vlen = src.fixed_vlen;
    r.fixed_vlen_put = si.has_put[s] ? src.fixed_vlen_put : 0;
    if (!e->finish_run(r, nullptr, RunAlloc::Try, bloom)) {
        e->free_run(r);
        return false;
    }
    *out = r;
    *bytes = kbytes + vbytes;
    return true;
}

int32_t rrdb_split(void *parent, void *child, int32_t new_partition_count,
                   rrdb_split_stats *stats)
{
    if (stats)
        *stats = rrdb_split_stats{};
    if (!parent || !child || parent == child)
        return RRDB_INVALID_ARGUMENT;
    auto *p = (HipEngine *)parent, *c = (HipEngine *)child;
    /* std::scoped_lock takes both mutexes with the deadlock-avoiding
     * std::lock, so two threads splitting (a,b) and (b,a) cannot deadlock */
    std::scoped_lock g(p->mu, c->mu);
    const int64_t npc = new_partition_count;
    if (npc < 2 || npc > (1ll << 30) || (npc & (npc - 1)) != 0)
        return RRDB_INVALID_ARGUMENT;
    if (p->pidx < 0 || p->pidx >= npc / 2 || c->pidx != p->pidx + npc / 2)
        return RRDB_INVALID_ARGUMENT;
    if (p->app_id != c->app_id || p->device != c->device || p->data_version != c->data_version)
        return RRDB_INVALID_ARGUMENT;
    if (!c->runs.empty() || !c->memtable.empty() || !c->ctxs.empty())
        return RRDB_INVALID_ARGUMENT;
    if (p->pend.active || c->pend.active || p->pend_scan.active || c->pend_scan.active)
        return RRDB_INVALID_ARGUMENT;
    p->activate();
    if (engine_flush(p) != RRDB_OK) /* as the compaction entry points */
        return RRDB_IO_ERROR;
    p->scratch_reset();
    rrdb_split_stats st{};
    const size_t R = p->runs.size();
    st.runs_in = R;
    uint64_t maxn = 0, max_kb = 0, max_vb = 0;
    bool any_var = false;
    for (auto &r : p->runs) {
        st.input_records += r.n;
        maxn = std::max(maxn, r.n);
        any_var = any_var || !r.fixed_klen || !r.fixed_vlen;
    }
    /* byte size of every run (koff[n] + voff[n]): stats for runs left whole,
     * and the anchor scratch of the variable-length copies */
    std::vector<uint64_t> run_kb(R, 0), run_vb(R, 0);
    for (size_t i = 0; i < R; i++) {
        const RunBuf &r = p->runs[i];
        HIP_OK(hipMemcpy(&run_kb[i], r.koff + r.n, 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(&run_vb[i], r.voff + r.n, 8, hipMemcpyDeviceToHost));
        max_kb = std::max(max_kb, run_kb[i]);
        max_vb = std::max(max_vb, run_vb[i]);
    }
    PhaseEvents<4> ev;
    SplitTmp t;
    ev.record(0, p->stream);

    /* classify + rank every run; one sync for all the counts */
    std::vector<SplitRunInfo> info(R);
    const uint64_t mask = (uint64_t)npc - 1;
    uint64_t *h_cnt = (uint64_t *)p->pinned_buf((R ? R : 1) * 4 * 8);
    ev.record(1, p->stream);
    for (size_t i = 0; i < R; i++) {
        const RunBuf &r = p->runs[i];
        SplitRunInfo &si = info[i];
        if (r.n == 0)
            continue;
        si.nw = (r.n + 63) / 64;
        si.side = p->talloc<uint8_t>(r.n);
        uint64_t *d_wcnt = p->talloc<uint64_t>(2 * si.nw * 8);
        si.wbase = p->talloc<uint64_t>(2 * si.nw * 8);
        uint32_t *d_has_put = p->talloc<uint32_t>(8);
        HIP_OK(hipMemsetAsync(d_has_put, 0, 8, p->stream));
        launch_split_classify(r.keys, r.koff, r.fixed_klen, r.sk, r.n, mask, (uint64_t)p->pidx,
                              (uint64_t)c->pidx, si.side, d_wcnt, d_has_put, p->split_crc_lds,
                              p->stream);
        launch_psum(d_wcnt, si.wbase, 2 * si.nw, p->psum_scratch(2 * si.nw), p->stream);
        /* parent total = scan value where the child section starts */
        HIP_OK(hipMemcpyAsync(&h_cnt[4 * i + 0], si.wbase + si.nw, 8, hipMemcpyDeviceToHost,
                              p->stream));
        HIP_OK(hipMemcpyAsync(&h_cnt[4 * i + 1], si.wbase + 2 * si.nw - 1, 8,
                              hipMemcpyDeviceToHost, p->stream));
        HIP_OK(hipMemcpyAsync(&h_cnt[4 * i + 2], d_wcnt + 2 * si.nw - 1, 8,
                              hipMemcpyDeviceToHost, p->stream));
        HIP_OK(hipMemcpyAsync(&h_cnt[4 * i + 3], d_has_put, 8, hipMemcpyDeviceToHost,
                              p->stream));
    }
    ev.record(2, p->stream);
    HIP_OK(hipStreamSynchronize(p->stream));
    for (size_t i = 0; i < R; i++) {
        SplitRunInfo &si = info[i];
        if (p->runs[i].n == 0)
            continue;
        si.cnt[0] = h_cnt[4 * i + 0];
        si.cnt[1] = h_cnt[4 * i + 1] + h_cnt[4 * i + 2] - si.cnt[0];
        si.has_put[0] = (uint32_t)h_cnt[4 * i + 3] != 0;
        si.has_put[1] = (uint32_t)(h_cnt[4 * i + 3] >> 32) != 0;
        st.child_records += si.cnt[1];
        st.dropped_records += p->runs[i].n - si.cnt[0] - si.cnt[1];
    }
    t.row_ksrc = p->talloc<uint64_t>(maxn * 8);
    t.row_vsrc = p->talloc<uint64_t>(maxn * 8);
    if (any_var) {
        t.ksz = p->talloc<uint64_t>(maxn * 8);
        t.kpos = p->talloc<uint64_t>(maxn * 8);
        t.vsz = p->talloc<uint64_t>(maxn * 8);
        t.vpos = p->talloc<uint64_t>(maxn * 8);
        t.psc_k = p->psum_scratch(maxn);
        t.psc_v = p->psum_scratch(maxn);
        t.kanch = p->talloc<uint64_t>((((max_kb + 15) >> 10) + 2) * 8);
        t.vanch = p->talloc<uint64_t>((((max_vb + 15) >> 10) + 2) * 8);
    }

    /* phase A: every child run, the parent untouched */
    std::vector<RunBuf> child_runs;
    for (size_t i = 0; i < R; i++) {
        if (info[i].cnt[1] == 0)
            continue; /* the engine never holds an empty run */
        RunBuf nr;
        uint64_t b = 0;
        if (!split_emit_side(p, p->runs[i], info[i], 1, t, c->bloom_enabled, &nr, &b)) {
            for (auto &r : child_runs)
                p->free_run(r);
            return RRDB_IO_ERROR; /* both handles as before */
        }
        child_runs.push_back(nr);
        st.child_bytes += b;
    }

    /* phase B: prune the parent run by run.  From here the parent's run list
     * changes: retire its resident kernel and parked views first. */
    p->before_run_free();
    std::vector<RunBuf> parent_runs;
    bool full = false;
    for (size_t i = 0; i < R; i++) {
        RunBuf &src = p->runs[i];
        const uint64_t np = info[i].cnt[0];
        if (np == 0) {
            p->free_run(src);
            continue;
        }
        RunBuf nr;
        uint64_t b = 0;
        if (np != src.n && !full)
            full = !split_emit_side(p, src, info[i], 0, t, p->bloom_enabled, &nr, &b);
        if (np == src.n || full) {
            /* nothing foreign in it, or the device is full: the run stays
             * whole (its foreign records are what the compaction filter's
             * stale-split-hash rule drops later) */
            if (np != src.n)
                st.parent_unpruned_runs++;
            st.parent_records += src.n;
            st.parent_bytes += run_kb[i] + run_vb[i];
            parent_runs.push_back(src);
            continue;
        }
        p->free_run(src);
        parent_runs.push_back(nr);
        st.parent_records += np;
        st.parent_bytes += b;
    }
    ev.record(3, p->stream);
    HIP_OK(hipStreamSynchronize(p->stream));
    float ms = 0;
    if (ev.ms(1, 2, &ms))
        p->phase_ms["split_classify"] = ms;
    p->phase_ms["split_emit"] = t.emit_ms;
    if (ev.ms(0, 3, &ms))
        p->phase_ms["split_total"] = ms;

    p->runs = parent_runs;
    c->runs = child_runs;
    st.parent_runs = p->runs.size();
    st.child_runs = c->runs.size();
    p->partition_version = c->partition_version = (int32_t)(npc - 1);
    /* later writes to the child outrank everything it inherited */
    c->next_seq_floor = p->next_seq_floor;
    p->runs_changed();
    c->runs_changed();
    if (stats)
        *stats = st;
    return RRDB_OK;
}

} /* extern "C" */

/* ================= write path (§8(f)1) =================
 * Host memtable + flush -> sorted run; mirrors pegasus_write_service
 * put/remove + rocksdb_wrapper::write_batch_put/_delete (reference
 * pegasus_write_service.h:119-207, rocksdb_wrapper.cpp:121-247).  Reads
 * flush lazily so committed writes are immediately visible (rocksdb
 * memtable read-path equivalent). */
extern "C" {

int32_t rrdb_put(void *h, const uint8_t *hash_key, uint64_t hklen, const uint8_t *sort_key,
                 uint64_t sklen, const uint8_t *value, uint64_t vlen, uint32_t expire_ts,
                 uint32_t epoch_now)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    if (!hklen_ok(hklen))
        return RRDB_INVALID_ARGUMENT;
    /* write-time default_ttl (rocksdb_wrapper::db_expire_ts, :280-286) */
    if (expire_ts == 0 && e->default_ttl != 0)
        expire_ts = epoch_now + e->default_ttl;
    std::string key = make_key(hash_key, hklen, sort_key, sklen);
    uint32_t hdr = hdr_len(e->data_version);
    std::string val(hdr + vlen, '\0');
    uint32_t off = (e->data_version == 2) ? 1 : 0;
    if (e->data_version == 2)
        val[0] = (char)0x82;
    val[off] = (char)(expire_ts >> 24);
    val[off + 1] = (char)(expire_ts >> 16);
    val[off + 2] = (char)(expire_ts >> 8);
    val[off + 3] = (char)expire_ts;
    if (vlen)
        memcpy(&val[hdr], value, vlen);
    e->memtable[key] = {std::move(val), e->next_seq_floor++, RRDB_KIND_PUT};
    return RRDB_OK;
}

int32_t rrdb_remove(void *h, const uint8_t *hash_key, uint64_t hklen, const uint8_t *sort_key,
                    uint64_t sklen)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    if (!hklen_ok(hklen))
        return RRDB_INVALID_ARGUMENT;
    std::string key = make_key(hash_key, hklen, sort_key, sklen);
    e->memtable[key] = {std::string(), e->next_seq_floor++, RRDB_KIND_DELETE};
    return RRDB_OK;
}

uint64_t rrdb_memtable_entries(void *h) { return ((HipEngine *)h)->memtable.size(); }

static int32_t engine_flush(HipEngine *e)
{
    if (e->memtable.empty())
        return RRDB_OK;
    e->activate();
    std::string keys, vals;
    std::vector<uint64_t> koff{0}, voff{0}, sk;
    for (auto &kv : e->memtable) {
        keys += kv.first;
        koff.push_back(keys.size());
        vals += std::get<0>(kv.second);
        voff.push_back(vals.size());
        sk.push_back((std::get<1>(kv.second) << 1) | (uint64_t)std::get<2>(kv.second));
    }
    int32_t rc = ingest_prepared(e, (const uint8_t *)keys.data(), koff.data(),
                                 (const uint8_t *)vals.data(), voff.data(), sk.data(), sk.size());
    if (rc != RRDB_OK)
        return rc; /* memtable retained: the write is not lost */
    e->memtable.clear();
    return RRDB_OK;
}

int32_t rrdb_flush(void *h)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    return engine_flush(e);
}

} /* extern "C" */

/* ---- batched writes (rrdb_write_batch, include/rrdb_engine_ext.h) ----
 * The host validates, stages the values (wb_stage.h) and uploads once; the
 * device sorts, dedups and emits the run (kernels.hip, "write batch").  Every
 * buffer proportional to the batch is a plain try allocation owned by WbBufs:
 * the scratch arena aborts when it has to grow, and a full device must come
 * back as kIOError. */
namespace {

/* the one host-to-device copy of the batch paths: a failed copy clears `ok`
 * (the call returns kIOError), and nothing is tried once it is clear */
bool try_upload(bool &ok, void *dst, const void *src, uint64_t bytes)
{
    if (ok && bytes && hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        ok = false;
    }
    return ok;
}

struct WbBufs {
    std::vector<void *> dev;
    std::vector<void *> host;
    bool ok = true;
    template <typename T> T *get(uint64_t bytes)
    {
        void *q = nullptr;
        if (!ok)
            return nullptr;
        if (hipMalloc(&q, bytes ? bytes : 1) != hipSuccess) {
            (void)hipGetLastError();
            ok = false;
            return nullptr;
        }
        dev.push_back(q);
        return (T *)q;
    }
    template <typename T> T *get_host(uint64_t bytes)
    {
        void *q = ok ? malloc(bytes ? bytes : 1) : nullptr;
        if (!q) {
            ok = false;
            return nullptr;
        }
        host.push_back(q);
        return (T *)q;
    }
    bool upload(void *dst, const void *src, uint64_t n) { return try_upload(ok, dst, src, n); }
    ~WbBufs()
    {
        for (void *q : dev)
            (void)hipFree(q);
        for (void *q : host)
            free(q);
    }
};

/* WbBufs' sibling for the incr, timetag and cas batches: their buffer sizes
 * are all known, or bounded, once n and the key bytes are, so they are pieces
 * of one try allocation (one hipMalloc and one hipFree per call instead of
 * thirty) */
struct BatchSlab {
    uint8_t *base = nullptr;
    uint64_t size = 0, used = 0;
    bool ok = true;
    /* before commit(): count the piece; after: hand it out.  Pieces are
     * 256-byte aligned. */
    template <typename T> void take(T **p, uint64_t bytes)
    {
        const uint64_t at = used;
        used += (bytes + 255) & ~255ull;
        if (base)
            *p = used <= size ? (T *)(base + at) : nullptr;
    }
    bool commit()
    {
        size = used;
        used = 0;
        if (hipMalloc((void **)&base, size ? size : 1) != hipSuccess) {
            (void)hipGetLastError();
            base = nullptr;
            ok = false;
        }
        return ok;
    }
    bool upload(void *dst, const void *src, uint64_t n) { return try_upload(ok, dst, src, n); }
    /* an optional per-op column: the caller's array, or zeros when it is null */
    void upload_or_zero(void *dst, const void *src_or_null, uint64_t bytes)
    {
        if (src_or_null) {
            upload(dst, src_or_null, bytes);
        } else if (ok && hipMemset(dst, 0, bytes) != hipSuccess) {
            (void)hipGetLastError();
            ok = false;
        }
    }
    ~BatchSlab()
    {
        if (base)
            (void)hipFree(base);
    }
};

/* ---- the shared batch-call skeleton: the steps the four batched-write entry
 * points below have in common, each a call.  What a path does differently
 * stays written out in its function. ---- */

/* a batch is refused between the begin and the finish of a split compaction
 * or of a count scan */
bool batch_blocked(const HipEngine *e) { return e->pend.active || e->pend_scan.active; }

/* after the path's validation.  Pending memtable entries are older than the
 * batch: their own run first. */
int32_t batch_begin(HipEngine *e)
{
    e->activate();
    return engine_flush(e);
}

/* the host-clock keys (<p>_stage, <p>_upload) */
using HostClock = std::chrono::steady_clock;
double ms_since(HostClock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(HostClock::now() - t0).count();
}

/* <p>_sort, <p>_lookup, <p>_apply, <p>_emit, <p>_total from events 0..5:
 * 0-1 sort, 1-2 lookup, 2-3 apply, 4-5 emit (0 when nothing was emitted);
 * the total leaves out the host's wait for the totals between 3 and 4 */
void batch_phase_timers(HipEngine *e, const char *prefix, const PhaseEvents<6> &ev, bool emitted)
{
    const std::string p(prefix);
    float ms = 0;
    if (ev.ms(0, 1, &ms))
        e->phase_ms[p + "_sort"] = ms;
    if (ev.ms(1, 2, &ms))
        e->phase_ms[p + "_lookup"] = ms;
    if (ev.ms(2, 3, &ms))
        e->phase_ms[p + "_apply"] = ms;
    double &emit = e->phase_ms[p + "_emit"];
    emit = 0.0;
    if (emitted && ev.ms(4, 5, &ms))
        emit = ms;
    if (ev.ms(0, 3, &ms))
        e->phase_ms[p + "_total"] = ms + emit;
}

/* the sorted batch: the words and the op index of every sorted position */
struct SortedOps {
    const uint64_t *d_w;
    const uint32_t *d_ix;
};
SortedOps batch_sort(const WbKeys &wk, uint64_t n, uint32_t *d_lcp, uint64_t *d_w0,
                     uint32_t *d_i0, uint64_t *d_w1, uint32_t *d_i1, hipStream_t s)
{
    const int cur = launch_wb_sort(wk, n, d_lcp, d_w0, d_i0, d_w1, d_i1, s);
    return {cur ? d_w1 : d_w0, cur ? d_i1 : d_i0};
}

/* one segment per distinct key: head flags, their scan, the segment starts
 * and the segment count (word 0 of d_red, which this initialises) */
void batch_segments(const WbKeys &wk, uint64_t n, const SortedOps &so, uint64_t *d_head,
                    uint64_t *d_hrank, uint64_t *d_seg_start, uint64_t *d_psc, uint64_t *d_red,
                    int red_words, uint32_t red_min_mask, hipStream_t s)
{
    launch_key_heads(wk, n, so.d_w, so.d_ix, d_head, d_red, red_words, red_min_mask, s);
    launch_psum(d_head, d_hrank, n, d_psc, s);
    launch_incr_segs(n, d_head, d_hrank, d_seg_start, d_red, s);
}

/* the bases of a batch: every op's (or check's) key against the runs as they
 * are now.  The columns exist only when there is something to look up;
 * status == nullptr is what tells the kernels that there was no lookup. */
struct BaseLookup {
    int32_t *status = nullptr;
    uint64_t *hit = nullptr, *ulen = nullptr;
    uint32_t *expire = nullptr;
    DevRun *runs = nullptr;
    void take(BatchSlab &b, bool lookup, uint64_t n)
    {
        if (!lookup)
            return;
        b.take(&status, n * 4);
        b.take(&hit, n * 8);
        b.take(&ulen, n * 8);
        b.take(&expire, n * 4);
    }
    void get(HipEngine *e, const uint8_t *d_keys, const uint64_t *d_koff, uint64_t n,
             uint32_t epoch_now)
    {
        if (!status)
            return;
        runs = e->dev_runs();
        launch_get(runs, (int)e->runs.size(), d_keys, d_koff, n, epoch_now, e->data_version,
                   status, hit, ulen, expire, e->stream);
    }
};

/* the stride detect_fixed_* would report for a column whose lengths span
 * [min, max]: the common length, 0 when they differ or it does not fit */
uint32_t fixed_stride_of(uint64_t min, uint64_t max)
{
    return min == max && min <= UINT32_MAX ? (uint32_t)min : 0;
}

/* the output row of every segment and, for a column that is not fixed-stride,
 * its byte offset; a fixed-stride column's *d_pos becomes null, which the
 * emit kernels read as "row x stride" */
void batch_emit_offsets(uint64_t n_seg, const uint64_t *d_seg_has, uint64_t *d_orank,
                        const uint64_t *d_seg_ksz, uint64_t **d_kpos, uint32_t out_fk,
                        const uint64_t *d_seg_vsz, uint64_t **d_vpos, uint32_t out_fv,
                        uint64_t *d_psc, hipStream_t s)
{
    if (out_fk)
        *d_kpos = nullptr;
    if (out_fv)
        *d_vpos = nullptr;
    launch_psum(d_seg_has, d_orank, n_seg, d_psc, s);
    if (*d_kpos)
        launch_psum(d_seg_ksz, *d_kpos, n_seg, d_psc, s);
    if (*d_vpos)
        launch_psum(d_seg_vsz, *d_vpos, n_seg, d_psc, s);
}

/* finish the emitted run and make it the handle's newest; the batch spent
 * seq_advance seqnos.  false: a try allocation failed, the run is freed.
 * Either way the stream is drained (finish_run). */
bool batch_commit_run(HipEngine *e, RunBuf &r, uint64_t seq_advance)
{
    if (!e->finish_run(r, nullptr, RunAlloc::Try, e->bloom_enabled)) {
        e->free_run(r);
        return false;
    }
    e->runs.push_back(r);
    e->runs_changed();
    e->next_seq_floor += seq_advance;
    return true;
}

} // namespace

extern "C" {

int32_t rrdb_write_batch(void *h, uint64_t n_ops, const uint8_t *keys, const uint64_t *key_offs,
                         const uint8_t *values, const uint64_t *val_offs,
                         const uint32_t *expire_ts, const uint8_t *kinds, uint32_t epoch_now,
                         rrdb_write_batch_stats *stats)
{
    if (stats)
        *stats = rrdb_write_batch_stats{};
    if (!h)
        return RRDB_INVALID_ARGUMENT;
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    if (n_ops == 0)
        return RRDB_OK;
    const auto t_host = HostClock::now();
    if (batch_blocked(e))
        return RRDB_INVALID_ARGUMENT;
    if (!wb_validate(n_ops, keys, key_offs, values, val_offs, kinds))
        return RRDB_INVALID_ARGUMENT;
    const uint64_t n = n_ops;
    uint64_t sv_bytes = 0;
    if (!wb_staged_bytes(n, val_offs, kinds, e->data_version, &sv_bytes))
        return RRDB_INVALID_ARGUMENT;

    if (const int32_t rc = batch_begin(e); rc != RRDB_OK)
        return rc;

    /* staging: keys verbatim, values with the header in front of every PUT */
    WbBufs b;
    uint8_t *h_svals = b.get_host<uint8_t>(sv_bytes);
    uint64_t *h_svoff = b.get_host<uint64_t>((n + 1) * 8);
    if (!b.ok)
        return RRDB_IO_ERROR;
    wb_stage_values(n, values, val_offs, expire_ts, kinds, e->data_version, e->default_ttl,
                    epoch_now, h_svals, h_svoff);
    const uint64_t in_fk = wb_fixed_stride(key_offs, n), in_fv = wb_fixed_stride(h_svoff, n);
    const uint64_t in_kbytes = key_offs[n];
    e->phase_ms["wb_stage"] = ms_since(t_host);

    const auto t_up = HostClock::now();
    uint8_t *d_keys = b.get<uint8_t>(in_kbytes);
    uint64_t *d_koff = in_fk ? nullptr : b.get<uint64_t>((n + 1) * 8);
    uint8_t *d_svals = b.get<uint8_t>(sv_bytes);
    uint64_t *d_svoff = in_fv ? nullptr : b.get<uint64_t>((n + 1) * 8);
    uint8_t *d_kinds = b.get<uint8_t>(n);
    uint32_t *d_lcp = b.get<uint32_t>(256);
    uint64_t *d_w0 = b.get<uint64_t>(n * 8), *d_w1 = b.get<uint64_t>(n * 8);
    uint32_t *d_i0 = b.get<uint32_t>(n * 4), *d_i1 = b.get<uint32_t>(n * 4);
    uint64_t *d_keep = b.get<uint64_t>(n * 8), *d_rank = b.get<uint64_t>(n * 8);
    uint64_t *d_psc = b.get<uint64_t>(psum_scratch_elems(n) * 8);
    uint64_t *d_ksz = in_fk ? nullptr : b.get<uint64_t>(n * 8);
    uint64_t *d_kpos = in_fk ? nullptr : b.get<uint64_t>(n * 8);
    uint64_t *d_vsz = in_fv ? nullptr : b.get<uint64_t>(n * 8);
    uint64_t *d_vpos = in_fv ? nullptr : b.get<uint64_t>(n * 8);
    uint64_t *d_red = b.get<uint64_t>(WBR_WORDS * 8);
    b.upload(d_keys, keys, in_kbytes);
    if (d_koff)
        b.upload(d_koff, key_offs, (n + 1) * 8);
    b.upload(d_svals, h_svals, sv_bytes);
    if (d_svoff)
        b.upload(d_svoff, h_svoff, (n + 1) * 8);
    b.upload(d_kinds, kinds, n);
    if (!b.ok)
        return RRDB_IO_ERROR;
    e->phase_ms["wb_upload"] = ms_since(t_up);

    PhaseEvents<4> ev;
    const WbKeys wk{d_keys, d_koff, in_fk, d_lcp};
    ev.record(0, e->stream);
    const SortedOps so = batch_sort(wk, n, d_lcp, d_w0, d_i0, d_w1, d_i1, e->stream);
    ev.record(1, e->stream);

    /* keep flags, rank, byte offsets; then the one read-back */
    launch_wb_flags(wk, d_svoff, in_fv, d_kinds, n, so.d_w, so.d_ix, d_keep, d_ksz, d_vsz, d_red,
                    e->stream);
    launch_psum(d_keep, d_rank, n, d_psc, e->stream);
    uint64_t tot[6] = {0, 0, 0, 0, 0, 0}, red[WBR_WORDS];
    scan_tail_async(d_rank, d_keep, n, &tot[0], e->stream);
    if (!in_fk) {
        launch_psum(d_ksz, d_kpos, n, d_psc, e->stream);
        scan_tail_async(d_kpos, d_ksz, n, &tot[2], e->stream);
    }
    if (!in_fv) {
        launch_psum(d_vsz, d_vpos, n, d_psc, e->stream);
        scan_tail_async(d_vpos, d_vsz, n, &tot[4], e->stream);
    }
    HIP_OK(hipMemcpyAsync(red, d_red, sizeof(red), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    const uint64_t n_out = tot[0] + tot[1];
    const uint64_t kbytes = in_fk ? n_out * in_fk : tot[2] + tot[3];
    const uint64_t vbytes = in_fv ? n_out * in_fv : tot[4] + tot[5];

    RunBuf r;
    uint64_t *d_row_ksrc = b.get<uint64_t>(n_out * 8), *d_row_vsrc = b.get<uint64_t>(n_out * 8);
    uint64_t *d_kanch = b.get<uint64_t>((((kbytes + 15) >> 10) + 2) * 8);
    uint64_t *d_vanch = b.get<uint64_t>((((vbytes + 15) >> 10) + 2) * 8);
    if (!b.ok || !e->alloc_base(r, n_out, kbytes, vbytes, RunAlloc::Try))
        return RRDB_IO_ERROR;
    /* the strides detect_fixed_* would report for the emitted run */
    r.fixed_klen = fixed_stride_of(red[WBR_KMIN], red[WBR_KMAX]);
    r.fixed_vlen = fixed_stride_of(red[WBR_VMIN], red[WBR_VMAX]);
    r.fixed_vlen_put = red[WBR_PUTS] ? fixed_stride_of(red[WBR_PVMIN], red[WBR_PVMAX]) : 0;
    ev.record(2, e->stream);
    launch_wb_scatter(wk, d_svals, d_svoff, in_fv, d_kinds, n, so.d_ix, d_keep, d_rank, d_kpos,
                      d_vpos, e->next_seq_floor, n_out, kbytes, vbytes, r.koff, r.voff, r.sk,
                      d_row_ksrc, d_row_vsrc, e->stream);
    launch_split_copy(d_row_ksrc, r.koff, n_out, r.fixed_klen, kbytes, d_kanch, r.keys,
                      e->stream);
    launch_split_copy(d_row_vsrc, r.voff, n_out, r.fixed_vlen, vbytes, d_vanch, r.vals,
                      e->stream);
    ev.record(3, e->stream);
    if (!batch_commit_run(e, r, n))
        return RRDB_IO_ERROR;
    float ms = 0, ms2 = 0;
    if (ev.ms(0, 1, &ms))
        e->phase_ms["wb_sort"] = ms;
    if (ev.ms(1, 2, &ms) && ev.ms(2, 3, &ms2))
        e->phase_ms["wb_emit"] = ms + ms2;
    if (ev.ms(0, 3, &ms))
        e->phase_ms["wb_total"] = ms;
    if (stats) {
        stats->input_ops = n;
        stats->output_records = n_out;
        stats->superseded = n - n_out;
        stats->puts = red[WBR_PUTS];
        stats->removes = n_out - red[WBR_PUTS];
        stats->key_bytes = kbytes;
        stats->value_bytes = vbytes;
    }
    return RRDB_OK;
}

/* ---- batched counter increments (rrdb_incr_batch, rrdb_engine_ext.h) ----
 * The host validates and uploads keys, increments and directives once; the
 * device sorts, looks the bases up, applies the chains and emits the run
 * (kernels.hip, "incr batch").  Two read-backs: the totals before the run is
 * allocated, the per-op results at the end. */
static_assert(INCR_ERR_INVALID == RRDB_INVALID_ARGUMENT, "the chain kernels write this code");
int32_t rrdb_incr_batch(void *h, uint64_t n_ops, const uint8_t *keys, const uint64_t *key_offs,
                        const int64_t *increments, const int32_t *expire_ts_seconds,
                        uint32_t epoch_now, int64_t *new_values, int32_t *errors,
                        rrdb_incr_batch_stats *stats)
{
    if (stats)
        *stats = rrdb_incr_batch_stats{};
    if (!h)
        return RRDB_INVALID_ARGUMENT;
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    if (n_ops == 0)
        return RRDB_OK;
    if (batch_blocked(e))
        return RRDB_INVALID_ARGUMENT;
    if (!increments || !wb_keys_ok(n_ops, keys, key_offs))
        return RRDB_INVALID_ARGUMENT;
    const uint64_t n = n_ops;

    if (const int32_t rc = batch_begin(e); rc != RRDB_OK)
        return rc;

    /* every buffer proportional to the batch is carved from one try
     * allocation: the sizes are all known from n and the key bytes, the later
     * ones (per segment, per output row) by their upper bound n */
    const uint64_t in_fk = wb_fixed_stride(key_offs, n), in_kbytes = key_offs[n];
    BatchSlab b;
    BaseLookup base;
    uint8_t *d_keys = nullptr;
    uint64_t *d_koff = nullptr, *d_w0 = nullptr, *d_w1 = nullptr, *d_head = nullptr,
             *d_hrank = nullptr, *d_seg_start = nullptr, *d_psc = nullptr, *d_ok = nullptr,
             *d_okrank = nullptr, *d_seg_has = nullptr, *d_orank = nullptr, *d_seg_ksz = nullptr,
             *d_seg_vsz = nullptr, *d_red = nullptr, *d_kpos = nullptr, *d_vpos = nullptr,
             *d_row_ksrc = nullptr, *d_kanch = nullptr;
    int64_t *d_inc = nullptr, *d_newv = nullptr, *d_seg_val = nullptr;
    int32_t *d_dir = nullptr, *d_err = nullptr;
    uint32_t *d_lcp = nullptr, *d_i0 = nullptr, *d_i1 = nullptr, *d_seg_exp = nullptr,
             *d_seg_last = nullptr;
    for (int pass = 0; pass < 2; pass++) { /* 0 sizes the slab, 1 hands the pieces out */
        b.take(&d_keys, in_kbytes);
        b.take(&d_koff, (n + 1) * 8); /* the lookup takes offsets */
        b.take(&d_inc, n * 8);
        b.take(&d_dir, n * 4);
        b.take(&d_lcp, 256);
        b.take(&d_w0, n * 8);
        b.take(&d_w1, n * 8);
        b.take(&d_i0, n * 4);
        b.take(&d_i1, n * 4);
        b.take(&d_head, n * 8);
        b.take(&d_hrank, n * 8);
        b.take(&d_seg_start, (n + 1) * 8);
        b.take(&d_psc, psum_scratch_elems(n) * 8);
        base.take(b, !e->runs.empty(), n);
        b.take(&d_newv, n * 8);
        b.take(&d_err, n * 4);
        b.take(&d_ok, n * 8);
        b.take(&d_okrank, n * 8);
        b.take(&d_seg_val, n * 8);
        b.take(&d_seg_exp, n * 4);
        b.take(&d_seg_last, n * 4);
        b.take(&d_seg_has, n * 8);
        b.take(&d_orank, n * 8);
        b.take(&d_seg_ksz, n * 8);
        b.take(&d_seg_vsz, n * 8);
        b.take(&d_red, IR_WORDS * 8);
        b.take(&d_kpos, n * 8);
        b.take(&d_vpos, n * 8);
        b.take(&d_row_ksrc, n * 8);
        b.take(&d_kanch, (((in_kbytes + 15) >> 10) + 2) * 8);
        if (pass == 0 && !b.commit())
            return RRDB_IO_ERROR;
    }
    b.upload(d_keys, keys, in_kbytes);
    b.upload(d_koff, key_offs, (n + 1) * 8);
    b.upload(d_inc, increments, n * 8);
    b.upload_or_zero(d_dir, expire_ts_seconds, n * 4);
    if (!b.ok)
        return RRDB_IO_ERROR;

    PhaseEvents<6> ev;
    /* sort, then the segments: one per distinct key */
    const WbKeys wk{d_keys, in_fk ? nullptr : d_koff, in_fk, d_lcp};
    ev.record(0, e->stream);
    const SortedOps so = batch_sort(wk, n, d_lcp, d_w0, d_i0, d_w1, d_i1, e->stream);
    batch_segments(wk, n, so, d_head, d_hrank, d_seg_start, d_psc, d_red, IR_WORDS, IR_MIN_MASK,
                   e->stream);
    ev.record(1, e->stream);
    base.get(e, d_keys, d_koff, n, epoch_now);
    ev.record(2, e->stream);

    IncrArgs a{};
    a.k = wk;
    a.n = n;
    a.ix = so.d_ix;
    a.seg_start = d_seg_start;
    a.inc = d_inc;
    a.dir = d_dir;
    a.status = base.status;
    a.hit = base.hit;
    a.expire = base.expire;
    a.runs = base.runs;
    a.data_version = e->data_version;
    a.epoch_now = epoch_now;
    a.default_ttl = e->default_ttl;
    a.lane_max = e->incr_lane_max;
    a.new_val = d_newv;
    a.err = d_err;
    a.ok = d_ok;
    a.seg_val = d_seg_val;
    a.seg_exp = d_seg_exp;
    a.seg_last = d_seg_last;
    a.seg_has = d_seg_has;
    a.seg_ksz = d_seg_ksz;
    a.seg_vsz = d_seg_vsz;
    a.red = (unsigned long long *)d_red;
    launch_incr_chain(a, e->stream);
    launch_psum(d_ok, d_okrank, n, d_psc, e->stream);
    ev.record(3, e->stream);

    /* the totals: one read */
    uint64_t red[IR_WORDS];
    HIP_OK(hipMemcpyAsync(red, d_red, sizeof(red), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    const uint64_t n_seg = red[IR_NSEG], n_out = red[IR_NOUT];
    const uint64_t kbytes = red[IR_KBYTES], vbytes = red[IR_VBYTES];
    const uint32_t out_fk = n_out ? fixed_stride_of(red[IR_KMIN], red[IR_KMAX]) : 0;
    const uint32_t out_fv = n_out ? fixed_stride_of(red[IR_VMIN], red[IR_VMAX]) : 0;

    auto results_out = [&]() {
        if (new_values)
            HIP_OK(hipMemcpy(new_values, d_newv, n * 8, hipMemcpyDeviceToHost));
        if (errors)
            HIP_OK(hipMemcpy(errors, d_err, n * 4, hipMemcpyDeviceToHost));
        if (stats) {
            stats->input_ops = n;
            stats->applied = red[IR_APPLIED];
            stats->failed_parse = red[IR_FPARSE];
            stats->failed_range = red[IR_FRANGE];
            stats->output_records = n_out;
            stats->key_bytes = kbytes;
            stats->value_bytes = vbytes;
        }
    };
    if (n_out == 0) { /* no op wrote: no run, the floor stays */
        batch_phase_timers(e, "incr", ev, false);
        results_out();
        return RRDB_OK;
    }

    RunBuf r;
    if (n_seg > n || n_out > n_seg || kbytes > in_kbytes ||
        !e->alloc_base(r, n_out, kbytes, vbytes, RunAlloc::Try))
        return RRDB_IO_ERROR;
    /* the strides detect_fixed_* would report for the emitted run: all PUTs */
    r.fixed_klen = out_fk;
    r.fixed_vlen = out_fv;
    r.fixed_vlen_put = out_fv;
    ev.record(4, e->stream);
    batch_emit_offsets(n_seg, d_seg_has, d_orank, d_seg_ksz, &d_kpos, out_fk, d_seg_vsz, &d_vpos,
                       out_fv, d_psc, e->stream);
    launch_incr_emit(a, n_seg, d_okrank, d_orank, d_kpos, d_vpos, e->next_seq_floor, n_out, kbytes,
                     vbytes, out_fk, out_fv, r.koff, r.voff, r.sk, d_row_ksrc, r.vals, e->stream);
    launch_split_copy(d_row_ksrc, r.koff, n_out, r.fixed_klen, kbytes, d_kanch, r.keys,
                      e->stream);
    ev.record(5, e->stream);
    if (!batch_commit_run(e, r, red[IR_APPLIED]))
        return RRDB_IO_ERROR;
    batch_phase_timers(e, "incr", ev, true);
    results_out();
    return RRDB_OK;
}

/* ---- batched writes with timetags (rrdb_write_batch_timetag,
 * rrdb_engine_ext.h) ----
 * The host validates (wb_validate), stages the values with the timetag in
 * the header and folds every op to its TT_OP_* bits (wb_stage_values_tt) and
 * uploads once; the device sorts, looks the bases up, walks every key's chain
 * with the rule of tt_verify.h and emits the run (kernels.hip, "timetag
 * batch").  Two read-backs: the totals before the run is allocated, and
 * `applied` at the end when the caller asked for it. */
int32_t rrdb_write_batch_timetag(void *h, uint64_t n_ops, const uint8_t *keys,
                                 const uint64_t *key_offs, const uint8_t *values,
                                 const uint64_t *val_offs, const uint32_t *expire_ts,
                                 const uint8_t *kinds, const uint64_t *timetags,
                                 const uint8_t *verify, uint32_t epoch_now, uint8_t *applied,
                                 rrdb_timetag_batch_stats *stats)
{
    if (stats)
        *stats = rrdb_timetag_batch_stats{};
    if (!h)
        return RRDB_INVALID_ARGUMENT;
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    if (n_ops == 0)
        return RRDB_OK;
    const auto t_host = HostClock::now();
    if (batch_blocked(e))
        return RRDB_INVALID_ARGUMENT;
    if (!wb_validate(n_ops, keys, key_offs, values, val_offs, kinds))
        return RRDB_INVALID_ARGUMENT;
    const uint64_t n = n_ops;
    uint64_t sv_bytes = 0;
    if (!wb_staged_bytes(n, val_offs, kinds, e->data_version, &sv_bytes))
        return RRDB_INVALID_ARGUMENT;

    if (const int32_t rc = batch_begin(e); rc != RRDB_OK)
        return rc;

    /* staging: keys verbatim, values with header and timetag in front of
     * every PUT, and the op flags the walk reads */
    WbBufs hb;
    uint8_t *h_svals = hb.get_host<uint8_t>(sv_bytes);
    uint64_t *h_svoff = hb.get_host<uint64_t>((n + 1) * 8);
    uint8_t *h_flags = hb.get_host<uint8_t>(n);
    if (!hb.ok)
        return RRDB_IO_ERROR;
    wb_stage_values_tt(n, values, val_offs, expire_ts, kinds, timetags, verify, e->data_version,
                       e->default_ttl, epoch_now, h_svals, h_svoff, h_flags);
    const uint64_t in_fk = wb_fixed_stride(key_offs, n), in_kbytes = key_offs[n];
    e->phase_ms["wbt_stage"] = ms_since(t_host);

    /* every device buffer proportional to the batch is carved from one try
     * allocation: the later ones (per segment, per output row) by their upper
     * bound n.  Without a verified op no base can matter: no lookup. */
    const auto t_up = HostClock::now();
    const bool lookup = !e->runs.empty() && verify != nullptr && e->data_version >= 1;
    BatchSlab b;
    BaseLookup base;
    uint8_t *d_keys = nullptr, *d_svals = nullptr, *d_flags = nullptr, *d_applied = nullptr;
    uint64_t *d_koff = nullptr, *d_svoff = nullptr, *d_tt = nullptr, *d_w0 = nullptr,
             *d_w1 = nullptr, *d_head = nullptr, *d_hrank = nullptr, *d_seg_start = nullptr,
             *d_psc = nullptr, *d_seg_has = nullptr, *d_orank = nullptr, *d_seg_ksz = nullptr,
             *d_seg_vsz = nullptr, *d_red = nullptr, *d_kpos = nullptr, *d_vpos = nullptr,
             *d_row_ksrc = nullptr, *d_row_vsrc = nullptr, *d_kanch = nullptr, *d_vanch = nullptr;
    uint32_t *d_lcp = nullptr, *d_i0 = nullptr, *d_i1 = nullptr, *d_seg_last = nullptr;
    for (int pass = 0; pass < 2; pass++) { /* 0 sizes the slab, 1 hands the pieces out */
        b.take(&d_keys, in_kbytes);
        b.take(&d_koff, (n + 1) * 8); /* the lookup takes offsets */
        b.take(&d_svals, sv_bytes);
        b.take(&d_svoff, (n + 1) * 8);
        b.take(&d_flags, n);
        b.take(&d_tt, n * 8);
        b.take(&d_lcp, 256);
        b.take(&d_w0, n * 8);
        b.take(&d_w1, n * 8);
        b.take(&d_i0, n * 4);
        b.take(&d_i1, n * 4);
        b.take(&d_head, n * 8);
        b.take(&d_hrank, n * 8);
        b.take(&d_seg_start, (n + 1) * 8);
        b.take(&d_psc, psum_scratch_elems(n) * 8);
        base.take(b, lookup, n);
        b.take(&d_applied, n);
        b.take(&d_seg_last, n * 4);
        b.take(&d_seg_has, n * 8);
        b.take(&d_orank, n * 8);
        b.take(&d_seg_ksz, n * 8);
        b.take(&d_seg_vsz, n * 8);
        b.take(&d_red, TR_WORDS * 8);
        b.take(&d_kpos, n * 8);
        b.take(&d_vpos, n * 8);
        b.take(&d_row_ksrc, n * 8);
        b.take(&d_row_vsrc, n * 8);
        b.take(&d_kanch, (((in_kbytes + 15) >> 10) + 2) * 8);
        b.take(&d_vanch, (((sv_bytes + 15) >> 10) + 2) * 8);
        if (pass == 0 && !b.commit())
            return RRDB_IO_ERROR;
    }
    b.upload(d_keys, keys, in_kbytes);
    b.upload(d_koff, key_offs, (n + 1) * 8);
    b.upload(d_svals, h_svals, sv_bytes);
    b.upload(d_svoff, h_svoff, (n + 1) * 8);
    b.upload(d_flags, h_flags, n);
    b.upload_or_zero(d_tt, timetags, n * 8);
    if (!b.ok)
        return RRDB_IO_ERROR;
    e->phase_ms["wbt_upload"] = ms_since(t_up);

    PhaseEvents<6> ev;
    /* sort, then the segments: one per distinct key */
    const WbKeys wk{d_keys, in_fk ? nullptr : d_koff, in_fk, d_lcp};
    ev.record(0, e->stream);
    const SortedOps so = batch_sort(wk, n, d_lcp, d_w0, d_i0, d_w1, d_i1, e->stream);
    batch_segments(wk, n, so, d_head, d_hrank, d_seg_start, d_psc, d_red, TR_WORDS, TR_MIN_MASK,
                   e->stream);
    ev.record(1, e->stream);
    base.get(e, d_keys, d_koff, n, epoch_now);
    ev.record(2, e->stream);

    TtArgs a{};
    a.k = wk;
    a.n = n;
    a.ix = so.d_ix;
    a.seg_start = d_seg_start;
    a.flags = d_flags;
    a.tt = d_tt;
    a.svals = d_svals;
    a.svoff = d_svoff;
    a.status = base.status;
    a.hit = base.hit;
    a.runs = base.runs;
    a.data_version = e->data_version;
    a.lane_max = e->wbt_lane_max;
    a.applied = d_applied;
    a.seg_last = d_seg_last;
    a.seg_has = d_seg_has;
    a.seg_ksz = d_seg_ksz;
    a.seg_vsz = d_seg_vsz;
    a.red = (unsigned long long *)d_red;
    launch_wbt_walk(a, e->stream);
    ev.record(3, e->stream);

    /* the totals: one read */
    uint64_t red[TR_WORDS];
    HIP_OK(hipMemcpyAsync(red, d_red, sizeof(red), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    const uint64_t n_seg = red[TR_NSEG], n_out = red[TR_NOUT];
    const uint64_t kbytes = red[TR_KBYTES], vbytes = red[TR_VBYTES];
    const uint32_t out_fk = n_out ? fixed_stride_of(red[TR_KMIN], red[TR_KMAX]) : 0;
    const uint32_t out_fv = n_out ? fixed_stride_of(red[TR_VMIN], red[TR_VMAX]) : 0;

    auto results_out = [&]() {
        if (applied)
            HIP_OK(hipMemcpy(applied, d_applied, n, hipMemcpyDeviceToHost));
        if (stats) {
            stats->input_ops = n;
            stats->applied = red[TR_APPLIED];
            stats->ignored = red[TR_IGNORED];
            stats->output_records = n_out;
            stats->superseded = red[TR_APPLIED] - n_out;
            stats->puts = red[TR_PUTS];
            stats->removes = n_out - red[TR_PUTS];
            stats->key_bytes = kbytes;
            stats->value_bytes = vbytes;
        }
    };
    if (n_seg > n || n_out > n_seg || red[TR_APPLIED] + red[TR_IGNORED] != n ||
        red[TR_APPLIED] < n_out || kbytes > in_kbytes || vbytes > sv_bytes)
        return RRDB_IO_ERROR; /* cannot happen: the walk's totals contradict the batch */
    if (n_out == 0) { /* every op was ignored: no run; the seqnos are spent all the same */
        batch_phase_timers(e, "wbt", ev, false);
        e->next_seq_floor += n;
        results_out();
        return RRDB_OK;
    }

    RunBuf r;
    if (!e->alloc_base(r, n_out, kbytes, vbytes, RunAlloc::Try))
        return RRDB_IO_ERROR;
    /* the strides detect_fixed_* would report for the emitted run */
    r.fixed_klen = out_fk;
    r.fixed_vlen = out_fv;
    r.fixed_vlen_put = red[TR_PUTS] ? fixed_stride_of(red[TR_PVMIN], red[TR_PVMAX]) : 0;
    ev.record(4, e->stream);
    batch_emit_offsets(n_seg, d_seg_has, d_orank, d_seg_ksz, &d_kpos, out_fk, d_seg_vsz, &d_vpos,
                       out_fv, d_psc, e->stream);
    launch_wbt_scatter(a, n_seg, d_orank, d_kpos, d_vpos, e->next_seq_floor, n_out, kbytes, vbytes,
                       out_fk, out_fv, r.koff, r.voff, r.sk, d_row_ksrc, d_row_vsrc, e->stream);
    launch_split_copy(d_row_ksrc, r.koff, n_out, r.fixed_klen, kbytes, d_kanch, r.keys,
                      e->stream);
    launch_split_copy(d_row_vsrc, r.voff, n_out, r.fixed_vlen, vbytes, d_vanch, r.vals,
                      e->stream);
    ev.record(5, e->stream);
    if (!batch_commit_run(e, r, n))
        return RRDB_IO_ERROR;
    batch_phase_timers(e, "wbt", ev, true);
    results_out();
    return RRDB_OK;
}

/* ---- batched check-and-mutate (rrdb_check_and_mutate_batch,
 * rrdb_engine_ext.h) ----
 * The host validates and stages the entry columns (cas_stage.h) into one
 * block that mirrors the front of the device slab and uploads it in one copy
 * (the arrays the kernels read verbatim go up from the caller's memory);
 * the device sorts, groups by hashkey, looks the check keys up, walks the ops
 * and emits the run (kernels.hip, "cas batch").  Two read-backs: the totals
 * before the run and the result arena are allocated, the per-op results at
 * the end. */
static_assert(CAS_ERR_INVALID == RRDB_INVALID_ARGUMENT && CAS_ERR_TRY_AGAIN == RRDB_TRY_AGAIN,
              "the walk kernel writes these codes");
int32_t rrdb_check_and_mutate_batch(
    void *h, uint64_t n_ops, const uint8_t *check_keys, const uint64_t *check_key_offs,
    const int32_t *check_types, const uint8_t *operands, const uint64_t *operand_offs,
    const uint64_t *mut_offs, const uint8_t *mut_keys, const uint64_t *mut_key_offs,
    const uint8_t *mut_values, const uint64_t *mut_val_offs, const uint32_t *mut_expire_ts,
    const uint8_t *mut_kinds, const uint8_t *return_check_value, uint32_t epoch_now,
    int32_t *errors, uint8_t *check_exist, rrdb_result *check_values,
    rrdb_cas_batch_stats *stats)
{
    if (stats)
        *stats = rrdb_cas_batch_stats{};
    if (check_values)
        memset(check_values, 0, sizeof(*check_values));
    if (!h)
        return RRDB_INVALID_ARGUMENT;
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    if (n_ops == 0)
        return RRDB_OK;
    if (batch_blocked(e))
        return RRDB_INVALID_ARGUMENT;
    uint64_t M = 0, sv_bytes = 0;
    if (!cas_validate(n_ops, check_keys, check_key_offs, check_types, operands, operand_offs,
                      mut_offs, mut_keys, mut_key_offs, mut_values, mut_val_offs, mut_kinds, &M) ||
        !wb_staged_bytes(M, mut_val_offs, mut_kinds, e->data_version, &sv_bytes))
        return RRDB_INVALID_ARGUMENT;
    const uint64_t n = n_ops, E = n + M;

    if (const int32_t rc = batch_begin(e); rc != RRDB_OK)
        return rc;

    /* one try allocation for everything proportional to n + M; the columns
     * the host stages come first, so that they go up in one copy */
    const uint64_t ck_bytes = check_key_offs[n], mk_bytes = mut_key_offs[M];
    const uint64_t ek_bytes = ck_bytes + mk_bytes, op_bytes = operand_offs[n];
    BatchSlab b;
    BaseLookup base;
    uint8_t *d_ekeys = nullptr, *d_evals = nullptr, *d_ekind = nullptr, *d_opfl = nullptr,
            *d_ckeys = nullptr, *d_opd = nullptr, *d_khead = nullptr, *d_words = nullptr,
            *d_exist = nullptr;
    uint64_t *d_ekoff = nullptr, *d_evoff = nullptr, *d_ckoff = nullptr, *d_opoff = nullptr,
             *d_moff = nullptr, *d_w0 = nullptr, *d_w1 = nullptr, *d_hhead = nullptr,
             *d_hrank = nullptr, *d_gw0 = nullptr, *d_gw1 = nullptr, *d_seg_start = nullptr,
             *d_psc = nullptr, *d_applied = nullptr, *d_arank = nullptr, *d_cv_src = nullptr,
             *d_cv_len = nullptr, *d_cv_off = nullptr, *d_row = nullptr, *d_orank = nullptr,
             *d_ksz = nullptr, *d_vsz = nullptr, *d_kpos = nullptr, *d_vpos = nullptr,
             *d_row_ksrc = nullptr, *d_row_vsrc = nullptr, *d_kanch = nullptr, *d_vanch = nullptr,
             *d_red = nullptr;
    uint32_t *d_lcp = nullptr, *d_i0 = nullptr, *d_i1 = nullptr, *d_pos = nullptr,
             *d_glcp = nullptr, *d_gi0 = nullptr, *d_gi1 = nullptr, *d_eff = nullptr;
    int32_t *d_ct = nullptr, *d_err = nullptr;
    uint64_t up_bytes = 0;
    for (int pass = 0; pass < 2; pass++) { /* 0 sizes the slab, 1 hands the pieces out */
        b.take(&d_ekeys, ek_bytes);
        b.take(&d_ekoff, (E + 1) * 8);
        b.take(&d_evals, sv_bytes);
        b.take(&d_evoff, (E + 1) * 8);
        b.take(&d_ekind, E);
        b.take(&d_opfl, n);
        up_bytes = b.used; /* the end of the staged front */
        b.take(&d_ckeys, ck_bytes);
        b.take(&d_ckoff, (n + 1) * 8);
        b.take(&d_opd, op_bytes);
        b.take(&d_opoff, (n + 1) * 8);
        b.take(&d_ct, n * 4);
        b.take(&d_moff, (n + 1) * 8);
        b.take(&d_lcp, 256);
        b.take(&d_w0, E * 8);
        b.take(&d_w1, E * 8);
        b.take(&d_i0, E * 4);
        b.take(&d_i1, E * 4);
        b.take(&d_khead, E);
        b.take(&d_hhead, E * 8);
        b.take(&d_hrank, E * 8);
        b.take(&d_pos, E * 4);
        b.take(&d_words, n * 8);
        b.take(&d_glcp, 256);
        b.take(&d_gw0, n * 8);
        b.take(&d_gw1, n * 8);
        b.take(&d_gi0, n * 4);
        b.take(&d_gi1, n * 4);
        b.take(&d_seg_start, (n + 1) * 8);
        b.take(&d_psc, psum_scratch_elems(E) * 8);
        base.take(b, !e->runs.empty(), n);
        b.take(&d_eff, E * 4);
        b.take(&d_applied, E * 8);
        b.take(&d_arank, E * 8);
        b.take(&d_err, n * 4);
        b.take(&d_exist, n);
        b.take(&d_cv_src, n * 8);
        b.take(&d_cv_len, n * 8);
        b.take(&d_cv_off, (n + 1) * 8);
        b.take(&d_row, E * 8);
        b.take(&d_orank, E * 8);
        b.take(&d_ksz, E * 8);
        b.take(&d_vsz, E * 8);
        b.take(&d_kpos, E * 8);
        b.take(&d_vpos, E * 8);
        b.take(&d_row_ksrc, M * 8);
        b.take(&d_row_vsrc, M * 8);
        b.take(&d_kanch, (((mk_bytes + 15) >> 10) + 2) * 8);
        b.take(&d_vanch, (((sv_bytes + 15) >> 10) + 2) * 8);
        b.take(&d_red, CR_WORDS * 8);
        if (pass == 0 && !b.commit())
            return RRDB_IO_ERROR;
    }
    WbBufs hb; /* host blocks of this call */
    uint8_t *h_up = hb.get_host<uint8_t>(up_bytes);
    if (!hb.ok)
        return RRDB_IO_ERROR;
    auto host_of = [&](const void *d) { return h_up + ((const uint8_t *)d - b.base); };
    uint64_t *h_ekoff = (uint64_t *)host_of(d_ekoff);
    cas_stage(n, check_keys, check_key_offs, check_types, mut_offs, mut_keys, mut_key_offs,
              mut_values, mut_val_offs, mut_expire_ts, mut_kinds, return_check_value,
              e->data_version, e->default_ttl, epoch_now, host_of(d_ekeys), h_ekoff,
              host_of(d_evals), (uint64_t *)host_of(d_evoff), host_of(d_ekind), host_of(d_opfl));
    const uint64_t in_fk = wb_fixed_stride(h_ekoff, E);
    b.upload(b.base, h_up, up_bytes);
    /* what the kernels read as the caller wrote it goes up from where it is */
    b.upload(d_ckeys, check_keys, ck_bytes);
    b.upload(d_ckoff, check_key_offs, (n + 1) * 8);
    b.upload(d_opd, operands, op_bytes);
    b.upload(d_opoff, operand_offs, (n + 1) * 8);
    b.upload(d_ct, check_types, n * 4);
    b.upload(d_moff, mut_offs, (n + 1) * 8);
    if (b.ok && (hipMemset(d_eff, 0xFF, E * 4) != hipSuccess ||
                 hipMemset(d_applied, 0, E * 8) != hipSuccess)) {
        (void)hipGetLastError();
        b.ok = false;
    }
    if (!b.ok)
        return RRDB_IO_ERROR;

    PhaseEvents<6> ev;
    /* sort the entries; key heads, hashkey groups, the ops by group */
    const WbKeys wk{d_ekeys, in_fk ? nullptr : d_ekoff, in_fk, d_lcp};
    ev.record(0, e->stream);
    const SortedOps so = batch_sort(wk, E, d_lcp, d_w0, d_i0, d_w1, d_i1, e->stream);
    launch_cas_heads(wk, E, so.d_w, so.d_ix, d_khead, d_hhead, d_pos, d_red, e->stream);
    launch_psum(d_hhead, d_hrank, E, d_psc, e->stream);
    launch_cas_group_words(n, E, d_moff, d_pos, d_hhead, d_hrank, d_words, d_red, e->stream);
    const WbKeys gk{d_words, nullptr, 8, d_glcp};
    const uint32_t *d_ops =
        batch_sort(gk, n, d_glcp, d_gw0, d_gi0, d_gw1, d_gi1, e->stream).d_ix;
    launch_cas_segs(n, d_words, d_ops, d_seg_start, e->stream);
    ev.record(1, e->stream);
    base.get(e, d_ckeys, d_ckoff, n, epoch_now); /* the check keys' */
    ev.record(2, e->stream);

    CasArgs a{};
    a.k = wk;
    a.n = n;
    a.E = E;
    a.ix = so.d_ix;
    a.pos = d_pos;
    a.khead = d_khead;
    a.svals = d_evals;
    a.svoff = d_evoff;
    a.kind = d_ekind;
    a.op_flags = d_opfl;
    a.ctype = d_ct;
    a.opd = d_opd;
    a.opoff = d_opoff;
    a.moff = d_moff;
    a.ops = d_ops;
    a.seg_start = d_seg_start;
    a.status = base.status;
    a.hit = base.hit;
    a.runs = base.runs;
    a.data_version = e->data_version;
    a.epoch_now = epoch_now;
    a.eff = d_eff;
    a.applied = d_applied;
    a.err = d_err;
    a.exist = d_exist;
    a.cv_src = d_cv_src;
    a.cv_len = d_cv_len;
    a.red = (unsigned long long *)d_red;
    launch_cas_walk(a, e->stream);
    launch_psum(d_applied, d_arank, E, d_psc, e->stream);
    launch_cas_rows(a, d_row, d_ksz, d_vsz, e->stream);
    launch_psum(d_row, d_orank, E, d_psc, e->stream);
    launch_psum(d_ksz, d_kpos, E, d_psc, e->stream);
    launch_psum(d_vsz, d_vpos, E, d_psc, e->stream);
    if (check_values)
        launch_psum(d_cv_len, d_cv_off, n, d_psc, e->stream);
    ev.record(3, e->stream);

    /* the totals: one read */
    uint64_t red[CR_WORDS];
    HIP_OK(hipMemcpyAsync(red, d_red, sizeof(red), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    const uint64_t n_out = red[CR_NOUT], kbytes = red[CR_KBYTES], vbytes = red[CR_VBYTES];
    const uint64_t applied = red[CR_APPLIED], ret_bytes = red[CR_RETBYTES];
    if (n_out > M || applied > M || kbytes > mk_bytes || vbytes > sv_bytes ||
        (n_out == 0) != (applied == 0))
        return RRDB_IO_ERROR; /* cannot happen: the totals come from the staged columns */

    /* the returned check values: gathered into one device buffer, then one
     * copy into the result's arena */
    ev.record(4, e->stream);
    WbBufs cvb;
    if (check_values) {
        Arena *ar = result_init(check_values);
        rrdb_slice *sl = (rrdb_slice *)ar->alloc(n * sizeof(rrdb_slice));
        uint8_t *blk = (uint8_t *)ar->alloc(ret_bytes);
        uint64_t *h_len = cvb.get_host<uint64_t>(n * 8);
        const uint64_t anch_bytes = ((((ret_bytes + 15) >> 10) + 2) * 8 + 255) & ~255ull;
        uint8_t *d_cv = ret_bytes ? cvb.get<uint8_t>(anch_bytes + ret_bytes) : nullptr;
        if (!sl || !blk || !cvb.ok)
            return RRDB_IO_ERROR;
        if (ret_bytes) {
            HIP_OK(hipMemcpyAsync(d_cv_off + n, d_red + CR_RETBYTES, 8, hipMemcpyDeviceToDevice,
                                  e->stream));
            launch_split_copy(d_cv_src, d_cv_off, n, 0, ret_bytes, (uint64_t *)d_cv,
                              d_cv + anch_bytes, e->stream);
            HIP_OK(hipMemcpyAsync(blk, d_cv + anch_bytes, ret_bytes, hipMemcpyDeviceToHost,
                                  e->stream));
        }
        HIP_OK(hipMemcpyAsync(h_len, d_cv_len, n * 8, hipMemcpyDeviceToHost, e->stream));
        HIP_OK(hipStreamSynchronize(e->stream));
        uint64_t at = 0;
        for (uint64_t i = 0; i < n; i++) {
            sl[i] = {blk + at, h_len[i]};
            at += h_len[i];
        }
        if (at != ret_bytes)
            return RRDB_IO_ERROR; /* cannot happen: one column, summed twice */
        check_values->values = sl;
        check_values->count = n;
        check_values->error = RRDB_OK;
    }

    auto results_out = [&]() {
        if (errors)
            HIP_OK(hipMemcpy(errors, d_err, n * 4, hipMemcpyDeviceToHost));
        if (check_exist)
            HIP_OK(hipMemcpy(check_exist, d_exist, n, hipMemcpyDeviceToHost));
        if (stats) {
            stats->input_ops = n;
            stats->passed = red[CR_PASSED];
            stats->failed_check = red[CR_FCHECK];
            stats->failed_invalid = red[CR_FINVALID];
            stats->malformed = red[CR_MALFORMED];
            stats->mutations_applied = applied;
            stats->output_records = n_out;
            stats->puts = red[CR_PUTS];
            stats->removes = n_out - red[CR_PUTS];
            stats->key_bytes = kbytes;
            stats->value_bytes = vbytes;
        }
    };
    /* cas_emit runs from event 4, so it covers the check-value gather above,
     * and is measured on the no-run path too */
    if (n_out == 0) { /* no check passed: no run, the floor stays */
        ev.record(5, e->stream);
        HIP_OK(hipStreamSynchronize(e->stream));
        batch_phase_timers(e, "cas", ev, true);
        results_out();
        return RRDB_OK;
    }

    RunBuf r;
    if (!e->alloc_base(r, n_out, kbytes, vbytes, RunAlloc::Try))
        return RRDB_IO_ERROR;
    /* the strides detect_fixed_* would report for the emitted run */
    r.fixed_klen = fixed_stride_of(red[CR_KMIN], red[CR_KMAX]);
    r.fixed_vlen = fixed_stride_of(red[CR_VMIN], red[CR_VMAX]);
    r.fixed_vlen_put = red[CR_PUTS] ? fixed_stride_of(red[CR_PVMIN], red[CR_PVMAX]) : 0;
    launch_cas_emit(a, d_row, d_orank, d_kpos, d_vpos, d_arank, e->next_seq_floor, n_out, kbytes,
                    vbytes, r.koff, r.voff, r.sk, d_row_ksrc, d_row_vsrc, e->stream);
    launch_split_copy(d_row_ksrc, r.koff, n_out, r.fixed_klen, kbytes, d_kanch, r.keys,
                      e->stream);
    launch_split_copy(d_row_vsrc, r.voff, n_out, r.fixed_vlen, vbytes, d_vanch, r.vals,
                      e->stream);
    ev.record(5, e->stream);
    if (!batch_commit_run(e, r, applied))
        return RRDB_IO_ERROR;
    HIP_OK(hipStreamSynchronize(e->stream));
    batch_phase_timers(e, "cas", ev, true);
    results_out();
    return RRDB_OK;
}

} /* extern "C" */

/* ================= checkpoint (§8(f)2) ================= */
#include <sys/stat.h>
#include <cstdio>

extern "C" {

static bool write_file(const std::string &path, const void *data, uint64_t n)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f)
        return false;
    bool ok = (n == 0) || fwrite(data, 1, n, f) == n;
    fclose(f);
    return ok;
}

static bool read_file(const std::string &path, std::vector<uint8_t> &out)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f)
        return false;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize((size_t)n);
    bool ok = (n == 0) || fread(out.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}

int32_t rrdb_checkpoint(void *h, const char *dir, uint64_t decree)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    engine_flush(e);
    e->activate();
    std::string path = std::string(dir) + "/checkpoint." + std::to_string(decree);
    mkdir(dir, 0755);
    if (mkdir(path.c_str(), 0755) != 0)
        return RRDB_IO_ERROR;
    /* run files first (crc64 of each goes into the MANIFEST; a restorer
     * verifies — the reference's checkpoints carry rocksdb's per-block
     * checksums, restated here at file granularity) */
    std::string crc_lines;
    char cl[128];
    std::vector<uint8_t> buf;
    for (size_t i = 0; i < e->runs.size(); i++) {
        const RunBuf &r = e->runs[i];
        /* offsets first (host copies give the blob sizes) */
        std::vector<uint64_t> koff(r.n + 1), voff(r.n + 1), sk(r.n);
        HIP_OK(hipMemcpy(koff.data(), r.koff, (r.n + 1) * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(voff.data(), r.voff, (r.n + 1) * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(sk.data(), r.sk, r.n * 8, hipMemcpyDeviceToHost));
        std::string base = path + "/run_" + std::to_string(i);
        auto emit = [&](const char *ext, const void *p, uint64_t n) {
            if (!write_file(base + "." + ext, p, n))
                return false;
            snprintf(cl, sizeof(cl), "crc run_%zu.%s %016llx\n", i, ext,
                     (unsigned long long)host_crc64(p, n));
            crc_lines += cl;
            return true;
        };
        buf.resize(koff[r.n]);
        HIP_OK(hipMemcpy(buf.data(), r.keys, koff[r.n], hipMemcpyDeviceToHost));
        if (!emit("keys", buf.data(), koff[r.n]))
            return RRDB_IO_ERROR;
        if (!emit("koff", koff.data(), (r.n + 1) * 8))
            return RRDB_IO_ERROR;
        buf.resize(voff[r.n]);
        HIP_OK(hipMemcpy(buf.data(), r.vals, voff[r.n], hipMemcpyDeviceToHost));
        if (!emit("vals", buf.data(), voff[r.n]))
            return RRDB_IO_ERROR;
        if (!emit("voff", voff.data(), (r.n + 1) * 8))
            return RRDB_IO_ERROR;
        if (!emit("sk", sk.data(), r.n * 8))
            return RRDB_IO_ERROR;
    }
    FILE *mf = fopen((path + "/MANIFEST").c_str(), "w");
    if (!mf)
        return RRDB_IO_ERROR;
    fprintf(mf, "rrdb-checkpoint 1\ndata_version %u\nnext_seq_floor %llu\nn_runs %d\n",
            e->data_version, (unsigned long long)e->next_seq_floor, (int)e->runs.size());
    for (size_t i = 0; i < e->runs.size(); i++)
        fprintf(mf, "run %zu %llu\n", i, (unsigned long long)e->runs[i].n);
    fputs(crc_lines.c_str(), mf); /* trailing lines; older restorers ignore */
    fclose(mf);
    return RRDB_OK;
}

int32_t rrdb_restore(void *h, const char *dir, uint64_t decree)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->runs.empty() || !e->memtable.empty())
        return RRDB_INVALID_ARGUMENT;
    e->activate();
    std::string path = std::string(dir) + "/checkpoint." + std::to_string(decree);
    FILE *mf = fopen((path + "/MANIFEST").c_str(), "r");
    if (!mf)
        return RRDB_IO_ERROR;
    unsigned dv = 1;
    unsigned long long floor_ = 0;
    int n_runs = 0, ver = 0;
    if (fscanf(mf, "rrdb-checkpoint %d\ndata_version %u\nnext_seq_floor %llu\nn_runs %d\n", &ver,
               &dv, &floor_, &n_runs) != 4 ||
        ver != 1 || n_runs < 0) {
        fclose(mf);
        return RRDB_CORRUPTION;
    }
    /* run record counts + optional per-file crc lines (older checkpoints
     * carry none; then crc validation is skipped) */
    std::vector<unsigned long long> mrows((size_t)n_runs, ~0ull);
    std::unordered_map<std::string, uint64_t> mcrc;
    {
        char line[256];
        while (fgets(line, sizeof(line), mf)) {
            unsigned long long a, b;
            char name[128];
            if (sscanf(line, "run %llu %llu", &a, &b) == 2) {
                if (a < (unsigned long long)n_runs)
                    mrows[(size_t)a] = b;
            } else if (sscanf(line, "crc %127s %llx", name, &b) == 2) {
                mcrc[name] = b;
            }
        }
    }
    fclose(mf);
    for (int i = 0; i < n_runs; i++)
        if (mrows[(size_t)i] == ~0ull)
            return RRDB_CORRUPTION; /* MANIFEST missing a run line */
    e->data_version = dv;
    for (int i = 0; i < n_runs; i++) {
        std::string base = path + "/run_" + std::to_string(i);
        std::vector<uint8_t> keys, koff, vals, voff, sk;
        if (!read_file(base + ".keys", keys) || !read_file(base + ".koff", koff) ||
            !read_file(base + ".vals", vals) || !read_file(base + ".voff", voff) ||
            !read_file(base + ".sk", sk))
            return RRDB_IO_ERROR;
        /* integrity validation: crc when present, sizes vs the
         * MANIFEST count, offset monotonicity, key sortedness — a truncated
         * or bit-flipped file returns kCorruption instead of corrupting the
         * engine (the reference restores from checksummed rocksdb
         * checkpoints; same guarantee at our file granularity) */
        auto crc_ok = [&](const char *ext, const std::vector<uint8_t> &data) {
            auto it = mcrc.find("run_" + std::to_string(i) + "." + ext);
            return it == mcrc.end() || it->second == host_crc64(data.data(), data.size());
        };
        if (!crc_ok("keys", keys) || !crc_ok("koff", koff) || !crc_ok("vals", vals) ||
            !crc_ok("voff", voff) || !crc_ok("sk", sk))
            return RRDB_CORRUPTION;
        uint64_t nrec = mrows[(size_t)i];
        if (koff.size() != (nrec + 1) * 8 || voff.size() != (nrec + 1) * 8 ||
            sk.size() != nrec * 8)
            return RRDB_CORRUPTION;
        const uint64_t *ko = (const uint64_t *)koff.data();
        const uint64_t *vo = (const uint64_t *)voff.data();
        if (ko[0] != 0 || vo[0] != 0 || ko[nrec] != keys.size() || vo[nrec] != vals.size())
            return RRDB_CORRUPTION;
        for (uint64_t j = 0; j < nrec; j++)
            if (ko[j + 1] <= ko[j] || vo[j + 1] < vo[j])
                return RRDB_CORRUPTION; /* keys nonempty+increasing offsets */
        for (uint64_t j = 0; j + 1 < nrec; j++) {
            uint64_t la = ko[j + 1] - ko[j], lb = ko[j + 2] - ko[j + 1];
            uint64_t m = la < lb ? la : lb;
            int c = memcmp(keys.data() + ko[j], keys.data() + ko[j + 1], m);
            if (c > 0 || (c == 0 && la >= lb))
                return RRDB_CORRUPTION; /* keys must be strictly increasing */
        }
        RunBuf r;
        KeyEnds ends;
        e->upload_run(r, keys.data(), ko, vals.data(), vo, (const uint64_t *)sk.data(), nrec,
                      RunAlloc::Abort, &ends);
        /* derived columns are rebuilt, not serialized */
        e->finish_run(r, &ends, RunAlloc::Abort, e->bloom_enabled);
        e->runs.push_back(r);
    }
    e->next_seq_floor = floor_;
    e->runs_changed();
    return RRDB_OK;
}

} /* extern "C" */

/* ================= batched multi_get =================
 * One workgroup per request (full-range multi_get per hashkey) — models the
 * reference's concurrent THREAD_POOL_SCAN handlers in a single launch.
 * Requests whose ranges exceed the fused budget (or exotic shared params)
 * fall back to the general per-request path. */
extern "C" int32_t rrdb_multi_get_batch(void *h, uint64_t n_req, const uint8_t *hash_keys,
                                        const uint64_t *hk_offs,
                                        const rrdb_multi_get_request *shared,
                                        uint32_t epoch_now, rrdb_result *out)
{
    auto *e = (HipEngine *)h;
    std::lock_guard<std::mutex> g(e->mu);
    if (engine_flush(e) != RRDB_OK) {
        result_init(out);
        out->error = RRDB_IO_ERROR;
        return out->error;
    }
    e->activate();
    /* bulk path: retire the resident serving kernel so its poll windows do
     * not share hardware queues with the 4096-workgroup batch launches */
    e->server_quit_sync();
    e->scratch_reset();
    Arena *a = result_init(out);
    e->last_mg_lane.batch_fused = 0;
    e->last_mg_lane.batch_fallback = 0;
    e->last_mg_lane.batch_device_out = 0;
    if (shared->n_sort_keys != 0 || shared->sort_key_filter_type < 0 ||
        shared->sort_key_filter_type > 3) {
        out->error = RRDB_INVALID_ARGUMENT;
        return out->error;
    }
    out->group_counts = (uint64_t *)a->alloc(n_req * 8);
    out->group_errors = (int32_t *)a->alloc(n_req * 4);
    /* fused batch only covers the full-range shape (no sortkey bounds, no
     * range-clamping prefix filter) over at most RRDB_MAX_RUNS runs (mg_core
     * indexes per-run LDS arrays of that size); others run per-request */
    bool fused_ok = shared->start_sortkey.len == 0 && shared->stop_sortkey.len == 0 &&
                    shared->start_inclusive &&
                    !(shared->sort_key_filter_type == RRDB_FT_MATCH_PREFIX &&
                      shared->sort_key_filter_pattern.len > 0) &&
                    !e->runs.empty() && (int)e->runs.size() <= RRDB_MAX_RUNS;
    const uint64_t BLOB_STRIDE = 64 << 10;
    std::vector<int64_t> hdrs(n_req * 4, -1);
    uint8_t *d_blobs = nullptr;
    std::vector<uint64_t> used(n_req, 0), pack_off(n_req + 1, 0);
    std::vector<uint8_t> packed_host;
    if (fused_ok && n_req > 0) {
        const MgLimits lim(e, shared);
        MgFusedArgs fa{};
        fa.start_inclusive = 1;
        fa.stop_inclusive = 0;
        fa.reverse = shared->reverse;
        fa.no_value = shared->no_value;
        fa.max_kv_count = lim.max_kv_count;
        fa.max_iteration_count = lim.max_iteration_count;
        fa.max_iteration_size = lim.max_iter_size;
        fa.sk_ft = shared->sort_key_filter_type;
        fa.sk_pat_len = shared->sort_key_filter_pattern.len;
        fa.sk_pat = e->upload_tmp(shared->sort_key_filter_pattern.data, fa.sk_pat_len);
        fa.epoch_now = epoch_now;
        fa.data_version = e->data_version;
        /* per-request hash_key_skip (= start key length) is computed
         * in-kernel so size caps count sortkey+value, as the reference does */
        uint8_t *d_hks = e->upload_tmp(hash_keys, hk_offs[n_req]);
        uint64_t *d_offs = (uint64_t *)e->upload_tmp(hk_offs, (n_req + 1) * 8);
        int64_t *d_hdrs = e->talloc<int64_t>(n_req * 4 * 8);
        HIP_OK(hipMemsetAsync(d_hdrs, 0xFF, n_req * 4 * 8, e->stream)); /* -1 fill */
        d_blobs = e->talloc<uint8_t>(n_req * BLOB_STRIDE);
        launch_multi_get_batch(e->dev_runs(), (int)e->runs.size(), fa, d_hks, d_offs, n_req,
                               d_hdrs, d_blobs, BLOB_STRIDE, e->stream);
        HIP_OK(hipMemcpyAsync(hdrs.data(), d_hdrs, n_req * 4 * 8, hipMemcpyDeviceToHost,
                              e->stream));
        HIP_OK(hipStreamSynchronize(e->stream));
        /* pack used regions, one D2H */
        uint64_t total = 0;
        for (uint64_t i = 0; i < n_req; i++) {
            if (hdrs[i * 4] >= 0) {
                uint64_t m = (uint64_t)hdrs[i * 4];
                used[i] = 2 * (m + 1) * 8 + (uint64_t)hdrs[i * 4 + 2] + (uint64_t)hdrs[i * 4 + 3];
            }
            pack_off[i] = total;
            total += used[i];
        }
        pack_off[n_req] = total;
        bool all_fused = true;
        for (uint64_t i = 0; i < n_req; i++)
            if (hdrs[i * 4] < 0)
                all_fused = false;
        if (total && shared->on_device_out && all_fused) {
            /* device-out: pack into caller-owned device memory, no host
             * marshal (the batched e2e limiter on slow-host boxes) */
            uint8_t *d_packed = nullptr;
            uint64_t *d_poff_out = nullptr;
            HIP_OK(hipMalloc(&d_packed, total));
            HIP_OK(hipMalloc(&d_poff_out, (n_req + 1) * 8));
            HIP_OK(hipMemcpyAsync(d_poff_out, pack_off.data(), (n_req + 1) * 8,
                                  hipMemcpyHostToDevice, e->stream));
            uint64_t *d_used = (uint64_t *)e->upload_tmp(used.data(), n_req * 8);
            uint64_t *d_poff = (uint64_t *)e->upload_tmp(pack_off.data(), (n_req + 1) * 8);
            launch_pack_blobs(d_blobs, BLOB_STRIDE, n_req, d_used, d_poff, d_packed, e->stream);
            HIP_OK(hipStreamSynchronize(e->stream));
            uint64_t rows = 0;
            for (uint64_t i = 0; i < n_req; i++) {
                out->group_counts[i] = (uint64_t)hdrs[i * 4];
                out->group_errors[i] = hdrs[i * 4 + 1] ? RRDB_OK : RRDB_INCOMPLETE;
                rows += (uint64_t)hdrs[i * 4];
            }
            out->dev_vals = d_packed;
            out->dev_val_offs = d_poff_out;
            e->last_mg_lane.batch_fused = n_req;
            e->last_mg_lane.batch_device_out = 1;
            a->dev_ptrs.insert(a->dev_ptrs.end(), {(void *)d_packed, (void *)d_poff_out});
            out->count = rows;
            out->error = RRDB_OK;
            return RRDB_OK;
        }
        if (total) {
            uint64_t *d_used = (uint64_t *)e->upload_tmp(used.data(), n_req * 8);
            uint64_t *d_poff = (uint64_t *)e->upload_tmp(pack_off.data(), (n_req + 1) * 8);
            uint8_t *d_packed = e->talloc<uint8_t>(total);
            launch_pack_blobs(d_blobs, BLOB_STRIDE, n_req, d_used, d_poff, d_packed, e->stream);
            packed_host.resize(total);
            e->d2h(packed_host.data(), d_packed, total);
        }
    }
    /* count rows (fused + fallback) */
    uint64_t total_rows = 0;
    std::vector<rrdb_result> fb(n_req);
    std::vector<uint8_t> is_fb(n_req, 0);
    for (uint64_t i = 0; i < n_req; i++) {
        if (hdrs[i * 4] >= 0) {
            total_rows += (uint64_t)hdrs[i * 4];
            e->last_mg_lane.batch_fused++;
        } else {
            e->last_mg_lane.batch_fallback++;
            /* general path per request (rare) */
            is_fb[i] = 1;
            rrdb_multi_get_request req = *shared;
            req.hash_key.data = hash_keys + hk_offs[i];
            req.hash_key.len = hk_offs[i + 1] - hk_offs[i];
            rrdb_multi_get_lane scratch_rep;
            multi_get_locked(h, &req, epoch_now, &fb[i], &scratch_rep);
            total_rows += fb[i].count;
        }
    }
    out->keys = (rrdb_slice *)a->alloc((total_rows ? total_rows : 1) * sizeof(rrdb_slice));
    out->values = (rrdb_slice *)a->alloc((total_rows ? total_rows : 1) * sizeof(rrdb_slice));
    uint8_t *pb = nullptr;
    if (!packed_host.empty()) {
        pb = (uint8_t *)a->alloc(packed_host.size());
        memcpy(pb, packed_host.data(), packed_host.size());
    }
    uint64_t m = 0;
    for (uint64_t i = 0; i < n_req; i++) {
        if (!is_fb[i]) {
            uint64_t n = (uint64_t)hdrs[i * 4];
            uint64_t kb = (uint64_t)hdrs[i * 4 + 2];
            out->group_counts[i] = n;
            out->group_errors[i] = hdrs[i * 4 + 1] ? RRDB_OK : RRDB_INCOMPLETE;
            if (n == 0)
                continue;
            uint8_t *base = pb + pack_off[i];
            const uint64_t *koffs = (const uint64_t *)base;
            const uint64_t *voffs = koffs + (n + 1);
            uint8_t *keys_b = base + 2 * (n + 1) * 8;
            uint8_t *vals_b = keys_b + kb;
            for (uint64_t j = 0; j < n; j++) {
                out->keys[m] = {keys_b + koffs[j], koffs[j + 1] - koffs[j]};
                out->values[m] = {vals_b + voffs[j], voffs[j + 1] - voffs[j]};
                m++;
            }
        } else {
            out->group_counts[i] = fb[i].count;
            out->group_errors[i] = fb[i].error;
            for (uint64_t j = 0; j < fb[i].count; j++) {
                uint64_t kl = fb[i].keys[j].len, vl = fb[i].values[j].len;
                uint8_t *kc = (uint8_t *)a->alloc(kl ? kl : 1);
                memcpy(kc, fb[i].keys[j].data, kl);
                uint8_t *vc = (uint8_t *)a->alloc(vl ? vl : 1);
                memcpy(vc, fb[i].values[j].data, vl);
                out->keys[m] = {kc, kl};
                out->values[m] = {vc, vl};
                m++;
            }
            rrdb_free_result(&fb[i]);
        }
    }
    out->count = m;
    out->error = RRDB_OK;
    return RRDB_OK;
}

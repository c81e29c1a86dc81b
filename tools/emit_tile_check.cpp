/* emit_tile_check.cpp — stand-alone CPU check of the indexing arithmetic of
 * the fused fixed-stride compaction emit (incubator_pegasus_amd/csrc/
 * emit_tile.h).  The device kernels compile the same header, so what holds
 * here holds there.  Every step of the emit is replayed thread by thread on
 * the host with the header's functions and compared with a brute-force loop:
 *   - tile spans: the tiles cut [0, total) without gap or overlap, and the
 *     (thread, j) slots of a tile cover it once, 64-rank segment by segment;
 *   - the multi-pass scan: tile bases and the grand total against a running
 *     sum, for tile counts below, at and above one pass;
 *   - output rows: every kept rank's row index and byte offsets, the terminal
 *     offsets, for keep patterns with an empty tile, only the first or only
 *     the last rank kept, nothing kept;
 *   - the copies: chunk -> (row, offset) for 16-byte-multiple strides and the
 *     word/tail pieces for the others write every byte of the tile's span
 *     once, from exact-size heap rows into an exact-size heap span, with the
 *     expire header patched at offset 0 and 1.
 * Meant to run under the address and undefined-behaviour sanitizers:
 *
 *   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       tools/emit_tile_check.cpp -o bin/emit_tile_check && bin/emit_tile_check
 *
 * No HIP, no GPU, nothing loaded into another process.  Exit status 0 and a
 * final "emit_tile_check OK" line mean every expectation held. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../incubator_pegasus_amd/csrc/emit_tile.h"

namespace {

int g_fail = 0;

#define EXPECT(c)                                                                                 \
    do {                                                                                          \
        if (!(c)) {                                                                               \
            if (g_fail < 20)                                                                      \
                fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c);                       \
            g_fail++;                                                                             \
        }                                                                                         \
    } while (0)

constexpr uint32_t WAVE = 64;
constexpr uint32_t NW = EMIT_THREADS / WAVE;

enum Pattern { P_RANDOM, P_ALL, P_NONE, P_FIRST, P_LAST, P_EMPTY_TILE };

std::vector<uint8_t> keep_flags(uint64_t total, Pattern p, uint32_t seed)
{
    std::vector<uint8_t> k(total, 0);
    std::mt19937 rng(seed);
    for (uint64_t i = 0; i < total; i++) {
        switch (p) {
        case P_RANDOM: k[i] = rng() % 8 != 0; break;
        case P_ALL: k[i] = 1; break;
        case P_NONE: break;
        case P_FIRST: k[i] = i == 0; break;
        case P_LAST: k[i] = i == total - 1; break;
        case P_EMPTY_TILE: k[i] = (i / EMIT_TILE) != 1 && rng() % 3 != 0; break;
        }
    }
    return k;
}

/* k_keep_tile_counts + k_keep_tile_scan, thread by thread */
void scan_tiles(const std::vector<uint8_t> &keep, std::vector<uint32_t> *counts,
                std::vector<uint64_t> *base, uint64_t *n_out)
{
    const uint64_t total = keep.size();
    const uint64_t n_tiles = emit_n_tiles(total);
    counts->assign(n_tiles, 0);
    base->assign(n_tiles, ~0ull);
    uint64_t covered = 0;
    for (uint64_t t = 0; t < n_tiles; t++) {
        const uint32_t len = emit_tile_len(total, t);
        EXPECT(len > 0 && len <= EMIT_TILE);
        EXPECT(t * EMIT_TILE == covered);
        covered += len;
        for (uint32_t j = 0; j < len; j++)
            (*counts)[t] += keep[t * EMIT_TILE + j];
    }
    EXPECT(covered == total);
    EXPECT(emit_tile_len(total, n_tiles) == 0);
    uint64_t carry = 0;
    const uint64_t passes = emit_scan_passes(n_tiles);
    EXPECT(passes * EMIT_SCAN_PASS >= n_tiles);
    EXPECT(n_tiles == 0 || (passes - 1) * EMIT_SCAN_PASS < n_tiles);
    for (uint64_t ps = 0; ps < passes; ps++) {
        uint32_t c[EMIT_SCAN_PASS], wsum[EMIT_SCAN_PASS / WAVE] = {};
        for (uint32_t tid = 0; tid < EMIT_SCAN_PASS; tid++) {
            const uint64_t t = emit_scan_tile(ps, tid);
            c[tid] = t < n_tiles ? (*counts)[t] : 0;
            wsum[tid / WAVE] += c[tid];
        }
        uint32_t ptot = 0;
        for (uint32_t w = 0; w < EMIT_SCAN_PASS / WAVE; w++)
            ptot += wsum[w];
        for (uint32_t tid = 0; tid < EMIT_SCAN_PASS; tid++) {
            const uint64_t t = emit_scan_tile(ps, tid);
            uint32_t wbase = 0, excl = 0;
            for (uint32_t w = 0; w < tid / WAVE; w++)
                wbase += wsum[w];
            for (uint32_t l = tid - tid % WAVE; l < tid; l++)
                excl += c[l];
            if (t < n_tiles) {
                EXPECT((*base)[t] == ~0ull); /* written once */
                (*base)[t] = emit_scan_base(carry, wbase, excl);
            }
        }
        carry = emit_scan_carry(carry, ptot);
    }
    *n_out = carry;
    uint64_t run = 0;
    for (uint64_t t = 0; t < n_tiles; t++) {
        EXPECT((*base)[t] == run);
        run += (*counts)[t];
    }
    EXPECT(*n_out == run);
}

/* the emit's scan of one tile: local row of every kept slot */
void check_rows(const std::vector<uint8_t> &keep, const std::vector<uint32_t> &counts,
                const std::vector<uint64_t> &base, uint64_t n_out, uint32_t fk, uint32_t fv)
{
    const uint64_t total = keep.size();
    std::vector<uint64_t> want_row(total, ~0ull);
    uint64_t o = 0;
    for (uint64_t p = 0; p < total; p++)
        if (keep[p])
            want_row[p] = o++;
    EXPECT(o == n_out);
    std::vector<uint8_t> row_seen(n_out, 0);
    for (uint64_t t = 0; t < emit_n_tiles(total); t++) {
        const uint32_t len = emit_tile_len(total, t);
        uint32_t seg[EMIT_RANKS_PER_THREAD * NW] = {};
        uint8_t slot_seen[EMIT_TILE] = {};
        for (uint32_t tid = 0; tid < EMIT_THREADS; tid++)
            for (uint32_t j = 0; j < EMIT_RANKS_PER_THREAD; j++) {
                const uint32_t l = emit_tile_slot(tid, j);
                EXPECT(l < EMIT_TILE && !slot_seen[l]);
                slot_seen[l] = 1;
                EXPECT(l / WAVE == j * NW + tid / WAVE && l % WAVE == tid % WAVE);
                if (l < len && keep[t * EMIT_TILE + l])
                    seg[j * NW + tid / WAVE]++;
            }
        uint32_t cnt = 0;
        for (uint32_t q = 0; q < EMIT_RANKS_PER_THREAD * NW; q++)
            cnt += seg[q];
        EXPECT(cnt == counts[t]);
        for (uint32_t tid = 0; tid < EMIT_THREADS; tid++)
            for (uint32_t j = 0; j < EMIT_RANKS_PER_THREAD; j++) {
                const uint32_t l = emit_tile_slot(tid, j);
                if (l >= len || !keep[t * EMIT_TILE + l])
                    continue;
                uint32_t pre = 0, below = 0;
                for (uint32_t q = 0; q < j * NW + tid / WAVE; q++)
                    pre += seg[q];
                for (uint32_t x = l - l % WAVE; x < l; x++)
                    below += x < len && keep[t * EMIT_TILE + x];
                const uint32_t loc = pre + below;
                EXPECT(loc < cnt);
                const uint64_t row = base[t] + loc;
                EXPECT(row == want_row[t * EMIT_TILE + l]);
                if (row < n_out) {
                    EXPECT(!row_seen[row]);
                    row_seen[row] = 1;
                }
                /* offsets are a running sum of the strides */
                EXPECT(emit_row_off(row, fk) + fk == emit_row_off(row + 1, fk));
                EXPECT(emit_row_off(row, fv) + fv == emit_row_off(row + 1, fv));
            }
    }
    for (uint64_t r = 0; r < n_out; r++)
        EXPECT(row_seen[r]);
    uint64_t kb = 0, vb = 0;
    for (uint64_t r = 0; r < n_out; r++) {
        kb += fk;
        vb += fv;
    }
    EXPECT(emit_row_off(n_out, fk) == kb && emit_row_off(n_out, fv) == vb); /* terminal */
    EXPECT(emit_row_off(0, fk) == 0);
}

/* emit_copy_span of kernels.hip on the host: cnt rows of `stride` bytes, each
 * source row its own exact-size allocation, into an exact-size span */
void check_copy(uint32_t cnt, uint32_t stride, uint32_t data_version, uint32_t seed)
{
    std::mt19937 rng(seed);
    const uint32_t hoff = emit_expire_off(data_version);
    EXPECT(hoff == (data_version == 2 ? 1u : 0u) && hoff + 4 <= 8);
    std::vector<std::unique_ptr<uint8_t[]>> src(cnt);
    std::vector<uint8_t> pat(cnt);
    std::vector<uint32_t> ts(cnt);
    const bool can_patch = stride >= hoff + 4;
    for (uint32_t r = 0; r < cnt; r++) {
        src[r].reset(new uint8_t[stride]);
        for (uint32_t b = 0; b < stride; b++)
            src[r][b] = (uint8_t)rng();
        pat[r] = can_patch && (r == 0 || r == cnt - 1 || rng() % 3 == 0);
        ts[r] = r % 5 == 0 ? 0xFFFFFFFFu : (uint32_t)rng();
    }
    const size_t bytes = (size_t)cnt * stride;
    std::unique_ptr<uint8_t[]> want(new uint8_t[bytes ? bytes : 1]);
    for (uint32_t r = 0; r < cnt; r++) {
        memcpy(want.get() + (size_t)r * stride, src[r].get(), stride);
        if (pat[r]) {
            uint8_t *v = want.get() + (size_t)r * stride + hoff;
            v[0] = (uint8_t)(ts[r] >> 24);
            v[1] = (uint8_t)(ts[r] >> 16);
            v[2] = (uint8_t)(ts[r] >> 8);
            v[3] = (uint8_t)ts[r];
        }
    }
    std::unique_ptr<uint8_t[]> dst(new uint8_t[bytes ? bytes : 1]);
    std::vector<uint8_t> written(bytes, 0);
    auto mark = [&](size_t at, size_t n) {
        for (size_t b = at; b < at + n; b++) {
            EXPECT(b < bytes && !written[b]);
            if (b < bytes)
                written[b] = 1;
        }
    };
    if (emit_stride_chunked(stride)) {
        const uint32_t cpr = emit_chunks_per_row(stride);
        const uint32_t n_chunks = emit_span_chunks(cnt, stride);
        EXPECT((size_t)n_chunks * 16 == bytes);
        for (uint32_t c = 0; c < n_chunks; c++) {
            uint32_t row, off;
            emit_chunk_row(c, cpr, &row, &off);
            EXPECT(row < cnt && off + 16 <= stride && off % 16 == 0);
            EXPECT((size_t)row * stride + off == (size_t)c * 16);
            if (row >= cnt || off + 16 > stride)
                continue;
            uint64_t w[2];
            memcpy(w, src[row].get() + off, 16);
            if (off == 0 && pat[row])
                w[0] = emit_patch_word(w[0], ts[row], hoff);
            mark((size_t)c << 4, 16);
            memcpy(dst.get() + ((size_t)c << 4), w, 16);
        }
    } else {
        const uint32_t nw = emit_row_words(stride);
        EXPECT(8 * nw + emit_row_tail(stride) == stride && emit_row_tail(stride) < 8);
        for (uint32_t row = 0; row < cnt; row++) {
            uint8_t *d = dst.get() + (size_t)row * stride;
            for (uint32_t q = 0; q < nw; q++) {
                uint64_t w;
                memcpy(&w, src[row].get() + 8 * q, 8);
                if (pat[row] && q == 0)
                    w = emit_patch_word(w, ts[row], hoff);
                mark((size_t)row * stride + 8 * q, 8);
                memcpy(d + 8 * q, &w, 8);
            }
            for (uint32_t b = 8 * nw; b < stride; b++) {
                mark((size_t)row * stride + b, 1);
                d[b] = (pat[row] && nw == 0) ? emit_patch_byte(src[row][b], b, ts[row], hoff)
                                             : src[row][b];
            }
        }
    }
    for (size_t b = 0; b < bytes; b++)
        EXPECT(written[b]);
    EXPECT(bytes == 0 || memcmp(dst.get(), want.get(), bytes) == 0);
}

void check_patch()
{
    std::mt19937_64 rng(5);
    for (int it = 0; it < 2000; it++) {
        const uint64_t w = rng();
        const uint32_t ts = it < 4 ? (it & 1 ? 0xFFFFFFFFu : 0u) : (uint32_t)rng();
        for (uint32_t hoff = 0; hoff < 2; hoff++) {
            uint8_t b[8];
            memcpy(b, &w, 8);
            b[hoff] = (uint8_t)(ts >> 24);
            b[hoff + 1] = (uint8_t)(ts >> 16);
            b[hoff + 2] = (uint8_t)(ts >> 8);
            b[hoff + 3] = (uint8_t)ts;
            uint64_t want;
            memcpy(&want, b, 8);
            EXPECT(emit_patch_word(w, ts, hoff) == want);
            uint8_t o[8];
            memcpy(o, &w, 8);
            for (uint32_t i = 0; i < 8; i++)
                EXPECT(emit_patch_byte(o[i], i, ts, hoff) == b[i]);
        }
    }
}

} // namespace

int main()
{
    static_assert(EMIT_TILE == 1024 && EMIT_TILE % WAVE == 0, "tile of whole waves");
    static_assert(EMIT_SCAN_PASS % WAVE == 0, "scan pass of whole waves");
    static_assert((uint64_t)EMIT_TILE * (EMIT_MAX_STRIDE >> 4) < (1ull << 32),
                  "chunk indices of a tile fit 32 bits");
    const uint64_t T = EMIT_TILE;
    /* the shapes of tests/test_fused_emit_gpu.py and the scan-pass edges */
    const uint64_t totals[] = {1, T - 1, T, T + 1, 2 * T + 3, 4 * T + 21,
                               EMIT_SCAN_PASS * T - 1, EMIT_SCAN_PASS * T, EMIT_SCAN_PASS * T + 1,
                               (EMIT_SCAN_PASS + 3) * T + 5, 2 * EMIT_SCAN_PASS * T + 7};
    const Pattern pats[] = {P_RANDOM, P_ALL, P_NONE, P_FIRST, P_LAST, P_EMPTY_TILE};
    uint32_t seed = 1;
    for (uint64_t total : totals)
        for (Pattern p : pats) {
            std::vector<uint8_t> keep = keep_flags(total, p, seed++);
            std::vector<uint32_t> counts;
            std::vector<uint64_t> base;
            uint64_t n_out = 0;
            scan_tiles(keep, &counts, &base, &n_out);
            if (p == P_NONE)
                EXPECT(n_out == 0);
            if (p == P_FIRST || p == P_LAST)
                EXPECT(n_out == 1);
            if (p == P_EMPTY_TILE && counts.size() > 1)
                EXPECT(counts[1] == 0);
            check_rows(keep, counts, base, n_out, 18, 112);
        }
    EXPECT(emit_n_tiles(0) == 0 && emit_scan_passes(0) == 0 && emit_tile_len(0, 0) == 0);
    /* offsets beyond 32 bits */
    EXPECT(emit_row_off(0x100000000ull, 112) == 0x100000000ull * 112);
    EXPECT(emit_row_off((1ull << 40) - 1, EMIT_MAX_STRIDE) ==
           ((1ull << 40) - 1) * (uint64_t)EMIT_MAX_STRIDE);
    const uint32_t strides[] = {4, 5, 7, 8, 12, 13, 16, 18, 19, 32, 33, 112, 116, 256};
    const uint32_t cnts[] = {0, 1, 2, 255, 256, 257, 1023, 1024};
    for (uint32_t stride : strides)
        for (uint32_t cnt : cnts)
            for (uint32_t dv = 0; dv < 3; dv++)
                check_copy(cnt, stride, dv, seed++);
    check_copy(3, EMIT_MAX_STRIDE, 2, seed++);
    check_patch();
    if (g_fail) {
        fprintf(stderr, "emit_tile_check: %d expectation(s) failed\n", g_fail);
        return 1;
    }
    printf("emit_tile_check OK\n");
    return 0;
}

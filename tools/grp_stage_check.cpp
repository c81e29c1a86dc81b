/* grp_stage_check.cpp — stand-alone CPU check of the index arithmetic behind
 * the batched memory loads of the group rank and the fused emit
 * (incubator_pegasus_amd/csrc/grp_stage.h and the copy schedule of
 * emit_tile.h).  The device kernels compile the same headers, so what holds
 * here holds there.  Each schedule is replayed thread by thread on the host,
 * the way the kernel walks it, and compared with a brute-force loop:
 *   - flat staging: for every group size in [0, 2048] and R in {2, 3, 8, 31,
 *     32}, with segment splits that leave segments empty (among them: all but
 *     two runs empty, one run holding everything), every staged position is
 *     written exactly once, with the (run, offset) a per-segment loop gives
 *     it; a slot past the group is clamped to a position inside it and is not
 *     written; no load index leaves its segment;
 *   - the chunk copy: for every span length up to two full batches + 1, every
 *     chunk is taken exactly once, by a full batch or by the remainder, and
 *     none at or beyond the span's end;
 *   - the row copy: for every stride up to 64 the words and the 4/2/1-byte
 *     tail pieces cover the row's bytes exactly once.
 * Meant to run under the address and undefined-behaviour sanitizers:
 *
 *   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *       tools/grp_stage_check.cpp -o bin/grp_stage_check && bin/grp_stage_check
 *
 * (-DEMIT_COPY_DEPTH=2 or 8 checks the other copy depths.)  No HIP, no GPU,
 * nothing loaded into another process.  Exit status 0 and a final
 * "grp_stage_check OK" line mean every expectation held. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../incubator_pegasus_amd/csrc/emit_tile.h"
#include "../incubator_pegasus_amd/csrc/grp_stage.h"

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

constexpr uint32_t GRP_CAP = GRP_STAGE_THREADS * GRP_STAGE_SLOTS;

enum Split { S_RANDOM, S_SPARSE, S_ONE_RUN, S_FIRST_LAST, S_EVEN };

/* segment lengths of R runs summing to gsize */
std::vector<uint64_t> split(uint64_t gsize, uint32_t R, Split how, std::mt19937 &rng)
{
    std::vector<uint64_t> len(R, 0);
    switch (how) {
    case S_RANDOM: /* random cuts: short and empty segments among long ones */
        for (uint64_t i = 0; i < gsize; i++)
            len[rng() % R]++;
        for (uint32_t q = 0; q < R; q++)
            if (rng() % 3 == 0) { /* empty it into a neighbour */
                len[(q + 1) % R] += len[q];
                len[q] = 0;
            }
        break;
    case S_SPARSE: { /* all but two runs hold nothing */
        const uint32_t a = rng() % R, b = (a + 1 + rng() % (R - 1)) % R;
        len[a] = gsize / 3;
        len[b] = gsize - len[a];
        break;
    }
    case S_ONE_RUN:
        len[rng() % R] = gsize;
        break;
    case S_FIRST_LAST:
        len[0] = gsize / 2;
        len[R - 1] = gsize - len[0];
        break;
    case S_EVEN:
        for (uint32_t q = 0; q < R; q++)
            len[q] = gsize / R + (q < gsize % R);
        break;
    }
    return len;
}

/* k_rank_grp's staging of one group, thread by thread */
void check_stage(uint64_t gsize, uint32_t R, Split how, std::mt19937 &rng)
{
    const std::vector<uint64_t> len = split(gsize, R, how, rng);
    std::vector<uint64_t> segoff(R + 1, 0);
    for (uint32_t q = 0; q < R; q++)
        segoff[q + 1] = segoff[q] + len[q];
    EXPECT(segoff[R] == gsize);
    /* brute force: position -> (run, offset) */
    std::vector<uint32_t> want_q(gsize), want_j(gsize);
    for (uint32_t q = 0; q < R; q++)
        for (uint64_t j = 0; j < len[q]; j++) {
            want_q[segoff[q] + j] = q;
            want_j[segoff[q] + j] = (uint32_t)j;
        }
    const uint32_t nk = grp_stage_slots(gsize);
    EXPECT(nk <= GRP_STAGE_SLOTS);
    EXPECT((uint64_t)nk * GRP_STAGE_THREADS >= gsize);
    EXPECT(nk == 0 || (uint64_t)(nk - 1) * GRP_STAGE_THREADS < gsize);
    std::vector<uint8_t> written(gsize, 0);
    if (gsize == 0)
        return; /* the kernel stages nothing */
    for (uint32_t tid = 0; tid < GRP_STAGE_THREADS; tid++) {
        uint32_t sq = 0;
        for (uint32_t k = 0; k < nk; k++) {
            const uint32_t e = grp_stage_pos(tid, k);
            const uint32_t ec = e < gsize ? e : (uint32_t)gsize - 1;
            sq = grp_stage_seg(segoff.data(), R, ec, sq);
            EXPECT(sq < R);
            if (sq >= R)
                return;
            EXPECT(segoff[sq] <= ec && ec < segoff[sq + 1]);
            const uint32_t j = ec - (uint32_t)segoff[sq];
            EXPECT(j < len[sq]); /* the load stays inside the run's segment */
            EXPECT(sq == want_q[ec] && j == want_j[ec]);
            if (e < gsize) {
                EXPECT(!written[e]);
                written[e] = 1;
            }
        }
    }
    for (uint64_t e = 0; e < gsize; e++)
        EXPECT(written[e]);
}

/* emit_copy_span's chunk schedule over a span of n_chunks */
void check_chunks(uint32_t n_chunks)
{
    std::vector<uint8_t> taken(n_chunks, 0);
    auto take = [&](uint32_t c) {
        EXPECT(c < n_chunks);
        if (c < n_chunks) {
            EXPECT(!taken[c]);
            taken[c] = 1;
        }
    };
    const uint32_t nb = emit_copy_full_batches(n_chunks);
    EXPECT(nb * EMIT_COPY_BATCH <= n_chunks && n_chunks - nb * EMIT_COPY_BATCH < EMIT_COPY_BATCH);
    EXPECT(emit_copy_rem_start(n_chunks) == nb * EMIT_COPY_BATCH);
    for (uint32_t tid = 0; tid < EMIT_THREADS; tid++) {
        for (uint32_t b = 0; b < nb; b++)
            for (uint32_t d = 0; d < EMIT_COPY_DEPTH; d++)
                take(emit_copy_chunk(b, d, tid));
        for (uint32_t c = emit_copy_rem_start(n_chunks) + tid; c < n_chunks; c += EMIT_THREADS)
            take(c);
    }
    for (uint32_t c = 0; c < n_chunks; c++)
        EXPECT(taken[c]);
}

/* the row copy's pieces over one row of `stride` bytes */
void check_row_pieces(uint32_t stride)
{
    std::vector<uint8_t> seen(stride, 0);
    auto mark = [&](uint32_t at, uint32_t n) {
        for (uint32_t b = at; b < at + n; b++) {
            EXPECT(b < stride && !seen[b]);
            if (b < stride)
                seen[b] = 1;
        }
    };
    const uint32_t nw = emit_row_words(stride), tail = emit_row_tail(stride);
    for (uint32_t q0 = 0; q0 < nw; q0 += EMIT_ROW_WORD_BATCH)
        for (uint32_t u = 0; u < EMIT_ROW_WORD_BATCH; u++)
            if (q0 + u < nw)
                mark(8 * (q0 + u), 8);
    for (uint32_t size : {4u, 2u, 1u})
        if (tail & size)
            mark(emit_row_tail_off(stride, size), size);
    for (uint32_t b = 0; b < stride; b++)
        EXPECT(seen[b]);
}

} // namespace

int main()
{
    static_assert(GRP_CAP == 2048, "the group cap the kernel stages");
    static_assert(EMIT_COPY_DEPTH >= 1 && EMIT_COPY_BATCH == EMIT_COPY_DEPTH * EMIT_THREADS,
                  "batch geometry");
    std::mt19937 rng(7);
    const uint32_t Rs[] = {2, 3, 8, 31, 32};
    const Split splits[] = {S_RANDOM, S_SPARSE, S_ONE_RUN, S_FIRST_LAST, S_EVEN};
    for (uint32_t R : Rs)
        for (uint64_t gsize = 0; gsize <= GRP_CAP; gsize++)
            for (Split how : splits)
                check_stage(gsize, R, how, rng);
    /* order word fields */
    EXPECT(emit_order_run(((uint64_t)63 << 40) | 0xFFFFFFFFFFull) == 63);
    EXPECT(emit_order_row(((uint64_t)63 << 40) | 0xFFFFFFFFFFull) == 0xFFFFFFFFFFull);
    EXPECT(emit_order_run(5) == 0 && emit_order_row(5) == 5);
    for (uint32_t n = 0; n <= 2 * EMIT_COPY_BATCH + 1; n++)
        check_chunks(n);
    check_chunks(7 * EMIT_COPY_BATCH + EMIT_THREADS + 3);
    for (uint32_t stride = 1; stride <= 64; stride++)
        check_row_pieces(stride);
    if (g_fail) {
        fprintf(stderr, "grp_stage_check: %d expectation(s) failed\n", g_fail);
        return 1;
    }
    printf("grp_stage_check OK\n");
    return 0;
}

/* emit_tile.h — indexing arithmetic of the fused fixed-stride compaction emit
 * (k_keep_tile_counts, k_keep_tile_scan, k_emit_fixed_fused in kernels.hip).
 * No HIP call and no engine type in here.  EMIT_HD makes every function host
 * code and device code: the kernels compile this header, and
 * tools/emit_tile_check.cpp runs the same functions on the CPU against
 * brute-force loops, under the address and undefined-behaviour sanitizers.
 *
 * The merged rank range [0, total) is cut into tiles of EMIT_TILE consecutive
 * ranks.  One workgroup of EMIT_THREADS threads owns a tile: its kept ranks
 * become the output rows [tile_base, tile_base + cnt), so with fixed strides
 * the tile's keys and values are two contiguous output spans, cnt * stride
 * bytes from byte tile_base * stride.  tile_base comes from an exclusive scan
 * of the per-tile keep counts that one workgroup runs in passes of
 * EMIT_SCAN_PASS counts, carrying the running total from pass to pass.
 */
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EMIT_HD __host__ __device__
#else
#define EMIT_HD
#endif

#define EMIT_THREADS 256u
#define EMIT_RANKS_PER_THREAD 4u
#define EMIT_TILE (EMIT_THREADS * EMIT_RANKS_PER_THREAD) /* 1024 ranks */
#define EMIT_SCAN_PASS 256u /* tile counts per scan pass: one per thread */
/* in-tile row and chunk indices are 32 bit (byte offsets are formed in 64):
 * EMIT_TILE * stride / 16 stays far below 2^32.  Wider rows take the
 * per-row-size emit. */
#define EMIT_MAX_STRIDE (1u << 22)

EMIT_HD static inline uint64_t emit_n_tiles(uint64_t total)
{
    return (total + EMIT_TILE - 1) / EMIT_TILE;
}

/* ranks of tile t that exist: EMIT_TILE but for the last tile */
EMIT_HD static inline uint32_t emit_tile_len(uint64_t total, uint64_t t)
{
    const uint64_t p0 = t * EMIT_TILE;
    if (p0 >= total)
        return 0;
    const uint64_t left = total - p0;
    return left < EMIT_TILE ? (uint32_t)left : EMIT_TILE;
}

/* in-tile rank of a thread's j-th element: consecutive threads read
 * consecutive ranks (coalesced), j strides by the workgroup */
EMIT_HD static inline uint32_t emit_tile_slot(uint32_t tid, uint32_t j)
{
    return j * EMIT_THREADS + tid;
}

/* scan passes over n_tiles counts, and the tiles pass `ps` covers */
EMIT_HD static inline uint64_t emit_scan_passes(uint64_t n_tiles)
{
    return (n_tiles + EMIT_SCAN_PASS - 1) / EMIT_SCAN_PASS;
}
EMIT_HD static inline uint64_t emit_scan_tile(uint64_t ps, uint32_t tid)
{
    return ps * EMIT_SCAN_PASS + tid;
}
/* exclusive base of a tile: the total carried in from earlier passes, the
 * counts of the pass's earlier waves, and the in-wave exclusive prefix */
EMIT_HD static inline uint64_t emit_scan_base(uint64_t carry, uint32_t wave_base,
                                              uint32_t lane_excl)
{
    return carry + wave_base + lane_excl;
}
EMIT_HD static inline uint64_t emit_scan_carry(uint64_t carry, uint32_t pass_total)
{
    return carry + pass_total;
}

/* byte offset of output row o; o == n_out gives the terminal entry */
EMIT_HD static inline uint64_t emit_row_off(uint64_t o, uint32_t stride)
{
    return o * (uint64_t)stride;
}

/* strides that are multiples of 16 move as 16-byte chunks */
EMIT_HD static inline bool emit_stride_chunked(uint32_t stride) { return (stride & 15u) == 0; }
EMIT_HD static inline uint32_t emit_chunks_per_row(uint32_t stride) { return stride >> 4; }
EMIT_HD static inline uint32_t emit_span_chunks(uint32_t cnt, uint32_t stride)
{
    return cnt * emit_chunks_per_row(stride);
}
/* chunk c of a tile's span -> local row and byte offset inside the row */
EMIT_HD static inline void emit_chunk_row(uint32_t c, uint32_t cpr, uint32_t *row, uint32_t *off)
{
    const uint32_t r = c / cpr;
    *row = r;
    *off = (c - r * cpr) << 4;
}

/* The chunk copy runs in batches: in a full batch every thread loads
 * EMIT_COPY_DEPTH chunks, one workgroup width apart, before it stores the
 * first, so that many 16-byte loads per lane are in flight.  The chunks past
 * the last full batch are the remainder: one chunk per thread per step. */
#ifndef EMIT_COPY_DEPTH
#define EMIT_COPY_DEPTH 4u
#endif
#define EMIT_COPY_BATCH (EMIT_COPY_DEPTH * EMIT_THREADS) /* chunks per full batch */
EMIT_HD static inline uint32_t emit_copy_full_batches(uint32_t n_chunks)
{
    return n_chunks / EMIT_COPY_BATCH;
}
/* chunk of thread tid's d-th load (d < EMIT_COPY_DEPTH) in full batch b */
EMIT_HD static inline uint32_t emit_copy_chunk(uint32_t b, uint32_t d, uint32_t tid)
{
    return b * EMIT_COPY_BATCH + d * EMIT_THREADS + tid;
}
/* first chunk of the remainder; thread tid takes emit_copy_rem_start + tid,
 * then steps by EMIT_THREADS while below n_chunks */
EMIT_HD static inline uint32_t emit_copy_rem_start(uint32_t n_chunks)
{
    return emit_copy_full_batches(n_chunks) * EMIT_COPY_BATCH;
}

/* other strides move one row per thread: u64 pieces, then the tail (< 8
 * bytes) as at most one 4-, one 2- and one 1-byte piece, in that order */
EMIT_HD static inline uint32_t emit_row_words(uint32_t stride) { return stride >> 3; }
EMIT_HD static inline uint32_t emit_row_tail(uint32_t stride) { return stride & 7u; }
/* the row's words are loaded EMIT_ROW_WORD_BATCH at a time before they are
 * stored; the tail pieces travel with the first batch */
#define EMIT_ROW_WORD_BATCH 4u
/* byte offset of the tail piece of `size` (4, 2 or 1) bytes; valid when
 * emit_row_tail(stride) & size */
EMIT_HD static inline uint32_t emit_row_tail_off(uint32_t stride, uint32_t size)
{
    const uint32_t tail = emit_row_tail(stride);
    return 8 * emit_row_words(stride) + (tail & ~(2 * size - 1));
}

/* the emit kernel keeps every run's keys / vals / voff / sk pointers in LDS:
 * one entry per run a handle can hold (RRDB_MAX_RUNS) */
#define EMIT_RUN_TAB 64u
/* order word -> run and row */
EMIT_HD static inline uint32_t emit_order_run(uint64_t id) { return (uint32_t)(id >> 40); }
EMIT_HD static inline uint64_t emit_order_row(uint64_t id) { return id & 0xFFFFFFFFFFull; }

/* rewritten expire timestamp: 4 bytes big-endian at byte hoff of the value
 * (1 for data version 2, whose values start with a format byte; else 0) */
EMIT_HD static inline uint32_t emit_expire_off(uint32_t data_version)
{
    return data_version == 2 ? 1u : 0u;
}
/* the row's first 8 bytes as a little-endian word, header replaced */
EMIT_HD static inline uint64_t emit_patch_word(uint64_t w, uint32_t ts, uint32_t hoff)
{
    const uint64_t be = ((uint64_t)(ts >> 24) & 0xFFu) | (((uint64_t)(ts >> 16) & 0xFFu) << 8) |
                        (((uint64_t)(ts >> 8) & 0xFFu) << 16) | (((uint64_t)ts & 0xFFu) << 24);
    const uint64_t mask = 0xFFFFFFFFull << (8 * hoff);
    return (w & ~mask) | (be << (8 * hoff));
}
/* byte b of a row shorter than one word: the patched value of that byte */
EMIT_HD static inline uint8_t emit_patch_byte(uint8_t v, uint32_t b, uint32_t ts, uint32_t hoff)
{
    if (b < hoff || b >= hoff + 4)
        return v;
    return (uint8_t)(ts >> (8 * (3 - (b - hoff))));
}

/* launch.h — the host entry points of kernels.hip, declared once.  engine.cpp
 * calls them and kernels.hip defines them; both include this file, and the
 * library links with -z defs, so a declaration and its definition cannot
 * drift apart without failing the build. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine_common.h"

/* ---- runs: tails, meta, bloom ---- */
void launch_crc64_table_init(const uint64_t *host_table);
void launch_build_tails(const uint8_t *keys, uint64_t fk, uint64_t n, uint64_t *tails,
                        hipStream_t s);
void launch_build_meta(const uint8_t *vals, const uint64_t *voff, uint64_t fixed_vlen,
                       const uint64_t *sk, uint64_t n, uint32_t dv, uint64_t *meta,
                       hipStream_t s);
void launch_bloom_build(const DevRun &run, uint64_t *d_bloom, uint64_t n_blocks, hipStream_t s);
void launch_bloom_pfx_build(const DevRun &run, uint64_t *d_bloom, uint64_t n_blocks,
                            hipStream_t s);

/* ---- bounds, rank, view ---- */
void launch_bounds(const DevRun *d_runs, int R, const uint8_t *d_key, uint64_t klen,
                   uint64_t *d_out, int upper, hipStream_t s);
void launch_rank(const DevRun *d_runs, int R, const uint64_t *d_lo, const uint64_t *d_hi,
                 const uint64_t *d_wprefix, uint64_t total, uint64_t *d_order,
                 uint8_t *d_shadowed, const uint64_t *d_bt_off, const uint64_t *d_bt,
                 int bt_shift, hipStream_t s);
void launch_rank_ldst(const DevRun *d_runs, int R, const uint64_t *d_lo, const uint64_t *d_hi,
                      const uint64_t *d_wprefix, uint64_t total, uint64_t *d_order,
                      uint8_t *d_shadow, const uint64_t *d_bt_off, const uint64_t *d_bt,
                      int bt_shift, hipStream_t s);
void launch_bound_table(const DevRun *d_runs, int R, const uint64_t *d_lo, const uint64_t *d_hi,
                        const uint64_t *d_bt_off, uint64_t total_rows, int bt_shift,
                        uint64_t *d_bt, const uint64_t *d_cbt_off, const uint64_t *d_cbt,
                        int cbt_shift, hipStream_t s);
void launch_anchor_rows(const DevRun *runs, int R, int q0, const uint64_t *d_lo,
                        const uint64_t *d_hi, int gs, uint64_t n_groups, uint64_t *d_anch,
                        hipStream_t s);
void launch_rank_grp_view(const DevRun *d_runs, int R, const uint64_t *d_lo,
                          const uint64_t *d_anch, uint64_t n_groups, uint64_t *d_order,
                          uint8_t *d_shadow, hipStream_t s);
void launch_visible(const DevRun *d_runs, const uint64_t *d_order, const uint8_t *d_shadowed,
                    uint64_t m, uint64_t *d_flags, hipStream_t s);
void launch_gather(const uint64_t *d_order, const uint64_t *d_flags, const uint64_t *d_pos,
                   uint64_t m, uint64_t *d_out, hipStream_t s);
void launch_valid_beyond(const DevRun *runs, int R, const uint8_t *bound, uint64_t blen,
                         int reverse, uint32_t *out, hipStream_t s);
void launch_first_eq(const DevRun *d_runs, const uint64_t *d_view, uint64_t n,
                     const uint8_t *d_key, uint64_t klen, uint32_t *d_out, hipStream_t s);

/* exclusive scan; caller provides scratch of psum_scratch_elems(n) u64s
 * (engine-owned arena — no per-call allocation) */
uint64_t psum_scratch_elems(uint64_t n);
void launch_psum(const uint64_t *d_in, uint64_t *d_out, uint64_t n, uint64_t *d_scratch,
                 hipStream_t s);

/* ---- get, scan, multi_get ---- */
void launch_get(const DevRun *d_runs, int R, const uint8_t *d_qkeys, const uint64_t *d_qoffs,
                uint64_t nq, uint32_t epoch_now, uint32_t dv, int32_t *d_status, uint64_t *d_hit,
                uint64_t *d_ulen, uint32_t *d_expire, hipStream_t s);
void launch_emit_values(const DevRun *d_runs, const uint64_t *d_hit, const int32_t *d_status,
                        uint64_t nq, uint32_t dv, const uint64_t *d_voffs, uint8_t *d_vout,
                        hipStream_t s);
void launch_scan_state(const DevRun *d_runs, const uint64_t *d_view, uint64_t w,
                       const ScanParams &sp, uint8_t *d_state, uint64_t *d_ksz, uint64_t *d_vsz,
                       hipStream_t s);
void launch_normal_flags(const uint8_t *d_state, uint64_t w, uint64_t *d_flags, hipStream_t s);
void launch_cutoff(const uint64_t *d_nprefix, const uint64_t *d_flags, uint64_t w,
                   uint64_t batch_count, uint64_t *d_out2, hipStream_t s);
void launch_cut_sizes(const uint8_t *d_state, uint64_t w, uint64_t consumed, uint64_t *d_ksz,
                      uint64_t *d_vsz, hipStream_t s);
void launch_emit_scan(const DevRun *d_runs, const uint64_t *d_view, uint64_t w,
                      const uint8_t *d_state, uint64_t consumed, const uint64_t *d_npos,
                      const uint64_t *d_koffs, const uint64_t *d_voffs, const ScanParams &sp,
                      uint8_t *d_kout, uint8_t *d_vout, uint64_t *d_kout_offs,
                      uint64_t *d_vout_offs, int32_t *d_ets, uint64_t n_out, hipStream_t s);
void launch_emit_rows(const DevRun *d_runs, const uint64_t *d_view, const uint64_t *d_rows,
                      uint64_t n_rows, const uint64_t *d_koffs, const uint64_t *d_voffs,
                      const ScanParams &sp, uint8_t *d_kout, uint8_t *d_vout, hipStream_t s);
void launch_multi_get_small(const DevRun *d_runs, int R, const MgFusedArgs &a, hipStream_t s);
void launch_multi_get_graph(const DevRun *runs, int R, const uint8_t *d_in, uint8_t *d_out,
                            hipStream_t s);
void launch_mg_server(const DevRun *runs, int R, MgMailbox *mb, uint8_t *d_out, hipStream_t s);
void launch_multi_get_batch(const DevRun *d_runs, int R, const MgFusedArgs &a,
                            const uint8_t *d_hks, const uint64_t *d_hk_offs, uint64_t n_req,
                            int64_t *d_hdrs, uint8_t *d_blobs, uint64_t blob_stride,
                            hipStream_t s);
void launch_pack_blobs(const uint8_t *d_blobs, uint64_t blob_stride, uint64_t n_req,
                       const uint64_t *d_used, const uint64_t *d_pack_off, uint8_t *d_packed,
                       hipStream_t s);

/* ---- compaction: rank + filter, count, emit ---- */
void launch_rank_compact(const DevRun *d_runs, int R, const uint64_t *d_lo, const uint64_t *d_hi,
                         const uint64_t *d_wprefix, uint64_t total, const CompactParams &cp,
                         uint64_t *d_order, uint64_t *d_keepw, uint8_t *d_changed,
                         uint32_t *d_new_expire, uint64_t *d_ksz, uint64_t *d_vsz,
                         uint64_t *d_rank_of, const uint64_t *d_bt_off, const uint64_t *d_bt,
                         int bt_shift, CompactStatsDev *d_stats, hipStream_t s);
void launch_rank_compact_ldst(const DevRun *d_runs, int R, const uint64_t *d_lo,
                              const uint64_t *d_hi, const uint64_t *d_wprefix, uint64_t total,
                              const CompactParams &cp, uint64_t *d_order, uint64_t *d_keepw,
                              uint8_t *d_changed, uint32_t *d_new_expire, uint64_t *d_ksz,
                              uint64_t *d_vsz, uint64_t *d_rank_of, const uint64_t *d_bt_off,
                              const uint64_t *d_bt, int bt_shift, CompactStatsDev *d_stats,
                              hipStream_t s);
void launch_rank_compact_lds(const DevRun *d_runs, int R, const uint64_t *d_lo,
                             const uint64_t *d_hi, const uint64_t *d_blk_prefix,
                             uint64_t n_blocks, const CompactParams &cp,
                             const uint64_t *d_bt8_off, const uint64_t *d_bt8,
                             uint64_t *d_order, uint64_t *d_keepw, uint8_t *d_changed,
                             uint32_t *d_new_expire, uint64_t *d_ksz, uint64_t *d_vsz,
                             CompactStatsDev *d_stats, hipStream_t s);
void launch_rank_grp_compact(const DevRun *d_runs, int R, const uint64_t *d_lo,
                             const uint64_t *d_anch, uint64_t n_groups, const CompactParams &cp,
                             uint64_t *d_order, uint64_t *d_keepw, uint8_t *d_changed,
                             uint32_t *d_new_expire, uint64_t *d_ksz, uint64_t *d_vsz,
                             CompactStatsDev *d_stats, int block_cap, hipStream_t s);
/* fused count scan: shadow + countability evaluated in-kernel, the count
 * lands in stats->output_records (banked); zero intermediate arrays */
void launch_rank_grp_count(const DevRun *d_runs, int R, const uint64_t *d_lo,
                           const uint64_t *d_anch, uint64_t n_groups, const ScanParams &sp,
                           CompactStatsDev *d_stats, hipStream_t s);
void launch_count_single(const DevRun *d_runs, const uint64_t *d_lo, const uint64_t *d_hi,
                         const ScanParams &sp, CompactStatsDev *d_stats, uint64_t n_max,
                         hipStream_t s);
void launch_emit_compact(const DevRun *d_runs, const uint64_t *d_order, uint64_t m,
                         const uint64_t *d_keepw, const uint8_t *d_changed,
                         const uint32_t *d_new_expire, const uint64_t *d_kpos,
                         const uint64_t *d_koffs, const uint64_t *d_voffs, uint32_t dv,
                         uint8_t *d_kout, uint8_t *d_vout, uint64_t *d_okoff, uint64_t *d_ovoff,
                         uint64_t *d_osk, uint64_t n_out, hipStream_t s);
void launch_emit_compact_inmajor(const DevRun *d_runs, int R, const uint64_t *d_wprefix,
                                 uint64_t total, const uint64_t *d_rank_of,
                                 const uint64_t *d_keepw, const uint8_t *d_changed,
                                 const uint32_t *d_new_expire, const uint64_t *d_kpos,
                                 const uint64_t *d_koffs, const uint64_t *d_voffs, uint32_t dv,
                                 uint8_t *d_kout, uint8_t *d_vout, uint64_t *d_okoff,
                                 uint64_t *d_ovoff, uint64_t *d_osk, uint64_t n_out,
                                 hipStream_t s);
void launch_emit_compact_chunked(const DevRun *d_runs, const uint64_t *d_order, uint64_t m,
                                 const uint64_t *d_keepw, const uint8_t *d_changed,
                                 const uint32_t *d_new_expire, const uint64_t *d_kpos,
                                 const uint64_t *d_koffs, const uint64_t *d_voffs, uint32_t dv,
                                 uint64_t n_out, uint64_t kbytes, uint64_t vbytes,
                                 uint64_t *d_row_ksrc, uint64_t *d_row_vsrc,
                                 uint32_t *d_row_patch, uint32_t *d_row_expire, uint8_t *d_kout,
                                 uint8_t *d_vout, uint64_t *d_okoff /* also the key row offsets */,
                                 uint64_t *d_ovoff /* also the value row offsets */,
                                 uint64_t *d_osk, uint64_t *d_kanchor, uint64_t *d_vanchor,
                                 hipStream_t s);
/* all-fixed-stride route, first half (compact_begin): per-tile keep counts
 * and their exclusive scan; *d_total receives the output row count */
void launch_keep_tile_scan(const uint64_t *d_keepw, uint64_t m, uint32_t *d_tile_cnt,
                           uint64_t *d_tile_base, uint64_t *d_total, hipStream_t s);
/* second half (compact_finish, n_out > 0): the fused scan + row build + copy.
 * d_changed / d_new_expire are null when the pass can rewrite nothing */
void launch_emit_fixed_fused(const DevRun *d_runs, int R, const uint64_t *d_order, uint64_t m,
                             const uint64_t *d_keepw, const uint64_t *d_tile_base,
                             const uint8_t *d_changed, const uint32_t *d_new_expire, uint32_t dv,
                             uint32_t fk, uint32_t fv, uint64_t n_out, uint8_t *d_kout,
                             uint8_t *d_vout, uint64_t *d_okoff, uint64_t *d_ovoff,
                             uint64_t *d_osk, hipStream_t s);

/* ---- split ---- */
void launch_split_classify(const uint8_t *keys, const uint64_t *koff, uint64_t fk,
                           const uint64_t *sk, uint64_t n, uint64_t mask, uint64_t ppidx,
                           uint64_t cpidx, uint8_t *d_side, uint64_t *d_wcnt, uint32_t *d_has_put,
                           int lds_table, hipStream_t s);
void launch_split_sizes(const uint8_t *d_side, uint32_t side, const uint64_t *koff,
                        const uint64_t *voff, uint64_t n, uint64_t *d_ksz, uint64_t *d_vsz,
                        hipStream_t s);
void launch_split_scatter(const uint8_t *keys, const uint64_t *koff, const uint8_t *vals,
                          const uint64_t *voff, const uint64_t *sk, uint64_t n, uint64_t fk,
                          uint64_t fv, const uint8_t *d_side, uint32_t side,
                          const uint64_t *d_wbase, uint64_t bias, const uint64_t *d_kpos,
                          const uint64_t *d_vpos, uint64_t n_side, uint64_t kbytes,
                          uint64_t vbytes, uint64_t *d_okoff, uint64_t *d_ovoff, uint64_t *d_osk,
                          uint64_t *d_row_ksrc, uint64_t *d_row_vsrc, hipStream_t s);
/* move one column's bytes (keys or values) of a split side: rows gathered
 * from d_row_src into the packed d_out.  stride != 0: every row has that
 * length; else d_row_off[n_rows+1] holds the 0-based output offsets and
 * d_anchor (((bytes+15)>>10)+1 words) is scratch for the chunk->row search */
void launch_split_copy(const uint64_t *d_row_src, const uint64_t *d_row_off, uint64_t n_rows,
                       uint64_t stride, uint64_t bytes, uint64_t *d_anchor, uint8_t *d_out,
                       hipStream_t s);

/* ---- batched writes.  Every d_red is that path's reduction block (WBR_*,
 * IR_*, TR_*, CR_* words), initialised by the path's first launcher. ---- */
/* sort the batch's (word, index) pairs; d_lcp is 4 bytes of scratch that
 * k.lcp points at.  Returns 0 / 1: the result is in (w0, i0) / (w1, i1). */
int launch_wb_sort(const WbKeys &k, uint64_t n, uint32_t *d_lcp, uint64_t *d_w0, uint32_t *d_i0,
                   uint64_t *d_w1, uint32_t *d_i1, hipStream_t s);
void launch_wb_flags(const WbKeys &k, const uint64_t *d_svoff, uint64_t fv,
                     const uint8_t *d_kinds, uint64_t n, const uint64_t *d_w,
                     const uint32_t *d_ix, uint64_t *d_keep, uint64_t *d_ksz, uint64_t *d_vsz,
                     uint64_t *d_red, hipStream_t s);
void launch_wb_scatter(const WbKeys &k, const uint8_t *d_svals, const uint64_t *d_svoff,
                       uint64_t fv, const uint8_t *d_kinds, uint64_t n, const uint32_t *d_ix,
                       const uint64_t *d_keep, const uint64_t *d_rank, const uint64_t *d_kpos,
                       const uint64_t *d_vpos, uint64_t seq_floor, uint64_t n_out,
                       uint64_t kbytes, uint64_t vbytes, uint64_t *d_okoff, uint64_t *d_ovoff,
                       uint64_t *d_osk, uint64_t *d_row_ksrc, uint64_t *d_row_vsrc, hipStream_t s);
/* head flags of the sorted keys (incr and timetag batch) and, after the
 * caller's launch_psum of them into d_hrank, the segment starts.  d_red:
 * `words` u64 words, those in min_mask start at ~0. */
void launch_key_heads(const WbKeys &k, uint64_t n, const uint64_t *d_w, const uint32_t *d_ix,
                      uint64_t *d_head, uint64_t *d_red, int words, uint32_t min_mask,
                      hipStream_t s);
void launch_incr_segs(uint64_t n, const uint64_t *d_head, const uint64_t *d_hrank,
                      uint64_t *d_seg_start, uint64_t *d_red, hipStream_t s);
/* both chain kernels; the segment count is read on the device, so the grids
 * are sized by the op count, which bounds it */
void launch_incr_chain(const IncrArgs &a, hipStream_t s);
void launch_incr_emit(const IncrArgs &a, uint64_t n_seg, const uint64_t *d_okrank,
                      const uint64_t *d_orank, const uint64_t *d_kpos, const uint64_t *d_vpos,
                      uint64_t seq_floor, uint64_t n_out, uint64_t kbytes, uint64_t vbytes,
                      uint64_t fk, uint64_t fv, uint64_t *d_okoff, uint64_t *d_ovoff,
                      uint64_t *d_osk, uint64_t *d_row_ksrc, uint8_t *d_ovals, hipStream_t s);
/* head flags and the inverse permutation */
void launch_cas_heads(const WbKeys &k, uint64_t E, const uint64_t *d_w, const uint32_t *d_ix,
                      uint8_t *d_khead, uint64_t *d_hhead, uint32_t *d_pos, uint64_t *d_red,
                      hipStream_t s);
/* after the caller's launch_psum of d_hhead into d_hrank: the words the
 * second sort orders the ops by */
void launch_cas_group_words(uint64_t n, uint64_t E, const uint64_t *d_moff, const uint32_t *d_pos,
                            const uint64_t *d_hhead, const uint64_t *d_hrank, uint8_t *d_words,
                            uint64_t *d_red, hipStream_t s);
void launch_cas_segs(uint64_t n, const uint8_t *d_words, const uint32_t *d_ops,
                     uint64_t *d_seg_start, hipStream_t s);
/* the group count is read on the device, so the grid is sized by the op
 * count, which bounds it */
void launch_cas_walk(const CasArgs &a, hipStream_t s);
void launch_cas_rows(const CasArgs &a, uint64_t *d_row, uint64_t *d_ksz, uint64_t *d_vsz,
                     hipStream_t s);
void launch_cas_emit(const CasArgs &a, const uint64_t *d_row, const uint64_t *d_orank,
                     const uint64_t *d_kpos, const uint64_t *d_vpos, const uint64_t *d_arank,
                     uint64_t seq_floor, uint64_t n_out, uint64_t kbytes, uint64_t vbytes,
                     uint64_t *d_okoff, uint64_t *d_ovoff, uint64_t *d_osk, uint64_t *d_row_ksrc,
                     uint64_t *d_row_vsrc, hipStream_t s);
/* both walk kernels; grids sized as launch_incr_chain's */
void launch_wbt_walk(const TtArgs &a, hipStream_t s);
void launch_wbt_scatter(const TtArgs &a, uint64_t n_seg, const uint64_t *d_orank,
                        const uint64_t *d_kpos, const uint64_t *d_vpos, uint64_t seq_floor,
                        uint64_t n_out, uint64_t kbytes, uint64_t vbytes, uint64_t fk, uint64_t fv,
                        uint64_t *d_okoff, uint64_t *d_ovoff, uint64_t *d_osk,
                        uint64_t *d_row_ksrc, uint64_t *d_row_vsrc, hipStream_t s);

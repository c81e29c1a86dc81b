/* grp_stage.h — indexing arithmetic of the group rank's staging (k_rank_grp in
 * kernels.hip).  No HIP call and no engine type in here.  GRP_HD makes every
 * function host code and device code: the kernel compiles this header, and
 * tools/grp_stage_check.cpp runs the same functions on the CPU against
 * brute-force loops.
 *
 * A group is the concatenation of R segments, one per run: segment q holds the
 * staged positions [segoff[q], segoff[q + 1]), segoff[R] == gsize.  Segments
 * may be empty.  The workgroup of GRP_STAGE_THREADS threads stages the group
 * flat: thread tid owns the positions e = tid + GRP_STAGE_THREADS * k for
 * k < grp_stage_slots(gsize), at most GRP_STAGE_SLOTS of them, and issues the
 * loads of all its positions before it waits for the first.
 */
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GRP_HD __host__ __device__
#else
#define GRP_HD
#endif

#define GRP_STAGE_THREADS 256u
#define GRP_STAGE_SLOTS 8u /* GRP_CAP / GRP_STAGE_THREADS */

/* slots a thread walks for a group of gsize staged positions (same for every
 * thread of the workgroup; the last one may lie past the group for some) */
GRP_HD static inline uint32_t grp_stage_slots(uint64_t gsize)
{
    return (uint32_t)((gsize + GRP_STAGE_THREADS - 1) / GRP_STAGE_THREADS);
}

/* staged position of a thread's k-th slot */
GRP_HD static inline uint32_t grp_stage_pos(uint32_t tid, uint32_t k)
{
    return k * GRP_STAGE_THREADS + tid;
}

/* segment of staged position e < segoff[R]: the q with
 * segoff[q] <= e < segoff[q + 1].  The walk starts at q0, the segment of an
 * earlier (smaller) position of the same thread or 0, so a thread's slots
 * cost R + slots steps together.  Empty segments are stepped over. */
template <typename OFF>
GRP_HD static inline uint32_t grp_stage_seg(const OFF *segoff, uint32_t R, uint64_t e,
                                            uint32_t q0)
{
    uint32_t q = q0;
    while (q + 1 < R && (uint64_t)segoff[q + 1] <= e)
        q++;
    return q;
}

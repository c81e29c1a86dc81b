/* wb_stage.h — host half of rrdb_write_batch: validation of the untrusted
 * input arrays, fixed-stride detection and value staging.  No HIP call and
 * no engine type in here: engine.cpp includes it, and tools/wb_stage_check.cpp
 * runs the same functions on the CPU under the address and undefined-behaviour
 * sanitizers.
 *
 * Staged layout.  The key blob is uploaded verbatim.  The value blob is
 * rebuilt: for every PUT the value header of the handle's data version (what
 * rrdb_put writes: [0x82 for v2][expire_ts BE][timetag 0 for v1/v2]) followed
 * by the user bytes; a remove contributes nothing, so its staged span is empty
 * whatever its val_offs span says.  rrdb_write_batch_timetag stages the same
 * layout with the op's timetag in the header (wb_stage_values_tt).
 */
#pragma once
#include <stdint.h>
#include <string.h>

#include "tt_verify.h"

#define WB_MAX_OPS 0x7FFFFFFFull /* the sort carries the op index in 32 bits */

static inline uint32_t wb_hdr_len(uint32_t ver) { return ver == 0 ? 4u : (ver == 1 ? 12u : 13u); }

/* n+1 offsets: start at 0, never decrease */
static inline bool wb_offsets_ok(const uint64_t *offs, uint64_t n)
{
    if (!offs || offs[0] != 0)
        return false;
    for (uint64_t i = 0; i < n; i++)
        if (offs[i + 1] < offs[i])
            return false;
    return true;
}

/* n full keys [u16 BE hklen][hashkey][sortkey]: the op count, the offsets and
 * every key's shape (rrdb_write_batch and rrdb_incr_batch share it).  Reads
 * keys only inside spans the offsets have already proven ordered. */
static inline bool wb_keys_ok(uint64_t n, const uint8_t *keys, const uint64_t *key_offs)
{
    if (n == 0 || n > WB_MAX_OPS || !keys || !wb_offsets_ok(key_offs, n))
        return false;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t kl = key_offs[i + 1] - key_offs[i];
        if (kl < 2)
            return false;
        const uint8_t *k = keys + key_offs[i];
        const uint64_t hl = ((uint64_t)k[0] << 8) | k[1];
        if (hl == 0xFFFFull || hl > kl - 2)
            return false;
    }
    return true;
}

/* everything rrdb_write_batch rejects that does not depend on the handle */
static inline bool wb_validate(uint64_t n, const uint8_t *keys, const uint64_t *key_offs,
                               const uint8_t *values, const uint64_t *val_offs,
                               const uint8_t *kinds)
{
    if (!kinds || !wb_keys_ok(n, keys, key_offs) || !wb_offsets_ok(val_offs, n))
        return false;
    for (uint64_t i = 0; i < n; i++) {
        if (kinds[i] > 1)
            return false;
        if (kinds[i] == 0 && val_offs[i + 1] != val_offs[i] && !values)
            return false;
    }
    return true;
}

/* the common length of all n spans, 0 when they differ, are empty or do not
 * fit 32 bits (detect_fixed_klen's rule) */
static inline uint32_t wb_fixed_stride(const uint64_t *offs, uint64_t n)
{
    if (n == 0)
        return 0;
    const uint64_t s = offs[1] - offs[0];
    if (s == 0 || s > UINT32_MAX)
        return 0;
    for (uint64_t i = 1; i < n; i++)
        if (offs[i + 1] - offs[i] != s)
            return 0;
    return (uint32_t)s;
}

/* bytes of the staged value blob; false when the sum overflows 64 bits */
static inline bool wb_staged_bytes(uint64_t n, const uint64_t *val_offs, const uint8_t *kinds,
                                   uint32_t data_version, uint64_t *out)
{
    const uint64_t hdr = wb_hdr_len(data_version);
    uint64_t tot = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (kinds[i] != 0)
            continue;
        const uint64_t add = hdr + (val_offs[i + 1] - val_offs[i]);
        if (add < hdr || tot + add < tot)
            return false;
        tot += add;
    }
    *out = tot;
    return true;
}

/* write the staged value blob (wb_staged_bytes long) and its n+1 offsets, with
 * timetags[i] big-endian in the 8 timetag bytes of every PUT header (data
 * version 1 and 2; version 0 has none).  expire_ts, timetags and verify may be
 * null (all zero).  out_flags, when not null, receives every op folded to the
 * TT_OP_* bits the conflict rule reads (tt_verify.h).  Input must have passed
 * wb_validate. */
static inline void wb_stage_values_tt(uint64_t n, const uint8_t *values, const uint64_t *val_offs,
                                      const uint32_t *expire_ts, const uint8_t *kinds,
                                      const uint64_t *timetags, const uint8_t *verify,
                                      uint32_t data_version, uint32_t default_ttl,
                                      uint32_t epoch_now, uint8_t *out_vals, uint64_t *out_voff,
                                      uint8_t *out_flags)
{
    const uint32_t hdr = wb_hdr_len(data_version);
    const uint32_t off = data_version == 2 ? 1 : 0;
    uint64_t pos = 0;
    out_voff[0] = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint32_t ts = 0;
        if (kinds[i] == 0) {
            /* write-time default_ttl, as rrdb_put */
            ts = tt_stored_expire(expire_ts ? expire_ts[i] : 0, default_ttl, epoch_now);
            uint8_t *v = out_vals + pos;
            memset(v, 0, hdr);
            if (data_version == 2)
                v[0] = 0x82;
            v[off] = (uint8_t)(ts >> 24);
            v[off + 1] = (uint8_t)(ts >> 16);
            v[off + 2] = (uint8_t)(ts >> 8);
            v[off + 3] = (uint8_t)ts;
            if (timetags && data_version >= 1)
                for (int j = 0; j < 8; j++)
                    v[off + 4 + j] = (uint8_t)(timetags[i] >> (8 * (7 - j)));
            const uint64_t vl = val_offs[i + 1] - val_offs[i];
            if (vl)
                memcpy(v + hdr, values + val_offs[i], vl);
            pos += hdr + vl;
        }
        if (out_flags)
            out_flags[i] = tt_op_flags(kinds[i], verify && verify[i] != 0, ts, epoch_now,
                                       data_version);
        out_voff[i + 1] = pos;
    }
}

/* the same with timetag 0 everywhere: what rrdb_write_batch stages */
static inline void wb_stage_values(uint64_t n, const uint8_t *values, const uint64_t *val_offs,
                                   const uint32_t *expire_ts, const uint8_t *kinds,
                                   uint32_t data_version, uint32_t default_ttl,
                                   uint32_t epoch_now, uint8_t *out_vals, uint64_t *out_voff)
{
    wb_stage_values_tt(n, values, val_offs, expire_ts, kinds, nullptr, nullptr, data_version,
                       default_ttl, epoch_now, out_vals, out_voff, nullptr);
}

/* cas_stage.h — host half of rrdb_check_and_mutate_batch: validation of the
 * untrusted input arrays and the staging of the entry columns.  No HIP call
 * and no engine type in here: engine.cpp includes it, and
 * tools/cas_check_check.cpp runs the same functions on the CPU under the
 * address and undefined-behaviour sanitizers.
 *
 * Entries.  Op i contributes its check entry followed by its mutation
 * entries, so with M mutations in all there are E = n + M entries, and op i's
 * check entry has ordinal i + mut_offs[i].  The staged columns are in ordinal
 * order: the key of every entry; for a PUT mutation the encoded value (what
 * rrdb_put writes: the header of the data version with the stored expire,
 * then the user bytes), for every other entry an empty span; and a kind byte.
 * A mutation whose kind is neither PUT nor DELETE makes its op malformed; it
 * is staged as a DELETE and never applied.
 */
#pragma once
#include "wb_stage.h"

#define CAS_ENT_PUT 0
#define CAS_ENT_DELETE 1
#define CAS_ENT_CHECK 2

#define CAS_OP_MALFORMED 1 /* op_flags bits */
#define CAS_OP_RETURN 2

/* everything rrdb_check_and_mutate_batch rejects that does not depend on the
 * handle.  The counts are bounded before any array is read, the offsets
 * before anything they index.  *m_out = M. */
static inline bool cas_validate(uint64_t n, const uint8_t *check_keys,
                                const uint64_t *check_key_offs, const int32_t *check_types,
                                const uint8_t *operands, const uint64_t *operand_offs,
                                const uint64_t *mut_offs, const uint8_t *mut_keys,
                                const uint64_t *mut_key_offs, const uint8_t *mut_values,
                                const uint64_t *mut_val_offs, const uint8_t *mut_kinds,
                                uint64_t *m_out)
{
    if (n == 0 || n > WB_MAX_OPS)
        return false;
    if (!check_types || !wb_offsets_ok(mut_offs, n))
        return false;
    const uint64_t M = mut_offs[n];
    if (M > WB_MAX_OPS - n)
        return false;
    if (!wb_keys_ok(n, check_keys, check_key_offs) || !wb_offsets_ok(operand_offs, n))
        return false;
    if (operand_offs[n] != 0 && !operands)
        return false;
    if (!wb_offsets_ok(mut_key_offs, M) || !wb_offsets_ok(mut_val_offs, M))
        return false;
    if (M != 0 && (!mut_kinds || !wb_keys_ok(M, mut_keys, mut_key_offs)))
        return false;
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t *ck = check_keys + check_key_offs[i];
        const uint64_t pfx = 2 + (((uint64_t)ck[0] << 8) | ck[1]);
        for (uint64_t j = mut_offs[i]; j < mut_offs[i + 1]; j++) {
            /* every mutation key carries its op's [hklen][hashkey] */
            if (mut_key_offs[j + 1] - mut_key_offs[j] < pfx ||
                memcmp(mut_keys + mut_key_offs[j], ck, pfx) != 0)
                return false;
            if (mut_kinds[j] == 0 && mut_val_offs[j + 1] != mut_val_offs[j] && !mut_values)
                return false;
        }
    }
    *m_out = M;
    return true;
}

/* write the entry columns: keys (check_key_offs[n] + mut_key_offs[M] bytes),
 * values (wb_staged_bytes over the mutations), their E+1 offsets, E kind
 * bytes and n flag bytes.  mut_expire_ts and return_check_value may be null.
 * Input must have passed cas_validate. */
static inline void cas_stage(uint64_t n, const uint8_t *check_keys,
                             const uint64_t *check_key_offs, const int32_t *check_types,
                             const uint64_t *mut_offs, const uint8_t *mut_keys,
                             const uint64_t *mut_key_offs, const uint8_t *mut_values,
                             const uint64_t *mut_val_offs, const uint32_t *mut_expire_ts,
                             const uint8_t *mut_kinds, const uint8_t *return_check_value,
                             uint32_t data_version, uint32_t default_ttl, uint32_t epoch_now,
                             uint8_t *ent_keys, uint64_t *ent_koff, uint8_t *ent_vals,
                             uint64_t *ent_voff, uint8_t *ent_kind, uint8_t *op_flags)
{
    const uint32_t hdr = wb_hdr_len(data_version);
    const uint32_t off = data_version == 2 ? 1 : 0;
    uint64_t e = 0, kpos = 0, vpos = 0;
    ent_koff[0] = 0;
    ent_voff[0] = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t ckl = check_key_offs[i + 1] - check_key_offs[i];
        memcpy(ent_keys + kpos, check_keys + check_key_offs[i], ckl);
        kpos += ckl;
        ent_kind[e] = CAS_ENT_CHECK;
        ent_koff[e + 1] = kpos;
        ent_voff[e + 1] = vpos;
        e++;
        bool bad = mut_offs[i + 1] == mut_offs[i] || check_types[i] < 0 || check_types[i] > 17;
        for (uint64_t j = mut_offs[i]; j < mut_offs[i + 1]; j++, e++) {
            const uint64_t kl = mut_key_offs[j + 1] - mut_key_offs[j];
            memcpy(ent_keys + kpos, mut_keys + mut_key_offs[j], kl);
            kpos += kl;
            if (mut_kinds[j] > 1)
                bad = true;
            ent_kind[e] = mut_kinds[j] == 0 ? CAS_ENT_PUT : CAS_ENT_DELETE;
            if (mut_kinds[j] == 0) {
                uint32_t ts = mut_expire_ts ? mut_expire_ts[j] : 0;
                /* write-time default_ttl, as rrdb_put */
                if (ts == 0 && default_ttl != 0)
                    ts = epoch_now + default_ttl;
                uint8_t *v = ent_vals + vpos;
                memset(v, 0, hdr);
                if (data_version == 2)
                    v[0] = 0x82;
                v[off] = (uint8_t)(ts >> 24);
                v[off + 1] = (uint8_t)(ts >> 16);
                v[off + 2] = (uint8_t)(ts >> 8);
                v[off + 3] = (uint8_t)ts;
                const uint64_t vl = mut_val_offs[j + 1] - mut_val_offs[j];
                if (vl)
                    memcpy(v + hdr, mut_values + mut_val_offs[j], vl);
                vpos += hdr + vl;
            }
            ent_koff[e + 1] = kpos;
            ent_voff[e + 1] = vpos;
        }
        op_flags[i] = (uint8_t)((bad ? CAS_OP_MALFORMED : 0) |
                                (return_check_value && return_check_value[i] ? CAS_OP_RETURN : 0));
    }
}

/* cas_check.h — the check half of rrdb_check_and_mutate_batch: the
 * reference's validate_check (pegasus_write_service_impl.h:1144-1270) over
 * byte spans.  No HIP call and no engine type in here.  INCR_HD makes the
 * function host code and device code at once: kernels.hip calls it from the
 * walk kernel, and tools/cas_check_check.cpp runs the very same function on
 * the CPU against a std::string restatement under the address and
 * undefined-behaviour sanitizers.
 *
 * check_type is numbered as cas_check_type in idl/rrdb.thrift:
 *   0 no check; 1 not exist; 2 not exist or empty; 3 exist; 4 not empty;
 *   5 / 6 / 7 match anywhere / prefix / postfix: the value must exist, an
 *     empty operand passes, an operand longer than the value fails;
 *   8..12 bytes <, <=, ==, >=, >: the value must exist; memcmp over the
 *     common length, then the shorter one is smaller;
 *   13..17 int <, <=, ==, >=, >: the value must exist; value and operand
 *     both go through dsn::buf2int64 (incr_parse_i64); either one failing
 *     sets *invalid_argument and fails the check.
 */
#pragma once
#include "incr_num.h"

/* the length of the common prefix of two n-byte spans, eight bytes at a time
 * (both targets are little-endian: the lowest set bit of the difference lies
 * in the first differing byte); never reads past either span */
INCR_HD static inline uint64_t cas_common(const uint8_t *a, const uint8_t *b, uint64_t n)
{
    uint64_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t x, y;
        __builtin_memcpy(&x, a + i, 8);
        __builtin_memcpy(&y, b + i, 8);
        if (x != y)
            return i + ((uint64_t)__builtin_ctzll(x ^ y) >> 3);
    }
    for (; i < n; i++)
        if (a[i] != b[i])
            return i;
    return n;
}

/* <0, 0, >0 as dsn::blob::compare orders two spans */
INCR_HD static inline int cas_bytes_cmp(const uint8_t *a, uint64_t al, const uint8_t *b,
                                        uint64_t bl)
{
    const uint64_t m = al < bl ? al : bl;
    const uint64_t c = cas_common(a, b, m);
    if (c < m)
        return a[c] < b[c] ? -1 : 1;
    return al < bl ? -1 : (al > bl ? 1 : 0);
}

INCR_HD static inline bool cas_span_eq(const uint8_t *a, const uint8_t *b, uint64_t n)
{
    return cas_common(a, b, n) == n;
}

/* true iff the check passes.  `val` is read only when value_exist. */
INCR_HD static inline bool cas_check(int32_t type, bool value_exist, const uint8_t *val,
                                     uint64_t vl, const uint8_t *opd, uint64_t ol,
                                     bool *invalid_argument)
{
    *invalid_argument = false;
    switch (type) {
    case 0:
        return true;
    case 1:
        return !value_exist;
    case 2:
        return !value_exist || vl == 0;
    case 3:
        return value_exist;
    case 4:
        return value_exist && vl != 0;
    case 5:
    case 6:
    case 7: {
        if (!value_exist)
            return false;
        if (ol == 0)
            return true;
        if (vl < ol)
            return false;
        if (type == 6)
            return cas_span_eq(val, opd, ol);
        if (type == 7)
            return cas_span_eq(val + (vl - ol), opd, ol);
        for (uint64_t at = 0; at + ol <= vl; at++)
            if (cas_span_eq(val + at, opd, ol))
                return true;
        return false;
    }
    case 8:
    case 9:
    case 10:
    case 11:
    case 12: {
        if (!value_exist)
            return false;
        const int c = cas_bytes_cmp(val, vl, opd, ol);
        if (c < 0)
            return type <= 9;
        if (c > 0)
            return type >= 11;
        return type >= 9 && type <= 11;
    }
    case 13:
    case 14:
    case 15:
    case 16:
    case 17: {
        if (!value_exist)
            return false;
        int64_t v = 0, o = 0;
        if (!incr_parse_i64(val, vl, &v) || !incr_parse_i64(opd, ol, &o)) {
            *invalid_argument = true;
            return false;
        }
        if (v < o)
            return type <= 14;
        if (v > o)
            return type >= 16;
        return type >= 14 && type <= 16;
    }
    default:
        return false; /* the caller rejects types outside 0..17 first */
    }
}

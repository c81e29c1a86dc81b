/* incr_num.h — the number half of rrdb_incr_batch: the int64 parse of a
 * stored counter and the decimal text of the new one.  No HIP call and no
 * engine type in here.  INCR_HD makes every function host code and device
 * code at once: kernels.hip calls them from the chain and emit kernels, and
 * tools/incr_num_check.cpp runs the very same functions on the CPU against
 * libc under the address and undefined-behaviour sanitizers.
 *
 * Parse.  What the reference's dsn::buf2int64 accepts: strtoll(s, &end, 0) in
 * the C locale over a copy of the span, with the whole span consumed and no
 * range error.  That is: optional leading isspace bytes (" \t\n\v\f\r"), an
 * optional sign, then 0x/0X + hex digits, or a leading 0 + octal digits, or
 * decimal digits; at least one digit; nothing after the digits (an embedded
 * NUL ends strtoll early, so it fails); the value inside int64.  strtoll
 * reads "0x" with no hex digit after it as the number 0 followed by "x", and
 * "09" as 0 followed by "9": both leave bytes over and fail.  There is no 0b
 * prefix ("0b1" is 0 followed by "b1").
 */
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define INCR_HD __host__ __device__
#else
#define INCR_HD
#endif

#define INCR_DEC_MAX 20 /* "-9223372036854775808" */

INCR_HD static inline bool incr_isspace(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }

INCR_HD static inline int incr_digit(uint8_t c)
{
    if (c >= '0' && c <= '9')
        return c - '0';
    if (c >= 'a' && c <= 'z')
        return c - 'a' + 10;
    if (c >= 'A' && c <= 'Z')
        return c - 'A' + 10;
    return 99;
}

/* true and *out set iff the n bytes at s are an int64 by the rule above */
INCR_HD static inline bool incr_parse_i64(const uint8_t *s, uint64_t n, int64_t *out)
{
    uint64_t i = 0;
    while (i < n && incr_isspace(s[i]))
        i++;
    bool neg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) {
        neg = s[i] == '-';
        i++;
    }
    uint32_t base = 10;
    if (i < n && s[i] == '0') {
        if (i + 2 < n && (s[i + 1] == 'x' || s[i + 1] == 'X') && incr_digit(s[i + 2]) < 16) {
            base = 16;
            i += 2;
        } else {
            base = 8; /* the 0 itself is the first digit */
        }
    }
    const uint64_t limit = neg ? 0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFull;
    uint64_t acc = 0, digits = 0;
    for (; i < n; i++, digits++) {
        const uint32_t d = (uint32_t)incr_digit(s[i]);
        if (d >= base)
            return false; /* a byte that is no digit: the span is not consumed */
        if (acc > (limit - d) / base)
            return false; /* leaves int64 */
        acc = acc * base + d;
    }
    if (digits == 0)
        return false;
    *out = neg ? (int64_t)(0ull - acc) : (int64_t)acc;
    return true;
}

/* bytes of std::to_string(v) */
INCR_HD static inline uint32_t incr_dec_len(int64_t v)
{
    uint64_t u = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
    uint32_t len = v < 0 ? 2 : 1;
    while (u >= 10) {
        u /= 10;
        len++;
    }
    return len;
}

/* std::to_string(v) into out (room for INCR_DEC_MAX bytes); returns its length */
INCR_HD static inline uint32_t incr_format_i64(int64_t v, uint8_t *out)
{
    const uint32_t len = incr_dec_len(v);
    uint64_t u = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
    uint32_t p = len;
    do {
        out[--p] = (uint8_t)('0' + u % 10);
        u /= 10;
    } while (u);
    if (v < 0)
        out[0] = '-';
    return len;
}

/* old + inc without leaving int64; false = it would */
INCR_HD static inline bool incr_safe_add(int64_t a, int64_t b, int64_t *out)
{
    if ((b > 0 && a > INT64_MAX - b) || (b < 0 && a < INT64_MIN - b))
        return false;
    *out = a + b;
    return true;
}

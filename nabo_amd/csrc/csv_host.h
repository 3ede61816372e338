// csv_host.h -- the host half of the CSV reader (include/nabo_csv.h), without a single HIP call: the geometry, the texts of
// the error codes, the buffer that turns bytes fed in any split into pieces of whole fields, where an offset of a piece lies
// (line, field), the table of 128-bit powers of five built by exact integer arithmetic, and the host's conversion of a
// field the device deferred.  csv_ingest.hip includes it; the tests compile it with a small main
// (tests/abi_c/csv_host_main.cpp) under the address and undefined-behaviour sanitizers.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/nabo_knn.h"
#include "csv_number.h"

namespace nabo {
namespace csv {

// TILE_BYTES: the text one workgroup owns; MAX_FIELD: the longest value field the device converts; MAX_NAME: the longest
// first field of a line with row names; HARD_FIELD: the longest field of any kind the host accepts
constexpr int TILE_BYTES = 16384, MAX_FIELD = 256, MAX_NAME = 1024, HARD_FIELD = 4096;
constexpr int64_t DEFAULT_CHUNK = (int64_t)16 << 20, MIN_CHUNK = 64, MAX_CHUNK = (int64_t)256 << 20;

inline const char *code_text(int code)
{
    switch (code) {
    case ERR_EMPTY_LINE: return "an empty line in front of the end of the table";
    case ERR_TOO_MANY: return "more fields than the table has columns";
    case ERR_EMPTY: return "an empty field";
    case ERR_BAD: return "not a number (no quotes, NA, hex, underscores or digits outside ASCII)";
    case ERR_FLOAT: return "not an integer, and the values were announced as int64";
    case ERR_RANGE: return "outside the range of int64";
    case ERR_NAME_LONG: return "the row name is longer than max_name bytes";
    case ERR_FIELD_LONG: return "the field is longer than 4096 bytes";
    case ERR_TOO_FEW: return "the line ends in front of this field";
    }
    return "?";
}

// The table's bytes, fed in any split, as pieces of whole fields.  buf has room for max_piece() bytes (the caller's: pinned
// memory in the library, a vector in the tests).  push() appends as much as fits; once size >= chunk, piece() is the length
// through the last separator or `\n` (0: none yet, and the unfinished field is too long when size > HARD_FIELD); drop(len)
// carries the rest to the front.  close() ends the stream: a last line without `\n` gets one.
struct FieldBuffer {
    uint8_t *buf = nullptr;
    uint8_t sep = ',';
    int64_t chunk = 0, size = 0;

    static int64_t clamp_chunk(int64_t c) { return c <= 0 ? DEFAULT_CHUNK : c < MIN_CHUNK ? MIN_CHUNK : c > MAX_CHUNK ? MAX_CHUNK : c; }
    int64_t fill() const { return chunk > HARD_FIELD + 1 ? chunk : HARD_FIELD + 1; }
    int64_t max_piece() const { return fill() + 1; }

    int64_t push(const uint8_t *p, int64_t n)
    {
        const int64_t take = n < fill() - size ? n : fill() - size;
        memcpy(buf + size, p, (size_t)take);
        size += take;
        return take;
    }
    bool ready() const { return size >= chunk; }
    int64_t piece() const
    {
        for (int64_t i = size; i > 0; --i)
            if (buf[i - 1] == '\n' || buf[i - 1] == sep) return i;
        return 0;
    }
    bool too_long() const { return size > HARD_FIELD; }
    void drop(int64_t len)
    {
        memmove(buf, buf + len, (size_t)(size - len));
        size -= len;
    }
    int64_t close()
    {
        if (size > 0 && buf[size - 1] != '\n') buf[size++] = '\n';
        return size;
    }
};

// Where the byte at `at` of a piece lies: the number of `\n` in front of it, and the 0-based field of its line (col0: the
// separators of the line in front of the piece, which count while no `\n` has been met)
struct Place {
    int64_t line, field;
};
inline Place locate(const uint8_t *buf, int64_t at, uint8_t sep, int64_t col0)
{
    Place p = {0, 0};
    int64_t i = at;
    while (i > 0 && buf[i - 1] != '\n') p.field += buf[--i] == sep;
    if (i == 0) p.field += col0;
    for (int64_t k = 0; k < i; ++k) p.line += buf[k] == '\n';
    return p;
}

// the bytes from `at` to the separator or `\n` that ends the field (there is one: a piece ends with either)
inline int64_t field_length(const uint8_t *buf, int64_t at, int64_t len, uint8_t sep)
{
    int64_t n = 0;
    while (at + n < len && buf[at + n] != '\n' && buf[at + n] != sep) ++n;
    return n;
}

// buf[from, len) is nothing but empty lines (`\n` or `\r\n`)
inline bool only_empty_lines(const uint8_t *buf, int64_t from, int64_t len)
{
    for (int64_t i = from; i < len; ++i)
        if (buf[i] != '\n' && !(buf[i] == '\r' && i + 1 < len && buf[i + 1] == '\n')) return false;
    return true;
}

// ---- the powers of five ---------------------------------------------------------------------------------------------
// A non-negative integer of up to 64 * 32 bits, little-endian 32-bit limbs: what the table below needs and no more
struct Big {
    static constexpr int LIMBS = 64;
    uint32_t d[LIMBS];
    Big() { memset(d, 0, sizeof d); }
    void mul_small(uint32_t m)
    {
        uint64_t carry = 0;
        for (int i = 0; i < LIMBS; ++i) {
            const uint64_t t = (uint64_t)d[i] * m + carry;
            d[i] = (uint32_t)t;
            carry = t >> 32;
        }
    }
    int bits() const
    {
        for (int i = LIMBS - 1; i >= 0; --i)
            if (d[i]) return 32 * i + 32 - __builtin_clz(d[i]);
        return 0;
    }
    bool bit(int k) const { return k < 32 * LIMBS && (d[k >> 5] >> (k & 31) & 1u); }
    void set_bit(int k) { d[k >> 5] |= 1u << (k & 31); }
    void shl1(unsigned in)
    {
        for (int i = LIMBS - 1; i > 0; --i) d[i] = d[i] << 1 | d[i - 1] >> 31;
        d[0] = d[0] << 1 | in;
    }
    bool ge(const Big &o) const
    {
        for (int i = LIMBS - 1; i >= 0; --i)
            if (d[i] != o.d[i]) return d[i] > o.d[i];
        return true;
    }
    void sub(const Big &o)
    {
        int64_t borrow = 0;
        for (int i = 0; i < LIMBS; ++i) {
            const int64_t t = (int64_t)d[i] - o.d[i] - borrow;
            d[i] = (uint32_t)t;
            borrow = t < 0;
        }
    }
    void add_one()
    {
        for (int i = 0; i < LIMBS && ++d[i] == 0; ++i) {}
    }
    // bits [top - 128, top) as (high, low); top >= 128
    void top128(int top, uint64_t *hi, uint64_t *lo) const
    {
        *hi = *lo = 0;
        for (int k = 0; k < 64; ++k) {
            *hi |= (uint64_t)bit(top - 64 + k) << k;
            *lo |= (uint64_t)bit(top - 128 + k) << k;
        }
    }
};

// out[2 (q + 342)], out[2 (q + 342) + 1] = the high and low 64 bits of the 128-bit power of five for q in [-342, 308]:
// q >= 0: 5^q shifted so that its highest bit is bit 127, the bits below bit 0 cut off; q < 0: with z the bits of 5^-q and
// b = z + 127 (q >= -27) or 2 z + 128 (below), floor(2^b / 5^-q) + 1 cut down to its highest 128 bits -- an upper bound of the
// reciprocal, as the Eisel-Lemire step is proven for.
inline void build_pow5(uint64_t *out)
{
    Big p;                                                      // 5^q, q = 0, 1, ...
    p.d[0] = 1;
    for (int q = 0; q <= POW5_MAX; ++q) {
        const int z = p.bits();
        if (z >= 128) p.top128(z, &out[2 * (q - POW5_MIN)], &out[2 * (q - POW5_MIN) + 1]);
        else {
            unsigned __int128 v = 0;
            for (int i = 3; i >= 0; --i) v = v << 32 | p.d[i];
            v <<= 128 - z;
            out[2 * (q - POW5_MIN)] = (uint64_t)(v >> 64), out[2 * (q - POW5_MIN) + 1] = (uint64_t)v;
        }
        p.mul_small(5);
    }
    Big f;                                                      // 5^k, k = 1, 2, ...
    f.d[0] = 5;
    for (int k = 1; k <= -POW5_MIN; ++k) {
        const int z = f.bits(), b = k <= 27 ? z + 127 : 2 * z + 128;
        Big quo, rem;                                           // 2^b / 5^k, bit by bit from the top
        for (int i = b; i >= 0; --i) {
            rem.shl1(i == b);
            if (rem.ge(f)) {
                rem.sub(f);
                quo.set_bit(i);
            }
        }
        quo.add_one();
        quo.top128(quo.bits(), &out[2 * (-k - POW5_MIN)], &out[2 * (-k - POW5_MIN) + 1]);
        f.mul_small(5);
    }
}

// ---- a deferred field on the host -----------------------------------------------------------------------------------
// s[0 .. n): the grammar again (a field longer than MAX_FIELD has not been looked at), then strtod or strtoll on the text
// without its blanks: 0 with the 8 bytes, or the error code
inline int host_convert(const uint8_t *s, int64_t n, bool line_end, int kind, uint64_t *bits)
{
    if (n > HARD_FIELD) return ERR_FIELD_LONG;
    Scan sc;
    int rc = scan_field(s, (int)n, line_end, &sc);
    if (rc) return rc;
    if (kind == KIND_INT64 && (sc.special || sc.point || sc.exp)) return ERR_FLOAT;
    char text[HARD_FIELD + 1];
    int m = 0;
    for (int64_t i = 0; i < n; ++i)
        if (!is_blank(s[i]) && s[i] != '\r') text[m++] = (char)s[i];
    text[m] = 0;
    char *end = nullptr;
    if (kind == KIND_INT64) {
        errno = 0;
        const long long v = strtoll(text, &end, 10);
        if (errno == ERANGE) return ERR_RANGE;
        *bits = (uint64_t)v;
    } else {
        const double v = strtod(text, &end);
        memcpy(bits, &v, 8);
        if (sc.special == 2) *bits = (sc.neg ? (uint64_t)1 << 63 : 0) | 0x7FF8000000000000ull;   // one NaN, whatever libc makes
    }
    return end == text + m ? 0 : ERR_BAD;
}

}  // namespace csv
}  // namespace nabo

// csv_number.h -- one value field of a CSV table to 8 bytes (include/nabo_csv.h states the grammar and the rule).  ONE piece
// of source for both sides: csv_ingest.hip compiles it for the device, csv_host.h and tests/abi_c/csv_host_main.cpp for the
// host, and the CPU tests hold the host build to the plain restatement (tests/_csv_ref.py) field by field, verdict included.
// Nothing here calls HIP or libc.
//
// decimal -> double.  The field is scanned into w (its first 19 significant digits at most, as a uint64) and a decimal
// exponent q, value = w * 10^q.  More than 19 significant digits: DEFER (the host's strtod decides).  Otherwise
//   (a) w = 0: a signed zero;  q < -342: w * 10^q < 2^64 * 10^-343 < 2^-1075, half the smallest subnormal: a signed zero;
//       q > 308: w >= 1 gives at least 10^309 > DBL_MAX: infinity;
//   (b) Clinger's fast path, w <= 2^53 and |q| <= 22: w and 10^|q| are exact doubles, so ONE IEEE multiply or divide is the
//       correctly rounded result (the device's f64 multiply and divide are correctly rounded, contraction is off);
//   (c) the Eisel-Lemire step: w normalised to 64 bits times the 128-bit truncated power of five for q (the table of
//       csv_host.h, q in [-342, 308]) gives the upper bits of the product; when its low word is all ones and q lies
//       outside [-27, 55] the truncation could hide a carry, the rounding is NOT proven, and the verdict is DEFER.  In every
//       other case the paper's argument (Lemire, "Number parsing at a gigabyte per second", 2021, sections 5 and 6) proves
//       the bits below, the ties-to-even case (q in [-4, 23]) and the subnormal and overflow edges included.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NABO_CSV_HD __host__ __device__ inline
#else
#define NABO_CSV_HD inline
#endif

namespace nabo {
namespace csv {

constexpr int POW5_MIN = -342, POW5_MAX = 308, POW5_WORDS = 2 * (POW5_MAX - POW5_MIN + 1);   // (high, low) per exponent
constexpr int KIND_FLOAT64 = 0, KIND_INT64 = 1;

// What a field, or a line, comes to.  The errors are ordered as they win at ONE byte offset (the lowest offset wins first):
// an excess field is judged before its own text, a missing field after everything that is there.
enum Code {
    VALUE = 0,            // converted: the 8 bytes are out
    DEFER = -1,           // not decided here: the host converts the text
    ERR_EMPTY_LINE = 1,
    ERR_TOO_MANY = 2,
    ERR_EMPTY = 3,
    ERR_BAD = 4,
    ERR_FLOAT = 5,
    ERR_RANGE = 6,
    ERR_NAME_LONG = 7,
    ERR_FIELD_LONG = 8,
    ERR_TOO_FEW = 9,
};

struct Scan {
    uint64_t w;           // the first 19 significant digits at most
    int32_t q;            // value = w * 10^q when nd <= 19
    int32_t nd;           // significant digits (leading zeros not counted)
    int32_t special;      // 0: a number, 1: inf, 2: nan
    bool neg, point, exp;
};

NABO_CSV_HD bool is_blank(uint8_t c) { return c == ' ' || c == '\t'; }

// s[i .. e) equals `word` (lower case) without regard to case
NABO_CSV_HD bool is_word(const uint8_t *s, int i, int e, const char *word, int len)
{
    if (e - i != len) return false;
    for (int k = 0; k < len; ++k)
        if ((s[i + k] | 0x20) != (uint8_t)word[k]) return false;
    return true;
}

// The grammar of a value field s[0 .. n) under value_kind 0; line_end: the field is the last of its line, so that a `\r`
// as its last byte is a blank.  0, or ERR_EMPTY (nothing but blanks) or ERR_BAD.
NABO_CSV_HD int scan_field(const uint8_t *s, int n, bool line_end, Scan *o)
{
    int i = 0, e = n;
    if (line_end && e > 0 && s[e - 1] == '\r') --e;
    while (i < e && is_blank(s[i])) ++i;
    while (e > i && is_blank(s[e - 1])) --e;
    o->w = 0, o->q = 0, o->nd = 0, o->special = 0, o->neg = false, o->point = false, o->exp = false;
    if (i == e) return ERR_EMPTY;
    if (s[i] == '+' || s[i] == '-') o->neg = s[i++] == '-';
    if (i == e) return ERR_BAD;
    const uint8_t c0 = s[i] | 0x20;
    if (c0 == 'i' || c0 == 'n') {
        if (is_word(s, i, e, "inf", 3) || is_word(s, i, e, "infinity", 8)) o->special = 1;
        else if (is_word(s, i, e, "nan", 3)) o->special = 2;
        else return ERR_BAD;
        return 0;
    }
    uint64_t w = 0;
    int nd = 0, q = 0;
    bool any = false;
    for (; i < e; ++i) {
        const unsigned d = (unsigned)s[i] - '0';
        if (d > 9) break;
        any = true;
        if (nd > 0 || d > 0) {
            if (nd < 19) w = w * 10 + d;
            else ++q;                                           // an integer digit that is not kept
            ++nd;
        }
    }
    if (i < e && s[i] == '.') {
        o->point = true;
        for (++i; i < e; ++i) {
            const unsigned d = (unsigned)s[i] - '0';
            if (d > 9) break;
            any = true;
            if (nd > 0 || d > 0) {
                if (nd < 19) w = w * 10 + d, --q;
                ++nd;
            } else
                --q;                                            // a zero right behind the point, in front of the first digit
        }
    }
    if (!any) return ERR_BAD;
    if (i < e && (s[i] | 0x20) == 'e') {
        o->exp = true;
        ++i;
        bool eneg = false;
        if (i < e && (s[i] == '+' || s[i] == '-')) eneg = s[i++] == '-';
        if (i == e) return ERR_BAD;
        int ex = 0;
        for (; i < e; ++i) {
            const unsigned d = (unsigned)s[i] - '0';
            if (d > 9) return ERR_BAD;
            if (ex < 100000) ex = ex * 10 + (int)d;             // saturates far outside [-342, 308] and the field's length
        }
        q += eneg ? -ex : ex;
    }
    if (i != e) return ERR_BAD;
    o->w = w, o->q = q, o->nd = nd;
    return 0;
}

NABO_CSV_HD uint64_t mul_hi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

NABO_CSV_HD uint64_t double_bits(double d)
{
    union {
        double d;
        uint64_t u;
    } x;
    x.d = d;
    return x.u;
}

// w * 10^q, w with 19 digits at most, to the bits of the nearest double (ties to even): VALUE or DEFER (see the top)
NABO_CSV_HD int decimal_to_double(uint64_t w, int q, const uint64_t *pow5, uint64_t *bits)
{
    const uint64_t INF = 0x7FF0000000000000ull;
    if (w == 0 || q < POW5_MIN) {
        *bits = 0;
        return VALUE;
    }
    if (q > POW5_MAX) {
        *bits = INF;
        return VALUE;
    }
    if (w <= ((uint64_t)1 << 53) && q >= -22 && q <= 22) {
        const double p10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
        const double x = (double)w;                             // exact
        *bits = double_bits(q < 0 ? x / p10[-q] : x * p10[q]);
        return VALUE;
    }
    int lz = __builtin_clzll(w);
    w <<= lz;
    const uint64_t t_hi = pow5[2 * (q - POW5_MIN)], t_lo = pow5[2 * (q - POW5_MIN) + 1];
    uint64_t hi = mul_hi(w, t_hi), lo = w * t_hi;
    if ((hi & 0x1FF) == 0x1FF) {                                // the 55 bits that are needed leave 9: all ones, the low half decides
        const uint64_t second_hi = mul_hi(w, t_lo);
        lo += second_hi;
        if (second_hi > lo) ++hi;
    }
    if (lo == ~(uint64_t)0 && (q < -27 || q > 55)) return DEFER;
    const int upper = (int)(hi >> 63);
    uint64_t m = hi >> (upper + 9);
    int p2 = (int)(((int64_t)217706 * q) >> 16) + 63 + upper - lz + 1023;
    if (p2 <= 0) {                                              // subnormal, or zero
        if (-p2 + 1 >= 64) {
            *bits = 0;
            return VALUE;
        }
        m >>= -p2 + 1;
        m += m & 1;
        m >>= 1;
        *bits = m;                                              // (m = 2^52 is the smallest normal number: the same bits)
        return VALUE;
    }
    if (lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << (upper + 9)) == hi) m &= ~(uint64_t)1;   // exactly halfway: to even
    m += m & 1;
    m >>= 1;
    if (m >= ((uint64_t)2 << 52)) {
        m = (uint64_t)1 << 52;
        ++p2;
    }
    m &= ~((uint64_t)1 << 52);
    if (p2 >= 0x7FF) {
        *bits = INF;
        return VALUE;
    }
    *bits = (uint64_t)p2 << 52 | m;
    return VALUE;
}

// One value field to its 8 bytes: VALUE, DEFER or what is wrong with it
NABO_CSV_HD int convert_field(const uint8_t *s, int n, bool line_end, int kind, const uint64_t *pow5, uint64_t *bits)
{
    Scan sc;
    const int rc = scan_field(s, n, line_end, &sc);
    if (rc) return rc;
    const uint64_t sign = sc.neg ? (uint64_t)1 << 63 : 0;
    if (kind == KIND_INT64) {
        if (sc.special || sc.point || sc.exp) return ERR_FLOAT;
        if (sc.nd > 18) return DEFER;
        *bits = sc.neg ? (uint64_t)0 - sc.w : sc.w;
        return VALUE;
    }
    if (sc.special) {
        *bits = sign | (sc.special == 1 ? 0x7FF0000000000000ull : 0x7FF8000000000000ull);
        return VALUE;
    }
    if (sc.nd > 19) return DEFER;
    const int v = decimal_to_double(sc.w, sc.q, pow5, bits);
    if (v == VALUE) *bits |= sign;
    return v;
}

// The entry rule on a converted value: below the threshold it is 0 (NaN < t is false), and it is kept iff it is not 0
NABO_CSV_HD bool keeps_value(int kind, uint64_t bits, bool has_thresh, double thresh)
{
    double v;
    if (kind == KIND_INT64) {
        if (bits == 0) return false;
        v = (double)(int64_t)bits;                              // (numpy compares an int64 with a float threshold as doubles)
    } else {
        union {
            uint64_t u;
            double d;
        } x;
        x.u = bits;
        v = x.d;
        if (v == 0.0) return false;                             // -0.0 too; a NaN stays
    }
    return !(has_thresh && v < thresh);
}

}  // namespace csv
}  // namespace nabo

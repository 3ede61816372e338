// bucket_skip.h -- which stretches of the two-level stream a workgroup of the ordered main launch cannot need (DESIGN.md
// 4.1f (g)): the bound, its rounding allowance and the run list, as functions the device kernels (bucket_skip.hip) and the
// host share.  tests/test_bucket_skip_cpu.py compiles this header for the host and holds it against a numpy restatement.
//
// Coordinates are the packer's: v~ = (v - centre) * scale.  The filter's score of a pair is ||y~||^2 - 2 x~.y~ =
// ||x~ - y~||^2 - ||x~||^2, and row i takes nothing whose score is >= its start threshold tau0_i (the threshold only falls).
// For ANY vector u with ||u|| <= 1:  ||x~ - y~|| >= (y~ - x~).u.  The references are cut into GROUPS of consecutive positions
// of the ordered copy (the sub-buckets; a bucket without a sub-order is one group).  With b the row's bucket, b' the
// group's and u[b][b'] the unit vector from the mean of b to the mean of b':
//     ymin[b][group] = min over the group's references of y~.u[b][b'],      reach_i[b'] = x~_i.u[b_i][b'] + sqrt(tau0_i + ||x~_i||^2)
// and   ymin[b_i][group] >= reach_i[b']   implies   score >= tau0_i   for every reference of the group.
// A workgroup skips a group when that holds for every live row of it; groups of the rows' own buckets are never skipped.
//
// THE ALLOWANCE.  Projections, norms and the square root are float64 sums of at most BSKIP_MAX_DIM products: the computed
// y~.u is within dim 2^-53 ||y~|| ||u|| of the exact one, u is normalised in float64 (||u|| <= 1 + 2^-50), and v~ itself
// carries one rounding per component (2^-53 |v~_k|).  All of it is below BSKIP_ALLOW x norm with BSKIP_ALLOW = 2^-40
// (dim <= 64: 2^-47 + 2^-50 + 2^-53 < 2^-46), so
//     ymin is stored as the float BELOW   y~.u - 2^-40 ||y~||,
//     reach as the float ABOVE            x~.u + 2^-40 ||x~|| + (1 + 2^-40) sqrt(max(tau0 + (1 + 2^-40) ||x~||^2, 0)),
// (the radius is the root of a DIFFERENCE -- tau0 is about -||x~||^2 plus a squared neighbour distance -- so the norm's own
// error, 2^-45 ||x~||^2, is added under the root and not as a factor on it), and the test itself is one fp32 comparison without arithmetic.  A row whose tau0 or norm is not finite has reach +inf:
// it vetoes every skip.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NABO_HD __host__ __device__
#else
#define NABO_HD
#endif

namespace nabo {

constexpr int BSKIP_MAX_DIM = 64;                       // components of a cell (the stream's slot order holds at most 59); the kernels' register tile
constexpr double BSKIP_ALLOW = 9.094947017729282e-13;   // 2^-40
constexpr int BSKIP_RUN_CAP = 256;                      // kept stretches per workgroup; a list that would overflow merges the rest
constexpr int BSKIP_RUN_INTS = 2 * (BSKIP_RUN_CAP + 1); // int32 per workgroup: [begin, end) pairs and the (0, 0) sentinel
constexpr int BSKIP_OWN_MAX = 32;                       // distinct buckets among a workgroup's rows (the rest class packs several); more: nothing is skipped
constexpr int BSKIP_WG_ROWS = 384;                      // positions of a workgroup of the ordered main launch (geometry B)
constexpr int64_t BSKIP_MAX_TILES = 1 << 19;            // longest stream a workgroup's bitmap of pairs of tiles serves (32 KB of LDS)

// the nearest float at or below / at or above a finite double (+-inf and NaN pass through the conversion)
NABO_HD inline float bskip_float_below(double v)
{
    float f = (float)v;
    if ((double)f > v) {
        int32_t bits;
        __builtin_memcpy(&bits, &f, 4);
        if (f > 0.0f) --bits;
        else if (f < 0.0f) ++bits;
        else bits = (int32_t)0x80000001u;               // below +-0: the smallest negative subnormal
        __builtin_memcpy(&f, &bits, 4);
    }
    return f;
}
NABO_HD inline float bskip_float_above(double v) { return -bskip_float_below(-v); }

NABO_HD inline bool bskip_finite(double v) { return v - v == 0.0; }

// a cell in the packer's coordinates, its projection on a direction and its squared norm (float64, in index order)
NABO_HD inline double bskip_coord(double v, double centre, double scale) { return (v - centre) * scale; }
NABO_HD inline double bskip_dot(int dim, const double *a, const double *b)
{
    double s = 0.0;
    for (int d = 0; d < dim; ++d) s = __builtin_fma(a[d], b[d], s);
    return s;
}

// u[b][b'] from the two means (dim doubles each): false, and u = 0, where the difference has no direction (the same
// bucket, equal means, a bucket without references -- the caller passes has_both -- or overflow).  A zero direction is
// valid (||u|| <= 1) and skips nothing but the degenerate case reach <= 0.
// (in two parts, so that a device thread needs no array: the scale 1 / ||difference||, 0 for no direction, and a component)
NABO_HD inline double bskip_direction_scale(int dim, const double *mean_from, const double *mean_to, bool has_both)
{
    double ss = 0.0;
    for (int d = 0; d < dim; ++d) {
        const double w = mean_to[d] - mean_from[d];
        ss = __builtin_fma(w, w, ss);
    }
    return has_both && ss > 0.0 && bskip_finite(ss) ? 1.0 / __builtin_sqrt(ss) : 0.0;
}
NABO_HD inline double bskip_direction_component(double from, double to, double scale) { return scale > 0.0 ? (to - from) * scale : 0.0; }
NABO_HD inline bool bskip_direction(int dim, const double *mean_from, const double *mean_to, bool has_both, double *u)
{
    const double scale = bskip_direction_scale(dim, mean_from, mean_to, has_both);
    for (int d = 0; d < dim; ++d) u[d] = bskip_direction_component(mean_from[d], mean_to[d], scale);
    return scale > 0.0;
}

// What a reference contributes to ymin: its projection less its allowance (bskip_ref_allow of norm2 = ||y~||^2), -inf where
// that is not finite.  ymin is the float below the smallest contribution (rounding is monotone: one rounding per minimum).
NABO_HD inline double bskip_ref_allow(double norm2) { return BSKIP_ALLOW * __builtin_sqrt(norm2); }
NABO_HD inline double bskip_ref_value(double proj, double allow)
{
    const double v = proj - allow;
    return bskip_finite(v) ? v : -__builtin_inf();
}

// How far row i reaches along a direction: its projection plus its RADIUS -- the root of its start threshold plus both
// allowances, a property of the row alone; +inf (a veto) for a seed or a norm that is not finite.  reach is the float above
// the largest value over the rows.
NABO_HD inline double bskip_row_radius(double norm2, float tau0)
{
    const double r2 = (double)tau0 + norm2 + BSKIP_ALLOW * norm2;
    if (!bskip_finite(r2)) return __builtin_inf();
    const double r = r2 > 0.0 ? __builtin_sqrt(r2) : 0.0;
    return BSKIP_ALLOW * __builtin_sqrt(norm2) + (1.0 + BSKIP_ALLOW) * r;
}
NABO_HD inline double bskip_row_reach(double proj, double radius)
{
    const double v = proj + radius;
    return v == v ? v : __builtin_inf();
}

// one row, one group (the workgroup's rule is the AND over its live rows)
// (a reach of +inf is a veto even against an empty group's ymin of +inf)
NABO_HD inline bool bskip_row_allows(float ymin, float reach) { return ymin >= reach && reach < __builtin_inff(); }

// The tiles a group of `count` consecutive positions from `first` touches: [*t0, *t1), empty for an empty group.  Groups are
// not padded to tiles: neighbours share a tile, and a kept group keeps the shared tile for both.
NABO_HD inline void bskip_group_tiles(int64_t first, int64_t count, int32_t *t0, int32_t *t1)
{
    *t0 = (int32_t)(first / 32);
    *t1 = count > 0 ? (int32_t)((first + count + 31) / 32) : *t0;
}

// The run list of a workgroup: the kept groups' tiles in stream order (t0 non-decreasing), each widened to even tile indices
// (the filter's loops step in twos) and clipped to [0, t_end) (t_end even); overlapping or adjacent runs merged; at most cap
// runs -- a list that would overflow stretches its last run over everything that follows, which keeps more, never less.
// runs: [begin, end) pairs, terminated by the pair (0, 0); room for 2 (cap + 1) ints.
// Built through a BITMAP of the stream's pairs of tiles (bit p: tiles 2p and 2p + 1 are kept), so that a workgroup's threads
// mark their groups side by side and find the runs a word each; the host walks the same words one after the other.
NABO_HD inline int64_t bskip_bitmap_words(int32_t t_end) { return ((int64_t)t_end / 2 + 31) / 32; }
// the pairs of tiles [*p0, *p1) a group's tiles [t0, t1) widen to, clipped to the stream
NABO_HD inline void bskip_group_pairs(int32_t t0, int32_t t1, int32_t t_end, int32_t *p0, int32_t *p1)
{
    *p0 = t0 >> 1;
    *p1 = t1 > t0 ? (t1 + 1) >> 1 : *p0;
    if (*p1 > t_end / 2) *p1 = t_end / 2;
}
// bits of word w that begin / end a run (below: the last bit of the word before it, above: the first bit of the next)
NABO_HD inline uint32_t bskip_start_bits(uint32_t w, uint32_t below) { return w & ~((w << 1) | (below & 1u)); }
NABO_HD inline uint32_t bskip_end_bits(uint32_t w, uint32_t above) { return w & ~((w >> 1) | ((above & 1u) << 31)); }
NABO_HD inline int bskip_popcount(uint32_t w)
{
    int n = 0;
    for (; w; w &= w - 1) ++n;
    return n;
}
NABO_HD inline int bskip_lowest_bit(uint32_t w)
{
    int n = 0;
    for (; !(w & 1u); w >>= 1) ++n;
    return n;
}
// run number k (of nruns) begins / ends with pair `pair`: the runs past the list's capacity are one run, the last
NABO_HD inline void bskip_emit_start(int32_t *runs, int cap, int64_t k, int64_t pair)
{
    if (k < cap) runs[2 * k] = (int32_t)(2 * pair);
}
NABO_HD inline void bskip_emit_end(int32_t *runs, int cap, int64_t k, int64_t nruns, int64_t pair)
{
    if (k < cap - 1) runs[2 * k + 1] = (int32_t)(2 * pair + 2);
    else if (k == nruns - 1) runs[2 * (cap - 1) + 1] = (int32_t)(2 * pair + 2);
}
NABO_HD inline void bskip_emit_sentinel(int32_t *runs, int cap, int64_t nruns)
{
    const int64_t n = nruns < cap ? nruns : cap;
    runs[2 * n] = runs[2 * n + 1] = 0;
}
// the whole construction, one word after the other (words: scratch of bskip_bitmap_words(t_end) entries); returns the runs
// written (at most cap)
inline int bskip_build_runs(int ngroup, const int32_t *t0, const int32_t *t1, const uint8_t *keep, int32_t t_end, int cap, uint32_t *words,
                            int32_t *runs)
{
    const int64_t nw = bskip_bitmap_words(t_end);
    for (int64_t j = 0; j < nw; ++j) words[j] = 0;
    for (int g = 0; g < ngroup; ++g) {
        if (!keep[g]) continue;
        int32_t p0, p1;
        bskip_group_pairs(t0[g], t1[g], t_end, &p0, &p1);
        for (int32_t p = p0; p < p1; ++p) words[p >> 5] |= 1u << (p & 31);
    }
    int64_t nruns = 0;
    for (int64_t j = 0; j < nw; ++j) nruns += bskip_popcount(bskip_start_bits(words[j], j ? words[j - 1] >> 31 : 0));
    int64_t ks = 0, ke = 0;
    for (int64_t j = 0; j < nw; ++j) {
        for (uint32_t m = bskip_start_bits(words[j], j ? words[j - 1] >> 31 : 0); m; m &= m - 1) bskip_emit_start(runs, cap, ks++, 32 * j + bskip_lowest_bit(m));
        for (uint32_t m = bskip_end_bits(words[j], j + 1 < nw ? words[j + 1] : 0); m; m &= m - 1) bskip_emit_end(runs, cap, ke++, nruns, 32 * j + bskip_lowest_bit(m));
    }
    bskip_emit_sentinel(runs, cap, nruns);
    return (int)(nruns < cap ? nruns : cap);
}

// tiles the list keeps (the launch skips the rest of its t_end tiles)
NABO_HD inline int64_t bskip_kept_tiles(const int32_t *runs)
{
    int64_t s = 0;
    for (int r = 0; runs[2 * r + 1] > runs[2 * r]; ++r) s += runs[2 * r + 1] - runs[2 * r];
    return s;
}

// The tables can be built for a stream of this many tiles and cells of this many components (the workgroup's bitmap of
// pairs of tiles lives in LDS, the kernels' register tile holds BSKIP_MAX_DIM components).  An index beyond either limit
// never skips -- and never waits for tables that cannot come.
inline bool bskip_buildable(int64_t ordered_tiles, int g) { return ordered_tiles >= 2 && ordered_tiles <= BSKIP_MAX_TILES && g >= 1 && g <= BSKIP_MAX_DIM; }

// Where the planner switches the skip on (option bucket_skip: 0 = where the stream runs at its default setting, 1 = off,
// 2 = wherever the ordered main launch runs).  tl_main: the plan streams; two_level: that option's value.
inline bool bskip_planned(int bucket_skip_option, bool tl_main, int two_level_option)
{
    if (!tl_main || bucket_skip_option == 1) return false;
    return bucket_skip_option >= 2 || two_level_option == 1;
}

}  // namespace nabo

// The rule by which the two-level stream skips sub-buckets (nabo_amd/csrc/bucket_skip.h) compiled for the host, put together
// from the header's functions the way the kernels of bucket_skip.hip put it together, callable from
// tests/test_bucket_skip_cpu.py.  Cells come in caller coordinates with the packer's centre and scale.
#include <cstddef>
#include <vector>

#include "bucket_skip.h"

using namespace nabo;

extern "C" void bskip_constants_host(int64_t *out)
{
    out[0] = BSKIP_RUN_CAP;
    out[1] = BSKIP_RUN_INTS;
    out[2] = BSKIP_OWN_MAX;
    out[3] = BSKIP_WG_ROWS;
    out[4] = BSKIP_MAX_DIM;
}

extern "C" float bskip_float_below_host(double v) { return bskip_float_below(v); }
extern "C" float bskip_float_above_host(double v) { return bskip_float_above(v); }

// The reference side: Y [n][dim], bucket [n] (-1: masked, no bucket), group [n] in [0, G) with group / S == bucket.
// Out: mean [C][dim], u [C][C][dim] (from b to b'), ymin [C][G].
extern "C" void bskip_refs_host(int64_t n, int dim, const double *Y, const double *centre, double scale, const int32_t *bucket,
                                const int32_t *group, int C, int S, double *mean, double *u, float *ymin)
{
    const int G = C * S;
    std::vector<int64_t> cnt(C, 0);
    std::vector<double> y(dim);
    for (int64_t i = 0; i < (int64_t)C * dim; ++i) mean[i] = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (bucket[i] < 0) continue;
        ++cnt[bucket[i]];
        for (int d = 0; d < dim; ++d) mean[(int64_t)bucket[i] * dim + d] += bskip_coord(Y[i * dim + d], centre[d], scale);
    }
    for (int b = 0; b < C; ++b)
        for (int d = 0; d < dim; ++d) mean[(int64_t)b * dim + d] = cnt[b] > 0 ? mean[(int64_t)b * dim + d] / (double)cnt[b] : 0.0;
    for (int b = 0; b < C; ++b)
        for (int bp = 0; bp < C; ++bp)
            bskip_direction(dim, mean + (int64_t)b * dim, mean + (int64_t)bp * dim, b != bp && cnt[b] > 0 && cnt[bp] > 0,
                            u + ((int64_t)b * C + bp) * dim);
    for (int64_t i = 0; i < (int64_t)C * G; ++i) ymin[i] = __builtin_inff();
    for (int64_t i = 0; i < n; ++i) {
        if (bucket[i] < 0) continue;
        for (int d = 0; d < dim; ++d) y[d] = bskip_coord(Y[i * dim + d], centre[d], scale);
        const double allow = bskip_ref_allow(bskip_dot(dim, y.data(), y.data()));
        for (int b = 0; b < C; ++b) {
            const float v = bskip_float_below(bskip_ref_value(bskip_dot(dim, y.data(), u + ((int64_t)b * C + bucket[i]) * dim), allow));
            float &m = ymin[(int64_t)b * G + group[i]];
            if (v < m) m = v;
        }
    }
}

// One workgroup: rows X [m][dim] with bucket [m] (-1: a padding position) and start thresholds tau0 [m].  keep [G]: 1 where
// the workgroup runs the group.  Returns the distinct own buckets, or -1 where there were more than BSKIP_OWN_MAX (a veto).
extern "C" int bskip_workgroup_host(int64_t m, int dim, const double *X, const double *centre, double scale, const int32_t *bucket,
                                    const float *tau0, int C, int S, const double *u, const float *ymin, uint8_t *keep)
{
    const int G = C * S;
    std::vector<int> own;
    std::vector<float> reach;
    std::vector<double> x(dim);
    bool veto = false;
    for (int64_t i = 0; i < m && !veto; ++i) {
        if (bucket[i] < 0) continue;
        int s = -1;
        for (size_t c = 0; c < own.size(); ++c)
            if (own[c] == bucket[i]) s = (int)c;
        if (s < 0) {
            if ((int)own.size() == BSKIP_OWN_MAX) { veto = true; break; }
            s = (int)own.size();
            own.push_back(bucket[i]);
            reach.resize(own.size() * C, -__builtin_inff());
        }
        for (int d = 0; d < dim; ++d) x[d] = bskip_coord(X[i * dim + d], centre[d], scale);
        const double radius = bskip_row_radius(bskip_dot(dim, x.data(), x.data()), tau0[i]);
        for (int bp = 0; bp < C; ++bp) {
            const float r = bskip_float_above(bskip_row_reach(bskip_dot(dim, x.data(), u + ((int64_t)bucket[i] * C + bp) * dim), radius));
            if (r > reach[(size_t)s * C + bp]) reach[(size_t)s * C + bp] = r;
        }
    }
    for (int gi = 0; gi < G; ++gi) {
        const int bp = gi / S;
        bool k = veto;
        for (size_t s = 0; s < own.size() && !k; ++s) k = own[s] == bp || !bskip_row_allows(ymin[(int64_t)own[s] * G + gi], reach[s * C + bp]);
        keep[gi] = k ? 1 : 0;
    }
    return veto ? -1 : (int)own.size();
}

extern "C" void bskip_group_tiles_host(int64_t first, int64_t count, int32_t *t0, int32_t *t1) { bskip_group_tiles(first, count, t0, t1); }

// runs: room for 2 (cap + 1) ints
extern "C" int bskip_build_runs_host(int ngroup, const int32_t *t0, const int32_t *t1, const uint8_t *keep, int32_t t_end, int cap, int32_t *runs)
{
    std::vector<uint32_t> words((size_t)bskip_bitmap_words(t_end) + 1);
    return bskip_build_runs(ngroup, t0, t1, keep, t_end, cap, words.data(), runs);
}

extern "C" int64_t bskip_kept_tiles_host(const int32_t *runs) { return bskip_kept_tiles(runs); }

extern "C" int bskip_buildable_host(int64_t ordered_tiles, int g) { return bskip_buildable(ordered_tiles, g) ? 1 : 0; }
extern "C" int64_t bskip_max_tiles_host() { return BSKIP_MAX_TILES; }

extern "C" int bskip_planned_host(int option, int tl_main, int two_level) { return bskip_planned(option, tl_main != 0, two_level) ? 1 : 0; }

// query.hip -- a query on an index: the three routes (exact float64 kernels, Euclidean / cosine filter passes, modified
// Canberra), the pass chain that sends uncertified rows one link down (rerun_failed_rows), copy-out and statistics.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "bucket_skip.h"
#include "index.h"
#include "local_seeds.h"

namespace nabo {

// Entries of the masked-reference list a row may continue with when it has fewer than k' unmasked references
// (numpy.ma's NaN fill sorts the ignored references last, by index: nabo/_mapping.py:135-146).  A SHARD must not do
// that: its masked references would enter the global merge as if they were neighbours (found by the randomised
// sweep: 40-reference shards, 60 % masked) -- there the tail is left absent (index -1), which the merge skips.
static int tail_len(const nabo_index *ix) { return ix->shard_mode ? 0 : ix->ref.n_masked_list; }

// The rows of the current batch listed in `d_rows` (device, nf entries) go on to the pass `code`: note it per top-level row and
// return their top-level row numbers in `map` (the inner query_impl's PassCtx::row_map).  The stream is synchronised.
static int note_row_pass(nabo_index *ix, const PassCtx &ctx, const uint32_t *d_rows, int64_t nf, uint8_t code, std::vector<uint32_t> &map)
{
    map.resize((size_t)nf);
    if (nf == 0) return NABO_OK;
    HIP_TRY(hipMemcpyAsync(map.data(), d_rows, (size_t)nf * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    for (int64_t i = 0; i < nf; ++i) {
        if (ctx.row_map) map[(size_t)i] = map[(size_t)i] < ctx.row_map->size() ? (*ctx.row_map)[map[(size_t)i]] : 0xFFFFFFFFu;
        if (map[(size_t)i] < ix->last.row_pass.size()) ix->last.row_pass[map[(size_t)i]] = code;
    }
    return NABO_OK;
}

// What every route of a query reads (query_body stages it), and what the route leaves for finish_query.
struct Query {
    const double *dX = nullptr;      // [m, g] targets on the device
    const double *dXp = nullptr;     // ... as the Euclidean / cosine filter packs them (cosine: the unit rows)
    int64_t m = 0;
    int k = 0, drop = 0, kk = 0;     // kk = k + drop
    int epl = 1, L = 32;             // emitted candidate lists hold L = 32 epl entries
    int64_t *d_oidx = nullptr;       // [m, k] results on the device
    double *d_odist = nullptr;
    bool cand_mode = false;
    double *out_bound = nullptr;
    bool top = false;                // this call owns the per-row pass record
    std::vector<uint32_t> pass_map;  // top-level rows of the batch an inner call works on
    unsigned int n_fail = 0;         // set by the route: counters[0], [1], [3] of nabo_index_last_stats
    int S = 1;
    int64_t n_wg = 0;
    // a call that reran rows one link down (rerun_failed_rows): its phases 0-2 from before the inner call, and that call's total
    bool ms_kept = false;
    float ms_keep[3] = {0, 0, 0};
    double ms_inner = 0.0;
};

// Rows of the exact kernels' distance workspace: ~1 GiB of float64 rows, at least one, at most `rows` and `cap`.
static int reserve_exact_ws(nabo_index *ix, uint64_t rows, uint64_t cap, unsigned int *d_rows)
{
    const IndexShape &sh = ix->shape;
    auto &ws = ix->ws;
    uint64_t r = (1ull << 30) / ((uint64_t)sh.n * sizeof(double));
    if (r < 1) r = 1;
    if (r > rows) r = rows;
    if (r > cap) r = cap;
    *d_rows = (unsigned int)r;
    return ws.exact_d.reserve((size_t)r * sh.n * sizeof(double));
}

// Shapes outside the instantiated filter kernels: the exact float64 kernels answer every row.
static int query_exact(nabo_index *ix, Query &q)
{
    const IndexShape &sh = ix->shape;
    auto &ref = ix->ref;
    auto &ws = ix->ws;
    hipStream_t st = ix->stream;
    int rc;
    unsigned int d_rows = 0;
    if (q.top) ix->last.row_pass.assign((size_t)q.m, (uint8_t)NABO_PASS_EXACT);
    if (q.m > 0xFFFFFFF0ll) return api_fail(NABO_E_UNSUPPORTED, "m=%lld: fewer than 2^32-16 rows per call", (long long)q.m);
    if ((rc = ws.fails.reserve((size_t)q.m * sizeof(uint32_t)))) return rc;
    if ((rc = reserve_exact_ws(ix, (uint64_t)q.m, 65528, &d_rows))) return rc;
    HIP_TRY(iota_launch(ws.fails.as<uint32_t>(), q.m, st));
    for (int i = 1; i <= 3; ++i) HIP_TRY(hipEventRecord(ix->ev[i], st));
    HIP_TRY(exact_rows_launch(q.dX, ref.dY, sh.n, sh.g, sh.metric, ix->f, ref.dmask, ws.fails.as<uint32_t>(),
                              (unsigned int)q.m, q.k, q.drop, ix->base, ref.mlistbuf.as<uint32_t>(), tail_len(ix),
                              q.d_oidx, q.d_odist, ws.exact_d.as<double>(), d_rows, st));
    HIP_TRY(hipEventRecord(ix->ev[4], st));
    q.n_fail = (unsigned int)q.m;
    q.S = 0;
    snprintf(ix->last.kernel, sizeof(ix->last.kernel), "exact_dist_rows_kernel + exact_select_rows_kernel (float64 brute force)");
    return NABO_OK;
}

// One of the two launches of a filter pass (plan_l2): the main launch, and the tail round of workgroups with its own split
// count.  Each has its own candidate lists, tournament seeds and merged lists.
struct L2Part {
    int64_t gx, row0, rows;          // column-workgroups, first target row, target rows (padded)
    int S;                           // reference splits
    int64_t tps;                     // reference tiles per split
    DevBuf *idx, *tau, *key, *mi, *mt, *pre;    // lists: indices, thresholds, filter keys; merged lists; tournament seeds
    bool merge = false;              // merge_lists_kernel reduces the S lists of a row to one of `keep` entries (lout slots)
    int keep = 0, lout = 0;
    int64_t end(int64_t m) const { return row0 + rows < m ? row0 + rows : m; }
    int64_t wgs(int rows_per_wg) const { return (rows + rows_per_wg - 1) / rows_per_wg; }     // of a plain launch (gx, or fewer: a main part cut on whole rounds of positions)
};

// positions of the bucket-ordered copy of `rows` target rows: whole columns (local_seeds.h)
static int64_t ordered_positions(const nabo_index *ix, int64_t rows) { return lseed_columns(rows, ix->ref.l2.buckets.buckets) * LSEED_COL_ROWS; }

// LOCAL tournament seeds of a one-split launch (local_seeds.hip): the launch's rows sorted by bucket (bucket_sort: a
// bucket-ordered copy of their tiles, for the tournament alone unless the launch streams it) and ONE tournament launch
// whose columns each run over their bucket's references; rows of buckets too small for one keep the stream's first tiles
// (pt, gt: l2c_pre_plan's; pt = 0: no tournament there, those rows start from +inf).  No host wait: counts, layout and
// ranges stay on the device.  sub: the launch streams the copy (two-level) -- its rows are sorted once more inside their
// buckets, by the sub-anchors the ordered references were sorted with (local_seeds.h).
static int local_seeds(nabo_index *ix, const Query &q, const L2Plan &P, L2Part &p, int pt, int gt, bool sub)
{
    const IndexShape &sh = ix->shape;
    auto &l2 = ix->ref.l2;
    auto &out = ix->ws.buckets.rows;
    hipStream_t st = ix->stream;
    int rc;
    const int kc = P.kcq;
    const int64_t nrows = p.end(q.m) - p.row0;
    const int64_t prow = ordered_positions(ix, nrows), ncol = prow / LSEED_COL_ROWS;
    // (a two-level launch reads the copy in whole workgroups: positions up to prow_wg, the ones past prow padding)
    const int64_t prow_wg = (prow + P.rows_per_wg - 1) / P.rows_per_wg * P.rows_per_wg;
    const size_t tile_bytes = (size_t)kc * 1024;
    if ((rc = p.pre->reserve((size_t)p.rows * sizeof(float))) || (rc = out.ordered.reserve((size_t)(prow_wg / 32) * tile_bytes)) ||
        (rc = out.map.reserve((size_t)prow_wg * sizeof(uint32_t))) || (rc = out.column_ranges.reserve((size_t)ncol * 4 * sizeof(int))))
        return rc;
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p.pre->p), 0x7F800000, (size_t)p.rows, st));      // +inf: rows without a tournament
    HIP_TRY(hipMemsetAsync(out.map.p, 0xFF, (size_t)prow_wg * sizeof(uint32_t), st));
    if (prow_wg > prow) HIP_TRY(hipMemsetAsync(out.ordered.as<unsigned char>() + (size_t)(prow / 32) * tile_bytes, 0, (size_t)((prow_wg - prow) / 32) * tile_bytes, st));
    HIP_TRY(hipMemsetAsync(out.column_ranges.p, 0, (size_t)ncol * 4 * sizeof(int), st));
    BucketSort sort;
    sort.rows = true;
    sort.kc = kc;
    sort.cells = ix->ws.xpk.as<unsigned char>() + (size_t)(p.row0 / 32) * tile_bytes;
    sort.ncell = nrows;
    sort.cap = l2.buckets.cap;
    sort.lkeep = P.lkeep;
    sort.tile0 = (int)sh.ref_tiles_alloc;
    sort.rest[1] = (int)p.tps;
    sort.rest[2] = pt;
    sort.rest[3] = pt > 0 ? gt : 0;
    sort.column_ranges = out.column_ranges.as<int>();
    sort.columns = ncol;
    sort.sub = sub ? BucketSort::USE_SUB_ANCHORS : BucketSort::CALLER_ORDER;
    sort.positions = prow;
    sort.dst = out.ordered.as<unsigned char>();
    sort.dst_map = out.map.as<uint32_t>();
    if ((rc = bucket_sort(ix, sort))) return rc;
    HIP_TRY(l2c_pre_launch(kc, P.lkeep, out.ordered.as<unsigned char>(), l2.ycpk1.as<unsigned char>(), (int)p.tps, 1, prow, 0, 0, 2,
                           sh.ref_tiles_alloc - 1, st, prow, p.pre->as<float>(), out.column_ranges.as<int>(), LSEED_COL_ROWS,
                           out.map.as<uint32_t>()));
    return NABO_OK;
}

// What the lists of one launch of the one-product pass start from: one threshold per (row, split) at `stride` per row
// (0: one per row), the reference tiles its tournament looked at, and whether its rows now lie in bucket order for the stream.
struct L2Seeds {
    const float *tau = nullptr;
    int stride = 0, pre_tiles = 0;
    bool ordered = false;
};

// Tournament seeds of one part (l2c_topk.hip: l2c_pre_kernel): every (row, split) list starts from an upper bound of its
// lkeep-th smallest score among some references instead of +inf -- the row's own bucket (local_seeds) where the planner
// takes local seeds, otherwise the split's first references.  stream: a part with local seeds is sorted for the two-level
// stream (the main launch of a plan with tl_main, where the ordered references exist and the verdict allows).
static int part_seeds(nabo_index *ix, const PassCtx &ctx, const Query &q, const L2Plan &P, L2Part &p, int pre_pct, bool stream, L2Seeds *s)
{
    const IndexShape &sh = ix->shape;
    auto &l2 = ix->ref.l2;
    int rc, pt = 0, gt = 2;
    l2c_pre_plan(P.kcq, P.lkeep, (int)p.tps, pre_pct, &pt, &gt);
    if (ctx.first() && p.gx > 0 && lseed_applies(sh, P, p.S, p.end(q.m) - p.row0)) {
        if ((rc = local_seeds(ix, q, P, p, pt, gt, stream && l2.buckets.sub_count > 1))) return rc;
        s->ordered = stream;
    } else {
        if (pt <= 0 || p.gx == 0) return NABO_OK;
        if ((rc = p.pre->reserve((size_t)p.rows * p.S * sizeof(float)))) return rc;
        HIP_TRY(l2c_pre_launch(P.kcq, P.lkeep, ix->ws.xpk.as<unsigned char>(), l2.ycpk1.as<unsigned char>(), (int)p.tps, p.S, p.rows,
                               p.row0 / 32, pt, gt, sh.ref_tiles_alloc - 1, ix->stream, q.m, p.pre->as<float>()));
    }
    s->tau = p.pre->as<float>();
    s->stride = p.S;
    s->pre_tiles = pt;
    return NABO_OK;
}

// The PROBE of an unknown verdict (two_level_verdict.h: when it is due, and what its counters mean): the ordered main
// launch's first workgroups over the stream's first tiles, as it always ran -- no progress window.  Its lists are scratch:
// the launch proper writes every row again.  One host wait.
static int probe_stream(nabo_index *ix, const L2Plan &P, L2Part &p, const L2Seeds &seed, int64_t prow, const L2cOrdered &ord)
{
    auto &l2 = ix->ref.l2;
    auto &in = ix->ws.buckets.rows;
    hipStream_t st = ix->stream;
    unsigned long long probe[3] = {0, 0, 0};
    L2cOrdered pord = ord;
    pord.window = -1;
    pord.runs = nullptr;
    HIP_TRY(hipMemsetAsync(in.tile_counters.p, 0, 4 * sizeof(unsigned long long), st));
    HIP_TRY(l2c_topk_launch(P.kcq, P.geo, in.ordered.as<unsigned char>(), l2.buckets.ordered.as<unsigned char>(), TL_PROBE_TILES, 1,
                            TL_PROBE_WORKGROUPS, 0, P.lkeep, p.idx->as<uint32_t>(), nullptr, p.tau->as<float>(), l2.buckets.ordered_tiles, st,
                            prow, seed.tau, seed.stride, 0, &pord));
    HIP_TRY(hipMemcpyAsync(probe, in.tile_counters.p, sizeof(probe), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
#ifdef NABO_TL_TRACE        // (a build of its own, _build.py --out ... -DNABO_TL_TRACE: the probe's counters, for the records)
    fprintf(stderr, "two-level probe: one-step %llu, refetched %llu, two-step %llu\n", probe[0], probe[1], probe[2]);
#endif
    l2.stream_verdict.give(tl_probe_verdict(probe[0], probe[2]));
    return NABO_OK;
}

// The ordered main launch of the two-level stream.  Targets: the bucket-ordered copy local_seeds made (whole workgroups of
// positions); references: the ordered copy and its two padding tiles; lists and seeds by the launch's rows, candidates as
// reference indices.
static int stream_launch(nabo_index *ix, const L2Plan &P, L2Part &p, const L2Seeds &seed, int64_t prow, const L2cOrdered &ord)
{
    auto &l2 = ix->ref.l2;
    auto &in = ix->ws.buckets.rows;
    hipStream_t st = ix->stream;
    HIP_TRY(hipMemsetAsync(in.tile_counters.p, 0, 4 * sizeof(unsigned long long), st));
    HIP_TRY(l2c_topk_launch(P.kcq, P.geo, in.ordered.as<unsigned char>(), l2.buckets.ordered.as<unsigned char>(), (int)l2.buckets.ordered_tiles, 1,
                            (int)((prow + P.rows_per_wg - 1) / P.rows_per_wg), 0, P.lkeep, p.idx->as<uint32_t>(),
                            p.merge ? p.key->as<float>() : nullptr, p.tau->as<float>(), l2.buckets.ordered_tiles, st, prow, seed.tau,
                            seed.stride, 0, &ord));
    in.streamed = true;
    in.positions = prow;
    return NABO_OK;
}

// A launch of the one-product kernel over the caller-order operands.  (Rows beyond the part's are padding to it: the main
// part of a plan cut on whole rounds of positions, run in caller order after all, ends inside a workgroup and the tail
// launch takes over there.)
static int plain_launch(nabo_index *ix, const Query &q, const L2Plan &P, L2Part &p, const L2Seeds &seed)
{
    const IndexShape &sh = ix->shape;
    HIP_TRY(l2c_topk_launch(P.kcq, P.geo, ix->ws.xpk.as<unsigned char>(), ix->ref.l2.ycpk1.as<unsigned char>(), (int)p.tps, p.S,
                            (int)p.wgs(P.rows_per_wg), p.row0 / 32, P.lkeep, p.idx->as<uint32_t>(), p.merge ? p.key->as<float>() : nullptr,
                            p.tau->as<float>(), sh.ref_tiles_alloc - 1, ix->stream, p.end(q.m), seed.tau, seed.stride, p.row0));
    return NABO_OK;
}

// The main launch of a part whose rows local_seeds sorted for the stream: behind a probe where one is due, and in caller
// order after all where the probe says no.
static int main_launch_ordered(nabo_index *ix, const Query &q, const L2Plan &P, L2Part &p, const L2Seeds &seed)
{
    const IndexShape &sh = ix->shape;
    auto &l2 = ix->ref.l2;
    auto &in = ix->ws.buckets.rows;
    int rc;
    const int64_t prow = ordered_positions(ix, p.end(q.m) - p.row0);
    if ((rc = in.tile_counters.reserve(4 * sizeof(unsigned long long)))) return rc;
    L2cOrdered ord = {in.map.as<uint32_t>(), l2.buckets.ordered_map.as<uint32_t>(), in.tile_counters.as<unsigned long long>(),
                            sh.opt.two_level_share, sh.opt.two_level_stretch, l2.buckets.bucket_ends.as<int32_t>(), l2.buckets.buckets,
                            sh.opt.two_level_burst, sh.opt.two_level_window, sh.opt.two_level_check, nullptr};
    const int64_t wgs = (prow + P.rows_per_wg - 1) / P.rows_per_wg;
    if (tl_probe_due(l2.stream_verdict, sh.opt.two_level, wgs, l2.buckets.ordered_tiles) && (rc = probe_stream(ix, P, p, seed, prow, ord)))
        return rc;
    if (!l2.stream_verdict.streams()) return plain_launch(ix, q, P, p, seed);
    // The run lists (bucket_skip.h): which stretches of the stream each workgroup's rows can take anything from, from the
    // seeds the tournament just wrote and the buckets the rows' sort left in its keys (no sort runs between the two: a plan
    // with tl_main has no tail launch with local seeds).  On the query's stream, no host wait.
    const BucketRefs &b = l2.buckets;
    if (P.tl_skip && b.skip_built && seed.tau && seed.stride == 1) {
        if ((rc = in.runs.reserve((size_t)wgs * BSKIP_RUN_INTS * sizeof(int32_t)))) return rc;
        HIP_TRY(bskip_runs_launch(q.dXp + (size_t)p.row0 * sh.g, l2.centre.as<double>(), l2.hscale, sh.g, b.buckets, b.sub_count, in.map.as<uint32_t>(),
                                  ix->ws.buckets.keys.as<uint32_t>(), seed.tau, b.skip_by_from.as<double>(), b.skip_ymin.as<float>(),
                                  b.skip_t0.as<int32_t>(), b.skip_t1.as<int32_t>(), b.ordered_tiles, wgs, in.runs.as<int32_t>(), ix->stream));
        ord.runs = in.runs.as<int32_t>();
    }
    return stream_launch(ix, P, p, seed, prow, ord);
}

// The filter kernels of a pass, main launch then tail: the one-product kernel behind its tournament seeds (l2c_topk.hip),
// or the f16x3 (l2q_topk.hip) / fp32 (l2_topk.hip) filter.  *beside: ev_main was recorded between the two launches -- the
// refine of the main launch's rows runs on the second stream beside the tail launch.
static int l2_filter(nabo_index *ix, const PassCtx &ctx, const Query &q, const L2Plan &P, L2Part (&part)[2], const float *seeds, bool *beside)
{
    const IndexShape &sh = ix->shape;
    auto &l2 = ix->ref.l2;
    auto &ws = ix->ws;
    hipStream_t st = ix->stream;
    int rc;
    *beside = false;
    if (!P.on_l2c) {
        const int64_t pad_tile = sh.ref_tiles_alloc - 1;
        for (L2Part &p : part) {
            if (p.gx == 0) continue;
            if (P.use_h)
                HIP_TRY(l2q_topk_launch(P.kcq, ws.xpk.as<unsigned char>(), P.use_1 ? l2.ycpk1.as<unsigned char>() : l2.ycpk.as<unsigned char>(),
                                        (int)p.tps, p.S, (int)p.gx, p.row0 / 32, P.lkeep, p.idx->as<uint32_t>(), nullptr, p.tau->as<float>(),
                                        pad_tile, st));
            else
                HIP_TRY(l2_topk_launch(sh.ksteps, P.r1 ? -1 : q.epl, ws.xpk.as<float>(), l2.ypk.as<float>(), (int)p.tps,
                                       p.S, (int)p.gx, p.row0 / 32, P.lkeep, p.idx->as<uint32_t>(), nullptr,
                                       p.tau->as<float>(), st));
        }
        return NABO_OK;
    }
    L2Part &pmain = part[0], &ptail = part[1];
    // Tournament seeds of both launches first -- not for a pass that has its seeds already.  Option prepass: 0 off,
    // otherwise percent of the planned length (same bits always).
    L2Seeds seed_main, seed_tail;
    seed_main.tau = seed_tail.tau = seeds;
    const int pre_pct = seeds ? 0 : sh.opt.prepass;
    if (pre_pct > 0 &&
        ((rc = part_seeds(ix, ctx, q, P, pmain, pre_pct, P.tl_main && l2.buckets.ordered_built && l2.stream_verdict.streams(), &seed_main)) ||
         (rc = part_seeds(ix, ctx, q, P, ptail, pre_pct, false, &seed_tail))))
        return rc;
    if (ctx.first()) ix->last.pre_tiles_last = seed_main.pre_tiles;
    if (pmain.gx > 0) {
        if ((rc = seed_main.ordered ? main_launch_ordered(ix, q, P, pmain, seed_main) : plain_launch(ix, q, P, pmain, seed_main))) return rc;
        // the tail launch (a fraction of a round, reference splits) leaves most CUs idle: the refine of the main
        // launch's rows (an HBM gather) runs beside it on the second stream
        if (ptail.gx > 0 && !q.cand_mode && sh.opt.refine_overlap != 0) {
            HIP_TRY(hipEventRecord(ix->ev_main, st));
            *beside = true;
        }
    }
    if (ptail.gx > 0 && (rc = plain_launch(ix, q, P, ptail, seed_tail))) return rc;
    return NABO_OK;
}

// The float64 re-evaluation of a pass's lists (refine.hip), main launch then tail, each behind the merge of its lists
// where the pass merges them: certified rows and the fail list, or in candidate mode candidates and bounds.  beside: the
// main launch's part runs on the second stream (l2_filter).
static int l2_refine(nabo_index *ix, const Query &q, const L2Plan &P, L2Part (&part)[2], bool beside, float *fail_seed)
{
    const IndexShape &sh = ix->shape;
    auto &ref = ix->ref;
    auto &l2 = ix->ref.l2;
    auto &ws = ix->ws;
    hipStream_t st = ix->stream;
    // rounding-error coefficient of the filter score, relative to (||x|| + max||y||)^2
    // (f16x3: one fp32 accumulation per product term, 16 per step, plus the dropped lo*lo term and the
    // representation error of the hi + lo split)
    // (one-product pass: the hi x lo, lo x hi and lo x lo terms are INSIDE its score -- the error slot of
    // pack_ctiles_kernel<.,.,1> -- so the same accumulation / representation coefficient applies to its kc1 steps)
    // (two-level slot order: two more terms, -2 tx2 ty and +2 tx2 ty, pass through the fp32 accumulation -- in g + 5 <= 64
    // slots, still 16 kc products, but their magnitudes add 4 tx2 ty <= 4.02 ||x|| ||y|| <= 1.005 (||x|| + ||y||)^2 to the
    // sum of magnitudes the accumulation error scales with: twice the coefficient of the accumulated part)
    const double acc_terms = P.slots2 ? 2.01 * 16.0 * P.kcq : 16.0 * P.kcq;
    const double err_coef = P.use_h ? 1.05 * ((acc_terms + 8.0) * std::ldexp(1.0, -24) + std::ldexp(1.0, -20) + std::ldexp(1.0, -21))
                                    : 1.05 * (2.0 * sh.ksteps + 4.0) * std::ldexp(1.0, -24);
    const double tau_scale = P.use_h ? 1.0 / (l2.hscale * l2.hscale) : 1.0 / (l2.fscale * l2.fscale);
    int rc;
    if ((rc = ymax_resolve(ix))) return rc;
    const double ymax_sqrt = P.use_h ? l2.ymax_sqrt_c : l2.ymax_sqrt;
    const int metric = sh.metric == NABO_METRIC_COSINE ? 2 : 0;
    const int64_t n_valid = sh.n - ref.n_masked;
    auto merge = [&](L2Part &p, hipStream_t s) {
        return merge_lists_launch(p.idx->as<uint32_t>(), p.key->as<float>(), p.tau->as<float>(), p.end(q.m) - p.row0, p.S,
                                  q.L, p.keep, p.lout, p.mi->as<uint32_t>(), p.mt->as<float>(), s);
    };
    // what the float64 step reads: the filter's lists, or ONE merged list per row
    struct Lists { const uint32_t *idx; const float *tau; int S, L; } lists[2];
    for (int i = 0; i < 2; ++i) {
        const L2Part &p = part[i];
        lists[i] = p.merge ? Lists{p.mi->as<uint32_t>(), p.mt->as<float>(), 1, p.lout} : Lists{p.idx->as<uint32_t>(), p.tau->as<float>(), p.S, q.L};
    }
    if (q.cand_mode) {
        for (L2Part &p : part)
            if (p.merge) HIP_TRY(merge(p, st));
        for (int i = 0; i < 2; ++i)
            if (part[i].gx > 0)
                HIP_TRY(refine_cand_launch(q.dX, part[i].row0, part[i].end(q.m), ref.dY, sh.g, lists[i].idx, lists[i].tau,
                                           lists[i].S, lists[i].L, ws.xnorm.as<double>(), err_coef, ymax_sqrt, tau_scale,
                                           q.k, ix->base, n_valid, q.d_oidx, q.d_odist, q.out_bound, st, metric, P.lkeep));
        return NABO_OK;
    }
    for (int i = 0; i < 2; ++i) {
        L2Part &p = part[i];
        if (p.gx == 0) continue;
        hipStream_t s = st;
        if (i == 0 && beside) {
            s = ix->stream2;
            HIP_TRY(hipStreamWaitEvent(s, ix->ev_main, 0));
        }
        if (p.merge) HIP_TRY(merge(p, s));
        HIP_TRY(refine_launch(q.dX, p.row0, p.end(q.m), ref.dY, sh.g, lists[i].idx, lists[i].tau, lists[i].S, lists[i].L,
                              ws.xnorm.as<double>(), err_coef, ymax_sqrt, tau_scale, q.k, q.drop, ix->base, n_valid, ref.mlistbuf.as<uint32_t>(),
                              tail_len(ix), q.d_oidx, q.d_odist, ws.fails.as<uint32_t>(), ws.failcnt.as<unsigned int>(),
                              s, metric, 0.0, 0.0f, p.merge ? p.keep : P.lkeep, nullptr, nullptr, fail_seed));
        if (i == 0 && beside) HIP_TRY(hipEventRecord(ix->ev_ref, s));
    }
    if (beside) HIP_TRY(hipStreamWaitEvent(st, ix->ev_ref, 0));
    return NABO_OK;
}

// The q.n_fail rows of this batch the pass could not certify (ws.fails) go on as a dense batch through query_impl one
// link down the pass chain: at pass level `level` (seeds: level 1's per-row thresholds) or, with `wide`, on 64-entry lists.
// They are gathered into the buffer set `b` of this frame, recorded as pass `code` (pass_rows[slot]), solved and scattered
// back; q.n_fail becomes the rows that still needed the exact kernels.  The inner call reuses ev[0..5]: phases 0-2 of
// this one are kept in q for finish_query.
static int rerun_failed_rows(nabo_index *ix, const PassCtx &ctx, Query &q, int level, bool wide, uint8_t code, int slot,
                             nabo_index::Workspace::RerunBufs &b, const float *seeds)
{
    hipStream_t st = ix->stream;
    const int g = ix->shape.g;
    const int64_t nf = q.n_fail;
    int rc;
    for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&q.ms_keep[i], ix->ev[i], ix->ev[i + 1]));
    if ((rc = b.rows.reserve((size_t)nf * sizeof(uint32_t))) || (rc = b.x.reserve((size_t)nf * g * sizeof(double))) ||
        (rc = b.idx.reserve((size_t)nf * q.k * sizeof(int64_t))) || (rc = b.dist.reserve((size_t)nf * q.k * sizeof(double))))
        return rc;
    HIP_TRY(hipMemcpyAsync(b.rows.p, ix->ws.fails.p, (size_t)nf * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    if (seeds) {
        if ((rc = b.seed.reserve((size_t)nf * sizeof(float)))) return rc;
        HIP_TRY(hipMemcpyAsync(b.seed.p, seeds, (size_t)nf * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(gather_rows_launch(q.dX, b.rows.as<uint32_t>(), nf, g, b.x.as<double>(), st));
    if ((rc = note_row_pass(ix, ctx, b.rows.as<uint32_t>(), nf, code, q.pass_map))) return rc;      // (synchronises the stream)
    // (wide: only ever entered from a frame on 32-entry lists)
    const PassCtx inner{level, wide, seeds ? b.seed.as<float>() : nullptr, &q.pass_map, false, ctx.coarse_weak};
    PassResult res;
    if ((rc = query_impl(ix, inner, b.x.as<double>(), 1, nf, q.k, q.drop, b.idx.as<int64_t>(), b.dist.as<double>(), 1, false,
                         nullptr, &res)))
        return rc;
    ix->last.pass_rows[slot] = nf;
    q.n_fail = res.n_fail;
    q.ms_inner = res.ms;
    q.ms_kept = true;
    HIP_TRY(scatter_rows_launch(b.idx.as<int64_t>(), b.dist.as<double>(), b.rows.as<uint32_t>(), nf, q.k, q.d_oidx,
                                q.d_odist, st));
    HIP_TRY(hipEventRecord(ix->ev[3], st));          // (ev[0..5] were reused by the inner call)
    return NABO_OK;
}

// Euclidean / cosine: plan_l2 -> pack the targets -> filter -> float64 refine and certificate; the rows the pass could not
// certify go one link down the pass chain (rerun_failed_rows) or to the exact kernels.
static int query_l2(nabo_index *ix, const PassCtx &ctx, Query &q)
{
    const IndexShape &sh = ix->shape;
    auto &ref = ix->ref;
    auto &l2 = ix->ref.l2;
    auto &ws = ix->ws;
    hipStream_t st = ix->stream;
    const int g = sh.g;
    const int64_t m = q.m;
    int rc;
    const double *dXp = q.dX;                        // what the filter packs
    if (sh.metric == NABO_METRIC_COSINE) {
        if ((rc = ws.xnbuf.reserve((size_t)m * g * sizeof(double)))) return rc;
        HIP_TRY(normalise_rows_launch(q.dX, m, g, ws.xnbuf.as<double>(), st));
        dXp = ws.xnbuf.as<double>();
    }
    q.dXp = dXp;
    L2Plan P;
    if ((rc = plan_l2(sh, ctx, m, q.k, q.drop, q.cand_mode, &P))) return rc;
    if (ctx.first()) {
        ix->last.pass_rows[0] = ix->last.pass_rows[1] = ix->last.pass_rows[2] = 0;
        snprintf(ix->last.kernel, sizeof(ix->last.kernel), "%s", P.kernel);
        ws.buckets.rows.streamed = false;
    }
    if ((rc = ensure_packed(ix, P.use_1 ? 2 : P.use_h ? 1 : 0))) return rc;
    // (before anything takes the operands' address: a change of options since the pack moves them)
    if (ctx.first() && (lseed_applies(sh, P, P.S, P.rows_main < m ? P.rows_main : m) ||
                          (P.gx_tail > 0 && lseed_applies(sh, P, P.S2, m - P.rows_main))) &&
        (rc = ensure_local_seeds(ix)))
        return rc;
    if (q.top) ix->last.row_pass.assign((size_t)m, (uint8_t)(P.use_1 ? NABO_PASS_ONE_PRODUCT : NABO_PASS_SECOND));
    // (the tail launch begins at row P.rows_main: whole workgroups of the main launch, or fewer rows where the two-level
    // main launch ends on whole rounds of POSITIONS, plan.hip)
    const int64_t rows_main = P.rows_main;
    L2Part part[2] = {
        {P.gx_main, 0, rows_main, P.S, P.tps, &ws.cand_idx, &ws.cand_tau, &ws.cand_key, &ws.cand_mi, &ws.cand_mt, &ws.taupre},
        {P.gx_tail, rows_main, P.gx_tail * P.rows_per_wg, P.S2, P.tps2, &ws.cand_idx2, &ws.cand_tau2, &ws.cand_key2,
         &ws.cand_mi2, &ws.cand_mt2, &ws.taupre2}};
    // Several lists per row (reference splits, the tail round): the l2c kernel also emits the entries' filter keys and
    // merge_lists_kernel reduces the lists to the ONE a single stream would have kept (refine.hip)
    // (first pass only: a seeded pass WANTS every list re-evaluated -- its rows have more than one list's worth of
    // references below their seeds: cosine d = 100, k = 50 with the merge there: 86 instead of 16 ms of later passes)
    // ... the SEEDED pass keeps up to 128: what lies below a seed is "a few more than one list", and
    // 128 candidates are two per lane for the float64 step where S x 32 were four to sixteen per lane, each walking
    // its own row (100k x 100k: refine of 108 rows' 1024 candidates 0.41 ms)
    const bool seeded_merge = ctx.pass_level == 1 && !ctx.wide_retry;          // (32- and 64-entry lists alike)
    const bool merging = P.on_l2c && sh.opt.merge_lists != 0 && !ctx.wide_retry && (ctx.pass_level == 0 || seeded_merge);
    const size_t xtile_bytes = P.use_h ? (size_t)P.kcq * 1024 : (size_t)((sh.ksteps + 3) / 4) * 256 * sizeof(float);
    if ((rc = ws.xpk.reserve((size_t)(P.rows_pad / 32) * xtile_bytes))) return rc;
    if ((rc = ws.xnorm.reserve((size_t)m * sizeof(double)))) return rc;
    for (L2Part &p : part) {
        if (p.gx == 0) continue;
        p.merge = merging && p.S > 1;
        p.keep = seeded_merge ? (p.S * q.L < 128 ? p.S * q.L : 128) : P.lkeep;
        p.lout = seeded_merge ? p.keep : q.L;
        // (whole workgroups: a plain launch writes the lists of all its rows, and a main part cut on whole rounds of
        // positions is no multiple of a workgroup's rows)
        const size_t rows_wg = (size_t)(p.wgs(P.rows_per_wg) * P.rows_per_wg);
        if ((rc = p.idx->reserve(rows_wg * p.S * q.L * sizeof(uint32_t) + 16))) return rc;
        if ((rc = p.tau->reserve(rows_wg * p.S * sizeof(float) + 16))) return rc;
        if (p.merge && ((rc = p.key->reserve(rows_wg * p.S * q.L * sizeof(float))) ||
                        (rc = p.mi->reserve((size_t)p.rows * p.lout * sizeof(uint32_t))) ||
                        (rc = p.mt->reserve((size_t)p.rows * sizeof(float)))))
            return rc;
    }
    if ((rc = ws.fails.reserve((size_t)m * sizeof(uint32_t)))) return rc;
    if ((rc = ws.failcnt.reserve(sizeof(unsigned int)))) return rc;
    HIP_TRY(hipMemsetAsync(ws.failcnt.p, 0, sizeof(unsigned int), st));
    if (P.use_h)
        HIP_TRY(pack_cquery_launch(dXp, m, g, l2.centre.as<double>(), l2.hscale, P.kcq, P.rows_pad / 32,
                                   ws.xpk.as<unsigned char>(), ws.xnorm.as<double>(), true, st, nullptr,
                                   P.use_1 ? (P.slots2 ? 2 : 1) : 3));
    else
        HIP_TRY(pack_query_launch(dXp, m, g, l2.centre.as<double>(), l2.fscale, sh.ksteps, P.rows_pad / 32,
                                  ws.xpk.as<float>(), ws.xnorm.as<double>(), st));
    HIP_TRY(hipEventRecord(ix->ev[1], st));
    // the l2c kernel ran: its failed rows can go through a seeded pass
    const bool seedable = P.on_l2c && !q.cand_mode && sh.opt.seeded_pass != 0;
    bool beside = false;
    if ((rc = l2_filter(ix, ctx, q, P, part, (seedable && ctx.pass_level == 1) ? ctx.seed_tau : nullptr, &beside))) return rc;
    HIP_TRY(hipEventRecord(ix->ev[2], st));
    float *fail_seed = nullptr;          // seeds for a seeded pass of the rows that fail (pass 0 on the l2c kernel)
    if (seedable && ctx.pass_level == 0) {
        if ((rc = ws.failseed.reserve((size_t)m * sizeof(float)))) return rc;
        fail_seed = ws.failseed.as<float>();
    }
    if ((rc = l2_refine(ix, q, P, part, beside, fail_seed))) return rc;
    HIP_TRY(hipEventRecord(ix->ev[3], st));
    q.S = P.S;
    q.n_wg = P.gx_main * P.S + P.gx_tail * P.S2;
    if (q.cand_mode) {
        HIP_TRY(hipEventRecord(ix->ev[4], st));
        return NABO_OK;
    }
    HIP_TRY(hipMemcpyAsync(&q.n_fail, ws.failcnt.p, sizeof(q.n_fail), hipMemcpyDeviceToHost, st));
    unsigned long long tl_tiles[4] = {0, 0, 0, 0};
    const bool tl_ran = ctx.first() && ws.buckets.rows.streamed;
    if (tl_ran) HIP_TRY(hipMemcpyAsync(tl_tiles, ws.buckets.rows.tile_counters.p, sizeof(tl_tiles), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (tl_ran) {
        // the two-level launch's tile counters: into the record (the kernel string carries them to nabo_index_last_kernel),
        // and the memory of a poor outcome: the next queries take the caller-order stream (two_level_verdict.h)
        const size_t len = strlen(ix->last.kernel);
        snprintf(ix->last.kernel + len, sizeof(ix->last.kernel) - len, " [two-level tiles: one-step %lld, refetched %lld, two-step %lld, skipped %lld]",
                 (long long)tl_tiles[0], (long long)tl_tiles[1], (long long)tl_tiles[2], (long long)tl_tiles[3]);
        // (a skipped tile is a tile that did not need its second step: it counts with the one-step tiles)
        if (tl_launch_says_no(m, sh.opt.coarse_adapt, tl_tiles[0] + tl_tiles[3], tl_tiles[2])) l2.stream_verdict.give(TwoLevelVerdict::CALLER_ORDER);
    }
    if (P.use_1 && q.n_fail > 0) {
        // Rows this one-product pass could not certify: from level 0 on the l2c kernel to the SEEDED one-product pass
        // (level 1: every row starts from the threshold refine.hip derived from its failed certificate), otherwise to
        // the f16x3 pass (level 2), which sends what IT cannot certify on to the 64-entry lists / the exact kernels.
        const int here = ctx.pass_level, next = (here == 0 && fail_seed) ? 1 : 2;
        if ((rc = rerun_failed_rows(ix, ctx, q, next, false, next == 1 ? NABO_PASS_SEEDED : NABO_PASS_SECOND, next - 1, ws.rerun[here],
                                    next == 1 ? fail_seed : nullptr)))
            return rc;
        if (here == 0 && m >= 1024 && ix->last.pass_rows[1] > m / 4) l2.coarse_weak = true;
    } else if (q.n_fail >= 16 && q.epl == 1 && !ctx.wide_retry && sh.opt.wide_retry != 0) {
        // Second chance: rows the 32-entry lists could not certify (ties / near-ties reaching past the kept
        // entries) go through the same filter once more with 64-entry lists before anything is brute-forced.
        if ((rc = rerun_failed_rows(ix, ctx, q, ctx.pass_level, true, NABO_PASS_WIDE, 2, ws.rerun[RERUN_WIDE], nullptr))) return rc;
    } else if (q.n_fail > 0) {
        unsigned int d_rows = 0;
        if ((rc = reserve_exact_ws(ix, q.n_fail, 65535, &d_rows))) return rc;
        if ((rc = note_row_pass(ix, ctx, ws.fails.as<uint32_t>(), q.n_fail, (uint8_t)NABO_PASS_EXACT, q.pass_map))) return rc;
        HIP_TRY(exact_rows_launch(q.dX, ref.dY, sh.n, g, sh.metric, ix->f, ref.dmask, ws.fails.as<uint32_t>(), q.n_fail,
                                  q.k, q.drop, ix->base, ref.mlistbuf.as<uint32_t>(), tail_len(ix), q.d_oidx, q.d_odist,
                                  ws.exact_d.as<double>(), d_rows, st));
    }
    HIP_TRY(hipEventRecord(ix->ev[4], st));
    return NABO_OK;
}

// The counting pass -> float64 refine + certificate -> exact re-solve of the uncertified rows.  *done stays false when
// the targets do not fit fp32: the exact kernel then answers every row.
static int canberra_filter(nabo_index *ix, const PassCtx &ctx, Query &q, const CbPlan &C, bool *done)
{
    const IndexShape &sh = ix->shape;
    auto &ref = ix->ref;
    auto &cb = ix->ref.cb;
    auto &ws = ix->ws;
    hipStream_t st = ix->stream;
    const int g = sh.g, gp = cb.gp;
    const int64_t m = q.m, n_valid = sh.n - ref.n_masked;
    int rc;
    float slack, plateau;
    cbf_constants(g, &slack, &plateau);
    if (C.bits) snprintf(ix->last.kernel, sizeof(ix->last.kernel), "cbb_filter_kernel<%d> (bit-sliced count on %d-bucket bitmaps + fp32 lower bound)", gp, cbb_buckets());
    else snprintf(ix->last.kernel, sizeof(ix->last.kernel), "cbf_filter_kernel<%d> (7-bit integer count + fp32 lower bound)", gp);
    struct { int64_t row0, rows; int SL; DevBuf *idx, *tau; } part[2] = {
        {0, C.rows_main, C.Sf * C.lists, &ws.cand_idx, &ws.cand_tau},
        {C.rows_main, m - C.rows_main, C.S2 * C.lists, &ws.cand_idx2, &ws.cand_tau2}};
    if ((rc = ws.xpk.reserve((size_t)m * gp * 2 * sizeof(float)))) return rc;
    if ((rc = ws.xh.reserve((size_t)m * gp * 2))) return rc;
    for (auto &p : part)
        if (p.rows > 0 && ((rc = p.idx->reserve((size_t)p.rows * p.SL * q.L * sizeof(uint32_t))) ||
                           (rc = p.tau->reserve((size_t)p.rows * p.SL * sizeof(float) + 16))))
            return rc;
    if ((rc = ws.fails.reserve((size_t)m * sizeof(uint32_t)))) return rc;
    HIP_TRY(hipMemsetAsync(cb.cbflag.p, 0, 4 * sizeof(unsigned int), st));
    unsigned int *d_failcnt = cb.cbflag.as<unsigned int>() + 1, *d_flag = cb.cbflag.as<unsigned int>();
    HIP_TRY(cbf_pack_targets_launch(q.dX, m, g, gp, ix->f, ws.xpk.as<float>(), d_flag, st));
    if (C.bits) {
        if ((rc = ws.cbrow.reserve((size_t)m * gp * sizeof(uint16_t)))) return rc;
        HIP_TRY(cbb_pack_targets_launch(q.dX, m, g, gp, ix->f, cb.cbedges.as<double>(), ws.cbrow.as<uint16_t>(), st));
    } else {
        HIP_TRY(cbf_pack_targets8_launch(q.dX, m, g, gp, ix->f, cb.cbscale.as<double>(), ws.xh.p, st));
    }
    HIP_TRY(hipEventRecord(ix->ev[1], st));
    for (auto &p : part) {
        if (p.rows == 0) continue;
        const float *xq = ws.xpk.as<float>() + (size_t)p.row0 * gp * 2;
        if (C.bits)
            HIP_TRY(cbb_filter_launch(gp, xq, ws.cbrow.as<uint16_t>() + (size_t)p.row0 * gp, p.rows, cb.yrow.as<float>(),
                                      cb.cbtab.as<uint32_t>(), cb.cbvalid.as<uint32_t>(), sh.n, g, p.SL / C.lists,
                                      p.idx->as<uint32_t>(), p.tau->as<float>(), st));
        else
            HIP_TRY(cbf_filter_launch(gp, q.epl, xq, ws.xh.as<unsigned char>() + (size_t)p.row0 * gp * 2, p.rows,
                                      cb.yrow.as<float>(), cb.ych.p, sh.n, g, ref.dmask, p.SL / C.lists,
                                      p.idx->as<uint32_t>(), p.tau->as<float>(), st));
    }
    HIP_TRY(hipEventRecord(ix->ev[2], st));
    for (auto &p : part)
        if (p.rows > 0)
            HIP_TRY(refine_launch(q.dX, p.row0, p.row0 + p.rows, ref.dY, g, p.idx->as<uint32_t>(), p.tau->as<float>(), p.SL,
                                  q.L, nullptr, 0.0, 0.0, 1.0, q.k, q.drop, ix->base, n_valid, ref.mlistbuf.as<uint32_t>(),
                                  tail_len(ix), q.d_oidx, q.d_odist, ws.fails.as<uint32_t>(), d_failcnt, st, 1, ix->f,
                                  plateau));
    HIP_TRY(hipEventRecord(ix->ev[3], st));
    unsigned int hf[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(hf, cb.cbflag.p, sizeof(hf), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hf[0] != 0) return NABO_OK;                  // targets do not fit fp32
    q.n_fail = hf[1];
    if (q.top) {
        ix->last.row_pass.assign((size_t)m, (uint8_t)NABO_PASS_CANBERRA);
        if ((rc = note_row_pass(ix, ctx, ws.fails.as<uint32_t>(), q.n_fail, (uint8_t)NABO_PASS_EXACT, q.pass_map))) return rc;
    }
    if (q.n_fail > 0) {                              // (the buffers of the 64-entry-list rerun: this route has none)
        const int64_t nf = q.n_fail;
        const int S3 = cb_exact_splits((nf + 63) / 64, (sh.n + 63) / 64);
        nabo_index::Workspace::RerunBufs &b = ws.rerun[RERUN_WIDE];      // (borrowed: this route never reruns rows)
        if ((rc = b.x.reserve((size_t)nf * g * sizeof(double))) || (rc = ws.cand_d.reserve((size_t)nf * S3 * q.L * sizeof(double))) ||
            (rc = ws.cand_idx2.reserve((size_t)nf * S3 * q.L * sizeof(uint32_t))) ||
            (rc = b.idx.reserve((size_t)nf * q.k * sizeof(int64_t))) || (rc = b.dist.reserve((size_t)nf * q.k * sizeof(double))))
            return rc;
        HIP_TRY(gather_rows_launch(q.dX, ws.fails.as<uint32_t>(), nf, g, b.x.as<double>(), st));
        HIP_TRY(canberra_topk_launch(q.epl, b.x.as<double>(), nf, cb.yt.as<double>(), sh.n, g, ix->f, ref.dmask, S3,
                                     ws.cand_d.as<double>(), ws.cand_idx2.as<uint32_t>(), st));
        HIP_TRY(merge_local_launch(ws.cand_d.as<double>(), ws.cand_idx2.as<uint32_t>(), nf, S3 * q.L, q.k, q.drop,
                                   ix->base, b.idx.as<int64_t>(), b.dist.as<double>(), nullptr, st));
        HIP_TRY(scatter_rows_launch(b.idx.as<int64_t>(), b.dist.as<double>(), ws.fails.as<uint32_t>(), nf, q.k,
                                    q.d_oidx, q.d_odist, st));
    }
    HIP_TRY(hipEventRecord(ix->ev[4], st));
    *done = true;
    return NABO_OK;
}

// Modified Canberra: the counting pass where the references have one (canberra_filter), otherwise -- or when too few
// references are unmasked -- the exact kernel for every row.
static int query_canberra(nabo_index *ix, const PassCtx &ctx, Query &q)
{
    const IndexShape &sh = ix->shape;
    auto &ref = ix->ref;
    auto &cb = ix->ref.cb;
    auto &ws = ix->ws;
    hipStream_t st = ix->stream;
    int rc;
    CbPlan C;
    plan_canberra(sh, q.m, q.epl, &C);
    snprintf(ix->last.kernel, sizeof(ix->last.kernel), "canberra_topk_kernel (float64)");
    if (q.top) ix->last.row_pass.assign((size_t)q.m, (uint8_t)NABO_PASS_EXACT);
    const int64_t n_valid = sh.n - ref.n_masked;
    bool done = false;
    if (cb.f32 && n_valid >= q.kk && (rc = canberra_filter(ix, ctx, q, C, &done))) return rc;
    q.S = done ? C.Sf : C.S_exact;
    q.n_wg = C.gx_exact * q.S;
    if (done) return NABO_OK;
    const int S = C.S_exact;
    if ((rc = ws.cand_d.reserve((size_t)q.m * S * q.L * sizeof(double))) ||
        (rc = ws.cand_idx.reserve((size_t)q.m * S * q.L * sizeof(uint32_t))))
        return rc;
    HIP_TRY(hipEventRecord(ix->ev[1], st));
    HIP_TRY(canberra_topk_launch(q.epl, q.dX, q.m, cb.yt.as<double>(), sh.n, sh.g, ix->f, ref.dmask, S,
                                 ws.cand_d.as<double>(), ws.cand_idx.as<uint32_t>(), st));
    HIP_TRY(hipEventRecord(ix->ev[2], st));
    HIP_TRY(merge_local_launch(ws.cand_d.as<double>(), ws.cand_idx.as<uint32_t>(), q.m, S * q.L, q.k, q.drop, ix->base,
                               q.d_oidx, q.d_odist, nullptr, st));
    HIP_TRY(hipEventRecord(ix->ev[3], st));
    if (n_valid < q.kk)
        HIP_TRY(masked_tail_launch(q.dX, q.m, ref.dY, sh.g, sh.metric, ix->f, ref.mlistbuf.as<uint32_t>(), tail_len(ix),
                                   (int)n_valid, q.k, q.drop, ix->base, q.d_oidx, q.d_odist, st));
    HIP_TRY(hipEventRecord(ix->ev[4], st));
    return NABO_OK;
}

// Copy-out, the phases of the query (ev[0..5] -> ms[0..4]), its counters and what an outer frame reads of it (*res).  A query that reran rows one level down
// (rerun_failed_rows) kept its phases 0-2 from before the inner call, whose total stands in for phase 3.
static int finish_query(nabo_index *ix, const Query &q, int64_t *out_idx, double *out_dist, int32_t out_on_device,
                        PassResult *res)
{
    hipStream_t st = ix->stream;
    if (!out_on_device) {
        const size_t ob = (size_t)q.m * q.k * 8;
        HIP_TRY(hipMemcpyAsync(out_idx, q.d_oidx, ob, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_dist, q.d_odist, ob, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipEventRecord(ix->ev[5], st));
    HIP_TRY(hipStreamSynchronize(st));
    float t = 0;
    for (int i = 0; i < 4; ++i) {
        HIP_TRY(hipEventElapsedTime(&t, ix->ev[i], ix->ev[i + 1]));
        ix->last.ms[i] = t;
    }
    HIP_TRY(hipEventElapsedTime(&t, ix->ev[0], ix->ev[5]));
    ix->last.ms[4] = t;
    if (q.ms_kept) {
        HIP_TRY(hipEventElapsedTime(&t, ix->ev[3], ix->ev[5]));
        for (int i = 0; i < 3; ++i) ix->last.ms[i] = q.ms_keep[i];
        ix->last.ms[3] = q.ms_inner + t;                // inner pass (its own total) + scatter / copy-out
        ix->last.ms[4] = ix->last.ms[0] + ix->last.ms[1] + ix->last.ms[2] + ix->last.ms[3];
    }
    ix->last.counters[0] = q.n_fail; ix->last.counters[1] = q.S; ix->last.counters[2] = q.L; ix->last.counters[3] = q.n_wg;
    res->n_fail = q.n_fail;
    res->ms = ix->last.ms[4];
    return NABO_OK;
}

// cand_mode: shard mode of nabo_index_query_candidates -- k is the number of candidates per row to emit,
// out_bound [m] receives the squared-distance bound of everything not emitted; no local certification.
static int query_body(nabo_index *ix, const PassCtx &ctx, const double *X, int32_t x_on_device, int64_t m, int32_t k,
                      int32_t drop_first, int64_t *out_idx, double *out_dist, int32_t out_on_device, bool cand_mode,
                      double *out_bound, PassResult *res)
{
    const IndexShape &sh = ix->shape;
    auto &ref = ix->ref;
    auto &ws = ix->ws;
    if (!ix || !X || !out_idx || !out_dist) return api_fail(NABO_E_INVALID, "NULL argument");
    if (!ref.have) return api_fail(NABO_E_INVALID, "nabo_index_set_ref has not been called");
    if (m < 0) return api_fail(NABO_E_INVALID, "m=%lld must be >= 0", (long long)m);
    if (m == 0) return NABO_OK;                      // no target cells: nothing to do (reference loops are empty)
    const int drop = drop_first ? 1 : 0;
    const int kk = k + drop;
    if (k < 1) return api_fail(NABO_E_INVALID, "k=%d must be >= 1", k);
    if (kk > sh.n && !cand_mode)
        return api_fail(NABO_E_INVALID, "k + drop_first = %d exceeds the %lld references", kk, (long long)sh.n);
    if (cand_mode && (sh.metric == NABO_METRIC_MOD_CANBERRA || !out_bound || !out_on_device || k > 32))
        return api_fail(NABO_E_INVALID, "candidate mode: Euclidean or cosine metric, device outputs, <= 32 candidates");
    // Shapes outside the instantiated filter kernels (k' > NABO_MAX_K, g > NABO_MAX_COMPS) are answered by the exact
    // float64 kernels for every row: the reference accepts any k / use_comps (nabo/_mapping.py:495-524).
    const bool exact_route = kk > NABO_MAX_K || (sh.metric != NABO_METRIC_MOD_CANBERRA && sh.ksteps < 0);
    if (exact_route && cand_mode)
        return api_fail(NABO_E_UNSUPPORTED, "candidate mode needs g <= %d (got %d)", NABO_MAX_COMPS, sh.g);
    int rc = use_device(ix->device);
    if (rc) return rc;
    hipStream_t st = ix->stream;
    Query q;
    q.m = m; q.k = k; q.drop = drop; q.kk = kk;
    q.epl = list_epl(ctx, kk, cand_mode);
    q.L = 32 * q.epl;
    q.cand_mode = cand_mode; q.out_bound = out_bound;
    q.top = ctx.top && !cand_mode;
    // operands / results on device
    q.dX = X;
    if (!x_on_device) {
        const size_t xb = (size_t)m * sh.g * sizeof(double);
        if ((rc = ws.xbuf.reserve(xb))) return rc;
        HIP_TRY(hipMemcpyAsync(ws.xbuf.p, X, xb, hipMemcpyHostToDevice, st));
        q.dX = ws.xbuf.as<double>();
    }
    q.d_oidx = out_idx;
    q.d_odist = out_dist;
    if (!out_on_device) {
        const size_t ob = (size_t)m * k * 8;
        if ((rc = ws.oidx.reserve(ob)) || (rc = ws.odist.reserve(ob))) return rc;
        q.d_oidx = ws.oidx.as<int64_t>();
        q.d_odist = ws.odist.as<double>();
    }
    HIP_TRY(hipEventRecord(ix->ev[0], st));
    rc = exact_route ? query_exact(ix, q) : sh.metric != NABO_METRIC_MOD_CANBERRA ? query_l2(ix, ctx, q) : query_canberra(ix, ctx, q);
    if (rc) return rc;
    return finish_query(ix, q, out_idx, out_dist, out_on_device, res);
}

int query_impl(nabo_index *ix, const PassCtx &ctx, const double *X, int32_t x_on_device, int64_t m, int32_t k, int32_t drop_first,
               int64_t *out_idx, double *out_dist, int32_t out_on_device, bool cand_mode, double *out_bound, PassResult *res)
{
    if (!ix) return api_fail(NABO_E_INVALID, "NULL argument");
    if (ctx.top) ix->last.row_pass.clear();          // a top-level query: the per-row record starts over
    return query_body(ix, ctx, X, x_on_device, m, k, drop_first, out_idx, out_dist, out_on_device, cand_mode, out_bound, res);
}

}  // namespace nabo

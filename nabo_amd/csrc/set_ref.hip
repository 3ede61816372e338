// set_ref.hip -- the resident references of an index: the mask, the packed operands of the Euclidean / cosine filters
// (ensure_packed) and of the modified-Canberra counting passes, nabo_index_set_ref and nabo_index_set_mask.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "bucket_skip.h"
#include "index.h"
#include "local_seeds.h"

namespace nabo {

// Pack the resident references for the fp32-MFMA kernel (want = 0), the f16x3 kernels (1: K-concatenated f16 tiles) or
// the one-product pass of the l2q kernel (2).
int ensure_packed(nabo_index *ix, int want)
{
    const IndexShape &sh = ix->shape;
    auto &ref = ix->ref;
    auto &l2 = ix->ref.l2;
    const bool want_h = want != 0;
    // (option two_level changed since the pack: the one-product operands are in the other slot order)
    if (want == 2 && l2.packed_c1 && l2.slots2 != two_level_slots(sh)) l2.packed_c1 = false;
    if (want == 2 ? l2.packed_c1 : want == 1 ? l2.packed_c16 : l2.packed_f32) return NABO_OK;
    hipStream_t st = ix->stream;
    int rc;
    if ((rc = ymax_resolve(ix))) return rc;                   // (a pack of other operands still owes its norm: normmax is reused)
    // normmax: [0] = max ||y~||^2 (float bits, SCALED units), [2..3] = max |y~ component| (double bits)
    if ((rc = l2.normmax.reserve(4 * sizeof(unsigned int)))) return rc;
    HIP_TRY(hipMemsetAsync(l2.normmax.p, 0, 4 * sizeof(unsigned int), st));
    unsigned int bits[4] = {0, 0, 0, 0};
    // power-of-two input scale from the largest centred component: the filter then works in a fixed numeric range
    // whatever the unit of the data (1e-30 or 1e+19 per component would under- / overflow fp32 squares otherwise)
    HIP_TRY(maxabs_launch(l2.dYp, sh.n, sh.g, l2.centre.as<double>(),
                          reinterpret_cast<unsigned long long *>(l2.normmax.as<unsigned int>() + 2), st));
    HIP_TRY(hipMemcpyAsync(bits, l2.normmax.p, sizeof(bits), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    double amax;
    memcpy(&amax, &bits[2], sizeof(amax));
    int e2 = 0;                                              // 2^e2 * amax in (1/2, 1]
    if (amax > 0 && std::isfinite(amax)) e2 = -(int)std::ceil(std::log2(amax));
    if (e2 > 480) e2 = 480;                                  // scale^2 must stay finite in float64
    if (e2 < -480) e2 = -480;
    double scale;
    if (want == 2) {
        // (behind the stream: the runs of the local tournament seeds, ensure_local_seeds)
        int lc = 0, lcap = 0;
        lseed_params(sh, &lc, &lcap);
        l2.buckets.runs_room = (int64_t)lc * (lcap / 32);
        l2.buckets.runs_built = l2.buckets.ordered_built = l2.buckets.skip_built = false;
        l2.slots2 = two_level_slots(sh);
        if ((rc = l2.ycpk1.reserve((size_t)(sh.ref_tiles_alloc + l2.buckets.runs_room) * sh.kc1 * 1024 + 128))) return rc;
        l2.hscale = scale = std::ldexp(1.0, e2 + 12);
        HIP_TRY(pack_cref_launch(l2.dYp, sh.n, sh.g, l2.centre.as<double>(), l2.hscale, sh.kc1,
                                 sh.ref_tiles_alloc, ref.dmask, l2.ycpk1.as<unsigned char>(),
                                 l2.normmax.as<unsigned int>(), true, st, nullptr, l2.slots2 ? 2 : 1));
    } else if (want_h) {
        if ((rc = l2.ycpk.reserve((size_t)sh.ref_tiles_alloc * sh.kc * 1024 + 128))) return rc;
        // |v| <= 2^12 after scaling (f16 overflows at 65504; targets carry a factor 2)
        l2.hscale = scale = std::ldexp(1.0, e2 + 12);
        HIP_TRY(pack_cref_launch(l2.dYp, sh.n, sh.g, l2.centre.as<double>(), l2.hscale, sh.kc,
                                 sh.ref_tiles_alloc, ref.dmask, l2.ycpk.as<unsigned char>(),
                                 l2.normmax.as<unsigned int>(), true, st));
    } else {
        const int Q = (sh.ksteps + 3) / 4;
        const size_t tile_bytes = ((size_t)Q * 256 + 32) * sizeof(float);
        if ((rc = l2.ypk.reserve((size_t)sh.ref_tiles_alloc * tile_bytes))) return rc;
        l2.fscale = scale = std::ldexp(1.0, e2);
        HIP_TRY(pack_ref_launch(l2.dYp, sh.n, sh.g, l2.centre.as<double>(), l2.fscale, sh.ksteps,
                                sh.ref_tiles_alloc, ref.dmask, l2.ypk.as<float>(), l2.normmax.as<unsigned int>(), st));
    }
    // The largest norm is read by nobody before the refine launch takes it as an argument: the copy goes to pinned memory
    // behind the pack and the host goes on enqueueing (target pack, tournament, filter); ymax_resolve waits for it.
    if (!l2.ymax_host) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&l2.ymax_host), sizeof(unsigned int), hipHostMallocDefault));
    HIP_TRY(hipMemcpyAsync(l2.ymax_host, l2.normmax.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(l2.ev_ymax, st));
    l2.ymax_pending = true;
    l2.ymax_f32 = !want_h;
    l2.ymax_scale = scale;
    if (want == 2) l2.packed_c1 = true;
    else if (want_h) l2.packed_c16 = true;
    else l2.packed_f32 = true;
    return NABO_OK;
}

// The bucket order of the references (bucket_order.h) for the index's current options: anchors, the first `cap` unmasked
// cells of every bucket copied behind the one-product operands (the runs of the local tournament seeds) and, for the
// two-level stream, ALL unmasked references in bucket order.  Enqueued on the stream behind the pack; a query that takes
// local seeds calls this first (everything is stale after every repack, and an option may have changed since).
int ensure_local_seeds(nabo_index *ix)
{
    const IndexShape &sh = ix->shape;
    auto &l2 = ix->ref.l2;
    BucketRefs &b = l2.buckets;
    hipStream_t st = ix->stream;
    int rc, C = 0, cap = 0;
    lseed_params(sh, &C, &cap);
    if (C == 0) return NABO_OK;
    if (l2.packed_c1 && l2.slots2 != two_level_slots(sh)) l2.packed_c1 = false;
    const int S = lseed_sub_param(sh), srank = sh.opt.two_level_sub_rank;
    // (a sub-order asked for since the copy was built, or another one: the ordered copy is built again)
    if (b.ordered_built && (b.sub_count != S || (S > 1 && b.sub_rank_rule != srank))) b.ordered_built = false;
    // (the skip tables where an option asks for them now and the copy was built without)
    if (b.ordered_built && !b.skip_built && bskip_wanted(sh)) b.ordered_built = false;
    if (b.runs_built && b.buckets == C && b.cap == cap && l2.packed_c1 && (b.ordered_built || !l2.slots2 || !l2.stream_verdict.streams()))
        return NABO_OK;
    if (!l2.packed_c1 || b.runs_room < (int64_t)C * (cap / 32)) {           // (options changed since the pack: room for the runs)
        l2.packed_c1 = false;
        if ((rc = ensure_packed(ix, 2))) return rc;
    }
    b.runs_built = b.ordered_built = b.skip_built = false;
    b.buckets = C;
    b.cap = cap;
    if ((rc = b.anchors.reserve(lseed_anchor_bytes(sh.kc1, C))) || (rc = b.bucket_count.reserve((size_t)C * sizeof(uint32_t)))) return rc;
    unsigned char *ypk = l2.ycpk1.as<unsigned char>();
    HIP_TRY(lseed_anchors_launch(sh.kc1, ypk, sh.n, sh.g, C, b.anchors.p, st, l2.slots2));
    BucketSort sort;
    sort.kc = sh.kc1;
    sort.cells = ypk;
    sort.ncell = sh.n;
    // (padding positions: a cell of the stream's last tile, which lies beyond the references -- +inf norm)
    sort.pad_cell = (sh.ref_tiles_alloc - 1) * 32;
    sort.cap = cap;
    sort.dst = ypk + (size_t)sh.ref_tiles_alloc * sh.kc1 * 1024;
    if ((rc = bucket_sort(ix, sort))) return rc;
    b.runs_built = true;
    if (!l2.slots2 || !l2.stream_verdict.streams()) return NABO_OK;
    // The two-level stream (not for data that is known not to take it): ALL unmasked references in bucket order (the same
    // keys and block offsets, no cap), every bucket in whole tiles, and the map from position to reference index.  The copy
    // starts as padding cells (+inf norm): what the buckets leave of its ref_tiles + C tiles, and the two tiles behind them
    // the filter's ring reads.  With a sub-order the sub-anchors are drawn from this copy's buckets; the runs of the
    // tournament above were drawn before it: a spread sample of their buckets, as they always were.
    const int64_t ot = lseed_ordered_tiles(sh.ref_tiles, C);
    b.sub_count = S;
    b.sub_rank_rule = srank;
    if ((rc = b.ordered.reserve((size_t)(ot + 2) * sh.kc1 * 1024 + 128)) || (rc = b.ordered_map.reserve((size_t)(ot + 2) * 32 * sizeof(uint32_t))) ||
        (rc = b.bucket_ends.reserve((size_t)C * sizeof(int32_t))))
        return rc;
    if (S > 1 && ((rc = b.sub_anchors.reserve(lseed_sub_anchor_bytes(sh.kc1, C, S))) || (rc = b.sub_norms.reserve((size_t)C * S * sizeof(float))) ||
                  (rc = b.sub_ranks.reserve((size_t)C * S))))
        return rc;
    HIP_TRY(lseed_fill_launch(sh.kc1, ypk, sort.pad_cell, b.ordered.as<unsigned char>(), (ot + 2) * 32, st));
    HIP_TRY(hipMemsetAsync(b.ordered_map.p, 0xFF, (size_t)(ot + 2) * 32 * sizeof(uint32_t), st));
    sort.assign = false;
    sort.cap = 0;
    sort.bucket_ends = b.bucket_ends.as<int32_t>();
    sort.sub = S > 1 ? BucketSort::BUILD_SUB_ANCHORS : BucketSort::CALLER_ORDER;
    sort.positions = ot * 32;
    sort.dst = b.ordered.as<unsigned char>();
    sort.dst_map = b.ordered_map.as<uint32_t>();
    if ((rc = bucket_sort(ix, sort))) return rc;
    b.ordered_tiles = ot;
    b.ordered_built = true;
    // What the main launch's workgroups skip by (bucket_skip.h), from the layouts the copy was just sorted with -- scratch the
    // next sort overwrites -- and the references' float64 rows; on the same stream, behind the sub-order.
    if (bskip_wanted(sh)) {
        const BucketScratch &ws = ix->ws.buckets;
        const int G = C * S;
        const size_t gi = (size_t)G * sizeof(int32_t);
        if ((rc = b.skip_first.reserve(gi)) || (rc = b.skip_count.reserve(gi)) || (rc = b.skip_t0.reserve(gi)) || (rc = b.skip_t1.reserve(gi)) ||
            (rc = b.skip_means.reserve((size_t)C * sh.g * sizeof(double))) || (rc = b.skip_mean_parts.reserve(bskip_mean_part_bytes(C, sh.g))) || (rc = b.skip_by_from.reserve(bskip_dir_bytes(C, sh.g))) ||
            (rc = b.skip_by_to.reserve(bskip_dir_bytes(C, sh.g))) || (rc = b.skip_ymin.reserve((size_t)C * G * sizeof(float))))
            return rc;
        HIP_TRY(bskip_refs_launch(l2.dYp, l2.centre.as<double>(), l2.hscale, sh.g, C, S, ws.layout.as<int64_t>(), b.bucket_count.as<uint32_t>(),
                                  S > 1 ? ws.sub_layout.as<int64_t>() : nullptr, S > 1 ? ws.sub_totals.as<uint32_t>() : nullptr,
                                  b.ordered_map.as<uint32_t>(), b.skip_first.as<int32_t>(), b.skip_count.as<int32_t>(), b.skip_t0.as<int32_t>(),
                                  b.skip_t1.as<int32_t>(), b.skip_mean_parts.as<double>(), b.skip_means.as<double>(), b.skip_by_from.as<double>(), b.skip_by_to.as<double>(),
                                  b.skip_ymin.as<float>(), st));
        b.skip_groups = G;
        b.skip_built = true;
    }
    return NABO_OK;
}

// ymax_sqrt / ymax_sqrt_c of the last pack, once its copy has arrived (every reader of the two calls this first)
int ymax_resolve(nabo_index *ix)
{
    auto &l2 = ix->ref.l2;
    if (!l2.ymax_pending) return NABO_OK;
    HIP_TRY(hipEventSynchronize(l2.ev_ymax));
    l2.ymax_pending = false;
    float fmax;
    memcpy(&fmax, l2.ymax_host, sizeof(fmax));
    const double v = std::sqrt((double)fmax) / l2.ymax_scale * (1.0 + 1e-6);      // unscaled units
    if (l2.ymax_f32) l2.ymax_sqrt = v;
    else l2.ymax_sqrt_c = v;
    return NABO_OK;
}

// mask + ascending list of the first masked indices (order-row tail, nabo/_mapping.py:135-144)
static int apply_mask(nabo_index *ix, const uint8_t *ref_mask)
{
    const IndexShape &sh = ix->shape;
    auto &ref = ix->ref;
    hipStream_t st = ix->stream;
    int rc;
    ref.dmask = nullptr;
    ref.n_masked = 0;
    ref.n_masked_list = 0;
    if (ref_mask) {
        std::vector<uint32_t> lst;
        for (int64_t j = 0; j < sh.n; ++j)
            if (ref_mask[j]) {
                ++ref.n_masked;
                lst.push_back((uint32_t)j);          // all of them: the exact route serves any k (order-row tail)
            }
        if (ref.n_masked > 0) {
            if ((rc = ref.maskbuf.reserve((size_t)sh.n))) return rc;
            HIP_TRY(hipMemcpyAsync(ref.maskbuf.p, ref_mask, (size_t)sh.n, hipMemcpyHostToDevice, st));
            ref.dmask = ref.maskbuf.as<uint8_t>();
            if ((rc = ref.mlistbuf.reserve(lst.size() * sizeof(uint32_t)))) return rc;
            HIP_TRY(hipMemcpyAsync(ref.mlistbuf.p, lst.data(), lst.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));      // lst goes out of scope
            ref.n_masked_list = (int)lst.size();
        }
    }
    return NABO_OK;
}

// References changed: operands and the pending norm read are stale, the weak-bound memory is cleared; the first pass's
// operands are packed again (masked cells carry ||y||^2 = +inf in the packed tiles)
static int repack_refs(nabo_index *ix)
{
    auto &l2 = ix->ref.l2;
    l2.packed_f32 = l2.packed_c16 = l2.packed_c1 = false;
    l2.ymax_pending = false;                      // (a read still in flight belongs to operands that are gone)
    l2.coarse_weak = false;
    l2.stream_verdict.repack();                   // (the two-level verdict: asked again now and then)
    return ensure_packed(ix, ix->shape.coarse ? 2 : ix->shape.mode == 1 ? 1 : 0);
}

// Euclidean / cosine references: the centre, the unit rows (cosine), the first pass's packed operands
static int prepare_l2(nabo_index *ix)
{
    const IndexShape &sh = ix->shape;
    auto &ref = ix->ref;
    auto &l2 = ix->ref.l2;
    hipStream_t st = ix->stream;
    int rc;
    if ((rc = l2.centre.reserve((size_t)sh.g * sizeof(double)))) return rc;
    if (sh.metric == NABO_METRIC_COSINE) {
        // cosine: the filter sees the unit-length rows x^, y^ and works on ||x^ - y^||^2 = 2 (1 - cos).  That quantity is
        // translation invariant like any Euclidean distance, so the UNIT rows are centred (a shift BEFORE the
        // normalisation would change angles; after it, it only shortens the vectors the error bounds scale with:
        // unit rows of PCA-like data sit in a cap around their mean direction, ||x^ - c|| is a fraction of 1)
        if ((rc = l2.ynbuf.reserve((size_t)sh.n * sh.g * sizeof(double)))) return rc;
        HIP_TRY(normalise_rows_launch(ref.dY, sh.n, sh.g, l2.ynbuf.as<double>(), st));
        if (sh.opt.cosine_centre != 0)
            HIP_TRY(centre_launch(l2.ynbuf.as<double>(), sh.n, sh.g, l2.centre.as<double>(), st));
        else
            HIP_TRY(hipMemsetAsync(l2.centre.p, 0, (size_t)sh.g * sizeof(double), st));
        l2.dYp = l2.ynbuf.as<double>();
    } else {
        HIP_TRY(centre_launch(ref.dY, sh.n, sh.g, l2.centre.as<double>(), st));
        l2.dYp = ref.dY;
    }
    return repack_refs(ix);
}

// Bit-sliced counting pass (canberra_bits.hip): per-dimension QUANTILE bucket edges from a strided sample of the references
// (any edges give correct results -- they only decide how sharp the count is), cumulative bitmaps per block of 2048
// references.
static int build_bitmaps(nabo_index *ix)
{
    auto &ref = ix->ref;
    auto &cb = ix->ref.cb;
    hipStream_t st = ix->stream;
    const int64_t n = ix->shape.n;
    const int G = ix->shape.g, B = cbb_buckets();
    int rc;
    int64_t ns = n < 2048 ? n : 2048;          // (32 sample values per bucket; the sort is host time inside set_ref)
    const int64_t stride = n / ns;
    std::vector<double> smp((size_t)ns * G), edges((size_t)G * (B - 1));
    {   // the sample rows: gathered on the device, ONE contiguous copy back (a strided 2-D copy of 2048 short rows
        // to pageable memory took milliseconds)
        std::vector<uint32_t> rows_h((size_t)ns);
        for (int64_t i = 0; i < ns; ++i) rows_h[(size_t)i] = (uint32_t)(i * stride);
        nabo_index::Workspace::RerunBufs &b = ix->ws.rerun[RERUN_WIDE];      // (borrowed: no query runs during set_ref)
        if ((rc = b.rows.reserve((size_t)ns * sizeof(uint32_t)))) return rc;
        if ((rc = b.x.reserve((size_t)ns * G * sizeof(double)))) return rc;
        HIP_TRY(hipMemcpyAsync(b.rows.p, rows_h.data(), (size_t)ns * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(gather_rows_launch(ref.dY, b.rows.as<uint32_t>(), ns, G, b.x.as<double>(), st));
        HIP_TRY(hipMemcpyAsync(smp.data(), b.x.p, (size_t)ns * G * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    // (one sort per dimension: a few host threads -- 50 sorts of 2048 values were 3.9 ms of every set_ref)
    auto edges_of = [&](int k0, int k1) {
        std::vector<double> colk((size_t)ns);
        for (int k = k0; k < k1; ++k) {
            size_t nf = 0;
            for (int64_t i = 0; i < ns; ++i) {
                const double v = smp[(size_t)i * G + k];
                if (std::isfinite(v)) colk[nf++] = v;
            }
            std::sort(colk.begin(), colk.begin() + nf);
            for (int b = 1; b < B; ++b)
                edges[(size_t)k * (B - 1) + (b - 1)] = nf ? colk[(size_t)((double)b * nf / B)] : 0.0;
        }
    };
    const int nt = G >= 16 ? 8 : 1;
    std::vector<std::thread> th;
    bool threaded = nt > 1;
    if (threaded) {
        try {
            for (int t = 0; t < nt; ++t) th.emplace_back(edges_of, G * t / nt, G * (t + 1) / nt);
        } catch (...) {
            threaded = false;
        }
        for (std::thread &t : th) t.join();
    }
    if (!threaded) edges_of(0, G);           // (also after a failed thread start: every dimension again)
    if ((rc = cb.cbedges.reserve(edges.size() * sizeof(double)))) return rc;
    if ((rc = cb.cbtab.reserve(cbb_table_bytes(n, G)))) return rc;
    if ((rc = cb.cbvalid.reserve(cbb_valid_bytes(n)))) return rc;
    HIP_TRY(hipMemcpyAsync(cb.cbedges.p, edges.data(), edges.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(cbb_pack_table_launch(ref.dY, n, G, cb.cbedges.as<double>(), cb.cbtab.as<uint32_t>(), st));
    HIP_TRY(cbb_valid_launch(ref.dmask, n, cb.cbvalid.as<uint32_t>(), st));
    HIP_TRY(hipStreamSynchronize(st));      // edges goes out of scope
    ix->shape.cb_bits = true;
    return NABO_OK;
}

// Modified-Canberra references: the exact kernel's transposed rows, and where they fit fp32 the counting pass's operands
static int prepare_canberra(nabo_index *ix)
{
    IndexShape &sh = ix->shape;
    auto &ref = ix->ref;
    auto &cb = ix->ref.cb;
    hipStream_t st = ix->stream;
    const int G = sh.g;
    const int64_t chunks = (sh.n + 63) / 64;
    int rc;
    if ((rc = cb.yt.reserve((size_t)chunks * 64 * G * sizeof(double)))) return rc;
    HIP_TRY(transpose_ref_launch(ref.dY, sh.n, G, cb.yt.as<double>(), st));
    cb.gp = cbf_pick_gp(G);
    cb.f32 = false;
    sh.cb_bits = false;
    if (cb.gp > 0 && ix->cb_mode != 1) {
        unsigned int flag = 0;
        if ((rc = cb.ycf.reserve((size_t)chunks * 64 * cb.gp * sizeof(float)))) return rc;      // chunk-major (range check)
        if ((rc = cb.yrow.reserve((size_t)sh.n * cb.gp * sizeof(float)))) return rc;           // row-major (bound pass)
        if ((rc = cb.cbflag.reserve(4 * sizeof(unsigned int)))) return rc;
        HIP_TRY(hipMemsetAsync(cb.cbflag.p, 0, 4 * sizeof(unsigned int), st));
        HIP_TRY(cbf_pack_refs_launch(ref.dY, sh.n, G, cb.gp, cb.ycf.as<float>(), cb.cbflag.as<unsigned int>(), st));
        HIP_TRY(hipMemcpyAsync(&flag, cb.cbflag.p, sizeof(flag), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        cb.f32 = (flag == 0);
    }
    if (cb.f32) {
        // per-dimension quantisation of the counting pass (canberra_f32.hip): min_k and 127 / (max_k - min_k) over the
        // references, from fp32 bounds that enclose every float64 value
        std::vector<unsigned int> cm((size_t)2 * G, 0u);
        std::vector<double> sc((size_t)2 * G, 0.0);
        auto unord = [](unsigned int u) {
            const unsigned int b = u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu);
            float f;
            memcpy(&f, &b, sizeof(f));
            return (double)f;
        };
        if ((rc = cb.cbscale.reserve((size_t)2 * G * sizeof(double)))) return rc;
        HIP_TRY(hipMemsetAsync(cb.cbscale.p, 0xFF, (size_t)G * sizeof(unsigned int), st));
        HIP_TRY(hipMemsetAsync(cb.cbscale.as<unsigned int>() + G, 0, (size_t)G * sizeof(unsigned int), st));
        HIP_TRY(cbf_colminmax_launch(ref.dY, sh.n, G, cb.cbscale.as<unsigned int>(), st));
        HIP_TRY(hipMemcpyAsync(cm.data(), cb.cbscale.p, (size_t)2 * G * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int k = 0; k < G; ++k) {
            const double lo = unord(cm[(size_t)k]), hi = unord(cm[(size_t)G + k]);
            sc[(size_t)k] = std::isfinite(lo) ? lo : 0.0;
            sc[(size_t)G + k] = (std::isfinite(lo) && std::isfinite(hi) && hi > lo && std::isfinite(127.0 / (hi - lo)))
                                    ? 127.0 / (hi - lo) : 0.0;              // 0: constant column, never counted as out
        }
        HIP_TRY(hipMemcpyAsync(cb.cbscale.p, sc.data(), (size_t)2 * G * sizeof(double), hipMemcpyHostToDevice, st));
        if ((rc = cb.ych.reserve((size_t)chunks * 64 * cb.gp * 2))) return rc;
        HIP_TRY(cbf_pack_refs_rows_launch(ref.dY, sh.n, G, cb.gp, cb.yrow.as<float>(), st));
        HIP_TRY(cbf_pack_refs8_launch(ref.dY, sh.n, G, cb.gp, cb.cbscale.as<double>(), cb.ych.p, st));
        HIP_TRY(hipStreamSynchronize(st));      // sc goes out of scope
        // The bitmaps are the default for reference sets of >= 12 blocks (25k cells; round 3, 128 blocks:
        // measured 2.0x the SWAR pass at 1M x 1M, level with it at 100k x 100k where building its table costs
        // what it saves; NABO_CANBERRA_MODE=swar pins the 7-bit SWAR pass, =bits the bitmaps at any size)
        // (round 4: from 12 blocks on -- with the four-words-per-lane kernel, its lists seeded before the count starts and
        // the edge sorts on eight host threads (set_ref 3.9 -> 1.2 ms) the bitmaps win from ~25k references even with
        // their table built inside the step: 100k x 100k 13.2 against 25.5 ms, 30k x 30k 3.0 against 3.6; 10k x 10k
        // 2.3 against 1.4 -- the same query time, the table build on top)
        const bool want_bits = ix->cb_mode ? ix->cb_mode == 3 : sh.n >= 12 * 2048;
        if (want_bits && cbb_available(G, cb.gp, 1) && (rc = build_bitmaps(ix))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return NABO_OK;
}

}  // namespace nabo

using namespace nabo;

int nabo_index_set_ref(nabo_index *ix, const double *Y, int32_t y_on_device, const uint8_t *ref_mask)
{
    if (!ix || !Y) return api_fail(NABO_E_INVALID, "NULL argument");
    int rc;
    if ((rc = index_idle(ix)) || (rc = use_device(ix->device))) return rc;
    auto &ref = ix->ref;
    if (y_on_device) {
        ref.dY = Y;
    } else {
        const size_t ybytes = (size_t)ix->shape.n * ix->shape.g * sizeof(double);
        if ((rc = ref.ybuf.reserve(ybytes))) return rc;
        HIP_TRY(hipMemcpyAsync(ref.ybuf.p, Y, ybytes, hipMemcpyHostToDevice, ix->stream));
        ref.dY = ref.ybuf.as<double>();
    }
    if ((rc = apply_mask(ix, ref_mask))) return rc;
    if (ix->shape.metric == NABO_METRIC_MOD_CANBERRA) rc = prepare_canberra(ix);
    else if (ix->shape.ksteps > 0) rc = prepare_l2(ix);
    else HIP_TRY(hipStreamSynchronize(ix->stream));             // exact route only: the float64 rows are all it needs
    if (rc) return rc;
    ref.have = true;
    return NABO_OK;
}

int nabo_index_set_mask(nabo_index *ix, const uint8_t *ref_mask)
{
    if (!ix) return api_fail(NABO_E_INVALID, "NULL index");
    int rc;
    if ((rc = index_idle(ix))) return rc;
    if (!ix->ref.have) return api_fail(NABO_E_INVALID, "nabo_index_set_ref has not been called");
    if ((rc = use_device(ix->device)) || (rc = apply_mask(ix, ref_mask))) return rc;
    if (ix->shape.metric == NABO_METRIC_MOD_CANBERRA && ix->shape.cb_bits) {
        HIP_TRY(cbb_valid_launch(ix->ref.dmask, ix->shape.n, ix->ref.cb.cbvalid.as<uint32_t>(), ix->stream));
        HIP_TRY(hipStreamSynchronize(ix->stream));
    }
    if (ix->shape.metric != NABO_METRIC_MOD_CANBERRA && ix->shape.ksteps > 0) return repack_refs(ix);
    return NABO_OK;
}

// plan.hip -- what the host decides from shapes alone: the option table, which filter kernels serve an index (make_shape),
// the launch plans of the Euclidean / cosine passes (plan_l2) and of a modified-Canberra query (plan_canberra), and
// nabo_query_plan, which returns a plan for an index that need not exist.  Nothing here touches the device.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bucket_skip.h"
#include "index.h"
#include "l2c_slots.h"
#include "l2c_window.h"
#include "local_seeds.h"

namespace nabo {

static int pick_ksteps(int g)
{
    const int need = (g + 1) / 2;
    const int inst[] = {8, 16, 25, 32, 50, 64};
    for (int v : inst)
        if (need <= v) return v;
    return -1;
}

struct OptionName { const char *name; int Options::*field; };
static const OptionName OPTION_NAMES[] = {
    {"splits", &Options::splits}, {"tail_split", &Options::tail_split}, {"lkeep", &Options::lkeep},
    {"coarse_slack", &Options::coarse_slack}, {"cand_slack", &Options::cand_slack}, {"seeded_pass", &Options::seeded_pass},
    {"coarse_adapt", &Options::coarse_adapt}, {"wide_retry", &Options::wide_retry}, {"refine_overlap", &Options::refine_overlap},
    {"prepass", &Options::prepass}, {"pieces", &Options::pieces}, {"merge_lists", &Options::merge_lists}, {"one_round", &Options::one_round}, {"l2c_geo", &Options::l2c_geo}, {"l2_r1", &Options::l2_r1},
    {"split_refs_max", &Options::split_refs_max}, {"cosine_centre", &Options::cosine_centre},
    {"coarse_kernel_q", &Options::coarse_kernel_q}, {"order_flags", &Options::order_flags},
};

// The local tournament seeds' options (local_seeds.hip).  A table of their own: tests/test_local_seeds_gpu.py runs them
// on and off against the oracle, the randomised option sweep (tests/test_option_sweep_gpu.py) draws from OPTION_NAMES
// above, and the stream sweep (tests/test_stream_sweep_gpu.py) draws from this table and the next one.
static const OptionName LOCAL_SEED_OPTION_NAMES[] = {
    {"local_seeds", &Options::local_seeds}, {"local_anchors", &Options::local_anchors}, {"local_cap", &Options::local_cap},
};

// The two-level stream's options (l2c_topk.hip): tests/test_two_level_gpu.py runs it on small shapes against the oracle,
// the stream sweep (tests/test_stream_sweep_gpu.py; values: STREAM_OPTION_VALUES of tests/_option_sweep.py) draws them,
// clamps included, with the main table's options on top.
static const OptionName TWO_LEVEL_OPTION_NAMES[] = {
    {"two_level", &Options::two_level}, {"two_level_share", &Options::two_level_share}, {"two_level_stretch", &Options::two_level_stretch},
    {"two_level_burst", &Options::two_level_burst}, {"two_level_window", &Options::two_level_window},
    {"two_level_check", &Options::two_level_check},
};

// The sub-order inside the stream's buckets (local_seeds.h).  A table of its own: tests/test_sub_order_gpu.py runs its
// values, clamps included, against the oracle.
static const OptionName SUB_ORDER_OPTION_NAMES[] = {
    {"two_level_sub", &Options::two_level_sub}, {"two_level_sub_rank", &Options::two_level_sub_rank},
};

// The skip of unreachable sub-buckets in the ordered main launch (bucket_skip.h).  A table of its own:
// tests/test_bucket_skip_gpu.py runs its values against the oracle.
static const OptionName BUCKET_SKIP_OPTION_NAMES[] = {
    {"bucket_skip", &Options::bucket_skip},
};

bool option_set(Options &o, const char *name, int64_t value)
{
    for (const OptionName &e : BUCKET_SKIP_OPTION_NAMES)
        if (strcmp(e.name, name) == 0) {            // clamped: 0 .. 2
            o.*(e.field) = (int)(value < 0 ? 0 : value > 2 ? 2 : value);
            return true;
        }
    for (const OptionName &e : SUB_ORDER_OPTION_NAMES)
        if (strcmp(e.name, name) == 0) {            // clamped: sub-anchors 0 .. LSEED_MAX_SUB, the ranking rule 0 .. 1
            const int64_t hi = e.field == &Options::two_level_sub ? LSEED_MAX_SUB : 1;
            o.*(e.field) = (int)(value < 0 ? 0 : value > hi ? hi : value);
            return true;
        }
    for (const OptionName &e : TWO_LEVEL_OPTION_NAMES)
        if (strcmp(e.name, name) == 0) {            // clamped: 0 .. 2, percent, refetches, tiles (the window: -1 = none)
            const int64_t hi = e.field == &Options::two_level ? 2 : e.field == &Options::two_level_share ? 100
                               : e.field == &Options::two_level_burst ? 64 : e.field == &Options::two_level_window ? L2C_WIN_MAX
                               : e.field == &Options::two_level_check ? L2C_WIN_CHECK_MAX : 1 << 20;
            const int64_t lo = e.field == &Options::two_level_window ? -1 : 0;
            o.*(e.field) = (int)(value < lo ? lo : value > hi ? hi : value);
            return true;
        }
    for (const OptionName &e : OPTION_NAMES)
        if (strcmp(e.name, name) == 0) {
            o.*(e.field) = (int)value;
            return true;
        }
    for (const OptionName &e : LOCAL_SEED_OPTION_NAMES)
        if (strcmp(e.name, name) == 0) {
            o.*(e.field) = (int)value;
            return true;
        }
    return false;
}

// The two-level slot order serves the l2c kernel's one-step loop, which exists for two operand steps (28 < g <= 59) and runs
// on launches that take local seeds: by default where those are on by default, with option two_level = 2 at any size.
static bool two_level_wanted(const IndexShape &sh)
{
    if (sh.opt.two_level == 0 || !sh.coarse || !l2c_slots_fit(sh.g) || sh.opt.local_seeds == 0 || sh.opt.prepass <= 0) return false;
    int c = sh.opt.local_anchors > 0 ? sh.opt.local_anchors : 64;
    if (sh.n < c) return false;
    return sh.opt.two_level >= 2 || sh.n >= LSEED_MIN_REFS;
}
bool two_level_slots(const IndexShape &sh) { return sh.kc1 == 4 && two_level_wanted(sh); }

// The operand steps of the one-product pass follow the options: g = 29 fills ONE step of 32 slots in the plain order
// (29 + 3) and needs two in the two-level order (29 + 5) -- twice the matrix work for nothing by default, so only option
// two_level = 2 asks for it (the smallest tail there is: tests).  Called wherever an option may have changed.
void shape_refresh(IndexShape &sh)
{
    if (!sh.coarse) return;
    sh.kc1 = l2c_pick_kc(sh.g);
    if (sh.kc1 == 2 && sh.opt.two_level >= 2 && two_level_wanted(sh)) sh.kc1 = 4;
}

void lseed_params(const IndexShape &sh, int *C, int *cap)
{
    int c = sh.opt.local_anchors > 0 ? sh.opt.local_anchors : 64;
    if (c > LSEED_MAX_ANCHORS) c = LSEED_MAX_ANCHORS;
    int k = sh.opt.local_cap > 0 ? sh.opt.local_cap : 16384;
    k = (k + 31) / 32 * 32;
    if (k > LSEED_MAX_CAP) k = LSEED_MAX_CAP;
    // no one-product operands, switched off, or fewer references than anchors
    if (!sh.coarse || sh.opt.local_seeds == 0 || sh.n < c) c = 0;
    // by default only where a launch can take them (lseed_applies): the runs cost C * cap cells of memory
    // (option two_level = 2 brings its buckets along at any size -- where its slot order fits)
    if (sh.opt.local_seeds == 1 && sh.n < LSEED_MIN_REFS && !(sh.opt.two_level >= 2 && l2c_slots_fit(sh.g))) c = 0;
    *C = c;
    *cap = k;
}

// Sub-anchors per bucket of the two-level stream's copies: only where the stream's operands exist
int lseed_sub_param(const IndexShape &sh) { return two_level_slots(sh) ? lseed_sub_count(sh.opt.two_level_sub) : 1; }

// The skip tables are built with the ordered copy wherever a main launch of this index could skip (bskip_planned) and the
// tables can be built at all (bskip_buildable): the ONE decision ensure_local_seeds and the planner share
bool bskip_wanted(const IndexShape &sh)
{
    int C = 0, cap = 0;
    lseed_params(sh, &C, &cap);
    return C > 0 && two_level_slots(sh) && bskip_planned(sh.opt.bucket_skip, true, sh.opt.two_level) &&
           bskip_buildable(lseed_ordered_tiles(sh.ref_tiles, C), sh.g);
}

// Local seeds serve a launch of the first one-product pass with ONE reference split (a seed bounds the lkeep-th smallest
// score over a split's own references only if the sample lies inside it: every bucket does for S = 1), where the tournament
// is on at all.  By default from 2^18 references and 2^16 rows on: below that the launch is cut into reference splits
// anyway, and the sort of the rows (assignment, two gathers) is no longer small against the list updates it saves.
// And by default in geometry B only (two operand steps, up to 23 kept entries: 1M x 1M, d = 50, k = 15: 95.5 -> 93.8 ms
// per step): on the 64-entry lists of geometry C the filter kernel itself ran twice as long behind local seeds (cosine
// 1M x 1M, d = 100, k = 50: 274 -> 522 ms, same rows per pass; not understood), geometry A has not been measured.
bool lseed_applies(const IndexShape &sh, const L2Plan &P, int S, int64_t rows)
{
    int C = 0, cap = 0;
    lseed_params(sh, &C, &cap);
    if (C == 0 || !P.on_l2c || S != 1 || rows < 1 || sh.opt.prepass <= 0) return false;
    return sh.opt.local_seeds >= 2 || (P.geo == 1 && (rows >= LSEED_MIN_ROWS || (sh.opt.two_level >= 2 && P.slots2)));
}

// Which filter kernels serve an index of this shape, and its reference tiles (IndexShape, index.h)
IndexShape make_shape(int64_t n, int g, int metric, int n_cu, const char *md)
{
    IndexShape sh;
    sh.n = n;
    sh.g = g;
    sh.metric = metric;
    sh.n_cu = n_cu;
    sh.ref_tiles = (n + 31) / 32;
    sh.ref_tiles_alloc = sh.ref_tiles + 64;      // room for split padding (+inf-norm tiles; up to 32 splits)
    if (metric == NABO_METRIC_MOD_CANBERRA) return sh;
    sh.ksteps = pick_ksteps(g);            // -1: g > NABO_MAX_COMPS, every query takes the exact float64 route
    const bool f32 = md && strcmp(md, "f32") == 0, f16x3 = md && strncmp(md, "f16x3", 5) == 0;
    if (sh.ksteps <= 0) return sh;
    if (!f32 && l2q_pick_kc(g) > 0) {
        sh.mode = 1;                        // an f16x3 kernel exists for this g (g < 64)
        sh.kc = l2q_pick_kc(g);
        sh.kc1 = l2c_pick_kc(g);
        sh.coarse = sh.kc1 > 0 && !f16x3;
    } else if (!f32 && !f16x3 && l2c_pick_kc(g) > 0) {
        // 64 <= g <= 125: no f16x3 kernel is instantiated, but the one-product operands (g + 3 slots: four steps of 32)
        // are -- the one-product pass runs first, the fp32-MFMA filter takes the rows it cannot certify
        sh.kc1 = l2c_pick_kc(g);
        sh.coarse = true;
    }
    return sh;
}

int plan_l2(const IndexShape &sh, const PassCtx &ctx, int64_t m, int k, int drop, bool cand_mode, L2Plan *P)
{
    const int kk = k + drop;
    const int epl = list_epl(ctx, kk, cand_mode);
    const int L = 32 * epl;
    int rows_per_wg = 256, wg_per_cu = 1, lkeep_max = L;
    bool use_h = false;                                  // an f16x3 kernel runs
    if (sh.mode == 1 && epl == 1) {
        nabo::l2q_topk_geometry(sh.kc, &rows_per_wg, &wg_per_cu, &lkeep_max);
        use_h = (cand_mode ? kk : kk + 4) <= lkeep_max;   // needs at least 4 entries of slack
    }
    // The one-product first pass (kc1-step operands; see IndexShape::coarse) -- on the l2c kernel, in the geometry that
    // serves the list length the pass wants (l2c_topk.hip: two waves per SIMD up to 23 kept entries, 32-entry lists,
    // 64-entry lists for k' > 24), unless option coarse_kernel_q sends the operands through the l2q kernel (32-entry lists
    // and g < 64 only).
    const bool pass1 = sh.coarse && !(ctx.coarse_weak && sh.opt.coarse_adapt != 0) && ctx.pass_level < 2 &&
                       !ctx.wide_retry && (!cand_mode || kk + 3 <= 32);
    // (k' > 24, the 64-entry lists: six entries more -- there a row the first pass fails is expensive, the pass behind the
    // seeded one is the fp32 filter: cosine 1M x 1M, d = 100, k = 50: 689 -> 597 ms per step)
    const int slack1 = sh.opt.coarse_slack >= 0 ? sh.opt.coarse_slack : (epl == 2 ? 6 : 0);
    const int cslack = sh.opt.cand_slack >= 0 ? sh.opt.cand_slack : sh.cand_slack;
    int want = cand_mode ? (kk < 4 ? 4 : kk) + cslack : kk + 8 + slack1;
    if (ctx.pass_level == 1) want = L;                   // seeded pass: room for everything below the seed
    if (epl == 1 && want > 32) want = 32;                // (the emitted lists hold 32 epl entries)
    if (epl == 2) want = want < 33 ? 33 : (want > 64 ? 64 : want);
    int geo = -1;
    if (pass1 && sh.opt.coarse_kernel_q == 0 && kk + 4 <= L) {
        geo = nabo::l2c_geometry(sh.kc1, want, sh.opt.l2c_geo);
        if (epl == 1 && geo == 2) geo = 0;               // (NABO_L2C_GEO=c with 32-entry emitted lists: geometry A)
    }
    const bool on_l2c = geo >= 0;
    const bool use_1 = on_l2c || (pass1 && use_h);
    if (on_l2c) {
        use_h = true;
        nabo::l2c_topk_geometry(sh.kc1, want, sh.opt.l2c_geo, &rows_per_wg, &wg_per_cu, &lkeep_max);
        if (geo == 0) { rows_per_wg = 4 * 128; lkeep_max = 32; }
    }
    const int kcq = use_1 ? sh.kc1 : sh.kc;
    // fewer rows than two-row-block workgroups fill the chip with: one row-block per wave, three waves per SIMD
    // (128-row workgroups balance the CUs and the third wave covers the list warm-up that dominates short streams)
    bool r1 = false;
    if (!use_h) {
        nabo::l2_topk_geometry(sh.ksteps, epl, &rows_per_wg, &wg_per_cu, &lkeep_max);
        const int r1_mode = sh.opt.l2_r1;             // -1 auto, 0 never, 1 always (experiments)
        // ... and also when the list warm-up is a large share of a workgroup's time (short reference streams,
        // e.g. one shard of eight): the same per-workgroup model as the split choice below, threshold measured
        // (the variant pays ~8 % more per reference tile, it wins from ~7.5 % warm-up share on)
        int lk_est = cand_mode ? (kk < 4 ? 4 : kk) : (kk + 8 < 16 ? 16 : kk + 8);
        if (lk_est > L) lk_est = L;
        const double stream_ms = (double)((sh.n + 31) / 32) * 3.36e-3 * (sh.ksteps / 25.0);
        const double lg_est = std::log((double)sh.n / lk_est > 2.0 ? (double)sh.n / lk_est : 2.0);
        const double warm_ms = 5.1 * (lk_est / 24.0) * (lg_est / 10.6);
        if (epl == 1 && sh.ksteps <= 25 && r1_mode != 0 &&
            (r1_mode == 1 || (m + rows_per_wg - 1) / rows_per_wg < (int64_t)sh.n_cu * wg_per_cu ||
             warm_ms > 0.075 * stream_ms)) {
            r1 = true;
            nabo::l2_topk_geometry(sh.ksteps, -1, &rows_per_wg, &wg_per_cu, &lkeep_max);
        }
    }
    const int64_t slots = (int64_t)sh.n_cu * wg_per_cu;          // workgroups resident at once
    const int64_t gx = (m + rows_per_wg - 1) / rows_per_wg;
    const int64_t rows_pad = gx * rows_per_wg;
    // kept-list length: k' + 8 slack (the certification needs a gap above the k'-th distance)
    int lkeep = kk + 8;
    if (lkeep < 16) lkeep = 16;
    if (ctx.wide_retry) lkeep = lkeep_max;              // as many kept entries as the 64-entry lists allow
    // one-product pass: its scores sit up to 2^-9 ||x|| ||y|| below the real ones and the gap above the k'-th distance
    // has to cover that -- 1M x 1M x 50: k' + 8 entries leave ~1 % of the rows to the f16x3 pass (7 ms), k' + 13 a
    // third of that, but every five entries more cost 14 ms of list updates in the kernel: no extra slack by default
    if (use_1) lkeep = kk + 8 + slack1;
    if (use_1 && ctx.pass_level == 1) lkeep = lkeep_max;       // seeded pass: room for everything below the seed
    if (on_l2c && lkeep > want) lkeep = want;
    if (cand_mode) lkeep = kk < 4 ? 4 : kk;
    // (candidate mode on the one-product pass: three kept entries more than are emitted, so that the bound is the exact
    // distance of the first candidate left out and not the one-product threshold, which sits 2^-9 ||x|| ||y|| lower)
    if (cand_mode && use_1) lkeep += cslack;
    if (lkeep > lkeep_max) lkeep = lkeep_max;
    // (experiments and tests: the first pass's list length; the passes behind it keep theirs)
    if (ctx.pass_level == 0 && !ctx.wide_retry) { const int lk = sh.opt.lkeep; if (lk >= kk && lk <= lkeep_max) lkeep = lk; }
    // Work decomposition.  Few target rows: split the reference range S ways (grid.y) so the
    // chip is full.  Many rows: the last, partially filled round of workgroups is launched with
    // its own split factor S2 so that it takes ~1/S2 of a round instead of a whole one.
    int64_t gx_main = gx, gx_tail = 0;
    int S2 = 1;
    int S = sh.opt.splits;
    const bool forced = S > 0;
    // Fewer column-workgroups than slots, one-product kernel, lists merged before the float64 step (so a row's list count
    // costs the refine nothing): ONE round of workgroups at full occupancy -- all the columns with floor(slots / gx) uniform
    // splits when that fills at least 80 % of the slots.  On LONG reference streams (>= 8192 tiles) also one split more on
    // the floor(slots / S) columns that fit, the columns left over as a tail launch with more splits (the main / tail pair
    // of the long queries): 120k x 1M: 256 x 2 + 57 x 8, 13.3 instead of 16.1 ms.  On short streams a tail costs more than
    // the idle slots (100k x 100k: 256 x 2 + 5 x 16 behind the main launch 2.44 ms, beside it on the second stream 2.55,
    // 261 x 1 2.42), and so did cutting the (column, tile) space into equal chunks ("pieces", removed): workgroups of a uniform
    // split stream the same tiles at the same time and share them in L2, unaligned pieces do not (49k x 100k: kernel
    // 1.99 ms as 603 pieces, 1.10 ms as 128 x 4).
    // split count of a tail launch of `tail` workgroups: the one that takes the smallest part of a round (1: none does)
    // (at most 8 splits: 11 would fill the chip exactly at 1M x 1M -- kernel 0.6 ms shorter, refine of the tail rows' 11
    // lists 1.1 ms longer)
    auto tail_splits = [&](int64_t tail) {
        int s = 1;
        double best = 1.0;
        for (int s2 = 2; s2 <= 8; ++s2) {
            const double t = (double)((tail * s2 + slots - 1) / slots) / s2;
            if (t < best - 1e-9) { best = t; s = s2; }
        }
        return s;
    };
    bool one_round = false;
    if (!forced && on_l2c && sh.opt.one_round != 0 && sh.opt.merge_lists != 0 && ctx.pass_level == 0 && !ctx.wide_retry &&
        gx < slots) {
        int64_t s_cap = sh.ref_tiles / 16 > 0 ? sh.ref_tiles / 16 : 1;     // >= 16 tiles per split
        if (s_cap > 1024 / L) s_cap = 1024 / L;
        int64_t s_exact = slots / gx;
        if (s_exact > s_cap) s_exact = s_cap;
        S = (int)s_exact;
        const double occ = (double)(gx * s_exact) / (double)slots;
        if (occ < 0.8 && s_exact + 1 <= s_cap && sh.opt.tail_split != 0 && sh.ref_tiles >= 8192) {
            const int64_t s_up = s_exact + 1, cols = slots / s_up, rest = gx - cols;
            if (cols >= 1 && rest >= 1 && rest * 4 <= gx) {           // (the tail is a quarter of the columns at most)
                int64_t s2 = slots / rest;
                if (s2 > s_cap) s2 = s_cap;
                if (s2 > 16) s2 = 16;
                if (s2 < s_up) s2 = s_up;
                S = (int)s_up;
                S2 = (int)s2;
                gx_main = cols;
                gx_tail = rest;
            }
        }
        one_round = occ >= 0.8 || gx_tail > 0;               // (otherwise the cost model below decides)
    }
    if (!forced && !one_round) {
        S = 1;
        if (gx < slots) {
            // Fewer workgroups than the chip holds: pick the split count from a cost model.  A workgroup costs
            // (reference tiles it streams) x t_tile for the MFMA chains PLUS a per-row list warm-up that does
            // not shrink with the stream (~lkeep * ln(stream / lkeep) appends per row: 5.1 ms per workgroup at
            // lkeep = 24 over 1M references, measured); every split pays the warm-up again.
            int64_t s_hi = sh.ref_tiles / 16 > 0 ? sh.ref_tiles / 16 : 1;
            if (s_hi > 1024 / L) s_hi = 1024 / L;
            // ms per reference tile and workgroup, measured: 105 ms / 31250 tiles (fp32, 256 rows, 25 k-steps); 1.2 us f16x3
            const double t_tile = use_h ? 1.1e-3 * kcq / 10.0 : 3.36e-3 * (rows_per_wg / 256.0) * (sh.ksteps / 25.0);
            double best = 1e30;
            for (int s2 = 1; s2 <= (int)s_hi; ++s2) {
                const double rounds = (double)((gx * s2 + slots - 1) / slots);
                const double stream = (double)sh.n / s2;
                double lg = std::log(stream / lkeep > 2.0 ? stream / lkeep : 2.0);
                const double warm = 5.1 * (lkeep / 24.0) * (lg / 10.6) * (rows_per_wg / 256.0);
                const double cost = rounds * ((double)sh.ref_tiles / s2 * t_tile + warm);
                if (cost < best * (1.0 - 1e-3)) { best = cost; S = s2; }
            }
        } else if (gx % slots != 0 && sh.opt.tail_split != 0 && sh.ref_tiles >= 256) {
            const int64_t tail = gx % slots;
            S2 = tail_splits(tail);
            if (S2 > 1) { gx_tail = tail; gx_main = gx - tail; }
        }
    }
    if (S > 1024 / L) S = 1024 / L;                     // refine merges at most 1024 candidates per row (32 or 16 lists)
    if (S < 1) S = 1;
    if ((int64_t)S > sh.ref_tiles) S = (int)sh.ref_tiles;
    // A seeded pass keeps at most L entries per list: where the first pass already kept (nearly) as many -- k' >= 43 on the
    // 64-entry lists: cosine d = 100, k = 50 -- one list per row certifies nothing the first pass could not.  Four
    // reference splits give a row four lists: the references below its seed (a few more than 64) spread over them.
    if (use_1 && ctx.pass_level == 1 && !forced && kk + 8 + slack1 + 8 > L) {
        if (S < 4) S = 4;
        if (gx_tail > 0 && S2 < 4) S2 = 4;
    }
    {   // a list entry holds 25 bits of offset into its split (topk_lists.h): very large sets take more splits
        // (NABO_SPLIT_REFS_MAX: tests lower the bound to see the rule at ordinary sizes)
        int64_t split_refs = sh.opt.split_refs_max;
        if (split_refs < 64 || split_refs > NABO_LIST_SPLIT_REFS) split_refs = NABO_LIST_SPLIT_REFS;
        const int64_t split_tiles = (split_refs - 1) / 32;
        const int64_t s_min = (sh.ref_tiles + split_tiles - 1) / split_tiles;
        if (s_min > 1024 / L) return api_fail(NABO_E_INVALID, "more than 2^25 x (1024 / list length) reference cells in one index");
        if (S < s_min) S = (int)s_min;
        if (gx_tail > 0 && S2 < s_min) S2 = (int)s_min;
    }
    const int64_t tps = (sh.ref_tiles + S - 1) / S;
    const int64_t tps2 = (sh.ref_tiles + S2 - 1) / S2;
    if (tps * S > sh.ref_tiles_alloc || tps2 * S2 > sh.ref_tiles_alloc)
        return api_fail(NABO_E_INVALID, "internal: split padding exceeds allocation");

    P->epl = epl; P->L = L;
    P->use_h = use_h; P->use_1 = use_1; P->on_l2c = on_l2c; P->r1 = r1;
    P->geo = geo; P->kcq = kcq; P->cslack = cslack;
    P->rows_per_wg = rows_per_wg; P->wg_per_cu = wg_per_cu; P->lkeep_max = lkeep_max; P->lkeep = lkeep; P->want = want;
    P->S = S; P->S2 = S2; P->one_round = one_round;
    P->gx = gx; P->gx_main = gx_main; P->gx_tail = gx_tail; P->rows_pad = rows_pad; P->tps = tps; P->tps2 = tps2;
    // the two-level stream: the main launch of the first pass in geometry B where it takes local seeds (their bucket-ordered
    // target copy is what it reads; a tail launch with local seeds of its own would overwrite that copy)
    P->slots2 = use_1 && two_level_slots(sh);
    {
        const int64_t rows_main = gx_main * rows_per_wg < m ? gx_main * rows_per_wg : m;
        P->tl_main = P->slots2 && on_l2c && geo == 1 && kcq == 4 && ctx.first() && !cand_mode && gx_main > 0 &&
                     lseed_applies(sh, *P, S, rows_main) && !(gx_tail > 0 && lseed_applies(sh, *P, S2, m - rows_main));
    }
    P->tl_skip = P->tl_main && bskip_wanted(sh) && rows_per_wg == BSKIP_WG_ROWS;
    // WHOLE ROUNDS for the two-level main launch.  It runs its rows as POSITIONS of the bucket-ordered copy:
    // lseed_columns(rows, C) columns of 128, every bucket padding its rows to whole columns -- gx_main workgroups' worth of
    // rows are up to (C + 1) x 128 positions more, a few workgroups of one more round, each streaming the whole reference set
    // while the chip idles.  So the main launch takes as many rows as fit gx_main workgroups as positions and the tail
    // launch the rest, its split count by the tail's rule.  Not where the index decided against the stream (ctx.tl_no: such
    // data must not pay for a larger tail), and not where the larger tail would no longer be a part of ONE round.
    P->rows_main = gx_main * rows_per_wg;
    if (P->tl_main && gx_tail > 0 && !ctx.tl_no) {
        int lc = 0, lcap = 0;
        lseed_params(sh, &lc, &lcap);
        const int64_t rows_tl = (gx_main * rows_per_wg / LSEED_COL_ROWS - (lc + 1)) * LSEED_COL_ROWS;
        const int64_t tail = rows_tl > 0 ? (m - rows_tl + rows_per_wg - 1) / rows_per_wg : 0;
        const int s2 = tail > 0 ? tail_splits(tail) : 1;
        const int64_t tps2_tl = (sh.ref_tiles + s2 - 1) / s2;
        if (s2 > 1 && tail * s2 <= slots && s2 <= 1024 / L && tps2_tl * s2 <= sh.ref_tiles_alloc && lseed_applies(sh, *P, S, rows_tl)) {
            P->rows_main = rows_tl;
            P->gx_tail = tail;
            P->S2 = s2;
            P->tps2 = tps2_tl;
            P->gx = gx_main + tail;
            P->rows_pad = P->gx * rows_per_wg;
        }
    }
    // (option coarse_kernel_q runs the one-product operands through the l2q kernel)
    if (use_1 && !on_l2c)
        snprintf(P->kernel, sizeof(P->kernel), "l2q_topk_kernel<%d,1,33> (v_mfma_f32_16x16x32_f16, one-product f16 filter with the split error as an operand slot)", kcq);
    else if (use_1) snprintf(P->kernel, sizeof(P->kernel), "l2c_topk_kernel<%d,%s> (v_mfma_f32_16x16x32_f16, one-product f16 filter with the split error as an operand slot)", kcq / 2, geo == 1 ? "1,23,6,32,4,2" : geo == 2 ? "2,65,4,64,4,1" : "1,33,8,64,4,1");
    else if (use_h) snprintf(P->kernel, sizeof(P->kernel), "l2q_topk_kernel<%d,1,33> (v_mfma_f32_16x16x32_f16, K-concatenated f16x3 split)", sh.kc);
    else snprintf(P->kernel, sizeof(P->kernel), "l2_topk_kernel<%d,%d,%d,%d> (v_mfma_f32_32x32x2_f32)", sh.ksteps,
                  r1 ? 1 : (epl == 1 ? 2 : 1), epl, epl == 1 ? 33 : 65);
    return NABO_OK;
}

// ---- the launch plan of a modified-Canberra query (a pure function of the index's shape and the query's, like plan_l2) ----
// Splits of the exact kernel (canberra_topk_kernel, gx workgroups of 64 rows): ~1024 workgroups in all, at most one split
// per 64-reference chunk and 16.
int cb_exact_splits(int64_t gx, int64_t n_chunks)
{
    if (gx >= 512) return 1;
    int64_t S = (1024 + gx - 1) / gx;
    if (S > n_chunks) S = n_chunks;
    return S > 16 ? 16 : (int)S;
}

// Time of a counting-pass launch of gx workgroups cut s ways, `slots` resident at once: full-length rounds of workgroups,
// and ~8 % more bound evaluations per extra split (every list warms up on its own): measured on 100k x 100k, d = 50
static double cb_split_cost(int64_t gx, int64_t slots, int s)
{
    return (double)((gx * s + slots - 1) / slots) / s * (1.0 + 0.08 * (s - 1));
}

static int cb_best_split(int64_t gx, int64_t slots, int s_max, double *cost)
{
    int best_s = 1;
    double best = 1e30;
    for (int s = 1; s <= s_max; ++s) {
        const double c = cb_split_cost(gx, slots, s);
        if (c < best - 1e-9) { best = c; best_s = s; }
    }
    *cost = best;
    return best_s;
}

void plan_canberra(const IndexShape &sh, int64_t m, int epl, CbPlan *C)
{
    const int64_t n_chunks = (sh.n + 63) / 64;
    C->gx_exact = (m + 63) / 64;
    const int S = sh.opt.splits > 0 ? sh.opt.splits : cb_exact_splits(C->gx_exact, n_chunks);
    C->S_exact = S > 16 ? 16 : S;
    // counting-pass geometry: rpw rows per workgroup, every (row, split) ends with `lists` candidate lists.  Splits fill
    // the chip when there are few rows and trim the last, partially filled round of workgroups when there are many.
    C->bits = sh.cb_bits && epl == 1;               // (the bitmap kernel is instantiated for 32-entry lists)
    C->lists = nabo::cbf_lists_per_split();
    const int rpw = C->bits ? nabo::cbb_rows_per_wg() : nabo::cbf_rows_per_wg(epl);
    const int64_t gxf = (m + rpw - 1) / rpw;
    // resident workgroups: SWAR pass -- one-wave workgroups, 2 per SIMD; bitmap pass -- ONE 8-wave workgroup per CU
    // (its LDS copy of the table rows + eight waves' lists fill the CU's LDS)
    const int64_t slots = C->bits ? (int64_t)sh.n_cu : (int64_t)sh.n_cu * 8;
    int s_max = 1024 / (C->lists * 32 * epl);        // refine handles <= 1024 candidates per row
    if (C->bits) {                                   // splits are ranges of 2048-reference blocks, >= 2 each
        const int64_t nb2 = ((sh.n + 2047) / 2048) / 2;
        if (s_max > nb2) s_max = (int)nb2;
    } else if (s_max > n_chunks / (8 * C->lists)) s_max = (int)(n_chunks / (8 * C->lists));
    if (s_max < 1) s_max = 1;
    double cost = 0;
    int Sf = sh.opt.splits > 0 ? sh.opt.splits : cb_best_split(gxf, slots, s_max, &cost);
    if (Sf > s_max) Sf = s_max;
    // "tail round": with many rows the last, partially filled round of workgroups gets its own (larger) split factor so
    // that it takes a fraction of a round -- same idea as in the Euclidean launch
    C->S2 = 1;
    C->rows_main = m;
    if (sh.opt.splits <= 0 && sh.opt.tail_split != 0 && gxf > slots && gxf % slots != 0 && s_max >= 2) {
        const int64_t tail = gxf % slots;
        double best_t = 0;
        const int best_s = cb_best_split(tail, slots, s_max, &best_t);
        if (best_s > 1 && (double)(gxf / slots) + best_t < cb_split_cost(gxf, slots, Sf) - 1e-9) {
            C->rows_main = (gxf - tail) * rpw;
            C->S2 = best_s;
            Sf = 1;
        }
    }
    C->Sf = Sf;
}

}  // namespace nabo

using namespace nabo;

int nabo_query_plan(int64_t n_ref, int32_t g, int32_t metric, int64_t m, int32_t k, int32_t drop_first, int32_t n_cand,
                    int32_t n_cu, const char *l2_mode, const char *options, int64_t out[NABO_PLAN_FIELDS], char *kernel,
                    size_t kernel_len)
{
    if (!out) return api_fail(NABO_E_INVALID, "NULL argument");
    if (n_ref < 1 || g < 1 || m < 1 || k < 1 || n_cu < 1) return api_fail(NABO_E_INVALID, "bad shape");
    if (metric != NABO_METRIC_EUCLIDEAN && metric != NABO_METRIC_COSINE)
        return api_fail(NABO_E_UNSUPPORTED, "nabo_query_plan describes the Euclidean / cosine filter launches");
    // a shape, never a device object: nothing here touches HIP
    IndexShape sh = make_shape(n_ref, g, metric, n_cu, (l2_mode && *l2_mode) ? l2_mode : nullptr);
    if (options && *options) {                       // "name=value,name=value"
        char buf[512];
        snprintf(buf, sizeof(buf), "%s", options);
        for (char *tok = strtok(buf, ","); tok; tok = strtok(nullptr, ",")) {
            char *eq = strchr(tok, '=');
            if (!eq) return api_fail(NABO_E_INVALID, "option '%s': expected name=value", tok);
            *eq = 0;
            if (!option_set(sh.opt, tok, atoll(eq + 1))) return api_fail(NABO_E_INVALID, "unknown option '%s'", tok);
        }
        shape_refresh(sh);
    }
    const int drop = drop_first ? 1 : 0;
    const bool cand = n_cand > 0;
    const int kq = cand ? n_cand : k;
    for (int i = 0; i < NABO_PLAN_FIELDS; ++i) out[i] = 0;
    if (kq + (cand ? 0 : drop) > NABO_MAX_K || sh.ksteps < 0) {          // the exact float64 kernels answer every row
        out[0] = NABO_PASS_EXACT;
        out[1] = -1;
        if (kernel && kernel_len) snprintf(kernel, kernel_len, "exact_dist_rows_kernel + exact_select_rows_kernel (float64 brute force)");
        return NABO_OK;
    }
    L2Plan P;
    int rc = plan_l2(sh, PassCtx(), m, kq, cand ? 0 : drop, cand, &P);
    if (rc) return rc;
    int pt = 0, gt = 0;
    if (P.on_l2c && sh.opt.prepass > 0) l2c_pre_plan(P.kcq, P.lkeep, (int)P.tps, sh.opt.prepass, &pt, &gt);
    // (out[16]: the launch cut into pieces, removed -- always 0)
    const int64_t fields[16] = {P.use_1 ? NABO_PASS_ONE_PRODUCT : NABO_PASS_SECOND, P.geo, P.rows_per_wg, P.gx_main, P.gx_tail, P.S, P.S2,
                                P.lkeep, P.L, P.tps, pt, gt, (int64_t)n_cu * P.wg_per_cu, P.gx_main * P.S + P.gx_tail * P.S2,
                                P.rows_pad, P.kcq};
    memcpy(out, fields, sizeof(fields));
    {   // out[17]: the buckets of the local tournament seeds where the main launch takes them (local_seeds.hip), else 0
        int lc = 0, lcap = 0;
        lseed_params(sh, &lc, &lcap);
        const int64_t rows_main = P.rows_main < m ? P.rows_main : m;
        out[17] = lseed_applies(sh, P, P.S, rows_main) ? lc : 0;
        out[19] = rows_main;
    }
    out[18] = P.tl_main ? 2 : P.slots2 ? 1 : 0;      // two-level: 2 the main launch streams one-step, 1 the slot order only
    out[20] = P.tl_skip ? 1 : 0;                     // ... and skips the sub-buckets a workgroup's rows cannot reach
    if (kernel && kernel_len) snprintf(kernel, kernel_len, "%s", P.kernel);
    return NABO_OK;
}

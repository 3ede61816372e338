// index.h -- the k-NN index behind the C ABI (include/nabo_knn.h) and what its host files share: plan.hip (launch plans
// from shapes alone), set_ref.hip (the resident references), bucket_order.hip (cells sorted into bucket order), query.hip (the
// pass chain), api.hip (the entry points).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/nabo_knn.h"
#include "bucket_order.h"
#include "host_common.h"
#include "knn_common.h"
#include "two_level_verdict.h"

namespace nabo {

// Tuning options of an index (nabo_index_set_option; the defaults are the product's behaviour).  EVERY setting returns the
// same bits -- an option chooses how a launch is cut or which filter pass answers a row, never what the answer is.  The
// library reads two environment variables, once, in nabo_index_create: NABO_L2_MODE and NABO_CANBERRA_MODE (which first
// filter).
struct Options {
    int splits = 0;            // reference splits of a filter launch (0: the cost model decides)
    int tail_split = 1;        // the last, partially filled round of workgroups gets its own split count
    int lkeep = 0;             // kept entries of the first pass's lists (0: k' + 8)
    int coarse_slack = -1;     // kept entries of the one-product pass beyond k' + 8 (-1: 0 on 32-entry lists, 6 on 64-entry lists)
    int cand_slack = -1;       // candidate mode on the one-product pass: kept entries beyond the emitted ones (-1: the sharded query's rule)
    int seeded_pass = 1;       // links of the pass chain: rows the first pass fails go through the seeded one-product pass,
    int coarse_adapt = 1;      //   a weak one-product bound is remembered until the references change,
    int wide_retry = 1;        //   rows the 32-entry lists fail get 64-entry lists before the exact kernels
    int refine_overlap = 1;    // the refine of the main launch's rows runs beside the filter's tail launch
    int prepass = 100;         // tournament seeds: percent of the planned length (0: lists start from +inf)
    int pieces = 0;            // accepted, no effect (the launch cut into pieces lost to uniform splits and was removed)
    int merge_lists = 1;       // several lists per row are merged by their filter keys before the float64 re-evaluation
    int one_round = 1;         // fewer column-workgroups than slots: splits (+ a tail launch) chosen to fill ONE round of workgroups
    int l2c_geo = -1;          // pin the one-product kernel's geometry: 0 = A, 1 = B, 2 = C (-1: by list length)
    int l2_r1 = -1;            // fp32 filter: one row-block per wave (-1 auto, 0 never, 1 always)
    int split_refs_max = 0;    // lower the 2^25-references-per-split bound (tests see the rule at ordinary sizes)
    int cosine_centre = 1;     // cosine: centre the unit rows before packing (takes effect at the next set_ref)
    int coarse_kernel_q = 0;   // the one-product operands through the l2q kernel instead of l2c
    int order_flags = 0;       // refused by nabo_index_set_option (locality-ordered streaming was removed)
    // local tournament seeds (local_seeds.hip): 0 off, 1 where the planner expects a gain (lseed_applies), 2 on every
    // one-split launch of the one-product pass; anchors (0: 64) and references kept per bucket (0: 16384) pinned for A/B runs
    int local_seeds = 1, local_anchors = 0, local_cap = 0;
    // the two-level stream of the one-product pass (l2c_topk.hip; operands in the two-level slot order, l2c_slots.h): 0 off,
    // 1 where local seeds apply by default and the slots fit, 2 on every one-split geometry-B launch of the first pass
    // (switches the local seeds' buckets on at any size); refetch share (percent, 0: 25) and credit (refetches, 0: the
    // control's default) of the kernel's mode control pinned for A/B runs; stretch > 0: the control that keeps no account
    // per reference bucket, with that first two-step stretch (tiles)
    int two_level = 1, two_level_share = 0, two_level_stretch = 0, two_level_burst = 0;
    int two_level_window = 0, two_level_check = 0;       // l2c_window.h: tiles; window -1 = none, 0 = the defaults
    // the order of the cells INSIDE a bucket of the stream's two copies (local_seeds.h): sub-anchors per bucket (0: the
    // default, 1: caller order, at most 64) and how they are ranked (0: along their first principal direction, 1: by index)
    int two_level_sub = 0, two_level_sub_rank = 0;
    // the ordered main launch skips the sub-buckets its workgroups' rows cannot reach (bucket_skip.h): 0 where the planner
    // took the stream at its default setting (two_level = 1), 1 off, 2 wherever the ordered main launch runs
    int bucket_skip = 0;
};
bool option_set(Options &o, const char *name, int64_t value);

// What the launch planners may read of an index: its shape, the filter kernels that serve it, its options.  make_shape
// decides it from the arguments and the mode string alone -- no device state -- so that nabo_query_plan can describe an
// index that does not exist.
//   mode (NABO_L2_MODE at nabo_index_create): unset / "f16x1" -- the DEFAULT chain: one-product pass (l2c_topk.hip, g <= 125)
//   -> seeded one-product pass -> f16x3 split (l2q_topk.hip, g < 64 and k' <= 28) or fp32-MFMA filter (l2_topk.hip) ->
//   64-entry lists -> exact float64 kernels;  "f16x3": the f16x3 split is the first pass;  "f32": the fp32-MFMA filter is.
//   (The match is on the prefix: "f16x3h" / "f16x3s" select the f16x3 chain, any other string the default one.)
struct IndexShape {
    int64_t n = 0;
    int g = 0;
    int metric = 0;
    int n_cu = 256;
    // Euclidean / cosine filter.  mode 0: fp32 MFMA only (l2_topk.hip); mode 1: f16x3 split on the f16 matrix pipe
    // (l2q_topk.hip: K-concatenated operands in the layout16 packing, kc steps of 16 slots; g < 64) -- and the fp32 kernel
    // for everything else
    int mode = 0;
    int kc = 0;
    // One-product first pass (l2q kernel on [hi | norm | error] operands of kc1 steps, pack_ctiles_kernel<.,.,1>): rows it
    // cannot certify go through the f16x3 pass (no_coarse), then the 64-entry lists, then the exact kernels.
    // Passes of a query, each on the rows the one before could not certify (PassCtx::pass_level while query_impl recurses):
    //   0  one-product pass, lists built from +inf;  1  one-product pass SEEDED with the thresholds refine.hip derived
    //   from the failed certificates (l2c kernel only; 32-entry lists);  2  the f16x3 pass;  then the 64-entry lists
    //   (wide_retry) and the exact float64 kernels.
    bool coarse = false;
    int kc1 = 0;
    int ksteps = 0;                // -1: g > NABO_MAX_COMPS, every query takes the exact float64 route
    int64_t ref_tiles = 0, ref_tiles_alloc = 0;      // 32-reference tiles; + room for split padding
    bool cb_bits = false;          // modified Canberra: these references have bitmaps (canberra_bits.hip; set at set_ref)
    int cand_slack = 3;            // candidate mode on the one-product pass: kept entries beyond the emitted ones
    Options opt;
};
IndexShape make_shape(int64_t n, int g, int metric, int n_cu, const char *l2_mode);

// Which link of the pass chain a call of query_impl is.  The entry points pass the top-level one; rerun_failed_rows
// builds the inner call's.
struct PassCtx {
    int pass_level = 0;
    bool wide_retry = false;       // the second-chance pass (64-entry lists for the rows the first pass could not certify)
    const float *seed_tau = nullptr;                     // level 1: one threshold per row of the batch
    const std::vector<uint32_t> *row_map = nullptr;      // rows of this batch -> rows of the top-level query (null at the top)
    bool top = true;               // the top-level call: the per-row pass record starts over
    bool coarse_weak = false;      // nabo_index::Refs::L2::coarse_weak when the query started
    bool tl_no = false;            // nabo_index::Refs::L2::stream_verdict said no when the query started: the caller-order stream
    bool first() const { return pass_level == 0 && !wide_retry; }
};

// What a call of query_impl hands back to the frame that reran rows through it.
struct PassResult {
    unsigned int n_fail = 0;       // rows that still needed the exact kernels
    double ms = 0.0;               // total of the call
};

// ---- the launch plan of an Euclidean / cosine filter pass -------------------------------------------------------------------
// Everything the launch logic decides -- which kernel, in which geometry, how long the lists, how the reference range and the
// target rows are cut -- from the index's SHAPE and options and the query's shape alone: no device call, no state change.
// query_body executes it; nabo_query_plan returns it for an index that need not exist (tests/test_host_logic.py checks the
// rules on the CPU box: >= 256 workgroups whenever m x n allows, list lengths per pass, split bounds).
struct L2Plan {
    int epl = 1, L = 32;                 // emitted candidate lists hold L = 32 epl entries
    bool use_h = false;                  // an f16 kernel runs (one-product or f16x3 operands); false: the fp32-MFMA filter
    bool use_1 = false;                  // one-product operands
    bool on_l2c = false;                 // ... on the l2c kernel (geo: its geometry)
    bool slots2 = false;                 // ... in the two-level slot order (two_level_slots: a property of the index)
    bool tl_main = false;                // the main launch streams bucket-ordered operands with the one-step loop (l2c_topk.hip)
    bool tl_skip = false;                // ... and skips the sub-buckets a workgroup's rows cannot reach (bucket_skip.h)
    bool r1 = false;                     // fp32 filter: one row-block per wave
    int geo = -1, kcq = 0, cslack = 0;
    int rows_per_wg = 256, wg_per_cu = 1, lkeep_max = 32, lkeep = 16, want = 16;
    int S = 1, S2 = 1;                   // reference splits of the main / tail launch
    bool one_round = false;              // fewer column-workgroups than slots: splits (+ a tail launch on long streams) fill one round
    int64_t gx = 0, gx_main = 0, gx_tail = 0, rows_pad = 0, tps = 0, tps2 = 0;
    // first target row of the tail launch: gx_main rows_per_wg, or fewer where the two-level main launch ends on whole rounds
    int64_t rows_main = 0;
    char kernel[160] = "";
};
// entries per lane of the emitted candidate lists (they hold 32 epl entries): 64-entry lists for k' > 24 and the wide retry
inline int list_epl(const PassCtx &ctx, int kk, bool cand_mode) { return ((kk <= 24 && !ctx.wide_retry) || cand_mode) ? 1 : 2; }
int plan_l2(const IndexShape &sh, const PassCtx &ctx, int64_t m, int k, int drop, bool cand_mode, L2Plan *P);
// local tournament seeds (local_seeds.hip): anchors and references kept per bucket of an index of this shape (*C = 0: none),
// and whether a launch of `rows` target rows over S reference splits takes its seeds from them
// the one-product operands of an index of this shape are packed in the two-level slot order (l2c_slots.h)
bool two_level_slots(const IndexShape &sh);
void shape_refresh(IndexShape &sh);          // kc1 after a change of options (g = 29 under option two_level = 2)
void lseed_params(const IndexShape &sh, int *C, int *cap);
int lseed_sub_param(const IndexShape &sh);      // sub-anchors per bucket of the two-level stream's copies (1: no sub-order)
bool bskip_wanted(const IndexShape &sh);        // the skip tables are built with the ordered copy (option bucket_skip, bucket_skip.h)
bool lseed_applies(const IndexShape &sh, const L2Plan &P, int S, int64_t rows);

struct CbPlan {
    int64_t gx_exact = 0;            // exact kernel: workgroups (64 rows each) and reference splits
    int S_exact = 1;
    bool bits = false;               // counting pass on bitmaps (canberra_bits.hip), else the SWAR count (canberra_f32.hip)
    int lists = 1;                   // candidate lists per (row, split): one per wave
    int Sf = 1, S2 = 1;              // counting pass: reference splits of the main launch / the tail round
    int64_t rows_main = 0;           // ... target rows of the main launch (the rest: the tail round)
};
int cb_exact_splits(int64_t gx, int64_t n_chunks);
void plan_canberra(const IndexShape &sh, int64_t m, int epl, CbPlan *C);

}  // namespace nabo

struct nabo_index {
    // ---- fixed at nabo_index_create (shape.opt: nabo_index_set_option) ----
    int device = 0;
    nabo::IndexShape shape;
    double f = 0.25;
    int64_t base = 0;
    int cb_mode = 0;              // NABO_CANBERRA_MODE at creation: 0 by size, 1 exact kernel only, 2 SWAR count, 3 bitmaps
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {};
    // second stream: the refine of the main launch's rows runs beside the (short, split) tail launch of the filter
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_main = nullptr, ev_ref = nullptr;
    bool shard_mode = false;       // set by nabo_sharded_query around its local queries: no masked tail (see tail_len)

    // ---- the resident references: change at nabo_index_set_ref / nabo_index_set_mask ----
    struct Refs {
        bool have = false;
        const double *dY = nullptr;      // [n,g] float64 on device (borrowed or == ybuf)
        nabo::DevBuf ybuf, maskbuf, mlistbuf;
        const uint8_t *dmask = nullptr;
        int64_t n_masked = 0;
        int n_masked_list = 0;
        struct L2 {                      // Euclidean / cosine: operands of the MFMA filters
            const double *dYp = nullptr;     // what the MFMA filter packs: dY, or the unit-length rows (cosine)
            nabo::DevBuf ynbuf;
            // Set when the one-product passes of a query (>= 1024 rows) left more than a quarter of the rows to the pass behind
            // them: the bound 2^-9 ||x|| ||y|| is too weak for this reference set (tight clusters far from the centre of the data),
            // and the next queries start with the pass behind it right away.  Cleared by set_ref / set_mask.
            bool coarse_weak = false;
            double hscale = 1.0;
            double fscale = 1.0;           // power-of-two input scale of the fp32 path: max |y~| * fscale in (1/2, 1]
            nabo::DevBuf centre, ypk, ycpk, ycpk1, normmax;
            bool packed_f32 = false, packed_c16 = false, packed_c1 = false;
            bool slots2 = false;             // the slot order ycpk1 was packed in (two_level_slots when it was packed)
            // the bucket order (bucket_order.h; ensure_local_seeds): anchors, the runs' room behind ycpk1, the ordered copy
            // the two-level stream reads and its sub-order; and whether this index's DATA takes that stream at all --
            // remembered across repacks, unlike everything else here (two_level_verdict.h)
            nabo::BucketRefs buckets;
            nabo::TwoLevelVerdict stream_verdict;
            double ymax_sqrt = 0.0, ymax_sqrt_c = 0.0;
            // the largest reference norm of the last pack, on its way to the host (ensure_packed / ymax_resolve): pinned word,
            // the event behind its copy, which of the two values it becomes and the scale it was packed with
            unsigned int *ymax_host = nullptr;
            hipEvent_t ev_ymax = nullptr;
            bool ymax_pending = false, ymax_f32 = false;
            double ymax_scale = 1.0;
        } l2;
        struct Canberra {                // exact kernel operands (yt) and the fp32 lower-bound filter's (ycf)
            nabo::DevBuf yt, ycf, yrow, cbflag, ych, cbscale;    // ych: 7-bit operands of the counting pass, cbscale [2g] doubles (min, 1/step)
            int gp = 0;
            bool f32 = false;             // filter usable for these references (fits fp32, g <= 128)
            // bit-sliced counting pass (canberra_bits.hip): quantile edges [g][B-1], cumulative bitmaps, valid bits
            nabo::DevBuf cbedges, cbtab, cbvalid;
        } cb;
    } ref;

    // ---- query workspace ----
    struct Workspace {
        // Rows a pass could not certify, rerun one link down the pass chain (rerun_failed_rows): their row numbers, targets,
        // the inner call's results and seeds.  One set per frame -- level 0, level 1, and [RERUN_WIDE] for the frame that sends
        // rows to the 64-entry lists -- so that nested frames never share one; the modified-Canberra re-solve and set_ref's
        // sample gather borrow [RERUN_WIDE].
        struct RerunBufs { nabo::DevBuf rows, x, idx, dist, seed; } rerun[3];
        nabo::DevBuf exact_d, failseed;
        nabo::DevBuf taupre, taupre2;             // tournament seeds of the main / tail launch of the one-product pass [rows][S]
        nabo::DevBuf cand_key, cand_key2, cand_mi, cand_mt, cand_mi2, cand_mt2;   // filter keys of the lists; merged lists (merge_lists_kernel)
        nabo::DevBuf xbuf, xnbuf, xpk, xnorm, cand_idx, cand_tau, cand_idx2, cand_tau2, cand_d, fails, failcnt, oidx, odist, nfound;
        nabo::DevBuf xh, cbrow;                   // modified Canberra: 7-bit target operands; target row numbers of the bitmap pass
        nabo::BucketScratch buckets;              // the sorts into bucket order, and what a launch's sort hands to its filter (bucket_order.h)
    } ws;

    // ---- the last query's record (the nabo_index_last_* getters) ----
    struct LastQuery {
        int64_t pre_tiles_last = 0;               // reference tiles per split the last query's tournament looked at (0: none)
        int64_t pass_rows[3] = {0, 0, 0};         // rows of the last query sent to the seeded pass / the f16x3 pass / the 64-entry lists
        // Which pass ANSWERED each row of the last top-level query (nabo_index_last_row_pass; NABO_PASS_* of nabo_knn.h): the
        // first filter's code for every row, overwritten as fail lists go down the chain.
        std::vector<uint8_t> row_pass;
        double ms[5] = {0, 0, 0, 0, 0};
        int64_t counters[4] = {0, 0, 0, 0};
        char kernel[256] = "";          // dominant kernel of the last query (nabo_index_last_kernel)
    } last;

    // nabo_index_query_async: the query runs on a host thread of its own (it synchronises its stream between its passes);
    // one in flight per index, joined by nabo_index_query_wait / any other call that needs the index
    std::thread async_thread;
    bool async_busy = false;
    int async_rc = NABO_OK;
    char async_msg[512] = "";
};

namespace nabo {

constexpr int RERUN_WIDE = 2;     // nabo_index::Workspace::rerun: the set of the frame that sends rows to the 64-entry lists

// api.hip: NABO_OK, or the refusal while an asynchronous query is in flight on the index
int index_idle(const nabo_index *ix);
// set_ref.hip
int ensure_packed(nabo_index *ix, int want);
int ymax_resolve(nabo_index *ix);
int ensure_local_seeds(nabo_index *ix);
// bucket_order.hip: bucket_sort (bucket_order.h)
// query.hip
int query_impl(nabo_index *ix, const PassCtx &ctx, const double *X, int32_t x_on_device, int64_t m, int32_t k, int32_t drop_first,
               int64_t *out_idx, double *out_dist, int32_t out_on_device, bool cand_mode, double *out_bound, PassResult *res);

}  // namespace nabo

// api.hip -- C ABI of libnabo_knn.so (include/nabo_knn.h).  Host orchestration only:
// buffer management, kernel sequencing on the index's HIP stream, HIP-event timing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/nabo_knn.h"
#include "host_common.h"
#include "knn_common.h"

using nabo::api_fail;
using nabo::DevBuf;
using nabo::use_device;

namespace {

int pick_ksteps(int g)
{
    const int need = (g + 1) / 2;
    const int inst[] = {8, 16, 25, 32, 50, 64};
    for (int v : inst)
        if (need <= v) return v;
    return -1;
}

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
};

struct OptionName { const char *name; int Options::*field; };
const OptionName OPTION_NAMES[] = {
    {"splits", &Options::splits}, {"tail_split", &Options::tail_split}, {"lkeep", &Options::lkeep},
    {"coarse_slack", &Options::coarse_slack}, {"cand_slack", &Options::cand_slack}, {"seeded_pass", &Options::seeded_pass},
    {"coarse_adapt", &Options::coarse_adapt}, {"wide_retry", &Options::wide_retry}, {"refine_overlap", &Options::refine_overlap},
    {"prepass", &Options::prepass}, {"pieces", &Options::pieces}, {"merge_lists", &Options::merge_lists}, {"one_round", &Options::one_round}, {"l2c_geo", &Options::l2c_geo}, {"l2_r1", &Options::l2_r1},
    {"split_refs_max", &Options::split_refs_max}, {"cosine_centre", &Options::cosine_centre},
    {"coarse_kernel_q", &Options::coarse_kernel_q}, {"order_flags", &Options::order_flags},
};

bool option_set(Options &o, const char *name, int64_t value)
{
    for (const OptionName &e : OPTION_NAMES)
        if (strcmp(e.name, name) == 0) {
            o.*(e.field) = (int)value;
            return true;
        }
    return false;
}

constexpr int RERUN_WIDE = 2;     // nabo_index::rerun: the set of the frame that sends rows to the 64-entry lists

}  // namespace

struct nabo_index {
    int device = 0;
    int64_t n = 0;
    int g = 0;
    int metric = 0;
    double f = 0.25;
    int64_t base = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {};
    // second stream: the refine of the main launch's rows runs beside the (short, split) tail launch of the filter
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_main = nullptr, ev_ref = nullptr;
    bool have_ref = false;

    const double *dY = nullptr;      // [n,g] float64 on device (borrowed or == ybuf)
    const double *dYp = nullptr;     // what the MFMA filter packs: dY, or the unit-length rows (cosine)
    DevBuf ybuf, ynbuf, xnbuf, maskbuf, mlistbuf;
    const uint8_t *dmask = nullptr;
    int64_t n_masked = 0;
    int n_masked_list = 0;
    bool shard_mode = false;       // set by nabo_sharded_query around its local queries: no masked tail (see tail_len)

    // Euclidean / cosine filter.  mode 0: fp32 MFMA only (l2_topk.hip); mode 1: f16x3 split on the f16 matrix pipe
    // (l2q_topk.hip: K-concatenated operands in the layout16 packing, kc steps of 16 slots; g < 64) -- and the fp32 kernel
    // for everything else
    int mode = 0;
    int kc = 0;
    // One-product first pass (l2q kernel on [hi | norm | error] operands of kc1 steps, pack_ctiles_kernel<.,.,1>): rows it
    // cannot certify go through the f16x3 pass (no_coarse), then the 64-entry lists, then the exact kernels.
    // Passes of a query, each on the rows the one before could not certify (pass_level while query_impl recurses):
    //   0  one-product pass, lists built from +inf;  1  one-product pass SEEDED with the thresholds refine.hip derived
    //   from the failed certificates (l2c kernel only; 32-entry lists);  2  the f16x3 pass;  then the 64-entry lists
    //   (wide_retry) and the exact float64 kernels.
    bool coarse = false;
    // Set when the one-product passes of a query (>= 1024 rows) left more than a quarter of the rows to the pass behind
    // them: the bound 2^-9 ||x|| ||y|| is too weak for this reference set (tight clusters far from the centre of the data),
    // and the next queries start with the pass behind it right away.  Cleared by set_ref / set_mask.
    bool coarse_weak = false;
    int pass_level = 0;
    const float *seed_tau = nullptr;      // level 1: one threshold per row of the batch
    int kc1 = 0;
    double hscale = 1.0;
    double fscale = 1.0;           // power-of-two input scale of the fp32 path: max |y~| * fscale in (1/2, 1]
    int ksteps = 0;
    DevBuf centre, ypk, ycpk, ycpk1, normmax;
    bool packed_f32 = false, packed_c16 = false, packed_c1 = false;
    int64_t ref_tiles = 0, ref_tiles_alloc = 0;
    double ymax_sqrt = 0.0, ymax_sqrt_c = 0.0;
    // the largest reference norm of the last pack, on its way to the host (ensure_packed / ymax_resolve): pinned word,
    // the event behind its copy, which of the two values it becomes and the scale it was packed with
    unsigned int *ymax_host = nullptr;
    hipEvent_t ev_ymax = nullptr;
    bool ymax_pending = false, ymax_f32 = false;
    double ymax_scale = 1.0;
    // Canberra path: exact kernel operands (yt) and the fp32 lower-bound filter's (ycf)
    DevBuf yt, ycf, yrow, cbflag, ych, cbscale, xh;    // ych/xh: 7-bit operands of the counting pass, cbscale [2g] doubles (min, 1/step)
    int cb_gp = 0;
    bool cb_f32 = false;          // filter usable for these references (fits fp32, g <= 128)
    // bit-sliced counting pass (canberra_bits.hip): quantile edges [g][B-1], cumulative bitmaps, valid bits, target row numbers
    DevBuf cbedges, cbtab, cbvalid, cbrow;
    bool cb_bits = false;
    int cb_mode = 0;              // NABO_CANBERRA_MODE at creation: 0 by size, 1 exact kernel only, 2 SWAR count, 3 bitmaps

    // query workspace
    // Rows a pass could not certify, rerun one link down the pass chain (rerun_failed_rows): their row numbers, targets,
    // the inner call's results and seeds.  One set per frame -- level 0, level 1, and [RERUN_WIDE] for the frame that sends
    // rows to the 64-entry lists -- so that nested frames never share one; the modified-Canberra re-solve and set_ref's
    // sample gather borrow [RERUN_WIDE].
    struct RerunBufs { DevBuf rows, x, idx, dist, seed; } rerun[3];
    DevBuf exact_d, failseed;
    DevBuf taupre, taupre2;                   // tournament seeds of the main / tail launch of the one-product pass [rows][S]
    DevBuf cand_key, cand_key2, cand_mi, cand_mt, cand_mi2, cand_mt2;   // filter keys of the lists; merged lists (merge_lists_kernel)
    int64_t pre_tiles_last = 0;               // reference tiles per split the last query's tournament looked at (0: none)
    int cand_slack = 3;                       // candidate mode on the one-product pass: kept entries beyond the emitted ones
    int64_t pass_rows[3] = {0, 0, 0};         // rows of the last query sent to the seeded pass / the f16x3 pass / the 64-entry lists
    // Which pass ANSWERED each row of the last top-level query (nabo_index_last_row_pass; NABO_PASS_* of nabo_knn.h): the
    // first filter's code for every row, overwritten as fail lists go down the chain.  row_map: rows of the batch a nested
    // query_impl works on -> rows of the top-level query (null at the top); depth: nesting level of query_impl.
    std::vector<uint8_t> row_pass;
    const std::vector<uint32_t> *row_map = nullptr;
    int depth = 0;
    float ms_keep[3] = {0, 0, 0};
    double ms_inner = 0.0;         // total of the most recent query_impl (read by the outer call of a retry)
    bool ms_keep_valid = false;
    bool wide_retry = false;       // inside the second-chance pass (64-entry lists for the rows the first pass could not certify)
    DevBuf xbuf, xpk, xnorm, cand_idx, cand_tau, cand_idx2, cand_tau2, cand_d, fails, failcnt, oidx, odist, nfound;
    int n_cu = 256;
    Options opt;

    double ms[5] = {0, 0, 0, 0, 0};
    int64_t counters[4] = {0, 0, 0, 0};
    char kernel[160] = "";          // dominant kernel of the last query (nabo_index_last_kernel)
    // nabo_index_query_async: the query runs on a host thread of its own (it synchronises its stream between its passes);
    // one in flight per index, joined by nabo_index_query_wait / any other call that needs the index
    std::thread async_thread;
    bool async_busy = false;
    int async_rc = NABO_OK;
    char async_msg[512] = "";
};

namespace nabo {
int index_device(const nabo_index *ix) { return ix->device; }
int index_g(const nabo_index *ix) { return ix->g; }
int64_t index_n(const nabo_index *ix) { return ix->n; }
int index_metric(const nabo_index *ix) { return ix->metric; }
bool index_can_emit_candidates(const nabo_index *ix) { return ix->metric != NABO_METRIC_MOD_CANBERRA && ix->ksteps > 0; }
void index_set_shard_mode(nabo_index *ix, bool on) { ix->shard_mode = on; }
void index_set_cand_slack(nabo_index *ix, int s) { ix->cand_slack = s < 0 ? 0 : s; }
}  // namespace nabo


// Which filter kernels serve an index of this shape (n, g, metric are set): decided from the arguments and the mode string
// alone -- no device state -- so that nabo_query_plan can describe an index that does not exist.
//   mode (NABO_L2_MODE at nabo_index_create): unset / "f16x1" -- the DEFAULT chain: one-product pass (l2c_topk.hip, g <= 125)
//   -> seeded one-product pass -> f16x3 split (l2q_topk.hip, g < 64 and k' <= 28) or fp32-MFMA filter (l2_topk.hip) ->
//   64-entry lists -> exact float64 kernels;  "f16x3": the f16x3 split is the first pass;  "f32": the fp32-MFMA filter is.
//   (The match is on the prefix: "f16x3h" / "f16x3s" select the f16x3 chain, any other string the default one.)
static void index_init_filters(nabo_index *ix, const char *md)
{
    const int g = ix->g;
    ix->mode = 0;
    ix->kc = ix->kc1 = 0;
    ix->coarse = false;
    ix->ksteps = 0;
    if (ix->metric == NABO_METRIC_MOD_CANBERRA) return;
    ix->ksteps = pick_ksteps(g);           // -1: g > NABO_MAX_COMPS, every query takes the exact float64 route
    const bool f32 = md && strcmp(md, "f32") == 0, f16x3 = md && strncmp(md, "f16x3", 5) == 0;
    if (ix->ksteps <= 0) return;
    if (!f32 && nabo::l2q_pick_kc(g) > 0) {
        ix->mode = 1;                       // an f16x3 kernel exists for this g (g < 64)
        ix->kc = nabo::l2q_pick_kc(g);
        ix->kc1 = nabo::l2c_pick_kc(g);
        ix->coarse = ix->kc1 > 0 && !f16x3;
    } else if (!f32 && !f16x3 && nabo::l2c_pick_kc(g) > 0) {
        // 64 <= g <= 125: no f16x3 kernel is instantiated, but the one-product operands (g + 3 slots: four steps of 32)
        // are -- the one-product pass runs first, the fp32-MFMA filter takes the rows it cannot certify
        ix->kc1 = nabo::l2c_pick_kc(g);
        ix->coarse = true;
    }
}

// Entries of the masked-reference list a row may continue with when it has fewer than k' unmasked references
// (numpy.ma's NaN fill sorts the ignored references last, by index: nabo/_mapping.py:135-146).  A SHARD must not do
// that: its masked references would enter the global merge as if they were neighbours (found by the randomised
// sweep: 40-reference shards, 60 % masked) -- there the tail is left absent (index -1), which the merge skips.
static int tail_len(const nabo_index *ix) { return ix->shard_mode ? 0 : ix->n_masked_list; }

// The rows of the current batch listed in `d_rows` (device, nf entries) go on to the pass `code`: note it per top-level row and
// return their top-level row numbers in `map` (the inner query_impl's row_map).  The stream is synchronised.
static int note_row_pass(nabo_index *ix, const uint32_t *d_rows, int64_t nf, uint8_t code, std::vector<uint32_t> &map)
{
    map.resize((size_t)nf);
    if (nf == 0) return NABO_OK;
    HIP_TRY(hipMemcpyAsync(map.data(), d_rows, (size_t)nf * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    for (int64_t i = 0; i < nf; ++i) {
        if (ix->row_map) map[(size_t)i] = map[(size_t)i] < ix->row_map->size() ? (*ix->row_map)[map[(size_t)i]] : 0xFFFFFFFFu;
        if (map[(size_t)i] < ix->row_pass.size()) ix->row_pass[map[(size_t)i]] = code;
    }
    return NABO_OK;
}

static int ymax_resolve(nabo_index *ix);

// Pack the resident references for the fp32-MFMA kernel (want = 0), the f16x3 kernels (1: K-concatenated f16 tiles) or
// the one-product pass of the l2q kernel (2).
static int ensure_packed(nabo_index *ix, int want)
{
    const bool want_h = want != 0;
    if (want == 2 ? ix->packed_c1 : want == 1 ? ix->packed_c16 : ix->packed_f32) return NABO_OK;
    hipStream_t st = ix->stream;
    int rc;
    if ((rc = ymax_resolve(ix))) return rc;                   // (a pack of other operands still owes its norm: normmax is reused)
    // normmax: [0] = max ||y~||^2 (float bits, SCALED units), [2..3] = max |y~ component| (double bits)
    if ((rc = ix->normmax.reserve(4 * sizeof(unsigned int)))) return rc;
    HIP_TRY(hipMemsetAsync(ix->normmax.p, 0, 4 * sizeof(unsigned int), st));
    unsigned int bits[4] = {0, 0, 0, 0};
    // power-of-two input scale from the largest centred component: the filter then works in a fixed numeric range
    // whatever the unit of the data (1e-30 or 1e+19 per component would under- / overflow fp32 squares otherwise)
    HIP_TRY(nabo::maxabs_launch(ix->dYp, ix->n, ix->g, ix->centre.as<double>(),
                                reinterpret_cast<unsigned long long *>(ix->normmax.as<unsigned int>() + 2), st));
    HIP_TRY(hipMemcpyAsync(bits, ix->normmax.p, sizeof(bits), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    double amax;
    memcpy(&amax, &bits[2], sizeof(amax));
    int e2 = 0;                                              // 2^e2 * amax in (1/2, 1]
    if (amax > 0 && std::isfinite(amax)) e2 = -(int)std::ceil(std::log2(amax));
    if (e2 > 480) e2 = 480;                                  // scale^2 must stay finite in float64
    if (e2 < -480) e2 = -480;
    double scale;
    if (want == 2) {
        if ((rc = ix->ycpk1.reserve((size_t)ix->ref_tiles_alloc * ix->kc1 * 1024 + 128))) return rc;
        ix->hscale = scale = std::ldexp(1.0, e2 + 12);
        HIP_TRY(nabo::pack_cref_launch(ix->dYp, ix->n, ix->g, ix->centre.as<double>(), ix->hscale, ix->kc1,
                                       ix->ref_tiles_alloc, ix->dmask, ix->ycpk1.as<unsigned char>(),
                                       ix->normmax.as<unsigned int>(), true, st, nullptr, 1));
    } else if (want_h) {
        if ((rc = ix->ycpk.reserve((size_t)ix->ref_tiles_alloc * ix->kc * 1024 + 128))) return rc;
        // |v| <= 2^12 after scaling (f16 overflows at 65504; targets carry a factor 2)
        ix->hscale = scale = std::ldexp(1.0, e2 + 12);
        HIP_TRY(nabo::pack_cref_launch(ix->dYp, ix->n, ix->g, ix->centre.as<double>(), ix->hscale, ix->kc,
                                       ix->ref_tiles_alloc, ix->dmask, ix->ycpk.as<unsigned char>(),
                                       ix->normmax.as<unsigned int>(), true, st));
    } else {
        const int Q = (ix->ksteps + 3) / 4;
        const size_t tile_bytes = ((size_t)Q * 256 + 32) * sizeof(float);
        if ((rc = ix->ypk.reserve((size_t)ix->ref_tiles_alloc * tile_bytes))) return rc;
        ix->fscale = scale = std::ldexp(1.0, e2);
        HIP_TRY(nabo::pack_ref_launch(ix->dYp, ix->n, ix->g, ix->centre.as<double>(), ix->fscale, ix->ksteps,
                                      ix->ref_tiles_alloc, ix->dmask, ix->ypk.as<float>(), ix->normmax.as<unsigned int>(), st));
    }
    // The largest norm is read by nobody before the refine launch takes it as an argument: the copy goes to pinned memory
    // behind the pack and the host goes on enqueueing (target pack, tournament, filter); ymax_resolve waits for it.
    if (!ix->ymax_host) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ix->ymax_host), sizeof(unsigned int), hipHostMallocDefault));
    HIP_TRY(hipMemcpyAsync(ix->ymax_host, ix->normmax.p, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(ix->ev_ymax, st));
    ix->ymax_pending = true;
    ix->ymax_f32 = !want_h;
    ix->ymax_scale = scale;
    if (want == 2) ix->packed_c1 = true;
    else if (want_h) ix->packed_c16 = true;
    else ix->packed_f32 = true;
    return NABO_OK;
}

// ymax_sqrt / ymax_sqrt_c of the last pack, once its copy has arrived (every reader of the two calls this first)
static int ymax_resolve(nabo_index *ix)
{
    if (!ix->ymax_pending) return NABO_OK;
    HIP_TRY(hipEventSynchronize(ix->ev_ymax));
    ix->ymax_pending = false;
    float fmax;
    memcpy(&fmax, ix->ymax_host, sizeof(fmax));
    const double v = std::sqrt((double)fmax) / ix->ymax_scale * (1.0 + 1e-6);      // unscaled units
    if (ix->ymax_f32) ix->ymax_sqrt = v;
    else ix->ymax_sqrt_c = v;
    return NABO_OK;
}

// mask + ascending list of the first masked indices (order-row tail, nabo/_mapping.py:135-144)
static int apply_mask(nabo_index *ix, const uint8_t *ref_mask)
{
    hipStream_t st = ix->stream;
    int rc;
    ix->dmask = nullptr;
    ix->n_masked = 0;
    ix->n_masked_list = 0;
    if (ref_mask) {
        std::vector<uint32_t> lst;
        for (int64_t j = 0; j < ix->n; ++j)
            if (ref_mask[j]) {
                ++ix->n_masked;
                lst.push_back((uint32_t)j);          // all of them: the exact route serves any k (order-row tail)
            }
        if (ix->n_masked > 0) {
            if ((rc = ix->maskbuf.reserve((size_t)ix->n))) return rc;
            HIP_TRY(hipMemcpyAsync(ix->maskbuf.p, ref_mask, (size_t)ix->n, hipMemcpyHostToDevice, st));
            ix->dmask = ix->maskbuf.as<uint8_t>();
            if ((rc = ix->mlistbuf.reserve(lst.size() * sizeof(uint32_t)))) return rc;
            HIP_TRY(hipMemcpyAsync(ix->mlistbuf.p, lst.data(), lst.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));      // lst goes out of scope
            ix->n_masked_list = (int)lst.size();
        }
    }
    return NABO_OK;
}

static thread_local char g_err[512] = "";      // nabo_last_error(): this thread's last message

int nabo::api_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" {

const char *nabo_version(void) { return "nabo_knn 0.1 (gfx950)"; }
const char *nabo_last_error(void) { return g_err; }

int nabo_device_count(void)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt < 0 ? 0 : cnt;
}

int nabo_index_create(nabo_index **out, int32_t device, int64_t n_ref, int32_t g, int32_t metric,
                      double dist_factor, int64_t ref_index_base)
{
    if (!out) return api_fail(NABO_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n_ref < 1 || n_ref >= 0xFFFFFFF0ll) return api_fail(NABO_E_INVALID, "n_ref=%lld out of range", (long long)n_ref);
    if (g < 1) return api_fail(NABO_E_INVALID, "g=%d must be >= 1", g);
    if (metric != NABO_METRIC_EUCLIDEAN && metric != NABO_METRIC_MOD_CANBERRA && metric != NABO_METRIC_COSINE)
        return api_fail(NABO_E_INVALID, "unknown metric %d", metric);
    if (metric == NABO_METRIC_MOD_CANBERRA && !(dist_factor > 0))
        return api_fail(NABO_E_INVALID, "dist_factor must be > 0");          // nabo/_mapping.py:516-521
    if (ref_index_base < 0) return api_fail(NABO_E_INVALID, "ref_index_base must be >= 0");
    // the shard merge carries global indices as 32-bit payloads (0xFFFFFFFF = absent)
    if (ref_index_base + n_ref > 0xFFFFFFFEll)
        return api_fail(NABO_E_UNSUPPORTED, "ref_index_base + n_ref = %lld exceeds 2^32 - 2", (long long)(ref_index_base + n_ref));
    int rc = use_device(device);
    if (rc) return rc;
    nabo_index *ix = new (std::nothrow) nabo_index();
    if (!ix) return api_fail(NABO_E_NOMEM, "host allocation failed");
    ix->device = device;
    ix->n = n_ref;
    ix->g = g;
    ix->metric = metric;
    ix->f = dist_factor;
    ix->base = ref_index_base;
    {   // NABO_CANBERRA_MODE = exact | swar | bits pins the modified-Canberra path (default: by the size of the reference set)
        const char *cmode = getenv("NABO_CANBERRA_MODE");
        ix->cb_mode = !cmode ? 0 : strcmp(cmode, "exact") == 0 ? 1 : strcmp(cmode, "swar") == 0 ? 2 : strcmp(cmode, "bits") == 0 ? 3 : 0;
    }
    index_init_filters(ix, getenv("NABO_L2_MODE"));
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
        ix->n_cu = cus;
    hipError_t e = hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking);
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipEventCreate(&ix->ev[i]);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ix->stream2, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ix->ev_main, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ix->ev_ref, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ix->ev_ymax, hipEventDisableTiming);
    if (e != hipSuccess) {
        nabo_index_destroy(ix);
        return api_fail(NABO_E_HIP, "stream/event creation failed: %s", hipGetErrorString(e));
    }
    *out = ix;
    return NABO_OK;
}

int nabo_index_set_option(nabo_index *ix, const char *name, int64_t value)
{
    if (!ix || !name) return api_fail(NABO_E_INVALID, "NULL argument");
    if (ix->async_busy) return api_fail(NABO_E_INVALID, "an asynchronous query is in flight on this index: nabo_index_query_wait first");
    if (!option_set(ix->opt, name, value)) return api_fail(NABO_E_INVALID, "unknown option '%s'", name);
    if (strcmp(name, "order_flags") == 0) {      // (locality-ordered streaming was measured slower and removed)
        ix->opt.order_flags = 0;
        return api_fail(NABO_E_UNSUPPORTED, "option '%s' (locality-ordered streaming, once in experiments builds only) was removed", name);
    }
    return NABO_OK;
}

int nabo_index_destroy(nabo_index *ix)
{
    if (!ix) return NABO_OK;
    if (ix->async_thread.joinable()) ix->async_thread.join();     // (an asynchronous query still in flight: its buffers are the index's)
    (void)hipSetDevice(ix->device);
    if (ix->stream) (void)hipStreamSynchronize(ix->stream);
    for (int i = 0; i < 6; ++i)
        if (ix->ev[i]) (void)hipEventDestroy(ix->ev[i]);
    if (ix->stream2) { (void)hipStreamSynchronize(ix->stream2); (void)hipStreamDestroy(ix->stream2); }
    if (ix->ev_main) (void)hipEventDestroy(ix->ev_main);
    if (ix->ev_ref) (void)hipEventDestroy(ix->ev_ref);
    if (ix->ev_ymax) (void)hipEventDestroy(ix->ev_ymax);
    if (ix->ymax_host) (void)hipHostFree(ix->ymax_host);
    if (ix->stream) (void)hipStreamDestroy(ix->stream);
    delete ix;                       // every DevBuf member frees its allocation (the device is current)
    return NABO_OK;
}

int nabo_index_set_ref(nabo_index *ix, const double *Y, int32_t y_on_device, const uint8_t *ref_mask)
{
    if (!ix || !Y) return api_fail(NABO_E_INVALID, "NULL argument");
    if (ix->async_busy) return api_fail(NABO_E_INVALID, "an asynchronous query is in flight on this index: nabo_index_query_wait first");
    int rc = use_device(ix->device);
    if (rc) return rc;
    hipStream_t st = ix->stream;
    const size_t ybytes = (size_t)ix->n * ix->g * sizeof(double);
    if (y_on_device) {
        ix->dY = Y;
    } else {
        if ((rc = ix->ybuf.reserve(ybytes))) return rc;
        HIP_TRY(hipMemcpyAsync(ix->ybuf.p, Y, ybytes, hipMemcpyHostToDevice, st));
        ix->dY = ix->ybuf.as<double>();
    }
    if ((rc = apply_mask(ix, ref_mask))) return rc;
    if (ix->metric != NABO_METRIC_MOD_CANBERRA && ix->ksteps < 0) {
        HIP_TRY(hipStreamSynchronize(st));             // exact route only: the float64 rows are all it needs
    } else if (ix->metric != NABO_METRIC_MOD_CANBERRA) {
        ix->ref_tiles = (ix->n + 31) / 32;
        ix->ref_tiles_alloc = ix->ref_tiles + 64;      // room for split padding (+inf-norm tiles; up to 32 splits)
        ix->packed_f32 = ix->packed_c16 = ix->packed_c1 = false;
        ix->ymax_pending = false;                      // (a read still in flight belongs to operands that are gone)
        ix->coarse_weak = false;
        if ((rc = ix->centre.reserve((size_t)ix->g * sizeof(double)))) return rc;
        if (ix->metric == NABO_METRIC_COSINE) {
            // cosine: the filter sees the unit-length rows x^, y^ and works on ||x^ - y^||^2 = 2 (1 - cos).  That quantity is
            // translation invariant like any Euclidean distance, so the UNIT rows are centred (a shift BEFORE the
            // normalisation would change angles; after it, it only shortens the vectors the error bounds scale with:
            // unit rows of PCA-like data sit in a cap around their mean direction, ||x^ - c|| is a fraction of 1)
            if ((rc = ix->ynbuf.reserve(ybytes))) return rc;
            HIP_TRY(nabo::normalise_rows_launch(ix->dY, ix->n, ix->g, ix->ynbuf.as<double>(), st));
            if (ix->opt.cosine_centre != 0)
                HIP_TRY(nabo::centre_launch(ix->ynbuf.as<double>(), ix->n, ix->g, ix->centre.as<double>(), st));
            else
                HIP_TRY(hipMemsetAsync(ix->centre.p, 0, (size_t)ix->g * sizeof(double), st));
            ix->dYp = ix->ynbuf.as<double>();
        } else {
            HIP_TRY(nabo::centre_launch(ix->dY, ix->n, ix->g, ix->centre.as<double>(), st));
            ix->dYp = ix->dY;
        }
        if ((rc = ensure_packed(ix, ix->coarse ? 2 : ix->mode == 1 ? 1 : 0))) return rc;
    } else {
        const int64_t chunks = (ix->n + 63) / 64;
        if ((rc = ix->yt.reserve((size_t)chunks * 64 * ix->g * sizeof(double)))) return rc;
        HIP_TRY(nabo::transpose_ref_launch(ix->dY, ix->n, ix->g, ix->yt.as<double>(), st));
        ix->cb_gp = nabo::cbf_pick_gp(ix->g);
        ix->cb_f32 = false;
        ix->cb_bits = false;
        if (ix->cb_gp > 0 && ix->cb_mode != 1) {
            unsigned int flag = 0;
            if ((rc = ix->ycf.reserve((size_t)chunks * 64 * ix->cb_gp * sizeof(float)))) return rc;      // chunk-major (range check)
            if ((rc = ix->yrow.reserve((size_t)ix->n * ix->cb_gp * sizeof(float)))) return rc;           // row-major (bound pass)
            if ((rc = ix->cbflag.reserve(4 * sizeof(unsigned int)))) return rc;
            HIP_TRY(hipMemsetAsync(ix->cbflag.p, 0, 4 * sizeof(unsigned int), st));
            HIP_TRY(nabo::cbf_pack_refs_launch(ix->dY, ix->n, ix->g, ix->cb_gp, ix->ycf.as<float>(), ix->cbflag.as<unsigned int>(), st));
            HIP_TRY(hipMemcpyAsync(&flag, ix->cbflag.p, sizeof(flag), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            ix->cb_f32 = (flag == 0);
            if (ix->cb_f32) {
                // per-dimension quantisation of the counting pass (canberra_f32.hip): min_k and 127 / (max_k - min_k) over the
                // references, from fp32 bounds that enclose every float64 value
                const int G = ix->g;
                std::vector<unsigned int> cm((size_t)2 * G, 0u);
                std::vector<double> sc((size_t)2 * G, 0.0);
                if ((rc = ix->cbscale.reserve((size_t)2 * G * sizeof(double)))) return rc;
                HIP_TRY(hipMemsetAsync(ix->cbscale.p, 0xFF, (size_t)G * sizeof(unsigned int), st));
                HIP_TRY(hipMemsetAsync(ix->cbscale.as<unsigned int>() + G, 0, (size_t)G * sizeof(unsigned int), st));
                HIP_TRY(nabo::cbf_colminmax_launch(ix->dY, ix->n, G, ix->cbscale.as<unsigned int>(), st));
                HIP_TRY(hipMemcpyAsync(cm.data(), ix->cbscale.p, (size_t)2 * G * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                for (int k = 0; k < G; ++k) {
                    auto unord = [](unsigned int u) {
                        const unsigned int b = u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu);
                        float f;
                        memcpy(&f, &b, sizeof(f));
                        return (double)f;
                    };
                    const double lo = unord(cm[(size_t)k]), hi = unord(cm[(size_t)G + k]);
                    sc[(size_t)k] = std::isfinite(lo) ? lo : 0.0;
                    sc[(size_t)G + k] = (std::isfinite(lo) && std::isfinite(hi) && hi > lo && std::isfinite(127.0 / (hi - lo)))
                                            ? 127.0 / (hi - lo) : 0.0;              // 0: constant column, never counted as out
                }
                HIP_TRY(hipMemcpyAsync(ix->cbscale.p, sc.data(), (size_t)2 * G * sizeof(double), hipMemcpyHostToDevice, st));
                if ((rc = ix->ych.reserve((size_t)chunks * 64 * ix->cb_gp * 2))) return rc;
                HIP_TRY(nabo::cbf_pack_refs_rows_launch(ix->dY, ix->n, ix->g, ix->cb_gp, ix->yrow.as<float>(), st));
                HIP_TRY(nabo::cbf_pack_refs8_launch(ix->dY, ix->n, ix->g, ix->cb_gp, ix->cbscale.as<double>(), ix->ych.p, st));
                HIP_TRY(hipStreamSynchronize(st));      // sc goes out of scope
                // Bit-sliced counting pass (canberra_bits.hip), the default for reference sets of >= 12 blocks (25k cells; round 3, 128 blocks:
                // measured 2.0x the SWAR pass at 1M x 1M, level with it at 100k x 100k where building its table costs
                // what it saves; NABO_CANBERRA_MODE=swar pins the 7-bit SWAR pass, =bits the bitmaps at any size): per-dimension
                // QUANTILE bucket edges from a strided sample of the references (any edges give correct results -- they
                // only decide how sharp the count is), cumulative bitmaps per block of 2048 references.
                ix->cb_bits = false;
                // (round 4: from 12 blocks on -- with the four-words-per-lane kernel, its lists seeded before the count starts and
                // the edge sorts on eight host threads (set_ref 3.9 -> 1.2 ms) the bitmaps win from ~25k references even with
                // their table built inside the step: 100k x 100k 13.2 against 25.5 ms, 30k x 30k 3.0 against 3.6; 10k x 10k
                // 2.3 against 1.4 -- the same query time, the table build on top)
                const bool want_bits = ix->cb_mode ? ix->cb_mode == 3 : ix->n >= 12 * 2048;
                if (want_bits && nabo::cbb_available(G, ix->cb_gp, 1)) {
                    const int B = nabo::cbb_buckets();
                    int64_t ns = ix->n < 2048 ? ix->n : 2048;          // (32 sample values per bucket; the sort is host time inside set_ref)
                    const int64_t stride = ix->n / ns;
                    std::vector<double> smp((size_t)ns * G), edges((size_t)G * (B - 1));
                    {   // the sample rows: gathered on the device, ONE contiguous copy back (a strided 2-D copy of 2048 short rows
                        // to pageable memory took milliseconds)
                        std::vector<uint32_t> rows_h((size_t)ns);
                        for (int64_t i = 0; i < ns; ++i) rows_h[(size_t)i] = (uint32_t)(i * stride);
                        nabo_index::RerunBufs &b = ix->rerun[RERUN_WIDE];
                        if ((rc = b.rows.reserve((size_t)ns * sizeof(uint32_t)))) return rc;
                        if ((rc = b.x.reserve((size_t)ns * G * sizeof(double)))) return rc;
                        HIP_TRY(hipMemcpyAsync(b.rows.p, rows_h.data(), (size_t)ns * sizeof(uint32_t), hipMemcpyHostToDevice, st));
                        HIP_TRY(nabo::gather_rows_launch(ix->dY, b.rows.as<uint32_t>(), ns, G, b.x.as<double>(), st));
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
                    {
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
                    }
                    if ((rc = ix->cbedges.reserve(edges.size() * sizeof(double)))) return rc;
                    if ((rc = ix->cbtab.reserve(nabo::cbb_table_bytes(ix->n, G)))) return rc;
                    if ((rc = ix->cbvalid.reserve(nabo::cbb_valid_bytes(ix->n)))) return rc;
                    HIP_TRY(hipMemcpyAsync(ix->cbedges.p, edges.data(), edges.size() * sizeof(double), hipMemcpyHostToDevice, st));
                    HIP_TRY(nabo::cbb_pack_table_launch(ix->dY, ix->n, G, ix->cbedges.as<double>(), ix->cbtab.as<uint32_t>(), st));
                    HIP_TRY(nabo::cbb_valid_launch(ix->dmask, ix->n, ix->cbvalid.as<uint32_t>(), st));
                    HIP_TRY(hipStreamSynchronize(st));      // edges goes out of scope
                    ix->cb_bits = true;
                }
            }
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    ix->have_ref = true;
    return NABO_OK;
}

int nabo_index_set_mask(nabo_index *ix, const uint8_t *ref_mask)
{
    if (!ix) return api_fail(NABO_E_INVALID, "NULL index");
    if (ix->async_busy) return api_fail(NABO_E_INVALID, "an asynchronous query is in flight on this index: nabo_index_query_wait first");
    if (!ix->have_ref) return api_fail(NABO_E_INVALID, "nabo_index_set_ref has not been called");
    int rc = use_device(ix->device);
    if (rc) return rc;
    if ((rc = apply_mask(ix, ref_mask))) return rc;
    if (ix->metric == NABO_METRIC_MOD_CANBERRA && ix->cb_bits) {
        HIP_TRY(nabo::cbb_valid_launch(ix->dmask, ix->n, ix->cbvalid.as<uint32_t>(), ix->stream));
        HIP_TRY(hipStreamSynchronize(ix->stream));
    }
    if (ix->metric != NABO_METRIC_MOD_CANBERRA && ix->ksteps > 0) {       // masked cells carry ||y||^2 = +inf in the packed tiles
        ix->packed_f32 = ix->packed_c16 = ix->packed_c1 = false;
        ix->ymax_pending = false;                      // (a read still in flight belongs to operands that are gone)
        ix->coarse_weak = false;
        if ((rc = ensure_packed(ix, ix->coarse ? 2 : ix->mode == 1 ? 1 : 0))) return rc;
    }
    return NABO_OK;
}

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
    bool r1 = false;                     // fp32 filter: one row-block per wave
    int geo = -1, kcq = 0, cslack = 0;
    int rows_per_wg = 256, wg_per_cu = 1, lkeep_max = 32, lkeep = 16, want = 16;
    int S = 1, S2 = 1;                   // reference splits of the main / tail launch
    bool one_round = false;              // fewer column-workgroups than slots: splits (+ a tail launch on long streams) fill one round
    int64_t gx = 0, gx_main = 0, gx_tail = 0, rows_pad = 0, tps = 0, tps2 = 0;
    char kernel[160] = "";
};

static int plan_l2(const nabo_index *ix, int64_t m, int k, int drop, bool cand_mode, L2Plan *P)
{
    const int kk = k + drop;
    const int epl = ((kk <= 24 && !ix->wide_retry) || cand_mode) ? 1 : 2;
    const int L = 32 * epl;
    int rows_per_wg = 256, wg_per_cu = 1, lkeep_max = L;
    bool use_h = false;                                  // an f16x3 kernel runs
    if (ix->mode == 1 && epl == 1) {
        nabo::l2q_topk_geometry(ix->kc, &rows_per_wg, &wg_per_cu, &lkeep_max);
        use_h = (cand_mode ? kk : kk + 4) <= lkeep_max;   // needs at least 4 entries of slack
    }
    // The one-product first pass (kc1-step operands; see nabo_index::coarse) -- on the l2c kernel, in the geometry that
    // serves the list length the pass wants (l2c_topk.hip: two waves per SIMD up to 23 kept entries, 32-entry lists,
    // 64-entry lists for k' > 24), unless option coarse_kernel_q sends the operands through the l2q kernel (32-entry lists
    // and g < 64 only).
    const bool pass1 = ix->coarse && !(ix->coarse_weak && ix->opt.coarse_adapt != 0) && ix->pass_level < 2 &&
                       !ix->wide_retry && (!cand_mode || kk + 3 <= 32);
    // (k' > 24, the 64-entry lists: six entries more -- there a row the first pass fails is expensive, the pass behind the
    // seeded one is the fp32 filter: cosine 1M x 1M, d = 100, k = 50: 689 -> 597 ms per step)
    const int slack1 = ix->opt.coarse_slack >= 0 ? ix->opt.coarse_slack : (epl == 2 ? 6 : 0);
    const int cslack = ix->opt.cand_slack >= 0 ? ix->opt.cand_slack : ix->cand_slack;
    int want = cand_mode ? (kk < 4 ? 4 : kk) + cslack : kk + 8 + slack1;
    if (ix->pass_level == 1) want = L;                   // seeded pass: room for everything below the seed
    if (epl == 1 && want > 32) want = 32;                // (the emitted lists hold 32 epl entries)
    if (epl == 2) want = want < 33 ? 33 : (want > 64 ? 64 : want);
    int geo = -1;
    if (pass1 && ix->opt.coarse_kernel_q == 0 && kk + 4 <= L) {
        geo = nabo::l2c_geometry(ix->kc1, want, ix->opt.l2c_geo);
        if (epl == 1 && geo == 2) geo = 0;               // (NABO_L2C_GEO=c with 32-entry emitted lists: geometry A)
    }
    const bool on_l2c = geo >= 0;
    const bool use_1 = on_l2c || (pass1 && use_h);
    if (on_l2c) {
        use_h = true;
        nabo::l2c_topk_geometry(ix->kc1, want, ix->opt.l2c_geo, &rows_per_wg, &wg_per_cu, &lkeep_max);
        if (geo == 0) { rows_per_wg = 4 * 128; lkeep_max = 32; }
    }
    const int kcq = use_1 ? ix->kc1 : ix->kc;
    // fewer rows than two-row-block workgroups fill the chip with: one row-block per wave, three waves per SIMD
    // (128-row workgroups balance the CUs and the third wave covers the list warm-up that dominates short streams)
    bool r1 = false;
    if (!use_h) {
        nabo::l2_topk_geometry(ix->ksteps, epl, &rows_per_wg, &wg_per_cu, &lkeep_max);
        const int r1_mode = ix->opt.l2_r1;             // -1 auto, 0 never, 1 always (experiments)
        // ... and also when the list warm-up is a large share of a workgroup's time (short reference streams,
        // e.g. one shard of eight): the same per-workgroup model as the split choice below, threshold measured
        // (the variant pays ~8 % more per reference tile, it wins from ~7.5 % warm-up share on)
        int lk_est = cand_mode ? (kk < 4 ? 4 : kk) : (kk + 8 < 16 ? 16 : kk + 8);
        if (lk_est > L) lk_est = L;
        const double stream_ms = (double)((ix->n + 31) / 32) * 3.36e-3 * (ix->ksteps / 25.0);
        const double lg_est = std::log((double)ix->n / lk_est > 2.0 ? (double)ix->n / lk_est : 2.0);
        const double warm_ms = 5.1 * (lk_est / 24.0) * (lg_est / 10.6);
        if (epl == 1 && ix->ksteps <= 25 && r1_mode != 0 &&
            (r1_mode == 1 || (m + rows_per_wg - 1) / rows_per_wg < (int64_t)ix->n_cu * wg_per_cu ||
             warm_ms > 0.075 * stream_ms)) {
            r1 = true;
            nabo::l2_topk_geometry(ix->ksteps, -1, &rows_per_wg, &wg_per_cu, &lkeep_max);
        }
    }
    const int64_t slots = (int64_t)ix->n_cu * wg_per_cu;          // workgroups resident at once
    const int64_t gx = (m + rows_per_wg - 1) / rows_per_wg;
    const int64_t rows_pad = gx * rows_per_wg;
    // kept-list length: k' + 8 slack (the certification needs a gap above the k'-th distance)
    int lkeep = kk + 8;
    if (lkeep < 16) lkeep = 16;
    if (ix->wide_retry) lkeep = lkeep_max;              // as many kept entries as the 64-entry lists allow
    // one-product pass: its scores sit up to 2^-9 ||x|| ||y|| below the real ones and the gap above the k'-th distance
    // has to cover that -- 1M x 1M x 50: k' + 8 entries leave ~1 % of the rows to the f16x3 pass (7 ms), k' + 13 a
    // third of that, but every five entries more cost 14 ms of list updates in the kernel: no extra slack by default
    if (use_1) lkeep = kk + 8 + slack1;
    if (use_1 && ix->pass_level == 1) lkeep = lkeep_max;       // seeded pass: room for everything below the seed
    if (on_l2c && lkeep > want) lkeep = want;
    if (cand_mode) lkeep = kk < 4 ? 4 : kk;
    // (candidate mode on the one-product pass: three kept entries more than are emitted, so that the bound is the exact
    // distance of the first candidate left out and not the one-product threshold, which sits 2^-9 ||x|| ||y|| lower)
    if (cand_mode && use_1) lkeep += cslack;
    if (lkeep > lkeep_max) lkeep = lkeep_max;
    // (experiments and tests: the first pass's list length; the passes behind it keep theirs)
    if (ix->pass_level == 0 && !ix->wide_retry) { const int lk = ix->opt.lkeep; if (lk >= kk && lk <= lkeep_max) lkeep = lk; }
    // Work decomposition.  Few target rows: split the reference range S ways (grid.y) so the
    // chip is full.  Many rows: the last, partially filled round of workgroups is launched with
    // its own split factor S2 so that it takes ~1/S2 of a round instead of a whole one.
    int64_t gx_main = gx, gx_tail = 0;
    int S2 = 1;
    int S = ix->opt.splits;
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
    bool one_round = false;
    if (!forced && on_l2c && ix->opt.one_round != 0 && ix->opt.merge_lists != 0 && ix->pass_level == 0 && !ix->wide_retry &&
        gx < slots) {
        int64_t s_cap = ix->ref_tiles / 16 > 0 ? ix->ref_tiles / 16 : 1;     // >= 16 tiles per split
        if (s_cap > 1024 / L) s_cap = 1024 / L;
        int64_t s_exact = slots / gx;
        if (s_exact > s_cap) s_exact = s_cap;
        S = (int)s_exact;
        const double occ = (double)(gx * s_exact) / (double)slots;
        if (occ < 0.8 && s_exact + 1 <= s_cap && ix->opt.tail_split != 0 && ix->ref_tiles >= 8192) {
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
            int64_t s_hi = ix->ref_tiles / 16 > 0 ? ix->ref_tiles / 16 : 1;
            if (s_hi > 1024 / L) s_hi = 1024 / L;
            // ms per reference tile and workgroup, measured: 105 ms / 31250 tiles (fp32, 256 rows, 25 k-steps); 1.2 us f16x3
            const double t_tile = use_h ? 1.1e-3 * kcq / 10.0 : 3.36e-3 * (rows_per_wg / 256.0) * (ix->ksteps / 25.0);
            double best = 1e30;
            for (int s2 = 1; s2 <= (int)s_hi; ++s2) {
                const double rounds = (double)((gx * s2 + slots - 1) / slots);
                const double stream = (double)ix->n / s2;
                double lg = std::log(stream / lkeep > 2.0 ? stream / lkeep : 2.0);
                const double warm = 5.1 * (lkeep / 24.0) * (lg / 10.6) * (rows_per_wg / 256.0);
                const double cost = rounds * ((double)ix->ref_tiles / s2 * t_tile + warm);
                if (cost < best * (1.0 - 1e-3)) { best = cost; S = s2; }
            }
        } else if (gx % slots != 0 && ix->opt.tail_split != 0 && ix->ref_tiles >= 256) {
            const int64_t tail = gx % slots;
            double best = 1.0;
            // (at most 8 splits: 11 would fill the chip exactly at 1M x 1M -- kernel 0.6 ms shorter, refine of the tail
            // rows' 11 lists 1.1 ms longer)
            for (int s2 = 2; s2 <= 8; ++s2) {
                const double t = (double)((tail * s2 + slots - 1) / slots) / s2;
                if (t < best - 1e-9) { best = t; S2 = s2; }
            }
            if (S2 > 1) { gx_tail = tail; gx_main = gx - tail; }
        }
    }
    if (S > 1024 / L) S = 1024 / L;                     // refine merges at most 1024 candidates per row (32 or 16 lists)
    if (S < 1) S = 1;
    if ((int64_t)S > ix->ref_tiles) S = (int)ix->ref_tiles;
    // A seeded pass keeps at most L entries per list: where the first pass already kept (nearly) as many -- k' >= 43 on the
    // 64-entry lists: cosine d = 100, k = 50 -- one list per row certifies nothing the first pass could not.  Four
    // reference splits give a row four lists: the references below its seed (a few more than 64) spread over them.
    if (use_1 && ix->pass_level == 1 && !forced && kk + 8 + slack1 + 8 > L) {
        if (S < 4) S = 4;
        if (gx_tail > 0 && S2 < 4) S2 = 4;
    }
    {   // a list entry holds 25 bits of offset into its split (topk_lists.h): very large sets take more splits
        // (NABO_SPLIT_REFS_MAX: tests lower the bound to see the rule at ordinary sizes)
        int64_t split_refs = ix->opt.split_refs_max;
        if (split_refs < 64 || split_refs > NABO_LIST_SPLIT_REFS) split_refs = NABO_LIST_SPLIT_REFS;
        const int64_t split_tiles = (split_refs - 1) / 32;
        const int64_t s_min = (ix->ref_tiles + split_tiles - 1) / split_tiles;
        if (s_min > 1024 / L) return api_fail(NABO_E_INVALID, "more than 2^25 x (1024 / list length) reference cells in one index");
        if (S < s_min) S = (int)s_min;
        if (gx_tail > 0 && S2 < s_min) S2 = (int)s_min;
    }
    const int64_t tps = (ix->ref_tiles + S - 1) / S;
    const int64_t tps2 = (ix->ref_tiles + S2 - 1) / S2;
    if (tps * S > ix->ref_tiles_alloc || tps2 * S2 > ix->ref_tiles_alloc)
        return api_fail(NABO_E_INVALID, "internal: split padding exceeds allocation");

    P->epl = epl; P->L = L;
    P->use_h = use_h; P->use_1 = use_1; P->on_l2c = on_l2c; P->r1 = r1;
    P->geo = geo; P->kcq = kcq; P->cslack = cslack;
    P->rows_per_wg = rows_per_wg; P->wg_per_cu = wg_per_cu; P->lkeep_max = lkeep_max; P->lkeep = lkeep; P->want = want;
    P->S = S; P->S2 = S2; P->one_round = one_round;
    P->gx = gx; P->gx_main = gx_main; P->gx_tail = gx_tail; P->rows_pad = rows_pad; P->tps = tps; P->tps2 = tps2;
    // (option coarse_kernel_q runs the one-product operands through the l2q kernel)
    if (use_1 && !on_l2c)
        snprintf(P->kernel, sizeof(P->kernel), "l2q_topk_kernel<%d,1,33> (v_mfma_f32_16x16x32_f16, one-product f16 filter with the split error as an operand slot)", kcq);
    else if (use_1) snprintf(P->kernel, sizeof(P->kernel), "l2c_topk_kernel<%d,%s> (v_mfma_f32_16x16x32_f16, one-product f16 filter with the split error as an operand slot)", kcq / 2, geo == 1 ? "1,23,6,32,4,2" : geo == 2 ? "2,65,4,64,4,1" : "1,33,8,64,4,1");
    else if (use_h) snprintf(P->kernel, sizeof(P->kernel), "l2q_topk_kernel<%d,1,33> (v_mfma_f32_16x16x32_f16, K-concatenated f16x3 split)", ix->kc);
    else snprintf(P->kernel, sizeof(P->kernel), "l2_topk_kernel<%d,%d,%d,%d> (v_mfma_f32_32x32x2_f32)", ix->ksteps,
                  r1 ? 1 : (epl == 1 ? 2 : 1), epl, epl == 1 ? 33 : 65);
    return NABO_OK;
}

// cand_mode: shard mode of nabo_index_query_candidates -- k is the number of candidates per row to emit,
// out_bound [m] receives the squared-distance bound of everything not emitted; no local certification.
static int query_body(nabo_index *ix, const double *X, int32_t x_on_device, int64_t m, int32_t k, int32_t drop_first,
                      int64_t *out_idx, double *out_dist, int32_t out_on_device, bool cand_mode, double *out_bound);

static int query_impl(nabo_index *ix, const double *X, int32_t x_on_device, int64_t m, int32_t k, int32_t drop_first,
                      int64_t *out_idx, double *out_dist, int32_t out_on_device, bool cand_mode, double *out_bound)
{
    if (!ix) return api_fail(NABO_E_INVALID, "NULL argument");
    if (ix->depth == 0) {                            // a top-level query: the per-row record starts over
        ix->row_pass.clear();
        ix->row_map = nullptr;
    }
    ++ix->depth;
    const int rc = query_body(ix, X, x_on_device, m, k, drop_first, out_idx, out_dist, out_on_device, cand_mode, out_bound);
    --ix->depth;
    return rc;
}

// What every route of a query reads (query_body stages it), and what the route leaves for finish_query.
struct Query {
    const double *dX = nullptr;      // [m, g] targets on the device
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
};

// Rows of the exact kernels' distance workspace: ~1 GiB of float64 rows, at least one, at most `rows` and `cap`.
static int reserve_exact_ws(nabo_index *ix, uint64_t rows, uint64_t cap, unsigned int *d_rows)
{
    uint64_t r = (1ull << 30) / ((uint64_t)ix->n * sizeof(double));
    if (r < 1) r = 1;
    if (r > rows) r = rows;
    if (r > cap) r = cap;
    *d_rows = (unsigned int)r;
    return ix->exact_d.reserve((size_t)r * ix->n * sizeof(double));
}

// Shapes outside the instantiated filter kernels: the exact float64 kernels answer every row.
static int query_exact(nabo_index *ix, Query &q)
{
    hipStream_t st = ix->stream;
    int rc;
    unsigned int d_rows = 0;
    if (q.top) ix->row_pass.assign((size_t)q.m, (uint8_t)NABO_PASS_EXACT);
    if (q.m > 0xFFFFFFF0ll) return api_fail(NABO_E_UNSUPPORTED, "m=%lld: fewer than 2^32-16 rows per call", (long long)q.m);
    if ((rc = ix->fails.reserve((size_t)q.m * sizeof(uint32_t)))) return rc;
    if ((rc = reserve_exact_ws(ix, (uint64_t)q.m, 65528, &d_rows))) return rc;
    HIP_TRY(nabo::iota_launch(ix->fails.as<uint32_t>(), q.m, st));
    for (int i = 1; i <= 3; ++i) HIP_TRY(hipEventRecord(ix->ev[i], st));
    HIP_TRY(nabo::exact_rows_launch(q.dX, ix->dY, ix->n, ix->g, ix->metric, ix->f, ix->dmask, ix->fails.as<uint32_t>(),
                                    (unsigned int)q.m, q.k, q.drop, ix->base, ix->mlistbuf.as<uint32_t>(), tail_len(ix),
                                    q.d_oidx, q.d_odist, ix->exact_d.as<double>(), d_rows, st));
    HIP_TRY(hipEventRecord(ix->ev[4], st));
    q.n_fail = (unsigned int)q.m;
    q.S = 0;
    snprintf(ix->kernel, sizeof(ix->kernel), "exact_dist_rows_kernel + exact_select_rows_kernel (float64 brute force)");
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
};

// The filter kernels of a pass, main launch then tail: the one-product kernel behind its tournament seeds (l2c_topk.hip),
// or the f16x3 (l2q_topk.hip) / fp32 (l2_topk.hip) filter.  *beside: ev_main was recorded between the two launches -- the
// refine of the main launch's rows runs on the second stream beside the tail launch.
static int l2_filter(nabo_index *ix, const Query &q, const L2Plan &P, L2Part (&part)[2], const float *seeds, bool *beside)
{
    hipStream_t st = ix->stream;
    int rc;
    const int64_t pad_tile = ix->ref_tiles_alloc - 1;
    const bool first = ix->pass_level == 0 && !ix->wide_retry;
    const unsigned char *xh = ix->xpk.as<unsigned char>();
    const unsigned char *yh = P.use_1 ? ix->ycpk1.as<unsigned char>() : ix->ycpk.as<unsigned char>();
    *beside = false;
    if (!P.on_l2c) {
        for (L2Part &p : part) {
            if (p.gx == 0) continue;
            if (P.use_h)
                HIP_TRY(nabo::l2q_topk_launch(P.kcq, xh, yh, (int)p.tps, p.S, (int)p.gx, p.row0 / 32, P.lkeep, p.idx->as<uint32_t>(),
                                              nullptr, p.tau->as<float>(), pad_tile, st));
            else
                HIP_TRY(nabo::l2_topk_launch(ix->ksteps, P.r1 ? -1 : q.epl, ix->xpk.as<float>(), ix->ypk.as<float>(), (int)p.tps,
                                             p.S, (int)p.gx, p.row0 / 32, P.lkeep, p.idx->as<uint32_t>(), nullptr,
                                             p.tau->as<float>(), st));
        }
        return NABO_OK;
    }
    // Tournament seeds (l2c_topk.hip: l2c_pre_kernel): every (row, split) list starts from an upper bound of its
    // lkeep-th smallest score among the split's first references instead of +inf -- not for a pass that has its
    // seeds already.  Option prepass: 0 off, otherwise percent of the planned length (same bits always).
    const int pre_pct = seeds ? 0 : ix->opt.prepass;
    const float *seed[2] = {seeds, seeds};
    int stride[2] = {0, 0};
    if (first) ix->pre_tiles_last = 0;
    for (int i = 0; i < 2 && pre_pct > 0; ++i) {
        L2Part &p = part[i];
        int pt = 0, gt = 2;
        nabo::l2c_pre_plan(P.kcq, P.lkeep, (int)p.tps, pre_pct, &pt, &gt);
        if (pt <= 0 || p.gx == 0) continue;
        if ((rc = p.pre->reserve((size_t)p.rows * p.S * sizeof(float)))) return rc;
        HIP_TRY(nabo::l2c_pre_launch(P.kcq, P.lkeep, xh, yh, (int)p.tps, p.S, p.rows, p.row0 / 32, pt, gt, pad_tile, st, q.m,
                                     p.pre->as<float>()));
        seed[i] = p.pre->as<float>();
        stride[i] = p.S;
        if (i == 0 && first) ix->pre_tiles_last = pt;
    }
    for (int i = 0; i < 2; ++i) {
        L2Part &p = part[i];
        if (p.gx == 0) continue;
        HIP_TRY(nabo::l2c_topk_launch(P.kcq, P.geo, xh, yh, (int)p.tps, p.S, (int)p.gx, p.row0 / 32, P.lkeep,
                                      p.idx->as<uint32_t>(), p.merge ? p.key->as<float>() : nullptr, p.tau->as<float>(),
                                      pad_tile, st, q.m, seed[i], stride[i], p.row0));
        // the tail launch (a fraction of a round, reference splits) leaves most CUs idle: the refine of the main
        // launch's rows (an HBM gather) runs beside it on the second stream
        if (i == 0 && part[1].gx > 0 && !q.cand_mode && ix->opt.refine_overlap != 0) {
            HIP_TRY(hipEventRecord(ix->ev_main, st));
            *beside = true;
        }
    }
    return NABO_OK;
}

// The float64 re-evaluation of a pass's lists (refine.hip), main launch then tail, each behind the merge of its lists
// where the pass merges them: certified rows and the fail list, or in candidate mode candidates and bounds.  beside: the
// main launch's part runs on the second stream (l2_filter).
static int l2_refine(nabo_index *ix, const Query &q, const L2Plan &P, L2Part (&part)[2], bool beside, float *fail_seed)
{
    hipStream_t st = ix->stream;
    // rounding-error coefficient of the filter score, relative to (||x|| + max||y||)^2
    // (f16x3: one fp32 accumulation per product term, 16 per step, plus the dropped lo*lo term and the
    // representation error of the hi + lo split)
    // (one-product pass: the hi x lo, lo x hi and lo x lo terms are INSIDE its score -- the error slot of
    // pack_ctiles_kernel<.,.,1> -- so the same accumulation / representation coefficient applies to its kc1 steps)
    const double err_coef = P.use_h ? 1.05 * ((16.0 * P.kcq + 8.0) * std::ldexp(1.0, -24) + std::ldexp(1.0, -20) + std::ldexp(1.0, -21))
                                    : 1.05 * (2.0 * ix->ksteps + 4.0) * std::ldexp(1.0, -24);
    const double tau_scale = P.use_h ? 1.0 / (ix->hscale * ix->hscale) : 1.0 / (ix->fscale * ix->fscale);
    int rc;
    if ((rc = ymax_resolve(ix))) return rc;
    const double ymax_sqrt = P.use_h ? ix->ymax_sqrt_c : ix->ymax_sqrt;
    const int metric = ix->metric == NABO_METRIC_COSINE ? 2 : 0;
    const int64_t n_valid = ix->n - ix->n_masked;
    auto merge = [&](L2Part &p, hipStream_t s) {
        return nabo::merge_lists_launch(p.idx->as<uint32_t>(), p.key->as<float>(), p.tau->as<float>(), p.end(q.m) - p.row0, p.S,
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
                HIP_TRY(nabo::refine_cand_launch(q.dX, part[i].row0, part[i].end(q.m), ix->dY, ix->g, lists[i].idx, lists[i].tau,
                                                 lists[i].S, lists[i].L, ix->xnorm.as<double>(), err_coef, ymax_sqrt, tau_scale,
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
        HIP_TRY(nabo::refine_launch(q.dX, p.row0, p.end(q.m), ix->dY, ix->g, lists[i].idx, lists[i].tau, lists[i].S, lists[i].L,
                                    ix->xnorm.as<double>(), err_coef, ymax_sqrt, tau_scale, q.k, q.drop, ix->base, n_valid, ix->mlistbuf.as<uint32_t>(),
                                    tail_len(ix), q.d_oidx, q.d_odist, ix->fails.as<uint32_t>(), ix->failcnt.as<unsigned int>(),
                                    s, metric, 0.0, 0.0f, p.merge ? p.keep : P.lkeep, nullptr, nullptr, fail_seed));
        if (i == 0 && beside) HIP_TRY(hipEventRecord(ix->ev_ref, s));
    }
    if (beside) HIP_TRY(hipStreamWaitEvent(st, ix->ev_ref, 0));
    return NABO_OK;
}

// The q.n_fail rows of this batch the pass could not certify (ix->fails) go on as a dense batch through query_impl one
// link down the pass chain: at pass level `level` (seeds: level 1's per-row thresholds) or, with `wide`, on 64-entry lists.
// They are gathered into the buffer set `b` of this frame, recorded as pass `code` (pass_rows[slot]), solved and scattered
// back; q.n_fail becomes the rows that still needed the exact kernels.  The inner call reuses ev[0..5]: phases 0-2 of
// this one are kept for finish_query.
static int rerun_failed_rows(nabo_index *ix, Query &q, int level, bool wide, uint8_t code, int slot, nabo_index::RerunBufs &b,
                             const float *seeds)
{
    hipStream_t st = ix->stream;
    const int64_t nf = q.n_fail;
    int rc;
    float ms_first[3] = {0, 0, 0};
    for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&ms_first[i], ix->ev[i], ix->ev[i + 1]));
    if ((rc = b.rows.reserve((size_t)nf * sizeof(uint32_t))) || (rc = b.x.reserve((size_t)nf * ix->g * sizeof(double))) ||
        (rc = b.idx.reserve((size_t)nf * q.k * sizeof(int64_t))) || (rc = b.dist.reserve((size_t)nf * q.k * sizeof(double))))
        return rc;
    HIP_TRY(hipMemcpyAsync(b.rows.p, ix->fails.p, (size_t)nf * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    if (seeds) {
        if ((rc = b.seed.reserve((size_t)nf * sizeof(float)))) return rc;
        HIP_TRY(hipMemcpyAsync(b.seed.p, seeds, (size_t)nf * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(nabo::gather_rows_launch(q.dX, b.rows.as<uint32_t>(), nf, ix->g, b.x.as<double>(), st));
    if ((rc = note_row_pass(ix, b.rows.as<uint32_t>(), nf, code, q.pass_map))) return rc;      // (synchronises the stream)
    const int level_saved = ix->pass_level;
    const float *seed_saved = ix->seed_tau;
    const std::vector<uint32_t> *map_saved = ix->row_map;
    ix->pass_level = level;
    ix->wide_retry = wide;                           // (only ever entered from a frame on 32-entry lists)
    ix->seed_tau = seeds ? b.seed.as<float>() : nullptr;
    ix->row_map = &q.pass_map;
    rc = query_impl(ix, b.x.as<double>(), 1, nf, q.k, q.drop, b.idx.as<int64_t>(), b.dist.as<double>(), 1, false, nullptr);
    ix->pass_level = level_saved;
    ix->wide_retry = false;
    ix->seed_tau = seed_saved;
    ix->row_map = map_saved;
    if (rc) return rc;
    ix->pass_rows[slot] = nf;
    q.n_fail = (unsigned int)ix->counters[0];
    HIP_TRY(nabo::scatter_rows_launch(b.idx.as<int64_t>(), b.dist.as<double>(), b.rows.as<uint32_t>(), nf, q.k, q.d_oidx,
                                      q.d_odist, st));
    HIP_TRY(hipEventRecord(ix->ev[3], st));          // (ev[0..5] were reused by the inner call)
    memcpy(ix->ms_keep, ms_first, sizeof(ms_first));
    ix->ms_keep_valid = true;
    return NABO_OK;
}

// Euclidean / cosine: plan_l2 -> pack the targets -> filter -> float64 refine and certificate; the rows the pass could not
// certify go one link down the pass chain (rerun_failed_rows) or to the exact kernels.
static int query_l2(nabo_index *ix, Query &q)
{
    hipStream_t st = ix->stream;
    const int g = ix->g;
    const int64_t m = q.m;
    int rc;
    const double *dXp = q.dX;                        // what the filter packs
    if (ix->metric == NABO_METRIC_COSINE) {
        if ((rc = ix->xnbuf.reserve((size_t)m * g * sizeof(double)))) return rc;
        HIP_TRY(nabo::normalise_rows_launch(q.dX, m, g, ix->xnbuf.as<double>(), st));
        dXp = ix->xnbuf.as<double>();
    }
    L2Plan P;
    if ((rc = plan_l2(ix, m, q.k, q.drop, q.cand_mode, &P))) return rc;
    if (ix->pass_level == 0 && !ix->wide_retry) {
        ix->pass_rows[0] = ix->pass_rows[1] = ix->pass_rows[2] = 0;
        snprintf(ix->kernel, sizeof(ix->kernel), "%s", P.kernel);
    }
    if ((rc = ensure_packed(ix, P.use_1 ? 2 : P.use_h ? 1 : 0))) return rc;
    if (q.top) ix->row_pass.assign((size_t)m, (uint8_t)(P.use_1 ? NABO_PASS_ONE_PRODUCT : NABO_PASS_SECOND));
    const int64_t rows_main = P.gx_main * P.rows_per_wg;
    L2Part part[2] = {
        {P.gx_main, 0, rows_main, P.S, P.tps, &ix->cand_idx, &ix->cand_tau, &ix->cand_key, &ix->cand_mi, &ix->cand_mt, &ix->taupre},
        {P.gx_tail, rows_main, P.gx_tail * P.rows_per_wg, P.S2, P.tps2, &ix->cand_idx2, &ix->cand_tau2, &ix->cand_key2,
         &ix->cand_mi2, &ix->cand_mt2, &ix->taupre2}};
    // Several lists per row (reference splits, the tail round): the l2c kernel also emits the entries' filter keys and
    // merge_lists_kernel reduces the lists to the ONE a single stream would have kept (refine.hip)
    // (first pass only: a seeded pass WANTS every list re-evaluated -- its rows have more than one list's worth of
    // references below their seeds: cosine d = 100, k = 50 with the merge there: 86 instead of 16 ms of later passes)
    // ... the SEEDED pass keeps up to 128: what lies below a seed is "a few more than one list", and
    // 128 candidates are two per lane for the float64 step where S x 32 were four to sixteen per lane, each walking
    // its own row (100k x 100k: refine of 108 rows' 1024 candidates 0.41 ms)
    const bool seeded_merge = ix->pass_level == 1 && !ix->wide_retry;          // (32- and 64-entry lists alike)
    const bool merging = P.on_l2c && ix->opt.merge_lists != 0 && !ix->wide_retry && (ix->pass_level == 0 || seeded_merge);
    const size_t xtile_bytes = P.use_h ? (size_t)P.kcq * 1024 : (size_t)((ix->ksteps + 3) / 4) * 256 * sizeof(float);
    if ((rc = ix->xpk.reserve((size_t)(P.rows_pad / 32) * xtile_bytes))) return rc;
    if ((rc = ix->xnorm.reserve((size_t)m * sizeof(double)))) return rc;
    for (L2Part &p : part) {
        if (p.gx == 0) continue;
        p.merge = merging && p.S > 1;
        p.keep = seeded_merge ? (p.S * q.L < 128 ? p.S * q.L : 128) : P.lkeep;
        p.lout = seeded_merge ? p.keep : q.L;
        if ((rc = p.idx->reserve((size_t)p.rows * p.S * q.L * sizeof(uint32_t) + 16))) return rc;
        if ((rc = p.tau->reserve((size_t)p.rows * p.S * sizeof(float) + 16))) return rc;
        if (p.merge && ((rc = p.key->reserve((size_t)p.rows * p.S * q.L * sizeof(float))) ||
                        (rc = p.mi->reserve((size_t)p.rows * p.lout * sizeof(uint32_t))) ||
                        (rc = p.mt->reserve((size_t)p.rows * sizeof(float)))))
            return rc;
    }
    if ((rc = ix->fails.reserve((size_t)m * sizeof(uint32_t)))) return rc;
    if ((rc = ix->failcnt.reserve(sizeof(unsigned int)))) return rc;
    HIP_TRY(hipMemsetAsync(ix->failcnt.p, 0, sizeof(unsigned int), st));
    if (P.use_h)
        HIP_TRY(nabo::pack_cquery_launch(dXp, m, g, ix->centre.as<double>(), ix->hscale, P.kcq, P.rows_pad / 32,
                                         ix->xpk.as<unsigned char>(), ix->xnorm.as<double>(), true, st, nullptr, P.use_1 ? 1 : 3));
    else
        HIP_TRY(nabo::pack_query_launch(dXp, m, g, ix->centre.as<double>(), ix->fscale, ix->ksteps, P.rows_pad / 32,
                                        ix->xpk.as<float>(), ix->xnorm.as<double>(), st));
    HIP_TRY(hipEventRecord(ix->ev[1], st));
    // the l2c kernel ran: its failed rows can go through a seeded pass
    const bool seedable = P.on_l2c && !q.cand_mode && ix->opt.seeded_pass != 0;
    bool beside = false;
    if ((rc = l2_filter(ix, q, P, part, (seedable && ix->pass_level == 1) ? ix->seed_tau : nullptr, &beside))) return rc;
    HIP_TRY(hipEventRecord(ix->ev[2], st));
    float *fail_seed = nullptr;          // seeds for a seeded pass of the rows that fail (pass 0 on the l2c kernel)
    if (seedable && ix->pass_level == 0) {
        if ((rc = ix->failseed.reserve((size_t)m * sizeof(float)))) return rc;
        fail_seed = ix->failseed.as<float>();
    }
    if ((rc = l2_refine(ix, q, P, part, beside, fail_seed))) return rc;
    HIP_TRY(hipEventRecord(ix->ev[3], st));
    q.S = P.S;
    q.n_wg = P.gx_main * P.S + P.gx_tail * P.S2;
    if (q.cand_mode) {
        HIP_TRY(hipEventRecord(ix->ev[4], st));
        return NABO_OK;
    }
    HIP_TRY(hipMemcpyAsync(&q.n_fail, ix->failcnt.p, sizeof(q.n_fail), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (P.use_1 && q.n_fail > 0) {
        // Rows this one-product pass could not certify: from level 0 on the l2c kernel to the SEEDED one-product pass
        // (level 1: every row starts from the threshold refine.hip derived from its failed certificate), otherwise to
        // the f16x3 pass (level 2), which sends what IT cannot certify on to the 64-entry lists / the exact kernels.
        const int here = ix->pass_level, next = (here == 0 && fail_seed) ? 1 : 2;
        if ((rc = rerun_failed_rows(ix, q, next, false, next == 1 ? NABO_PASS_SEEDED : NABO_PASS_SECOND, next - 1, ix->rerun[here],
                                    next == 1 ? fail_seed : nullptr)))
            return rc;
        if (here == 0 && m >= 1024 && ix->pass_rows[1] > m / 4) ix->coarse_weak = true;
    } else if (q.n_fail >= 16 && q.epl == 1 && !ix->wide_retry && ix->opt.wide_retry != 0) {
        // Second chance: rows the 32-entry lists could not certify (ties / near-ties reaching past the kept
        // entries) go through the same filter once more with 64-entry lists before anything is brute-forced.
        if ((rc = rerun_failed_rows(ix, q, ix->pass_level, true, NABO_PASS_WIDE, 2, ix->rerun[RERUN_WIDE], nullptr))) return rc;
    } else if (q.n_fail > 0) {
        unsigned int d_rows = 0;
        if ((rc = reserve_exact_ws(ix, q.n_fail, 65535, &d_rows))) return rc;
        if ((rc = note_row_pass(ix, ix->fails.as<uint32_t>(), q.n_fail, (uint8_t)NABO_PASS_EXACT, q.pass_map))) return rc;
        HIP_TRY(nabo::exact_rows_launch(q.dX, ix->dY, ix->n, g, ix->metric, ix->f, ix->dmask, ix->fails.as<uint32_t>(), q.n_fail,
                                        q.k, q.drop, ix->base, ix->mlistbuf.as<uint32_t>(), tail_len(ix), q.d_oidx, q.d_odist,
                                        ix->exact_d.as<double>(), d_rows, st));
    }
    HIP_TRY(hipEventRecord(ix->ev[4], st));
    return NABO_OK;
}

// ---- the launch plan of a modified-Canberra query (a pure function of the index's shape and the query's, like plan_l2) ----
// Splits of the exact kernel (canberra_topk_kernel, gx workgroups of 64 rows): ~1024 workgroups in all, at most one split
// per 64-reference chunk and 16.
static int cb_exact_splits(int64_t gx, int64_t n_chunks)
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

struct CbPlan {
    int64_t gx_exact = 0;            // exact kernel: workgroups (64 rows each) and reference splits
    int S_exact = 1;
    bool bits = false;               // counting pass on bitmaps (canberra_bits.hip), else the SWAR count (canberra_f32.hip)
    int lists = 1;                   // candidate lists per (row, split): one per wave
    int Sf = 1, S2 = 1;              // counting pass: reference splits of the main launch / the tail round
    int64_t rows_main = 0;           // ... target rows of the main launch (the rest: the tail round)
};

static void plan_canberra(const nabo_index *ix, int64_t m, int epl, CbPlan *C)
{
    const int64_t n_chunks = (ix->n + 63) / 64;
    C->gx_exact = (m + 63) / 64;
    const int S = ix->opt.splits > 0 ? ix->opt.splits : cb_exact_splits(C->gx_exact, n_chunks);
    C->S_exact = S > 16 ? 16 : S;
    // counting-pass geometry: rpw rows per workgroup, every (row, split) ends with `lists` candidate lists.  Splits fill
    // the chip when there are few rows and trim the last, partially filled round of workgroups when there are many.
    C->bits = ix->cb_bits && epl == 1;               // (the bitmap kernel is instantiated for 32-entry lists)
    C->lists = nabo::cbf_lists_per_split();
    const int rpw = C->bits ? nabo::cbb_rows_per_wg() : nabo::cbf_rows_per_wg(epl);
    const int64_t gxf = (m + rpw - 1) / rpw;
    // resident workgroups: SWAR pass -- one-wave workgroups, 2 per SIMD; bitmap pass -- ONE 8-wave workgroup per CU
    // (its LDS copy of the table rows + eight waves' lists fill the CU's LDS)
    const int64_t slots = C->bits ? (int64_t)ix->n_cu : (int64_t)ix->n_cu * 8;
    int s_max = 1024 / (C->lists * 32 * epl);        // refine handles <= 1024 candidates per row
    if (C->bits) {                                   // splits are ranges of 2048-reference blocks, >= 2 each
        const int64_t nb2 = ((ix->n + 2047) / 2048) / 2;
        if (s_max > nb2) s_max = (int)nb2;
    } else if (s_max > n_chunks / (8 * C->lists)) s_max = (int)(n_chunks / (8 * C->lists));
    if (s_max < 1) s_max = 1;
    double cost = 0;
    int Sf = ix->opt.splits > 0 ? ix->opt.splits : cb_best_split(gxf, slots, s_max, &cost);
    if (Sf > s_max) Sf = s_max;
    // "tail round": with many rows the last, partially filled round of workgroups gets its own (larger) split factor so
    // that it takes a fraction of a round -- same idea as in the Euclidean launch
    C->S2 = 1;
    C->rows_main = m;
    if (ix->opt.splits <= 0 && ix->opt.tail_split != 0 && gxf > slots && gxf % slots != 0 && s_max >= 2) {
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

// The counting pass -> float64 refine + certificate -> exact re-solve of the uncertified rows.  *done stays false when
// the targets do not fit fp32: the exact kernel then answers every row.
static int canberra_filter(nabo_index *ix, Query &q, const CbPlan &C, bool *done)
{
    hipStream_t st = ix->stream;
    const int g = ix->g, gp = ix->cb_gp;
    const int64_t m = q.m, n_valid = ix->n - ix->n_masked;
    int rc;
    float slack, plateau;
    nabo::cbf_constants(g, &slack, &plateau);
    if (C.bits) snprintf(ix->kernel, sizeof(ix->kernel), "cbb_filter_kernel<%d> (bit-sliced count on %d-bucket bitmaps + fp32 lower bound)", gp, nabo::cbb_buckets());
    else snprintf(ix->kernel, sizeof(ix->kernel), "cbf_filter_kernel<%d> (7-bit integer count + fp32 lower bound)", gp);
    struct { int64_t row0, rows; int SL; DevBuf *idx, *tau; } part[2] = {
        {0, C.rows_main, C.Sf * C.lists, &ix->cand_idx, &ix->cand_tau},
        {C.rows_main, m - C.rows_main, C.S2 * C.lists, &ix->cand_idx2, &ix->cand_tau2}};
    if ((rc = ix->xpk.reserve((size_t)m * gp * 2 * sizeof(float)))) return rc;
    if ((rc = ix->xh.reserve((size_t)m * gp * 2))) return rc;
    for (auto &p : part)
        if (p.rows > 0 && ((rc = p.idx->reserve((size_t)p.rows * p.SL * q.L * sizeof(uint32_t))) ||
                           (rc = p.tau->reserve((size_t)p.rows * p.SL * sizeof(float) + 16))))
            return rc;
    if ((rc = ix->fails.reserve((size_t)m * sizeof(uint32_t)))) return rc;
    HIP_TRY(hipMemsetAsync(ix->cbflag.p, 0, 4 * sizeof(unsigned int), st));
    unsigned int *d_failcnt = ix->cbflag.as<unsigned int>() + 1, *d_flag = ix->cbflag.as<unsigned int>();
    HIP_TRY(nabo::cbf_pack_targets_launch(q.dX, m, g, gp, ix->f, ix->xpk.as<float>(), d_flag, st));
    if (C.bits) {
        if ((rc = ix->cbrow.reserve((size_t)m * gp * sizeof(uint16_t)))) return rc;
        HIP_TRY(nabo::cbb_pack_targets_launch(q.dX, m, g, gp, ix->f, ix->cbedges.as<double>(), ix->cbrow.as<uint16_t>(), st));
    } else {
        HIP_TRY(nabo::cbf_pack_targets8_launch(q.dX, m, g, gp, ix->f, ix->cbscale.as<double>(), ix->xh.p, st));
    }
    HIP_TRY(hipEventRecord(ix->ev[1], st));
    for (auto &p : part) {
        if (p.rows == 0) continue;
        const float *xq = ix->xpk.as<float>() + (size_t)p.row0 * gp * 2;
        if (C.bits)
            HIP_TRY(nabo::cbb_filter_launch(gp, xq, ix->cbrow.as<uint16_t>() + (size_t)p.row0 * gp, p.rows, ix->yrow.as<float>(),
                                            ix->cbtab.as<uint32_t>(), ix->cbvalid.as<uint32_t>(), ix->n, g, p.SL / C.lists,
                                            p.idx->as<uint32_t>(), p.tau->as<float>(), st));
        else
            HIP_TRY(nabo::cbf_filter_launch(gp, q.epl, xq, ix->xh.as<unsigned char>() + (size_t)p.row0 * gp * 2, p.rows,
                                            ix->yrow.as<float>(), ix->ych.p, ix->n, g, ix->dmask, p.SL / C.lists,
                                            p.idx->as<uint32_t>(), p.tau->as<float>(), st));
    }
    HIP_TRY(hipEventRecord(ix->ev[2], st));
    for (auto &p : part)
        if (p.rows > 0)
            HIP_TRY(nabo::refine_launch(q.dX, p.row0, p.row0 + p.rows, ix->dY, g, p.idx->as<uint32_t>(), p.tau->as<float>(), p.SL,
                                        q.L, nullptr, 0.0, 0.0, 1.0, q.k, q.drop, ix->base, n_valid, ix->mlistbuf.as<uint32_t>(),
                                        tail_len(ix), q.d_oidx, q.d_odist, ix->fails.as<uint32_t>(), d_failcnt, st, 1, ix->f,
                                        plateau));
    HIP_TRY(hipEventRecord(ix->ev[3], st));
    unsigned int hf[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(hf, ix->cbflag.p, sizeof(hf), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hf[0] != 0) return NABO_OK;                  // targets do not fit fp32
    q.n_fail = hf[1];
    if (q.top) {
        ix->row_pass.assign((size_t)m, (uint8_t)NABO_PASS_CANBERRA);
        if ((rc = note_row_pass(ix, ix->fails.as<uint32_t>(), q.n_fail, (uint8_t)NABO_PASS_EXACT, q.pass_map))) return rc;
    }
    if (q.n_fail > 0) {                              // (the buffers of the 64-entry-list rerun: this route has none)
        const int64_t nf = q.n_fail;
        const int S3 = cb_exact_splits((nf + 63) / 64, (ix->n + 63) / 64);
        nabo_index::RerunBufs &b = ix->rerun[RERUN_WIDE];
        if ((rc = b.x.reserve((size_t)nf * g * sizeof(double))) || (rc = ix->cand_d.reserve((size_t)nf * S3 * q.L * sizeof(double))) ||
            (rc = ix->cand_idx2.reserve((size_t)nf * S3 * q.L * sizeof(uint32_t))) ||
            (rc = b.idx.reserve((size_t)nf * q.k * sizeof(int64_t))) || (rc = b.dist.reserve((size_t)nf * q.k * sizeof(double))))
            return rc;
        HIP_TRY(nabo::gather_rows_launch(q.dX, ix->fails.as<uint32_t>(), nf, g, b.x.as<double>(), st));
        HIP_TRY(nabo::canberra_topk_launch(q.epl, b.x.as<double>(), nf, ix->yt.as<double>(), ix->n, g, ix->f, ix->dmask, S3,
                                           ix->cand_d.as<double>(), ix->cand_idx2.as<uint32_t>(), st));
        HIP_TRY(nabo::merge_local_launch(ix->cand_d.as<double>(), ix->cand_idx2.as<uint32_t>(), nf, S3 * q.L, q.k, q.drop,
                                         ix->base, b.idx.as<int64_t>(), b.dist.as<double>(), nullptr, st));
        HIP_TRY(nabo::scatter_rows_launch(b.idx.as<int64_t>(), b.dist.as<double>(), ix->fails.as<uint32_t>(), nf, q.k,
                                          q.d_oidx, q.d_odist, st));
    }
    HIP_TRY(hipEventRecord(ix->ev[4], st));
    *done = true;
    return NABO_OK;
}

// Modified Canberra: the counting pass where the references have one (canberra_filter), otherwise -- or when too few
// references are unmasked -- the exact kernel for every row.
static int query_canberra(nabo_index *ix, Query &q)
{
    hipStream_t st = ix->stream;
    int rc;
    CbPlan C;
    plan_canberra(ix, q.m, q.epl, &C);
    snprintf(ix->kernel, sizeof(ix->kernel), "canberra_topk_kernel (float64)");
    if (q.top) ix->row_pass.assign((size_t)q.m, (uint8_t)NABO_PASS_EXACT);
    const int64_t n_valid = ix->n - ix->n_masked;
    bool done = false;
    if (ix->cb_f32 && n_valid >= q.kk && (rc = canberra_filter(ix, q, C, &done))) return rc;
    q.S = done ? C.Sf : C.S_exact;
    q.n_wg = C.gx_exact * q.S;
    if (done) return NABO_OK;
    const int S = C.S_exact;
    if ((rc = ix->cand_d.reserve((size_t)q.m * S * q.L * sizeof(double))) ||
        (rc = ix->cand_idx.reserve((size_t)q.m * S * q.L * sizeof(uint32_t))))
        return rc;
    HIP_TRY(hipEventRecord(ix->ev[1], st));
    HIP_TRY(nabo::canberra_topk_launch(q.epl, q.dX, q.m, ix->yt.as<double>(), ix->n, ix->g, ix->f, ix->dmask, S,
                                       ix->cand_d.as<double>(), ix->cand_idx.as<uint32_t>(), st));
    HIP_TRY(hipEventRecord(ix->ev[2], st));
    HIP_TRY(nabo::merge_local_launch(ix->cand_d.as<double>(), ix->cand_idx.as<uint32_t>(), q.m, S * q.L, q.k, q.drop, ix->base,
                                     q.d_oidx, q.d_odist, nullptr, st));
    HIP_TRY(hipEventRecord(ix->ev[3], st));
    if (n_valid < q.kk)
        HIP_TRY(nabo::masked_tail_launch(q.dX, q.m, ix->dY, ix->g, ix->metric, ix->f, ix->mlistbuf.as<uint32_t>(), tail_len(ix),
                                         (int)n_valid, q.k, q.drop, ix->base, q.d_oidx, q.d_odist, st));
    HIP_TRY(hipEventRecord(ix->ev[4], st));
    return NABO_OK;
}

// Copy-out, the phases of the query (ev[0..5] -> ms[0..4]) and its counters.  A query that reran rows one level down
// (rerun_failed_rows) kept its phases 0-2 from before the inner call, whose total stands in for phase 3.
static int finish_query(nabo_index *ix, const Query &q, int64_t *out_idx, double *out_dist, int32_t out_on_device)
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
        ix->ms[i] = t;
    }
    HIP_TRY(hipEventElapsedTime(&t, ix->ev[0], ix->ev[5]));
    ix->ms[4] = t;
    if (ix->ms_keep_valid) {
        ix->ms_keep_valid = false;
        HIP_TRY(hipEventElapsedTime(&t, ix->ev[3], ix->ev[5]));
        for (int i = 0; i < 3; ++i) ix->ms[i] = ix->ms_keep[i];
        ix->ms[3] = ix->ms_inner + t;              // inner pass (its own total) + scatter / copy-out
        ix->ms[4] = ix->ms[0] + ix->ms[1] + ix->ms[2] + ix->ms[3];
    }
    ix->ms_inner = ix->ms[4];
    ix->counters[0] = q.n_fail; ix->counters[1] = q.S; ix->counters[2] = q.L; ix->counters[3] = q.n_wg;
    return NABO_OK;
}

static int query_body(nabo_index *ix, const double *X, int32_t x_on_device, int64_t m, int32_t k, int32_t drop_first,
                      int64_t *out_idx, double *out_dist, int32_t out_on_device, bool cand_mode, double *out_bound)
{
    if (!ix || !X || !out_idx || !out_dist) return api_fail(NABO_E_INVALID, "NULL argument");
    if (!ix->have_ref) return api_fail(NABO_E_INVALID, "nabo_index_set_ref has not been called");
    if (m < 0) return api_fail(NABO_E_INVALID, "m=%lld must be >= 0", (long long)m);
    if (m == 0) return NABO_OK;                      // no target cells: nothing to do (reference loops are empty)
    const int drop = drop_first ? 1 : 0;
    const int kk = k + drop;
    if (k < 1) return api_fail(NABO_E_INVALID, "k=%d must be >= 1", k);
    if (kk > ix->n && !cand_mode)
        return api_fail(NABO_E_INVALID, "k + drop_first = %d exceeds the %lld references", kk, (long long)ix->n);
    if (cand_mode && (ix->metric == NABO_METRIC_MOD_CANBERRA || !out_bound || !out_on_device || k > 32))
        return api_fail(NABO_E_INVALID, "candidate mode: Euclidean or cosine metric, device outputs, <= 32 candidates");
    // Shapes outside the instantiated filter kernels (k' > NABO_MAX_K, g > NABO_MAX_COMPS) are answered by the exact
    // float64 kernels for every row: the reference accepts any k / use_comps (nabo/_mapping.py:495-524).
    const bool exact_route = kk > NABO_MAX_K || (ix->metric != NABO_METRIC_MOD_CANBERRA && ix->ksteps < 0);
    if (exact_route && cand_mode)
        return api_fail(NABO_E_UNSUPPORTED, "candidate mode needs g <= %d (got %d)", NABO_MAX_COMPS, ix->g);
    int rc = use_device(ix->device);
    if (rc) return rc;
    hipStream_t st = ix->stream;
    Query q;
    q.m = m; q.k = k; q.drop = drop; q.kk = kk;
    q.epl = ((kk <= 24 && !ix->wide_retry) || cand_mode) ? 1 : 2;
    q.L = 32 * q.epl;
    q.cand_mode = cand_mode; q.out_bound = out_bound;
    q.top = ix->depth == 1 && !cand_mode;
    // operands / results on device
    q.dX = X;
    if (!x_on_device) {
        const size_t xb = (size_t)m * ix->g * sizeof(double);
        if ((rc = ix->xbuf.reserve(xb))) return rc;
        HIP_TRY(hipMemcpyAsync(ix->xbuf.p, X, xb, hipMemcpyHostToDevice, st));
        q.dX = ix->xbuf.as<double>();
    }
    q.d_oidx = out_idx;
    q.d_odist = out_dist;
    if (!out_on_device) {
        const size_t ob = (size_t)m * k * 8;
        if ((rc = ix->oidx.reserve(ob)) || (rc = ix->odist.reserve(ob))) return rc;
        q.d_oidx = ix->oidx.as<int64_t>();
        q.d_odist = ix->odist.as<double>();
    }
    HIP_TRY(hipEventRecord(ix->ev[0], st));
    rc = exact_route ? query_exact(ix, q) : ix->metric != NABO_METRIC_MOD_CANBERRA ? query_l2(ix, q) : query_canberra(ix, q);
    if (rc) return rc;
    return finish_query(ix, q, out_idx, out_dist, out_on_device);
}

// (every entry point that touches an index first waits for the asynchronous query it may have in flight and hands its
// status to nabo_index_query_wait)
static void async_join(nabo_index *ix)
{
    if (ix && ix->async_thread.joinable()) ix->async_thread.join();
}

int nabo_index_query(nabo_index *ix, const double *X, int32_t x_on_device, int64_t m, int32_t k,
                     int32_t drop_first, int64_t *out_idx, double *out_dist, int32_t out_on_device)
{
    if (ix && ix->async_busy) return api_fail(NABO_E_INVALID, "an asynchronous query is in flight on this index: nabo_index_query_wait first");
    return query_impl(ix, X, x_on_device, m, k, drop_first, out_idx, out_dist, out_on_device, false, nullptr);
}

int nabo_index_query_async(nabo_index *ix, const double *X, int32_t x_on_device, int64_t m, int32_t k,
                           int32_t drop_first, int64_t *out_idx, double *out_dist, int32_t out_on_device)
{
    if (!ix) return api_fail(NABO_E_INVALID, "NULL argument");
    if (ix->async_busy) return api_fail(NABO_E_INVALID, "an asynchronous query is in flight on this index: nabo_index_query_wait first");
    async_join(ix);
    ix->async_busy = true;
    ix->async_rc = NABO_OK;
    ix->async_msg[0] = 0;
    try {
        ix->async_thread = std::thread([=]() {
            const int rc = query_impl(ix, X, x_on_device, m, k, drop_first, out_idx, out_dist, out_on_device, false, nullptr);
            ix->async_rc = rc;
            if (rc) snprintf(ix->async_msg, sizeof(ix->async_msg), "%s", nabo_last_error());   // (this thread's message)
        });
    } catch (...) {
        ix->async_busy = false;
        return api_fail(NABO_E_NOMEM, "could not start the query's host thread");
    }
    return NABO_OK;
}

int nabo_index_query_wait(nabo_index *ix)
{
    if (!ix) return api_fail(NABO_E_INVALID, "NULL argument");
    if (!ix->async_busy) return NABO_OK;
    async_join(ix);
    ix->async_busy = false;
    return ix->async_rc ? api_fail(ix->async_rc, "%s", ix->async_msg) : NABO_OK;
}

int nabo_index_query_candidates(nabo_index *ix, const double *X, int32_t x_on_device, int64_t m, int32_t n_cand,
                                int64_t *out_idx, double *out_dist, double *out_bound)
{
    if (ix && ix->async_busy) return api_fail(NABO_E_INVALID, "an asynchronous query is in flight on this index: nabo_index_query_wait first");
    return query_impl(ix, X, x_on_device, m, n_cand, 0, out_idx, out_dist, 1, true, out_bound);
}

int nabo_index_last_stats(const nabo_index *ix, double ms[5], int64_t counters[4])
{
    if (!ix) return api_fail(NABO_E_INVALID, "NULL index");
    if (ms) memcpy(ms, ix->ms, sizeof(ix->ms));
    if (counters) memcpy(counters, ix->counters, sizeof(ix->counters));
    return NABO_OK;
}

int nabo_index_last_passes(const nabo_index *ix, int64_t rows[3])
{
    if (!ix || !rows) return api_fail(NABO_E_INVALID, "NULL argument");
    rows[0] = ix->pass_rows[0];
    rows[1] = ix->pass_rows[1];
    rows[2] = ix->pass_rows[2];
    return NABO_OK;
}

int nabo_query_plan(int64_t n_ref, int32_t g, int32_t metric, int64_t m, int32_t k, int32_t drop_first, int32_t n_cand,
                    int32_t n_cu, const char *l2_mode, const char *options, int64_t out[NABO_PLAN_FIELDS], char *kernel,
                    size_t kernel_len)
{
    if (!out) return api_fail(NABO_E_INVALID, "NULL argument");
    if (n_ref < 1 || g < 1 || m < 1 || k < 1 || n_cu < 1) return api_fail(NABO_E_INVALID, "bad shape");
    if (metric != NABO_METRIC_EUCLIDEAN && metric != NABO_METRIC_COSINE)
        return api_fail(NABO_E_UNSUPPORTED, "nabo_query_plan describes the Euclidean / cosine filter launches");
    nabo_index ix;                                   // a shape, never a device object: nothing here touches HIP
    ix.n = n_ref;
    ix.g = g;
    ix.metric = metric;
    ix.n_cu = n_cu;
    if (options && *options) {                       // "name=value,name=value"
        char buf[512];
        snprintf(buf, sizeof(buf), "%s", options);
        for (char *tok = strtok(buf, ","); tok; tok = strtok(nullptr, ",")) {
            char *eq = strchr(tok, '=');
            if (!eq) return api_fail(NABO_E_INVALID, "option '%s': expected name=value", tok);
            *eq = 0;
            if (!option_set(ix.opt, tok, atoll(eq + 1))) return api_fail(NABO_E_INVALID, "unknown option '%s'", tok);
        }
    }
    index_init_filters(&ix, (l2_mode && *l2_mode) ? l2_mode : nullptr);
    ix.ref_tiles = (n_ref + 31) / 32;
    ix.ref_tiles_alloc = ix.ref_tiles + 64;
    const int drop = drop_first ? 1 : 0;
    const bool cand = n_cand > 0;
    const int kq = cand ? n_cand : k;
    for (int i = 0; i < NABO_PLAN_FIELDS; ++i) out[i] = 0;
    if (kq + (cand ? 0 : drop) > NABO_MAX_K || ix.ksteps < 0) {          // the exact float64 kernels answer every row
        out[0] = NABO_PASS_EXACT;
        out[1] = -1;
        if (kernel && kernel_len) snprintf(kernel, kernel_len, "exact_dist_rows_kernel + exact_select_rows_kernel (float64 brute force)");
        return NABO_OK;
    }
    L2Plan P;
    int rc = plan_l2(&ix, m, kq, cand ? 0 : drop, cand, &P);
    if (rc) return rc;
    int pt = 0, gt = 0;
    if (P.on_l2c && ix.opt.prepass > 0) nabo::l2c_pre_plan(P.kcq, P.lkeep, (int)P.tps, ix.opt.prepass, &pt, &gt);
    out[0] = P.use_1 ? NABO_PASS_ONE_PRODUCT : NABO_PASS_SECOND;
    out[1] = P.geo;
    out[2] = P.rows_per_wg;
    out[3] = P.gx_main;
    out[4] = P.gx_tail;
    out[5] = P.S;
    out[6] = P.S2;
    out[7] = P.lkeep;
    out[8] = P.L;
    out[9] = P.tps;
    out[10] = pt;
    out[11] = gt;
    out[12] = (int64_t)n_cu * P.wg_per_cu;
    out[13] = P.gx_main * P.S + P.gx_tail * P.S2;
    out[14] = P.rows_pad;
    out[15] = P.kcq;                                 // (out[16], out[17]: the launch cut into pieces, removed -- always 0)
    if (kernel && kernel_len) snprintf(kernel, kernel_len, "%s", P.kernel);
    return NABO_OK;
}

int nabo_index_last_row_pass(const nabo_index *ix, uint8_t *out, int64_t m)
{
    if (!ix || !out) return api_fail(NABO_E_INVALID, "NULL argument");
    if ((int64_t)ix->row_pass.size() != m)
        return api_fail(NABO_E_INVALID, "the last nabo_index_query on this index had %lld rows, not %lld (candidate queries keep no record)",
                        (long long)ix->row_pass.size(), (long long)m);
    if (m > 0) memcpy(out, ix->row_pass.data(), (size_t)m);
    return NABO_OK;
}

int nabo_index_last_kernel(const nabo_index *ix, char *buf, size_t n)
{
    if (!ix || !buf || n == 0) return api_fail(NABO_E_INVALID, "NULL argument");
    snprintf(buf, n, "%s", ix->kernel);
    return NABO_OK;
}

int nabo_knn(const double *X, int64_t m, const double *Y, int64_t n, int32_t g, int32_t k, int32_t metric,
             double dist_factor, const uint8_t *ref_mask, int32_t drop_first, int64_t *out_idx, double *out_dist,
             int32_t device)
{
    if (!X || !Y || !out_idx || !out_dist) return api_fail(NABO_E_INVALID, "NULL argument");
    nabo_index *ix = nullptr;
    int rc = nabo_index_create(&ix, device, n, g, metric, dist_factor, 0);
    if (rc) return rc;
    rc = nabo_index_set_ref(ix, Y, 0, ref_mask);
    if (!rc) rc = nabo_index_query(ix, X, 0, m, k, drop_first, out_idx, out_dist, 0);
    nabo_index_destroy(ix);
    return rc;
}

int nabo_pairwise(const double *X, int64_t m, const double *Y, int64_t n, int32_t g, int32_t metric,
                  double dist_factor, double *D, int32_t device)
{
    if (!X || !Y || !D) return api_fail(NABO_E_INVALID, "NULL argument");
    if (m < 1 || n < 1 || g < 1) return api_fail(NABO_E_INVALID, "empty operand");
    if (metric != NABO_METRIC_EUCLIDEAN && metric != NABO_METRIC_MOD_CANBERRA && metric != NABO_METRIC_COSINE)
        return api_fail(NABO_E_INVALID, "unknown metric %d", metric);
    if (m > 65535) return api_fail(NABO_E_UNSUPPORTED, "nabo_pairwise is the tile-sized seam: m <= 65535");
    int rc = use_device(device);
    if (rc) return rc;
    DevBuf dx, dy, dd;
    const size_t xb = (size_t)m * g * 8, yb = (size_t)n * g * 8, db = (size_t)m * n * 8;
    if ((rc = dx.reserve(xb)) || (rc = dy.reserve(yb)) || (rc = dd.reserve(db))) {
        dx.release(); dy.release(); dd.release();
        return rc;
    }
    hipError_t e = hipMemcpy(dx.p, X, xb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dy.p, Y, yb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = nabo::pairwise_launch(dx.as<double>(), m, dy.as<double>(), n, g, metric, dist_factor,
                                                   dd.as<double>(), nullptr);
    if (e == hipSuccess) e = hipMemcpy(D, dd.p, db, hipMemcpyDeviceToHost);
    dx.release(); dy.release(); dd.release();
    if (e != hipSuccess) return api_fail(NABO_E_HIP, "nabo_pairwise: %s", hipGetErrorString(e));
    return NABO_OK;
}

int nabo_merge_topk(int32_t device, const int64_t *parts_idx, const double *parts_dist, int32_t n_parts, int64_t m,
                    int32_t kp, int32_t k, int32_t drop_first, int64_t *out_idx, double *out_dist)
{
    if (!parts_idx || !parts_dist || !out_idx || !out_dist) return api_fail(NABO_E_INVALID, "NULL argument");
    const int drop = drop_first ? 1 : 0;
    if (n_parts < 1 || m < 1 || kp < 1 || k < 1) return api_fail(NABO_E_INVALID, "bad shape");
    if (k + drop > n_parts * kp) return api_fail(NABO_E_INVALID, "k + drop_first exceeds n_parts * kp");
    if ((int64_t)n_parts * kp > 1024) return api_fail(NABO_E_UNSUPPORTED, "n_parts * kp > 1024");
    int rc = use_device(device);
    if (rc) return rc;
    HIP_TRY(nabo::merge_parts_launch(parts_dist, parts_idx, n_parts, m, kp, k, drop, out_idx, out_dist, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NABO_OK;
}

int nabo_snn_counts(int32_t device, const int64_t *t_idx, int64_t m, const int64_t *r_idx, int64_t n, int32_t k,
                    int32_t *out_snn)
{
    if (!t_idx || !r_idx || !out_snn) return api_fail(NABO_E_INVALID, "NULL argument");
    if (m < 1 || n < 1 || k < 1) return api_fail(NABO_E_INVALID, "bad shape");
    int rc = use_device(device);
    if (rc) return rc;
    HIP_TRY(nabo::snn_counts_launch(t_idx, m, r_idx, n, k, out_snn, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return NABO_OK;
}

int nabo_dev_malloc(int32_t device, void **ptr, size_t bytes)
{
    if (!ptr) return api_fail(NABO_E_INVALID, "NULL argument");
    int rc = use_device(device);
    if (rc) return rc;
    HIP_TRY(hipMalloc(ptr, bytes ? bytes : 1));
    return NABO_OK;
}

int nabo_dev_free(int32_t device, void *ptr)
{
    int rc = use_device(device);
    if (rc) return rc;
    if (ptr) HIP_TRY(hipFree(ptr));
    return NABO_OK;
}

int nabo_memcpy_h2d(int32_t device, void *dst, const void *src, size_t bytes)
{
    int rc = use_device(device);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return NABO_OK;
}

int nabo_memcpy_d2h(int32_t device, void *dst, const void *src, size_t bytes)
{
    int rc = use_device(device);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return NABO_OK;
}

int nabo_dev_mem_info(int32_t device, size_t *free_bytes, size_t *total_bytes)
{
    if (!free_bytes || !total_bytes) return api_fail(NABO_E_INVALID, "NULL argument");
    int rc = use_device(device);
    if (rc) return rc;
    HIP_TRY(hipMemGetInfo(free_bytes, total_bytes));
    return NABO_OK;
}

int nabo_dev_synchronize(int32_t device)
{
    int rc = use_device(device);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return NABO_OK;
}

}  // extern "C"

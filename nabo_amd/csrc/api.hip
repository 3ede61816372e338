// api.hip -- C ABI of libnabo_knn.so (include/nabo_knn.h).  Host orchestration only:
// buffer management, kernel sequencing on the index's HIP stream, HIP-event timing.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/nabo_knn_inspect.h"
#include "index.h"

using namespace nabo;

namespace nabo {
int index_device(const nabo_index *ix) { return ix->device; }
int index_g(const nabo_index *ix) { return ix->shape.g; }
int64_t index_n(const nabo_index *ix) { return ix->shape.n; }
int index_metric(const nabo_index *ix) { return ix->shape.metric; }
bool index_can_emit_candidates(const nabo_index *ix) { return ix->shape.metric != NABO_METRIC_MOD_CANBERRA && ix->shape.ksteps > 0; }
void index_set_shard_mode(nabo_index *ix, bool on) { ix->shard_mode = on; }
void index_set_cand_slack(nabo_index *ix, int s) { ix->shape.cand_slack = s < 0 ? 0 : s; }

// one asynchronous query may be in flight per index: every other call on it is refused until nabo_index_query_wait
int index_idle(const nabo_index *ix)
{
    if (ix && ix->async_busy) return api_fail(NABO_E_INVALID, "an asynchronous query is in flight on this index: nabo_index_query_wait first");
    return NABO_OK;
}
}  // namespace nabo

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
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    ix->device = device;
    ix->shape = make_shape(n_ref, g, metric, cus, getenv("NABO_L2_MODE"));
    ix->f = dist_factor;
    ix->base = ref_index_base;
    {   // NABO_CANBERRA_MODE = exact | swar | bits pins the modified-Canberra path (default: by the size of the reference set)
        const char *cmode = getenv("NABO_CANBERRA_MODE");
        ix->cb_mode = !cmode ? 0 : strcmp(cmode, "exact") == 0 ? 1 : strcmp(cmode, "swar") == 0 ? 2 : strcmp(cmode, "bits") == 0 ? 3 : 0;
    }
    hipError_t e = hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking);
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipEventCreate(&ix->ev[i]);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ix->stream2, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ix->ev_main, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ix->ev_ref, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ix->ref.l2.ev_ymax, hipEventDisableTiming);
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
    if (int rc = index_idle(ix)) return rc;
    if (!option_set(ix->shape.opt, name, value)) return api_fail(NABO_E_INVALID, "unknown option '%s'", name);
    if (strcmp(name, "order_flags") == 0) {      // (locality-ordered streaming was measured slower and removed)
        ix->shape.opt.order_flags = 0;
        return api_fail(NABO_E_UNSUPPORTED, "option '%s' (locality-ordered streaming, once in experiments builds only) was removed", name);
    }
    const int kc1 = ix->shape.kc1;
    shape_refresh(ix->shape);
    if (ix->shape.kc1 != kc1) ix->ref.l2.packed_c1 = false;      // (the one-product operands have another number of steps now)
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
    if (ix->ref.l2.ev_ymax) (void)hipEventDestroy(ix->ref.l2.ev_ymax);
    if (ix->ref.l2.ymax_host) (void)hipHostFree(ix->ref.l2.ymax_host);
    if (ix->stream) (void)hipStreamDestroy(ix->stream);
    delete ix;                       // every DevBuf member frees its allocation (the device is current)
    return NABO_OK;
}

// (every entry point that touches an index first waits for the asynchronous query it may have in flight and hands its
// status to nabo_index_query_wait)
static void async_join(nabo_index *ix)
{
    if (ix && ix->async_thread.joinable()) ix->async_thread.join();
}

// a top-level query: the first link of the pass chain, with the references' weak-bound memory as it stands
static int query_top(nabo_index *ix, const double *X, int32_t x_on_device, int64_t m, int32_t k, int32_t drop_first,
                     int64_t *out_idx, double *out_dist, int32_t out_on_device, bool cand_mode, double *out_bound)
{
    if (!ix) return api_fail(NABO_E_INVALID, "NULL argument");
    PassCtx top;
    top.coarse_weak = ix->ref.l2.coarse_weak;
    top.tl_no = !ix->ref.l2.stream_verdict.streams();
    PassResult res;
    return query_impl(ix, top, X, x_on_device, m, k, drop_first, out_idx, out_dist, out_on_device, cand_mode, out_bound, &res);
}

int nabo_index_query(nabo_index *ix, const double *X, int32_t x_on_device, int64_t m, int32_t k,
                     int32_t drop_first, int64_t *out_idx, double *out_dist, int32_t out_on_device)
{
    if (int rc = index_idle(ix)) return rc;
    return query_top(ix, X, x_on_device, m, k, drop_first, out_idx, out_dist, out_on_device, false, nullptr);
}

int nabo_index_query_async(nabo_index *ix, const double *X, int32_t x_on_device, int64_t m, int32_t k,
                           int32_t drop_first, int64_t *out_idx, double *out_dist, int32_t out_on_device)
{
    if (!ix) return api_fail(NABO_E_INVALID, "NULL argument");
    if (int rc = index_idle(ix)) return rc;
    async_join(ix);
    ix->async_busy = true;
    ix->async_rc = NABO_OK;
    ix->async_msg[0] = 0;
    try {
        ix->async_thread = std::thread([=]() {
            const int rc = query_top(ix, X, x_on_device, m, k, drop_first, out_idx, out_dist, out_on_device, false, nullptr);
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
    if (int rc = index_idle(ix)) return rc;
    return query_top(ix, X, x_on_device, m, n_cand, 0, out_idx, out_dist, 1, true, out_bound);
}

int nabo_index_last_stats(const nabo_index *ix, double ms[5], int64_t counters[4])
{
    if (!ix) return api_fail(NABO_E_INVALID, "NULL index");
    if (ms) memcpy(ms, ix->last.ms, sizeof(ix->last.ms));
    if (counters) memcpy(counters, ix->last.counters, sizeof(ix->last.counters));
    return NABO_OK;
}

int nabo_index_last_passes(const nabo_index *ix, int64_t rows[3])
{
    if (!ix || !rows) return api_fail(NABO_E_INVALID, "NULL argument");
    memcpy(rows, ix->last.pass_rows, sizeof(ix->last.pass_rows));
    return NABO_OK;
}

int nabo_index_last_row_pass(const nabo_index *ix, uint8_t *out, int64_t m)
{
    if (!ix || !out) return api_fail(NABO_E_INVALID, "NULL argument");
    if ((int64_t)ix->last.row_pass.size() != m)
        return api_fail(NABO_E_INVALID, "the last nabo_index_query on this index had %lld rows, not %lld (candidate queries keep no record)",
                        (long long)ix->last.row_pass.size(), (long long)m);
    if (m > 0) memcpy(out, ix->last.row_pass.data(), (size_t)m);
    return NABO_OK;
}

int nabo_index_stream_order(nabo_index *ix, uint32_t *row_map, int64_t *n_row_pos, uint32_t *ref_map, int64_t *n_ref_pos)
{
    if (!ix || !n_row_pos || !n_ref_pos) return api_fail(NABO_E_INVALID, "NULL argument");
    int rc;
    if ((rc = index_idle(ix)) || (rc = use_device(ix->device))) return rc;
    const auto &refs = ix->ref.l2.buckets;
    const auto &rows = ix->ws.buckets.rows;
    if (!rows.streamed || !refs.ordered_built || rows.positions <= 0)
        return api_fail(NABO_E_INVALID, "the last query on this index did not take the two-level stream");
    *n_row_pos = rows.positions;
    *n_ref_pos = refs.ordered_tiles * 32;
    if (!row_map || !ref_map) return NABO_OK;
    HIP_TRY(hipMemcpyAsync(row_map, rows.map.p, (size_t)*n_row_pos * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipMemcpyAsync(ref_map, refs.ordered_map.p, (size_t)*n_ref_pos * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    return NABO_OK;
}

int nabo_index_last_kernel(const nabo_index *ix, char *buf, size_t n)
{
    if (!ix || !buf || n == 0) return api_fail(NABO_E_INVALID, "NULL argument");
    snprintf(buf, n, "%s", ix->last.kernel);
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

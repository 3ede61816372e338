// sharded.hip -- reference rows sharded over the GPUs of one node: the sharded query of the C ABI
// (include/nabo_knn.h: nabo_sharded_query), on the communicators and collectives of comm.h / comm.hip.
//
// The reference has no multi-device path (its _calc_dist, nabo/_mapping.py:48-148, is one Python loop); the call
// site this entry point serves is Mapping.calc_dist (nabo/_mapping.py:441-444).
//
// Protocol (rank r of N holds reference rows [base_r, base_r + n_r); every rank sees all m target rows; rank r OWNS
// target rows [r*mr, (r+1)*mr), mr = ceil(m/N)):
//   global certification (Euclidean / cosine, k' = k + drop_first):
//     1. nabo_index_query_candidates: the first Ls entries of the shard's order rows + a lower bound on the squared
//        distance of everything the shard did not emit (Ls = nabo_candidates_per_shard(k', N, m));
//     2. one exchange: owner(row) receives N lists + N bounds;
//     3. merge by (distance, index) to k' entries; the owner accepts a row when d_k'^2 (1+1e-12) < min bound: no
//        unreported reference anywhere can then enter or tie;
//     4. refused rows (a shard held >= Ls of the global top-k'): MAX-all-reduce of the count; if any, all-gather of the
//        row ids, exact local top-k' of just those rows on every shard (nabo_index_query), all-gather, merge;
//     5. positional drop (nabo/_mapping.py:142 is positional) AFTER the merge, all-gather of the [mr,k] slices.
//   local certification (modified Canberra, or k'/N beyond the candidate lists): every shard's certified top-k',
//     the same exchange and merge.
// The merge is deterministic, so N shards == 1 shard bit for bit.
//
// Failure semantics (the reference is one process, nabo/_mapping.py:48-148: there is nothing to match -- the rule here
// is "no rank ever waits for a peer that has already given up"; the transport's half: comm.hip):
//   * every phase a rank can fail in ALONE (argument checks, buffer reservation, its local queries) ends in a status
//     agreement -- one small MAX all-reduce that also checks that all ranks were handed the same m / k / drop_first /
//     protocol -- so either every rank goes on or every rank returns an error; the communicator stays usable.  So every
//     buffer of a stretch is reserved BEFORE the agreement that opens it, and nothing that can fail alone happens
//     between two collectives;
//   * an error between two collectives or inside one aborts the communicator (nabo_sharded_query): peers return
//     NABO_E_COMM instead of hanging;
//   * a shard with fewer than k' references takes part with absent entries (-1) instead of failing its local query.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "comm.h"

namespace {

using namespace nabo;

// ---- small kernels of the protocol ------------------------------------------------------------------------
// owner's certificate: row r of my slice is final when its k'-th merged distance lies below every shard's bound
__global__ void certify_kernel(const int64_t *__restrict__ mi, const double *__restrict__ md, int kk,
                               const double *__restrict__ bounds /*[N][mr]*/, int N, int64_t mr, int64_t row0, int64_t m,
                               int64_t *__restrict__ bad_rows, unsigned long long *__restrict__ bad_count)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= mr || row0 + r >= m) return;                     // padding rows are nobody's
    double b = bounds[r];
    for (int s = 1; s < N; ++s) b = fmin(b, bounds[(int64_t)s * mr + r]);
    const double dk = md[r * kk + kk - 1];
    const bool ok = mi[r * kk + kk - 1] >= 0 && dk * dk * (1.0 + 1e-12) < b;
    if (!ok) bad_rows[atomicAdd(bad_count, 1ull)] = row0 + r;
}

// columns [d0, d0+k) of the merged [mr, kk] rows (the positional drop comes AFTER the merge)
__global__ void slice_kernel(const int64_t *__restrict__ mi, const double *__restrict__ md, int64_t mr, int kk, int d0,
                             int k, int64_t *__restrict__ oi, double *__restrict__ od)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= mr * k) return;
    const int64_t r = e / k;
    const int c = (int)(e - r * k);
    oi[e] = mi[r * kk + d0 + c];
    od[e] = md[r * kk + d0 + c];
}

// second round: rows of `sel` that I own replace my merged rows
__global__ void adopt_kernel(const uint32_t *__restrict__ sel, int64_t nb, const int64_t *__restrict__ fi,
                             const double *__restrict__ fd, int kk, int64_t row0, int64_t mr, int64_t *__restrict__ mi,
                             double *__restrict__ md)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nb * kk) return;
    const int64_t b = e / kk;
    const int64_t row = (int64_t)sel[b] - row0;
    if (row < 0 || row >= mr) return;
    mi[row * kk + (e - b * kk)] = fi[e];
    md[row * kk + (e - b * kk)] = fd[e];
}

__global__ void fill_absent_kernel(int64_t *__restrict__ idx, double *__restrict__ dist, int64_t n_idx, double *__restrict__ bnd, int64_t n_bnd)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_idx) { idx[e] = -1; dist[e] = __builtin_inf(); }
    if (bnd && e < n_bnd) bnd[e] = __builtin_inf();
}

// rows of kq entries -> rows of kk >= kq entries, the tail absent (a shard with fewer than k' references)
__global__ void widen_kernel(const int64_t *__restrict__ si, const double *__restrict__ sd, int64_t m, int kq, int kk,
                             int64_t *__restrict__ oi, double *__restrict__ od)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * kk) return;
    const int64_t r = e / kk;
    const int c = (int)(e - r * kk);
    oi[e] = c < kq ? si[r * kq + c] : -1;
    od[e] = c < kq ? sd[r * kq + c] : __builtin_inf();
}

// one thread per element, n of them, on the communicator's stream; the caller decides where the status goes: out of the
// call (between two collectives) or into the next agreement (in a local phase)
template <typename... P, typename... A> hipError_t launch_1d(nabo_comm *c, void (*kernel)(P...), int64_t n, A... args)
{
    const unsigned blk = 256;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + blk - 1) / blk)), dim3(blk), 0, c->stream, args...);
    return hipGetLastError();
}

// absent entries in idx / dist [n_idx], +inf in bnd [n_bnd] (either may be empty); a local phase's step: a NABO code
int fill_absent(nabo_comm *c, int64_t *idx, double *dist, int64_t n_idx, double *bnd, int64_t n_bnd)
{
    if (launch_1d(c, fill_absent_kernel, std::max(n_idx, n_bnd), idx, dist, n_idx, bnd, n_bnd) != hipSuccess)
        return api_fail(NABO_E_HIP, "fill_absent_kernel launch failed");
    return NABO_OK;
}

int reserve_all(std::initializer_list<std::pair<DevBuf *, size_t>> bufs)
{
    for (const auto &b : bufs)
        if (int rc = b.first->reserve(b.second)) return rc;
    return NABO_OK;
}

float ev_ms(nabo_comm *c, int a, int b)
{
    float t = 0;
    (void)hipEventElapsedTime(&t, c->ev[a], c->ev[b]);
    return t;
}

// ---- phase 0: the layout of one call ------------------------------------------------------------------------
struct ShardPlan {
    int N, R;                 // ranks; reference pieces (R divides N; R = N: every rank its own piece, the 1-D form)
    int k, d0, kk;            // columns asked for, leading ones dropped after the merge (0 / 1), k' = k + d0
    int g;                    // coordinates per row
    bool global;              // global certification (candidate lists + bounds), else local (every shard's top-k')
    int Ls;                   // entries per list a shard emits under global certification (0 under local)
    int64_t m, mr, m_pad;     // target rows; rows per owner, ceil(m / N); N mr
    int64_t row0;             // first row this rank owns
    // 2-D layout: R reference pieces x N / R target slices; my group = the R ranks [gfirst, gfirst + R) that hold the
    // pieces for my slice, rows [s0, s0 + ms_pad = R mr) (ms of them exist).  R = N: one group, the whole batch.
    int gfirst;
    int64_t s0, ms, ms_pad;
};

// Fills *p for good arguments (m, k >= 1): no HIP call, no collective.  What it returns -- NABO_OK, or the refusal of a
// protocol this layout cannot run -- goes into the first agreement.
int plan_query(const nabo_comm *c, const nabo_index *ix, int64_t m, int k, int drop_first, int protocol, ShardPlan *p)
{
    const int N = p->N = c->world, R = p->R = c->ref_shards > 0 ? c->ref_shards : N;
    p->k = k;
    p->d0 = drop_first ? 1 : 0;
    const int kk = p->kk = k + p->d0;
    p->g = index_g(ix);
    p->m = m;
    p->mr = (m + N - 1) / N;
    p->m_pad = p->mr * N;
    p->row0 = (int64_t)c->rank * p->mr;
    p->gfirst = (c->rank / R) * R;
    p->s0 = (int64_t)p->gfirst * p->mr;
    p->ms_pad = (int64_t)R * p->mr;
    p->ms = std::max<int64_t>(0, std::min(m - p->s0, p->ms_pad));
    // protocol: 0 auto, 1 global certification, 2 local certification
    const bool can_cand = index_can_emit_candidates(ix) && (kk + R - 1) / R <= 32;
    if (protocol < 0 || protocol > 2) return api_fail(NABO_E_INVALID, "protocol %d (0 auto, 1 global, 2 local certification)", protocol);
    if (R != N && R != 1 && (protocol == 2 || !can_cand))
        return api_fail(NABO_E_UNSUPPORTED, "the 2-D shard layout (ref_shards = %d of %d ranks) needs the global-certification protocol", R, N);
    if (R == 1 && N > 1 && protocol == 2)
        return api_fail(NABO_E_UNSUPPORTED, "pure target slicing (ref_shards = 1) runs through the global protocol's merge and gather (protocol 0 or 1)");
    if (protocol == 1 && !can_cand && R != 1)
        return api_fail(NABO_E_UNSUPPORTED, "global certification needs the Euclidean / cosine filter and k'/N <= 32");
    // (R = 1: every metric -- a rank's certified local query of its own slice needs no candidate lists)
    p->global = protocol == 1 || (protocol == 0 && (can_cand || R == 1) && N > 1);
    // (R = 1, pure target slicing: a rank holds ALL the references, its own certified first k' entries ARE the answer --
    // they travel through the same merge / certificate / gather with a bound of +inf)
    p->Ls = p->global ? (R == 1 ? kk : nabo_candidates_per_shard(kk, R, m)) : 0;
    // the owner's merge sorts one wave-wide batch of at most 1024 (distance, index) pairs per row
    if (p->global && (int64_t)R * p->Ls > 1024)
        return api_fail(NABO_E_UNSUPPORTED, "ref_shards * candidates per shard = %d x %d exceeds the merge width 1024", R, p->Ls);
    if ((int64_t)(p->global ? R : N) * kk > 1024)
        return api_fail(NABO_E_UNSUPPORTED, "shards * (k + drop_first) = %d x %d exceeds the merge width 1024", p->global ? R : N, kk);
    return NABO_OK;
}

// what the first round touches (the second round reserves its own, before its own agreements)
int reserve_first_round(nabo_comm *c, const ShardPlan &p)
{
    const size_t lists = p.global ? (size_t)p.ms_pad * p.Ls * 8 : (size_t)p.m_pad * p.kk * 8, bounds = p.global ? (size_t)p.ms_pad * 8 : 0;
    const size_t merged = (size_t)p.mr * p.kk * 8, out = (size_t)p.mr * p.k * 8, full = p.m_pad != p.m ? (size_t)p.m_pad * p.k * 8 : 0;
    return reserve_all({{&c->merged.idx, merged}, {&c->merged.dist, merged}, {&c->sent.idx, lists}, {&c->sent.dist, lists},
                        {&c->received.idx, lists}, {&c->received.dist, lists}, {&c->sent.bound, bounds}, {&c->received.bound, bounds},
                        {&c->refused_count, 64}, {&c->refused_rows, (size_t)p.mr * 8}, {&c->out.idx, out}, {&c->out.dist, out},
                        {&c->full.idx, full}, {&c->full.dist, full}});
}

// ---- phase 1 (local): this shard's lists --------------------------------------------------------------------
// This rank's first kk order-row entries of rows X [m,g] into out_i / out_d [m,kk]; a shard with fewer than kk
// references answers with what it has and absent entries behind (nabo_index_query itself refuses kk > n_ref).
int local_topk(nabo_comm *c, nabo_index *ix, const double *X, int64_t m, int kk, int64_t *out_i, double *out_d)
{
    const int64_t n = index_n(ix);
    if ((int64_t)kk <= n) return nabo_index_query(ix, X, 1, m, kk, 0, out_i, out_d, 1);
    const int kq = (int)n;
    int rc;
    if ((rc = reserve_all({{&c->short_.idx, (size_t)m * kq * 8}, {&c->short_.dist, (size_t)m * kq * 8}}))) return rc;
    if ((rc = nabo_index_query(ix, X, 1, m, kq, 0, c->short_.i(), c->short_.d(), 1))) return rc;
    (void)hipSetDevice(c->device);
    HIP_TRY(launch_1d(c, widen_kernel, m * kk, c->short_.i(), c->short_.d(), m, kq, kk, out_i, out_d));
    return NABO_OK;
}

// A failure here does not leave the call: the status it returns is carried into the next agreement.
int local_lists(nabo_comm *c, const ShardPlan &p, nabo_index *ix, const double *X)
{
    int rc = NABO_OK;
    const Lists &l = c->sent;
    if (p.global) {
        if (p.ms_pad != p.ms)      // ragged tail of my slice: absent entries, +inf bounds
            rc = fill_absent(c, l.i() + p.ms * p.Ls, l.d() + p.ms * p.Ls, (p.ms_pad - p.ms) * p.Ls, l.b() + p.ms, p.ms_pad - p.ms);
        // One-product first pass (plan.hip): with few pieces a shard's Ls-th candidate is close to the global k'-th, and the
        // certificate needs the exact distance of the first candidate left out, not the one-product threshold (three
        // kept entries more than emitted); with many pieces it lies far beyond it and the shorter lists win (one rank of
        // eight: 25 instead of 32 ms, one refused row at 1M x 1M).
        index_set_cand_slack(ix, p.Ls >= p.kk ? 3 : 0);
        if (!rc && p.ms > 0 && p.R == 1) {
            // one piece: the certified local query (with its whole chain of passes behind the first filter), nothing is left out
            rc = fill_absent(c, nullptr, nullptr, 0, l.b(), p.ms);
            if (!rc) rc = local_topk(c, ix, X + p.s0 * p.g, p.ms, p.kk, l.i(), l.d());
        } else if (!rc && p.ms > 0)
            rc = nabo_index_query_candidates(ix, X + p.s0 * p.g, 1, p.ms, p.Ls, l.i(), l.d(), l.b());
    } else {
        // local certification: every shard's own first k' order-row entries
        if (p.m_pad != p.m) rc = fill_absent(c, l.i() + p.m * p.kk, l.d() + p.m * p.kk, (p.m_pad - p.m) * p.kk, nullptr, 0);
        if (!rc) rc = local_topk(c, ix, X, p.m, p.kk, l.i(), l.d());
    }
    (void)hipSetDevice(c->device);          // (the index selects its own device)
    if (!rc) {          // the dominant kernel of this rank's share (a second round would overwrite the index's own record)
        double ims[5] = {0, 0, 0, 0, 0};
        (void)nabo_index_last_stats(ix, ims, nullptr);
        c->ms[MS_TOPK] = ims[1];
    }
    return rc;
}

// ---- phase 2 (collective): exchange, merge, certificate ------------------------------------------------------
// *refused: the largest number of rows any owner could not certify (0 under local certification)
int exchange_and_certify(nabo_comm *c, const ShardPlan &p, int64_t *refused)
{
    int rc;
    hipStream_t st = c->stream;
    *refused = 0;
    if (!p.global) {
        if (p.N > 1) {
            Group grp(c);
            if ((rc = grp.begin())) return rc;
            if ((rc = all_to_all(c, c->sent.idx.p, c->received.idx.p, (size_t)p.mr * p.kk * 8))) return rc;
            if ((rc = all_to_all(c, c->sent.dist.p, c->received.dist.p, (size_t)p.mr * p.kk * 8))) return rc;
            if ((rc = grp.end())) return rc;
        }
        HIP_TRY(hipEventRecord(c->ev[EV_EXCHANGED], st));
        const IdxDist &parts = p.N > 1 ? c->received : c->sent;
        HIP_TRY(merge_parts_launch(parts.d(), parts.i(), p.N, p.mr, p.kk, p.kk, 0, c->merged.i(), c->merged.d(), st));
        HIP_TRY(hipEventRecord(c->ev[EV_CERTIFIED], st));
        return NABO_OK;
    }
    {
        Group grp(c);
        if ((rc = grp.begin())) return rc;
        if ((rc = all_to_all(c, c->sent.idx.p, c->received.idx.p, (size_t)p.mr * p.Ls * 8, p.gfirst, p.R))) return rc;
        if ((rc = all_to_all(c, c->sent.dist.p, c->received.dist.p, (size_t)p.mr * p.Ls * 8, p.gfirst, p.R))) return rc;
        if ((rc = all_to_all(c, c->sent.bound.p, c->received.bound.p, (size_t)p.mr * 8, p.gfirst, p.R))) return rc;
        if ((rc = grp.end())) return rc;
    }
    HIP_TRY(hipEventRecord(c->ev[EV_EXCHANGED], st));
    HIP_TRY(merge_parts_launch(c->received.d(), c->received.i(), p.R, p.mr, p.Ls, p.kk, 0, c->merged.i(), c->merged.d(), st));
    HIP_TRY(hipMemsetAsync(c->refused_count.p, 0, 16, st));
    HIP_TRY(launch_1d(c, certify_kernel, p.mr, c->merged.i(), c->merged.d(), p.kk, c->received.b(), p.R, p.mr, p.row0, p.m,
                      c->refused_rows.as<int64_t>(), c->refused_count.as<unsigned long long>()));
    HIP_TRY(hipEventRecord(c->ev[EV_CERTIFIED], st));
    // my count stays in refused_count[0]; the MAX over ranks goes through [1]
    HIP_TRY(hipMemcpyAsync(c->refused_count.as<int64_t>() + 1, c->refused_count.p, 8, hipMemcpyDeviceToDevice, st));
    return all_reduce_max(c, c->refused_count.as<int64_t>() + 1, refused);
}

// ---- second round: rows some owner refused (at most nb_max per owner), re-solved exactly on every piece -------------
int second_round(nabo_comm *c, const ShardPlan &p, nabo_index *ix, const double *X, int64_t nb_max)
{
    int rc;
    hipStream_t st = c->stream;
    SecondRound &s = c->second;
    int64_t mine = 0;
    std::vector<int64_t> ids((size_t)nb_max, -1);
    HIP_TRY(hipMemcpyAsync(&mine, c->refused_count.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (mine > 0) {
        HIP_TRY(hipMemcpyAsync(ids.data(), c->refused_rows.p, (size_t)mine * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::sort(ids.begin(), ids.begin() + mine);           // the atomics' order is not reproducible
    }
    rc = reserve_all({{&s.my_rows, (size_t)nb_max * 8}, {&s.all_rows, (size_t)p.N * nb_max * 8}});
    if ((rc = agree(c, rc, "second-round buffers"))) return rc;
    HIP_TRY(hipMemcpyAsync(s.my_rows.p, ids.data(), (size_t)nb_max * 8, hipMemcpyHostToDevice, st));
    if ((rc = all_gather(c, s.my_rows.p, s.all_rows.p, (size_t)nb_max * 8))) return rc;
    std::vector<int64_t> all((size_t)p.N * nb_max);
    HIP_TRY(hipMemcpyAsync(all.data(), s.all_rows.p, all.size() * 8, hipMemcpyDeviceToHost, st));
    if ((rc = stream_wait(c))) return rc;
    std::vector<uint32_t> sel;                                 // rank-major, identical on every rank
    for (int64_t v : all)
        if (v >= 0) sel.push_back((uint32_t)v);
    const int64_t nb = (int64_t)sel.size();
    c->counters[CNT_UNCERTIFIED] = nb;
    // (local again: buffers for, and the exact query of, the refused rows on this rank's piece)
    const size_t part = (size_t)nb * p.kk * 8;
    rc = reserve_all({{&s.rows, (size_t)nb * 4}, {&s.x, (size_t)nb * p.g * 8}, {&s.mine.idx, part}, {&s.mine.dist, part},
                      {&s.gathered.idx, p.N * part}, {&s.gathered.dist, p.N * part}, {&s.merged.idx, part}, {&s.merged.dist, part}});
    if (!rc) {
        hipError_t e = hipMemcpyAsync(s.rows.p, sel.data(), (size_t)nb * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = gather_rows_launch(X, s.rows.as<uint32_t>(), nb, p.g, s.x.as<double>(), st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = api_fail(NABO_E_HIP, "second round: %s", hipGetErrorString(e));
    }
    if (!rc) rc = local_topk(c, ix, s.x.as<double>(), nb, p.kk, s.mine.i(), s.mine.d());
    (void)hipSetDevice(c->device);
    if ((rc = agree(c, rc, "second-round query"))) return rc;
    {
        Group grp(c);
        if ((rc = grp.begin())) return rc;
        if ((rc = all_gather(c, s.mine.idx.p, s.gathered.idx.p, part))) return rc;
        if ((rc = all_gather(c, s.mine.dist.p, s.gathered.dist.p, part))) return rc;
        if ((rc = grp.end())) return rc;
    }
    // (every rank re-solved every refused row on its reference piece; the R parts of MY group cover all pieces)
    HIP_TRY(merge_parts_launch(s.gathered.d() + (size_t)p.gfirst * nb * p.kk, s.gathered.i() + (size_t)p.gfirst * nb * p.kk, p.R, nb,
                               p.kk, p.kk, 0, s.merged.i(), s.merged.d(), st));
    HIP_TRY(launch_1d(c, adopt_kernel, nb * p.kk, s.rows.as<uint32_t>(), nb, s.merged.i(), s.merged.d(), p.kk, p.row0, p.mr,
                      c->merged.i(), c->merged.d()));
    return NABO_OK;
}

// ---- positional drop after the merge, then every rank gets every owner's slice --------------------------------
int slice_and_gather(nabo_comm *c, const ShardPlan &p, int64_t *out_idx, double *out_dist)
{
    int rc;
    hipStream_t st = c->stream;
    const size_t slice = (size_t)p.mr * p.k * 8;
    HIP_TRY(launch_1d(c, slice_kernel, p.mr * p.k, c->merged.i(), c->merged.d(), p.mr, p.kk, p.d0, p.k, c->out.i(), c->out.d()));
    HIP_TRY(hipEventRecord(c->ev[EV_SLICED], st));
    // (the gather writes N whole slices: into the caller's arrays only when they hold as many rows)
    int64_t *fi = p.m_pad != p.m ? c->full.i() : out_idx;
    double *fd = p.m_pad != p.m ? c->full.d() : out_dist;
    if (p.N > 1) {
        Group grp(c);
        if ((rc = grp.begin())) return rc;
        if ((rc = all_gather(c, c->out.idx.p, fi, slice))) return rc;
        if ((rc = all_gather(c, c->out.dist.p, fd, slice))) return rc;
        if ((rc = grp.end())) return rc;
    } else {
        HIP_TRY(hipMemcpyAsync(fi, c->out.idx.p, slice, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(fd, c->out.dist.p, slice, hipMemcpyDeviceToDevice, st));
    }
    if (p.m_pad != p.m) {
        HIP_TRY(hipMemcpyAsync(out_idx, fi, (size_t)p.m * p.k * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(out_dist, fd, (size_t)p.m * p.k * 8, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipEventRecord(c->ev[EV_GATHERED], st));
    return NABO_OK;
}

int sharded_query_impl(nabo_comm *c, nabo_index *ix, const double *X, int64_t m, int32_t k, int32_t drop_first,
                       int64_t *out_idx, double *out_dist, int32_t protocol)
{
    // ---- phase 0 (local): arguments, protocol, buffers; agreed on before anything is exchanged ----------------
    int rc;
    ShardPlan p = {};
    if (!ix || !X || !out_idx || !out_dist) rc = api_fail(NABO_E_INVALID, "NULL argument");
    else if (m < 1 || k < 1) rc = api_fail(NABO_E_INVALID, "bad shape m=%lld k=%d", (long long)m, k);
    else if (index_device(ix) != c->device) rc = api_fail(NABO_E_INVALID, "index and communicator live on different devices");
    else rc = use_device(c->device);
    if (!rc) rc = plan_query(c, ix, m, k, drop_first, protocol, &p);
    for (double &v : c->ms) v = 0.0;
    c->counters[CNT_UNCERTIFIED] = c->counters[CNT_UNUSED] = 0;
    c->counters[CNT_CANDIDATES] = p.Ls;
    c->counters[CNT_PROTOCOL] = p.global ? 1 : 2;
    // every buffer of the call is reserved HERE, before the agreement: an allocation that fails later would fail
    // between two collectives
    if (!rc) rc = reserve_first_round(c, p);
    const int64_t args[3] = {m, (int64_t)k * 2 + (drop_first ? 1 : 0), protocol};
    if ((rc = agree(c, rc, "argument", args, 3))) return rc;
    HIP_TRY(hipEventRecord(c->ev[EV_START], c->stream));

    rc = local_lists(c, p, ix, X);
    if ((rc = agree(c, rc, "local query"))) return rc;
    HIP_TRY(hipEventRecord(c->ev[EV_LISTS], c->stream));

    // ---- collective from here on: an error leaves the call, and nabo_sharded_query aborts the communicator -------
    int64_t refused = 0;
    if ((rc = exchange_and_certify(c, p, &refused))) return rc;
    if (refused > 0 && (rc = second_round(c, p, ix, X, refused))) return rc;      // (with two agreements of its own)
    HIP_TRY(hipEventRecord(c->ev[EV_SECOND], c->stream));
    if ((rc = slice_and_gather(c, p, out_idx, out_dist))) return rc;
    if ((rc = stream_wait(c))) return rc;
    for (int ph = MS_LOCAL; ph <= MS_GATHER; ++ph) c->ms[ph] = ev_ms(c, ph, ph + 1);
    c->ms[MS_TOTAL] = ev_ms(c, EV_START, EV_GATHERED);
    return NABO_OK;
}

}  // namespace

extern "C" {

int32_t nabo_candidates_per_shard(int32_t kk, int32_t world, int64_t m)
{
    // smallest list length that leaves an expected < 0.1 rows of the batch for the second round:
    // world * m * P[Bin(kk, 1/world) >= Ls] < 0.1 (exchangeable shards); never more than kk+1, at least ceil(kk/world)
    if (kk < 1 || world < 1) return 0;
    const int cap = std::min(kk + 1, 32);
    const double p = 1.0 / world;
    double tail = 0.0;
    int ls = cap;
    for (int j = kk; j >= 1; --j) {
        double cb = 1.0;                       // C(kk, j)
        for (int i = 1; i <= j; ++i) cb = cb * (double)(kk - j + i) / (double)i;
        tail += cb * std::pow(p, j) * std::pow(1.0 - p, kk - j);
        if (tail * world * (double)(m > 0 ? m : 1) >= 0.1) { ls = j + 1; break; }
        ls = j;
    }
    ls = std::min(ls, cap);
    ls = std::max(ls, (kk + world - 1) / world);
    return std::max(ls, 1);
}

int nabo_sharded_query(nabo_comm *c, nabo_index *ix, const double *X, int64_t m, int32_t k, int32_t drop_first,
                       int64_t *out_idx, double *out_dist, int32_t protocol)
{
    if (!c) return api_fail(NABO_E_INVALID, "NULL communicator");
    if (c->aborted) return comm_dead(c);
    // With more than one shard, a shard's local queries must not continue a short row with its MASKED references
    // (query.hip: tail_len): they would enter the merge as neighbours.  Rows with fewer than k' unmasked references in
    // the WHOLE reference set then end in absent entries (-1 / NaN) instead of the ignored references by index.
    const bool shards = ix && c->world > 1;
    if (shards) index_set_shard_mode(ix, true);
    c->agreed = false;
    const int rc = sharded_query_impl(c, ix, X, m, k, drop_first, out_idx, out_dist, protocol);
    if (shards) index_set_shard_mode(ix, false);
    // An error every rank agreed on leaves the communicator usable; anything else happened between two collectives
    // (or inside one): peers may be waiting for this rank -- release them.
    if (rc && !c->agreed && c->world > 1) {
        char keep[512];
        snprintf(keep, sizeof(keep), "%s", nabo_last_error());
        comm_abort(c);
        (void)api_fail(rc, "%s", keep);
    }
    return rc;
}

int nabo_sharded_last_stats(const nabo_comm *c, double ms[8], int64_t counters[4])
{
    if (!c) return api_fail(NABO_E_INVALID, "NULL communicator");
    if (ms) memcpy(ms, c->ms, sizeof(c->ms));
    if (counters) memcpy(counters, c->counters, sizeof(c->counters));
    return NABO_OK;
}

}  // extern "C"

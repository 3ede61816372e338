// comm.hip -- the transports under the sharded query (sharded.hip): communicators of the C ABI (include/nabo_knn.h:
// nabo_comm_*), the collectives and the status agreement declared in comm.h.  Everything that knows whether a rank talks
// RCCL or loopback is in this file.  No torch, no MPI.
//
// Transports
//   * RCCL over xGMI (the product path): librccl.so is dlopen'ed on first use -- a host that never shards does not
//     need it -- one communicator per GPU, created either per rank (one process per GPU: ncclCommInitRank with a
//     unique id the caller passes around) or for all devices of one process (ncclCommInitAll; one host thread per
//     device then drives its rank).  Every exchange is ONE grouped operation: the candidate lists, their distances and
//     the bounds go out as ncclSend/ncclRecv pairs inside a single ncclGroupStart/End, the result slices as two
//     ncclAllGather in one group.  xGMI is point to point: each peer pair moves only the m/N rows the receiver owns.
//   * loopback: N ranks as host threads of ONE process, rendezvous through a host barrier and device-to-device
//     copies.  Same call sequence, same buffers, same kernels -- it exists so that the whole protocol can be run (and
//     is tested) with N shards on a single GPU; it is also a correct transport for several peer-accessible devices.
//
// Failure semantics, the transport's half (the protocol's half: sharded.hip): an error INSIDE a collective (RCCL
// failure, a kernel launch between two collectives, a peer that never arrives) aborts the communicator: ncclCommAbort
// for RCCL, the hub's abort flag for the loopback transport; an opened RCCL group is always closed first.  Peers blocked
// in the same collective then return NABO_E_COMM instead of hanging: host waits on an RCCL stream poll hipStreamQuery +
// ncclCommGetAsyncError with a deadline (nabo_comm_set_timeout, NABO_COMM_TIMEOUT_S, default 600 s), the loopback
// barrier is a timed condition wait.
#include <dlfcn.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "comm.h"

// ---- loopback rendezvous ---------------------------------------------------------------------------------
// An abortable, timed barrier: a rank that fails, or nabo_comm_abort from any thread, releases everyone who waits (and
// everyone who will), and a rank whose peers never arrive gives up after the deadline and aborts the hub itself.
constexpr int NABO_AGREE_MAX = 8;

struct nabo::LoopHub {
    int n = 0;
    int refs = 0;
    pthread_mutex_t lock = PTHREAD_MUTEX_INITIALIZER;
    pthread_cond_t cv = PTHREAD_COND_INITIALIZER;
    int arrived = 0;
    unsigned long gen = 0;
    bool aborted = false;
    std::vector<const void *> ptr;
    std::vector<int64_t> vals;          // [n][NABO_AGREE_MAX]
};

namespace {

using namespace nabo;

// ---- librccl.so, resolved at run time -------------------------------------------------------------------
#define NABO_RCCL_SYMBOLS(X)                                                                                         \
    X(GetUniqueId) X(CommInitRank) X(CommInitAll) X(CommDestroy) X(CommAbort) X(CommCount) X(CommGetAsyncError)      \
    X(AllReduce) X(AllGather) X(Send) X(Recv) X(GroupStart) X(GroupEnd) X(GetErrorString)

struct Rccl {
    void *h = nullptr;
#define NABO_SYM(name) decltype(&nccl##name) name = nullptr;
    NABO_RCCL_SYMBOLS(NABO_SYM)
#undef NABO_SYM
};

Rccl g_rccl;
pthread_mutex_t g_rccl_lock = PTHREAD_MUTEX_INITIALIZER;

int load_rccl()
{
    pthread_mutex_lock(&g_rccl_lock);
    if (!g_rccl.h) {
        const char *env = getenv("NABO_RCCL_LIB");
        const char *names[] = {env, "librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"};
        void *h = nullptr;
        for (const char *nm : names)
            if (nm && *nm && (h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!h) {
            pthread_mutex_unlock(&g_rccl_lock);
            return api_fail(NABO_E_UNSUPPORTED, "librccl.so could not be loaded (%s): multi-GPU sharding needs RCCL", dlerror());
        }
        bool ok = true;
#define NABO_SYM(name) ok = (g_rccl.name = reinterpret_cast<decltype(g_rccl.name)>(dlsym(h, "nccl" #name))) && ok;
        NABO_RCCL_SYMBOLS(NABO_SYM)
#undef NABO_SYM
        if (!ok) {
            dlclose(h);
            pthread_mutex_unlock(&g_rccl_lock);
            return api_fail(NABO_E_UNSUPPORTED, "librccl.so lacks a required entry point");
        }
        g_rccl.h = h;
    }
    pthread_mutex_unlock(&g_rccl_lock);
    return NABO_OK;
}

double now_s()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

double default_timeout_s()
{
    const char *s = getenv("NABO_COMM_TIMEOUT_S");
    const double v = (s && *s) ? atof(s) : 0.0;
    return v > 0.0 ? v : 600.0;
}

// An RCCL call of the rank's own thread failed: an open group is closed FIRST (ncclGroupEnd on operations of a freed
// communicator is undefined), then the communicator is aborted.
void rccl_failed(nabo_comm *c)
{
    if (c->group_open) {
        c->group_open = false;
        (void)g_rccl.GroupEnd();
    }
    comm_abort(c);
}

#define RCCL_TRY(expr)                                                                                  \
    do {                                                                                                \
        if (c->aborted.load()) return comm_dead(c);      /* the handle may be gone: never enqueue on it */ \
        ncclResult_t r__ = (expr);                                                                      \
        if (r__ != ncclSuccess) {                                                                       \
            const int rc__ = api_fail(NABO_E_COMM, "%s failed: %s", #expr, g_rccl.GetErrorString(r__)); \
            rccl_failed(c);                                                                             \
            return rc__;                                                                                \
        }                                                                                               \
    } while (0)

// loopback barrier: NABO_OK when all n ranks arrived; NABO_E_COMM when the hub was aborted or the deadline passed
int hub_wait(nabo_comm *c)
{
    LoopHub *h = c->hub;
    int rc = NABO_OK;
    pthread_mutex_lock(&h->lock);
    if (h->aborted) {
        rc = NABO_E_COMM;
    } else {
        const unsigned long gen0 = h->gen;
        if (++h->arrived == h->n) {
            h->arrived = 0;
            ++h->gen;
            pthread_cond_broadcast(&h->cv);
        } else {
            timespec dl;
            clock_gettime(CLOCK_REALTIME, &dl);
            const double t = (double)dl.tv_sec + 1e-9 * (double)dl.tv_nsec + c->timeout_s;
            dl.tv_sec = (time_t)t;
            dl.tv_nsec = (long)((t - (double)dl.tv_sec) * 1e9);
            while (h->gen == gen0 && !h->aborted)
                if (pthread_cond_timedwait(&h->cv, &h->lock, &dl) != 0 && h->gen == gen0) {      // ETIMEDOUT: give up for everyone
                    h->aborted = true;
                    pthread_cond_broadcast(&h->cv);
                }
            if (h->gen == gen0) rc = NABO_E_COMM;
        }
    }
    pthread_mutex_unlock(&h->lock);
    if (rc) {
        c->aborted.store(true);
        return api_fail(NABO_E_COMM, "rank %d: the loopback group was aborted (a peer failed, or did not arrive within %.0f s)", c->rank, c->timeout_s);
    }
    return NABO_OK;
}

// loopback exchange: every rank publishes its send buffer; block b of `recv` (bytes each, `count` of them) is copied
// from byte `off` of peer first + b's
int hub_exchange(nabo_comm *c, const void *send, void *recv, size_t bytes, int first, int count, size_t off)
{
    int rc;
    HIP_TRY(hipStreamSynchronize(c->stream));                 // my send buffer is final
    c->hub->ptr[c->rank] = send;
    if ((rc = hub_wait(c))) return rc;
    for (int b = 0; b < count; ++b)
        HIP_TRY(hipMemcpyAsync(static_cast<char *>(recv) + (size_t)b * bytes, static_cast<const char *>(c->hub->ptr[first + b]) + off,
                               bytes, hipMemcpyDefault, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return hub_wait(c);                                       // nobody reuses a send buffer before all have copied
}

// loopback MAX over ranks of nv (<= NABO_AGREE_MAX) int64 host values
int hub_max(nabo_comm *c, const int64_t *mine, int64_t *out, int nv)
{
    int rc;
    for (int i = 0; i < nv; ++i) c->hub->vals[(size_t)c->rank * NABO_AGREE_MAX + i] = mine[i];
    if ((rc = hub_wait(c))) return rc;
    for (int i = 0; i < nv; ++i) {
        int64_t mx = c->hub->vals[i];
        for (int p = 1; p < c->world; ++p) mx = std::max(mx, c->hub->vals[(size_t)p * NABO_AGREE_MAX + i]);
        out[i] = mx;
    }
    return hub_wait(c);                                       // nobody overwrites its values before all have read
}

int comm_alloc(nabo_comm **out, Transport transport, int device, int rank, int world)
{
    nabo_comm *c = new (std::nothrow) nabo_comm();
    if (!c) return api_fail(NABO_E_NOMEM, "host allocation failed");
    c->transport = transport; c->device = device; c->rank = rank; c->world = world;
    c->timeout_s = default_timeout_s();
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int i = 0; i < N_SHARD_EVENTS && e == hipSuccess; ++i) e = hipEventCreate(&c->ev[i]);
    if (e != hipSuccess) {
        (void)hipGetLastError();          // (the thread's sticky copy: a later launch check must not report THIS failure)
        delete c;
        return api_fail(e == hipErrorInvalidDevice ? NABO_E_NODEVICE : NABO_E_HIP, "communicator on device %d: %s", device,
                        hipGetErrorString(e));
    }
    *out = c;
    return NABO_OK;
}

}  // namespace

namespace nabo {

// RCCL: ncclCommAbort (peers' pending operations end with an error, our own stream is released); loopback: the hub's
// flag + a broadcast.
void comm_abort(nabo_comm *c)
{
    if (!c || c->aborted.exchange(true)) return;             // one caller aborts, every other one returns
    if (c->transport == TRANSPORT_RCCL) {
        pthread_mutex_lock(&c->nccl_lock);
        if (c->nccl && !c->nccl_dead && g_rccl.CommAbort) { (void)g_rccl.CommAbort(c->nccl); c->nccl_dead = true; }
        pthread_mutex_unlock(&c->nccl_lock);
    } else if (c->hub) {
        pthread_mutex_lock(&c->hub->lock);
        c->hub->aborted = true;
        pthread_cond_broadcast(&c->hub->cv);
        pthread_mutex_unlock(&c->hub->lock);
    }
}

int comm_dead(nabo_comm *c)
{
    return api_fail(NABO_E_COMM, "rank %d: the communicator was aborted (an earlier collective failed or timed out)", c->rank);
}

int Group::begin()
{
    if (c->transport == TRANSPORT_RCCL) {
        RCCL_TRY(g_rccl.GroupStart());
        open = c->group_open = true;
    }
    return NABO_OK;
}

int Group::end()
{
    if (open) {
        open = false;
        if (!c->group_open) return comm_dead(c);          // rccl_failed closed it on the way out of a failed call
        c->group_open = false;
        ncclResult_t r = g_rccl.GroupEnd();
        if (r != ncclSuccess) {
            const int rc = api_fail(NABO_E_COMM, "ncclGroupEnd failed: %s", g_rccl.GetErrorString(r));
            comm_abort(c);
            return rc;
        }
    }
    return NABO_OK;
}

Group::~Group()
{
    // (an error return between begin and end: the thread's group state must not leak into its next RCCL call)
    if (open && c->group_open) {
        c->group_open = false;
        (void)g_rccl.GroupEnd();
    }
}

// Work that depends on peers (RCCL kernels) is waited for by polling, with the asynchronous error state of the
// communicator and a deadline in the loop.
int stream_wait(nabo_comm *c)
{
    if (c->transport != TRANSPORT_RCCL || c->world == 1 || !c->nccl) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        return NABO_OK;
    }
    if (c->aborted.load()) return comm_dead(c);
    const double t0 = now_s();
    for (unsigned spins = 1;; ++spins) {
        const hipError_t e = hipStreamQuery(c->stream);
        if (e == hipSuccess) return NABO_OK;
        if (e != hipErrorNotReady) {
            const int rc = api_fail(NABO_E_HIP, "hipStreamQuery failed: %s", hipGetErrorString(e));
            comm_abort(c);
            return rc;
        }
        if ((spins & 255) == 0) {
            ncclResult_t ar = ncclSuccess;
            bool dead;
            pthread_mutex_lock(&c->nccl_lock);                // (an abort from another thread frees the handle)
            dead = c->nccl_dead;
            const bool have = !dead && g_rccl.CommGetAsyncError(c->nccl, &ar) == ncclSuccess;
            pthread_mutex_unlock(&c->nccl_lock);
            if (dead) return comm_dead(c);
            if (have && ar != ncclSuccess && ar != ncclInProgress) {
                const int rc = api_fail(NABO_E_COMM, "rank %d: RCCL reported an asynchronous error: %s", c->rank, g_rccl.GetErrorString(ar));
                comm_abort(c);
                return rc;
            }
            if (now_s() - t0 > c->timeout_s) {
                const int rc = api_fail(NABO_E_COMM, "rank %d: a collective did not complete within %.0f s (a peer is missing or has failed); "
                                        "communicator aborted", c->rank, c->timeout_s);
                comm_abort(c);
                return rc;
            }
            if (spins > 65536) usleep(50);
        }
    }
}

// ---- collectives -----------------------------------------------------------------------------------------
int all_to_all(nabo_comm *c, const void *send, void *recv, size_t bytes, int first, int count)
{
    const int N = count < 0 ? c->world : count;
    if (bytes == 0) return NABO_OK;
    if (c->transport == TRANSPORT_RCCL) {
        for (int b = 0; b < N; ++b) {
            RCCL_TRY(g_rccl.Send(static_cast<const char *>(send) + (size_t)b * bytes, bytes, ncclUint8, first + b, c->nccl, c->stream));
            RCCL_TRY(g_rccl.Recv(static_cast<char *>(recv) + (size_t)b * bytes, bytes, ncclUint8, first + b, c->nccl, c->stream));
        }
        return NABO_OK;
    }
    return hub_exchange(c, send, recv, bytes, first, N, (size_t)(c->rank - first) * bytes);
}

int all_gather(nabo_comm *c, const void *send, void *recv, size_t bytes)
{
    if (bytes == 0) return NABO_OK;
    if (c->transport == TRANSPORT_RCCL) {
        RCCL_TRY(g_rccl.AllGather(send, recv, bytes, ncclUint8, c->nccl, c->stream));
        return NABO_OK;
    }
    return hub_exchange(c, send, recv, bytes, 0, c->world, 0);
}

int all_reduce_max(nabo_comm *c, int64_t *dev_val, int64_t *host_out, int nv)
{
    if (c->transport == TRANSPORT_RCCL) {
        RCCL_TRY(g_rccl.AllReduce(dev_val, dev_val, (size_t)nv, ncclInt64, ncclMax, c->nccl, c->stream));
        HIP_TRY(hipMemcpyAsync(host_out, dev_val, sizeof(int64_t) * nv, hipMemcpyDeviceToHost, c->stream));
        return stream_wait(c);
    }
    int64_t mine[NABO_AGREE_MAX];
    HIP_TRY(hipMemcpyAsync(mine, dev_val, sizeof(int64_t) * nv, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return hub_max(c, mine, host_out, nv);
}

int agree(nabo_comm *c, int rc_local, const char *phase, const int64_t *args, int n_args)
{
    c->agreed = false;
    if (c->world == 1) { c->agreed = rc_local != NABO_OK; return rc_local; }
    char keep[512] = "";
    if (rc_local) snprintf(keep, sizeof(keep), "%s", nabo_last_error());
    int64_t v[NABO_AGREE_MAX] = {0, 0, 0, 0, 0, 0, 0, 0}, out[NABO_AGREE_MAX];
    v[0] = rc_local ? -(int64_t)rc_local : 0;                  // status codes are negative
    for (int i = 0; i < n_args && i < 3; ++i) { v[1 + 2 * i] = args[i]; v[2 + 2 * i] = -args[i]; }
    const int nv = 1 + 2 * (n_args < 3 ? n_args : 3);
    int rc = c->status.reserve(sizeof(v));
    if (!rc) {
        hipError_t e = hipMemcpyAsync(c->status.p, v, sizeof(int64_t) * nv, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);           // v is a stack array
        if (e != hipSuccess) rc = api_fail(NABO_E_HIP, "status agreement: %s", hipGetErrorString(e));
    }
    if (rc) {               // this rank cannot even take part: release the others
        comm_abort(c);
        return rc;
    }
    if ((rc = all_reduce_max(c, c->status.as<int64_t>(), out, nv))) return rc;      // (the communicator is aborted already)
    c->agreed = true;
    if (rc_local) return api_fail(rc_local, "%s", keep);
    if (out[0] != 0)
        return api_fail(NABO_E_COMM, "rank %d: a peer failed in the %s phase (status %lld); no rank went on", c->rank, phase, -(long long)out[0]);
    for (int i = 0; i < n_args && i < 3; ++i)
        if (out[1 + 2 * i] != -out[2 + 2 * i])
            return api_fail(NABO_E_INVALID, "rank %d: the ranks were handed different arguments (%s: argument %d ranges over [%lld, %lld])",
                            c->rank, phase, i, -(long long)out[2 + 2 * i], (long long)out[1 + 2 * i]);
    c->agreed = false;
    return NABO_OK;
}

}  // namespace nabo

extern "C" {

int nabo_comm_unique_id(void *id128)
{
    if (!id128) return api_fail(NABO_E_INVALID, "NULL argument");
    int rc = load_rccl();
    if (rc) return rc;
    ncclUniqueId id;
    const ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess) return api_fail(NABO_E_COMM, "ncclGetUniqueId failed: %s", g_rccl.GetErrorString(r));
    static_assert(sizeof(id) == NABO_COMM_ID_BYTES, "unique id size");
    memcpy(id128, &id, sizeof(id));
    return NABO_OK;
}

int nabo_comm_create(nabo_comm **out, int32_t device, int32_t rank, int32_t world, const void *id128)
{
    if (!out || !id128) return api_fail(NABO_E_INVALID, "NULL argument");
    *out = nullptr;
    if (world < 1 || rank < 0 || rank >= world) return api_fail(NABO_E_INVALID, "rank %d of %d", rank, world);
    int rc = load_rccl();
    if (rc) return rc;
    nabo_comm *c = nullptr;
    if ((rc = comm_alloc(&c, TRANSPORT_RCCL, device, rank, world))) return rc;
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclResult_t r = g_rccl.CommInitRank(&c->nccl, world, id, rank);
    if (r != ncclSuccess) {
        c->nccl = nullptr;
        nabo_comm_destroy(c);
        return api_fail(NABO_E_COMM, "ncclCommInitRank(rank %d of %d, device %d) failed: %s", rank, world, device, g_rccl.GetErrorString(r));
    }
    *out = c;
    return NABO_OK;
}

int nabo_comm_create_all(nabo_comm **out, const int32_t *devices, int32_t n)
{
    if (!out || !devices || n < 1) return api_fail(NABO_E_INVALID, "bad argument");
    int rc = load_rccl();
    if (rc) return rc;
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return api_fail(NABO_E_NODEVICE, "no HIP device is available");
    for (int i = 0; i < n; ++i) {
        if (devices[i] < 0 || devices[i] >= cnt)
            return api_fail(NABO_E_NODEVICE, "device %d out of range (have %d): RCCL needs one GPU per rank", devices[i], cnt);
        for (int j = 0; j < i; ++j)
            if (devices[j] == devices[i])
                return api_fail(NABO_E_INVALID, "device %d listed twice: RCCL needs one GPU per rank (the loopback transport allows repeats)", devices[i]);
    }
    std::vector<ncclComm_t> comms((size_t)n);
    std::vector<int> devs(devices, devices + n);
    const ncclResult_t r = g_rccl.CommInitAll(comms.data(), n, devs.data());
    if (r != ncclSuccess) return api_fail(NABO_E_COMM, "ncclCommInitAll over %d devices failed: %s", n, g_rccl.GetErrorString(r));
    for (int i = 0; i < n; ++i) out[i] = nullptr;
    for (int i = 0; i < n; ++i) {
        nabo_comm *c = nullptr;
        if ((rc = comm_alloc(&c, TRANSPORT_RCCL, devices[i], i, n))) {
            for (int j = 0; j < n; ++j) {
                if (out[j]) { out[j]->nccl = nullptr; nabo_comm_destroy(out[j]); out[j] = nullptr; }
                (void)g_rccl.CommDestroy(comms[(size_t)j]);
            }
            return rc;
        }
        c->nccl = comms[(size_t)i];
        out[i] = c;
    }
    return NABO_OK;
}

int nabo_comm_create_loopback(nabo_comm **out, const int32_t *devices, int32_t n)
{
    if (!out || !devices || n < 1) return api_fail(NABO_E_INVALID, "bad argument");
    LoopHub *hub = new (std::nothrow) LoopHub();
    if (!hub) return api_fail(NABO_E_NOMEM, "host allocation failed");
    hub->n = n;
    hub->refs = n;
    hub->ptr.assign((size_t)n, nullptr);
    hub->vals.assign((size_t)n * NABO_AGREE_MAX, 0);
    for (int i = 0; i < n; ++i) out[i] = nullptr;
    for (int i = 0; i < n; ++i) {
        nabo_comm *c = nullptr;
        int rc = comm_alloc(&c, TRANSPORT_LOOPBACK, devices[i], i, n);
        if (rc) {
            for (int j = 0; j < i; ++j) { out[j]->hub = nullptr; nabo_comm_destroy(out[j]); out[j] = nullptr; }
            delete hub;
            return rc;
        }
        c->hub = hub;
        out[i] = c;
    }
    return NABO_OK;
}

int nabo_comm_destroy(nabo_comm *c)
{
    if (!c) return NABO_OK;
    (void)hipSetDevice(c->device);
    if (c->nccl && !c->nccl_dead && g_rccl.CommDestroy) {
        // a stream that still waits for a peer must not block the teardown
        if (c->stream && hipStreamQuery(c->stream) == hipErrorNotReady && g_rccl.CommAbort) (void)g_rccl.CommAbort(c->nccl);
        else (void)g_rccl.CommDestroy(c->nccl);
        c->nccl = nullptr;
    }
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->hub) {
        pthread_mutex_lock(&c->hub->lock);
        const int left = --c->hub->refs;
        if (left > 0 && c->hub->arrived > 0) {          // peers are waiting for a rank that is going away
            c->hub->aborted = true;
            pthread_cond_broadcast(&c->hub->cv);
        }
        pthread_mutex_unlock(&c->hub->lock);
        if (left == 0) delete c->hub;
    }
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return NABO_OK;
}

int nabo_comm_rank(const nabo_comm *c) { return c ? c->rank : -1; }
int nabo_comm_world(const nabo_comm *c) { return c ? c->world : -1; }

int nabo_comm_transport_ranks(nabo_comm *c)
{
    if (!c) return api_fail(NABO_E_INVALID, "NULL communicator");
    if (c->aborted.load()) return comm_dead(c);
    if (c->transport != TRANSPORT_RCCL) return c->hub ? c->hub->n : 1;
    int count = -1;
    pthread_mutex_lock(&c->nccl_lock);
    const ncclResult_t r = (c->nccl && !c->nccl_dead) ? g_rccl.CommCount(c->nccl, &count) : ncclSuccess;
    pthread_mutex_unlock(&c->nccl_lock);
    if (r != ncclSuccess || count < 0) return api_fail(NABO_E_COMM, "ncclCommCount failed");
    return count;
}

int nabo_comm_abort(nabo_comm *c)
{
    if (!c) return api_fail(NABO_E_INVALID, "NULL communicator");
    comm_abort(c);
    return NABO_OK;
}

int nabo_comm_set_timeout(nabo_comm *c, double seconds)
{
    if (!c || !(seconds > 0.0)) return api_fail(NABO_E_INVALID, "bad argument");
    c->timeout_s = seconds;
    return NABO_OK;
}

int nabo_comm_set_ref_shards(nabo_comm *c, int32_t ref_shards)
{
    if (!c) return api_fail(NABO_E_INVALID, "NULL communicator");
    if (ref_shards < 0 || (ref_shards > 0 && c->world % ref_shards != 0))
        return api_fail(NABO_E_INVALID, "ref_shards = %d does not divide the world size %d", ref_shards, c->world);
    c->ref_shards = ref_shards == c->world ? 0 : ref_shards;
    return NABO_OK;
}

int nabo_comm_allreduce_max_f64(nabo_comm *c, double *value)
{
    if (!c || !value) return api_fail(NABO_E_INVALID, "NULL argument");
    if (c->aborted) return comm_dead(c);
    int rc = use_device(c->device);
    if (rc) return rc;
    if (c->world == 1) return NABO_OK;
    if ((rc = c->f64_scratch.reserve(64))) { comm_abort(c); return rc; }
    if (c->transport == TRANSPORT_RCCL) {
        HIP_TRY(hipMemcpyAsync(c->f64_scratch.p, value, sizeof(double), hipMemcpyHostToDevice, c->stream));
        RCCL_TRY(g_rccl.AllReduce(c->f64_scratch.p, c->f64_scratch.p, 1, ncclFloat64, ncclMax, c->nccl, c->stream));
        HIP_TRY(hipMemcpyAsync(value, c->f64_scratch.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        return stream_wait(c);
    }
    int64_t bits, mx;
    memcpy(&bits, value, sizeof(bits));        // callers pass non-negative times: IEEE order == integer order
    if ((rc = hub_max(c, &bits, &mx, 1))) return rc;
    memcpy(value, &mx, sizeof(mx));
    return NABO_OK;
}

int nabo_comm_barrier(nabo_comm *c)
{
    double z = 0.0;
    return nabo_comm_allreduce_max_f64(c, &z);
}

}  // extern "C"

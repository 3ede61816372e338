// comm.h -- the communicator of the C ABI (include/nabo_knn.h: nabo_comm) and what the sharded query protocol
// (sharded.hip) asks of its transport (comm.hip): abort, the status agreement, three collectives, the stream wait.
// sharded.hip never asks which transport a rank talks.  Host types only: tests/host_shim compiles both files with g++.
#pragma once
#include <pthread.h>

#include <atomic>
#include <cstdint>
#ifdef NABO_SHARDED_HOST
#include "hip_shim.h"
#else
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#endif

#include "../../include/nabo_knn.h"
#include "host_common.h"

namespace nabo {

struct LoopHub;        // comm.hip: the loopback rendezvous
enum Transport { TRANSPORT_RCCL, TRANSPORT_LOOPBACK };

// nabo_sharded_last_stats, slot by slot (ABI).  Events on the communicator's stream bound the timed phases: phase p
// (MS_LOCAL .. MS_GATHER) runs from event p to event p + 1, MS_TOTAL from the first event to the last.
enum ShardEvent { EV_START, EV_LISTS, EV_EXCHANGED, EV_CERTIFIED, EV_SECOND, EV_SLICED, EV_GATHERED, N_SHARD_EVENTS };
enum ShardMs {
    MS_LOCAL, MS_EXCHANGE, MS_CERTIFY /* merge + certificate */, MS_SECOND, MS_SLICE, MS_GATHER, MS_TOTAL,
    MS_TOPK /* the distance + top-k kernel inside MS_LOCAL */, N_SHARD_MS
};
enum ShardCounter { CNT_UNCERTIFIED, CNT_CANDIDATES, CNT_UNUSED /* always 0 */, CNT_PROTOCOL /* 1 global, 2 local */, N_SHARD_COUNTERS };

// neighbour lists [rows][width] as two parallel device buffers
struct IdxDist {
    DevBuf idx, dist;
    int64_t *i() const { return idx.as<int64_t>(); }
    double *d() const { return dist.as<double>(); }
};
// ... with, per row, a lower bound on the squared distance of everything the shard did not emit (global certification)
struct Lists : IdxDist {
    DevBuf bound;
    double *b() const { return bound.as<double>(); }
};
// the second round: nb rows some owner refused, re-solved exactly on every piece
struct SecondRound {
    DevBuf my_rows, all_rows;            // refused row ids (int64, -1 behind the last): this owner's [nb_max], every owner's [N][nb_max]
    DevBuf rows, x;                      // the nb refused rows, rank-major (uint32), and their coordinates [nb, g]
    IdxDist mine, gathered, merged;      // their exact top-k' on my piece [nb, kk], on every rank's [N][nb, kk], merged [nb, kk]
    __attribute__((visibility("hidden"))) ~SecondRound() = default;      // (emitted out of line: not a symbol of the library)
};

}  // namespace nabo

struct nabo_comm {
    nabo::Transport transport = nabo::TRANSPORT_RCCL;
    int device = 0, rank = 0, world = 1;
    ncclComm_t nccl = nullptr;
    nabo::LoopHub *hub = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev[nabo::N_SHARD_EVENTS] = {};
    // device buffers of the sharded query, grow-only and kept between calls
    nabo::Lists sent, received;          // this rank's lists by owner, [parts][mr, width]; what the owner received, [parts][mr, width]
    nabo::IdxDist merged, out, full;     // the owner's merged rows [mr, kk], their slice [mr, k], everyone's slices [m_pad, k]
    nabo::IdxDist short_;                // local_topk: the rows of a shard with fewer than k' references, [m, n_ref]
    nabo::DevBuf refused_count;          // u64 x 2: rows this owner refused, and the MAX of that over the ranks
    nabo::DevBuf refused_rows;           // their global row ids, in the order the atomics gave
    nabo::SecondRound second;
    nabo::DevBuf status, f64_scratch;    // the operands of agree() and nabo_comm_allreduce_max_f64
    double ms[nabo::N_SHARD_MS] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t counters[nabo::N_SHARD_COUNTERS] = {0, 0, 0, 0};
    // 2-D layout (nabo_comm_set_ref_shards): the references are cut into ref_shards pieces, rank r holds piece
    // r % ref_shards and answers for target slice r / ref_shards; 0 = world (every rank its own piece: the 1-D form)
    int ref_shards = 0;
    double timeout_s = 600.0;        // deadline of every wait on a peer
    std::atomic<bool> aborted{false};   // set once (exchange: one thread wins); every later call fails with NABO_E_COMM
    // nabo_comm_abort may come from ANY thread while the rank's own thread polls the handle: ncclCommAbort frees it, so the
    // handle is only touched under this lock and never again once nccl_dead is set (the pointer itself stays until destroy)
    pthread_mutex_t nccl_lock = PTHREAD_MUTEX_INITIALIZER;
    bool nccl_dead = false;
    bool group_open = false;         // the rank's thread has an RCCL group open (closed BEFORE an abort: see rccl_failed)
    bool agreed = false;             // the error being returned was agreed on by all ranks (no abort needed)
};

#pragma GCC visibility push(hidden)          // (internal to libnabo_knn.so: not in its dynamic symbol table)
namespace nabo {

// The communicator is finished: release whoever waits on it.  Idempotent; callable from any thread.
void comm_abort(nabo_comm *c);
// the error every call on an aborted communicator returns
int comm_dead(nabo_comm *c);

// Several collectives as ONE grouped operation (RCCL; the loopback transport has nothing to group): closed on every path
// out of the scope that opened it.
struct Group {
    nabo_comm *c;
    bool open = false;
    explicit Group(nabo_comm *cc) : c(cc) {}
    int begin();
    int end();
    ~Group();
};

// Host wait for the communicator's stream: a peer that died or never entered the collective turns into an error, not a hang.
int stream_wait(nabo_comm *c);

// Collectives on device pointers, on c->stream; every rank of the world makes the call.
// Among the ranks [first, first + count) (the caller's rank is one of them, each rank with its own group): block b of
// `send` (bytes each) goes to peer first + b; block b of `recv` comes from peer first + b.  The caller holds an open Group.
int all_to_all(nabo_comm *c, const void *send, void *recv, size_t bytes, int first = 0, int count = -1);
int all_gather(nabo_comm *c, const void *send, void *recv, size_t bytes);
// MAX over ranks of `nv` (<= 8) int64 values living on the device (in place) -- returned on the host too
int all_reduce_max(nabo_comm *c, int64_t *dev_val, int64_t *host_out, int nv = 1);

// Status agreement at the end of a phase a rank can fail in ALONE: every rank enters with its own status; either all
// return NABO_OK or all return an error (a rank with a local error keeps its own code and message).  `args` (optional,
// n_args <= 3 values): what every rank must have been handed identically -- a mismatch is an error on every rank.
int agree(nabo_comm *c, int rc_local, const char *phase, const int64_t *args = nullptr, int n_args = 0);

}  // namespace nabo
#pragma GCC visibility pop

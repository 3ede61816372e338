// two_level_verdict.h -- whether an index's DATA takes the two-level stream (l2c_topk.hip): the remembered
// verdict and every rule that sets, asks or forgets it, in plain C++ so that the host compiles it without HIP
// (tests/test_two_level_verdict_cpu.py holds the rules against a restatement).
//
// On data without clusters the bounds of the first operand step reject nothing, the waves run the two-step loop anyway, and
// the bucket-ordered stream is the worst order for their lists (every row of a wave meets its neighbours at once: one broad
// Gaussian cloud, 1M x 1M: 119 ms per step against 89).  The kernel's own tile counters tell the two kinds of data apart.
// The verdict is a HEURISTIC, and it is remembered across set_ref / set_mask -- the usual caller refreshes the same kind of
// data --: a wrong "yes" is corrected by the next launch's counters, a wrong "no" costs the gain until the verdict expires.
// While the verdict is no, the queries stream the caller-order operands and the ordered copy of the references is not built.
#pragma once
#include <cstdint>

namespace nabo {

// repacks of the references a verdict outlives: the question is asked again now and then
constexpr int TL_VERDICT_REPACKS = 16;
// A PROBE decides an unknown verdict on long launches: the first TL_PROBE_WORKGROUPS workgroups (rows of the first buckets)
// over the first TL_PROBE_TILES tiles (the same buckets' references, own and foreign) -- a few hundred microseconds and one
// host wait.  Two or three buckets stand for all; only launches with several times that many workgroups and tiles are
// worth the question.
constexpr int TL_PROBE_WORKGROUPS = 128, TL_PROBE_TILES = 1024;
constexpr int64_t TL_PROBE_MIN_WORKGROUPS = 512, TL_PROBE_MIN_TILES = 4096;
// fewer than 30 % of the probe's tiles run one-step: the data does not take the stream (set on two kinds of data)
constexpr uint64_t TL_PROBE_ONE_STEP_NUM = 3, TL_PROBE_ONE_STEP_DEN = 10;
// A launch proper whose waves ran fewer than a quarter of their tiles one-step (one_step * 3 < two_step) paid the
// bucket-ordered stream for nothing; asked of queries of at least TL_LAUNCH_MIN_ROWS rows (the bound of the weak-bound
// memory, Refs::L2::coarse_weak) and only under option coarse_adapt
constexpr uint64_t TL_LAUNCH_TWO_STEP_RATIO = 3;
constexpr int64_t TL_LAUNCH_MIN_ROWS = 1024;

struct TwoLevelVerdict {
    enum State : int { NOT_KNOWN = 0, STREAMS = 1, CALLER_ORDER = 2 };
    State state = NOT_KNOWN;
    int age = 0;                     // repacks since the verdict was given
    bool known() const { return state != NOT_KNOWN; }
    bool streams() const { return state != CALLER_ORDER; }      // (not known: the stream is taken, a long query probes)
    void give(State s) { state = s; age = 0; }
    // the references were packed again: the verdict is forgotten at the TL_VERDICT_REPACKS-th repack after it was given
    void repack() { if (++age >= TL_VERDICT_REPACKS) give(NOT_KNOWN); }
};

// A probe is due: nothing is known, the option leaves the decision to the data (two_level = 1; 2 pins the stream), and the
// ordered main launch is long enough in workgroups and in reference tiles
inline bool tl_probe_due(const TwoLevelVerdict &v, int two_level_option, int64_t ordered_workgroups, int64_t ordered_tiles)
{
    return !v.known() && two_level_option == 1 && ordered_workgroups >= TL_PROBE_MIN_WORKGROUPS && ordered_tiles >= TL_PROBE_MIN_TILES;
}

// the verdict of a probe's tile counters (the count of refetched tiles takes no part)
inline TwoLevelVerdict::State tl_probe_verdict(uint64_t one_step, uint64_t two_step)
{
    return one_step * TL_PROBE_ONE_STEP_DEN < (one_step + two_step) * TL_PROBE_ONE_STEP_NUM ? TwoLevelVerdict::CALLER_ORDER : TwoLevelVerdict::STREAMS;
}

// the tile counters of a launch proper of a query of m rows say no (they never say yes: a verdict in force stays)
inline bool tl_launch_says_no(int64_t m, int coarse_adapt, uint64_t one_step, uint64_t two_step)
{
    return coarse_adapt != 0 && m >= TL_LAUNCH_MIN_ROWS && one_step * TL_LAUNCH_TWO_STEP_RATIO < two_step;
}

}  // namespace nabo

// The rules of the two-level stream's verdict (nabo_amd/csrc/two_level_verdict.h) compiled for the host, callable from
// tests/test_two_level_verdict_cpu.py.  A verdict crosses the boundary as its two ints: state[0] = state, state[1] = age.
#include "two_level_verdict.h"

using namespace nabo;

static TwoLevelVerdict load(const int *v)
{
    TwoLevelVerdict t;
    t.state = (TwoLevelVerdict::State)v[0];
    t.age = v[1];
    return t;
}
static void store(const TwoLevelVerdict &t, int *v)
{
    v[0] = (int)t.state;
    v[1] = t.age;
}

extern "C" void tl_constants_host(int64_t *out)
{
    const int64_t c[9] = {TL_VERDICT_REPACKS, TL_PROBE_WORKGROUPS, TL_PROBE_TILES, TL_PROBE_MIN_WORKGROUPS, TL_PROBE_MIN_TILES,
                          (int64_t)TL_PROBE_ONE_STEP_NUM, (int64_t)TL_PROBE_ONE_STEP_DEN, (int64_t)TL_LAUNCH_TWO_STEP_RATIO, TL_LAUNCH_MIN_ROWS};
    for (int i = 0; i < 9; ++i) out[i] = c[i];
}
extern "C" void tl_states_host(int *out)
{
    out[0] = TwoLevelVerdict::NOT_KNOWN;
    out[1] = TwoLevelVerdict::STREAMS;
    out[2] = TwoLevelVerdict::CALLER_ORDER;
}
extern "C" void tl_fresh_host(int *v) { store(TwoLevelVerdict(), v); }
extern "C" int tl_known_host(const int *v) { return load(v).known(); }
extern "C" int tl_streams_host(const int *v) { return load(v).streams(); }
extern "C" void tl_give_host(int *v, int state)
{
    TwoLevelVerdict t = load(v);
    t.give((TwoLevelVerdict::State)state);
    store(t, v);
}
extern "C" void tl_repack_host(int *v)
{
    TwoLevelVerdict t = load(v);
    t.repack();
    store(t, v);
}
extern "C" int tl_probe_due_host(const int *v, int two_level_option, int64_t ordered_workgroups, int64_t ordered_tiles)
{
    return tl_probe_due(load(v), two_level_option, ordered_workgroups, ordered_tiles);
}
extern "C" int tl_probe_verdict_host(uint64_t one_step, uint64_t two_step) { return (int)tl_probe_verdict(one_step, two_step); }
extern "C" int tl_launch_says_no_host(int64_t m, int coarse_adapt, uint64_t one_step, uint64_t two_step)
{
    return tl_launch_says_no(m, coarse_adapt, one_step, two_step);
}

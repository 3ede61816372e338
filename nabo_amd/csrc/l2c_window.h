// l2c_window.h -- the PROGRESS WINDOW of a workgroup in the two-level stream (l2c_topk.hip): the rule, in
// plain C++ so that the host compiles it too (tests/wave_window_host drives four threads through it as four waves).
//
// The four waves of a workgroup stream the same reference tiles, each for its own rows, and each asks L2 for every tile
// itself.  A tile stays in L2 for about the time a wave needs for eight tiles; waves that start together and drift apart by
// more than that all miss.  Kept within a few tiles of one another, the wave that runs ahead misses and the three behind
// it hit.  So every wave publishes the tile it is at in a slot of LDS (one int32 per wave, behind the lists), and every
// `check` tiles it reads all four: a wave more than `window` tiles ahead of the slowest LIVE wave sleeps until it is not.
//   * A wave's computation does not depend on when it runs: the window changes speed, never a result.
//   * The slowest wave never waits (its distance is 0), so somebody always moves.  Before any exit a wave publishes
//     L2C_WIN_DONE, which no minimum notices: a finished wave holds nobody back.
//   * Should a slot stop moving all the same, a wave gives up after L2C_WIN_POLLS polls of one wait and runs
//     unsynchronised for the rest of the launch (it keeps publishing: the others may still follow it).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define L2C_WIN_FN __host__ __device__ inline
#else
#define L2C_WIN_FN inline
#endif

namespace nabo {

constexpr int32_t L2C_WIN_DONE = INT32_MAX;      // a slot's value once its wave has left the stream
constexpr int L2C_WIN_SLOTS = 4;                 // waves per workgroup (geometry B)
constexpr int L2C_WIN_BYTES = 4 * L2C_WIN_SLOTS; // one broadcast ds_read_b128
constexpr int L2C_WIN_MAX = 4096;                // option "two_level_window": largest window, in tiles
constexpr int L2C_WIN_CHECK_MAX = 64;            // option "two_level_check": most tiles between two looks at the slots
constexpr int L2C_WIN_DEFAULT = 8;               // tiles (profiles/README.md, "wave window": the grid)
constexpr int L2C_WIN_CHECK_DEFAULT = 16;
// One poll is s_sleep L2C_WIN_SLEEP (64 cycles each) and one LDS read: >= 512 cycles, ~0.25 us at 2.1 GHz, about a one-step
// tile.  2^16 polls are >= 3.3e7 cycles, ~15 ms: a fifth of the headline launch, thousands of list drains (the longest
// thing a partner legitimately does between two tiles), and far below anything a watchdog would notice.
constexpr int L2C_WIN_SLEEP = 8;
constexpr int L2C_WIN_POLLS = 1 << 16;

enum L2cWinVerdict { L2C_WIN_GO = 0, L2C_WIN_WAIT = 1, L2C_WIN_GIVE_UP = 2 };

// option value -> tiles: < 0 off (0), 0 the default, otherwise 1 .. L2C_WIN_MAX
L2C_WIN_FN int l2c_win_window(int opt)
{
    return opt < 0 ? 0 : opt == 0 ? L2C_WIN_DEFAULT : opt > L2C_WIN_MAX ? L2C_WIN_MAX : opt;
}
// option value -> tiles between two checks: even (the loops run in pairs of tiles), 2 .. L2C_WIN_CHECK_MAX, 0 the default
L2C_WIN_FN int l2c_win_check(int opt)
{
    const int c = opt <= 0 ? L2C_WIN_CHECK_DEFAULT : opt > L2C_WIN_CHECK_MAX ? L2C_WIN_CHECK_MAX : opt;
    return (c + 1) & ~1;
}

// the slowest live wave: done slots are INT32_MAX; the caller's own slot is among the four, so the result is <= its tile
L2C_WIN_FN int32_t l2c_win_min(int32_t s0, int32_t s1, int32_t s2, int32_t s3)
{
    const int32_t a = s0 < s1 ? s0 : s1, b = s2 < s3 ? s2 : s3;
    return a < b ? a : b;
}

// A wave at tile t, the slowest live wave at tile `slowest`, `polls` polls into this wait (0: the first look).
L2C_WIN_FN L2cWinVerdict l2c_win_verdict(int32_t t, int32_t slowest, int window, int polls, int polls_max = L2C_WIN_POLLS)
{
    if (slowest >= t - window) return L2C_WIN_GO;       // (t - window: no overflow, both are tile counts; DONE passes)
    return polls >= polls_max ? L2C_WIN_GIVE_UP : L2C_WIN_WAIT;
}

}  // namespace nabo

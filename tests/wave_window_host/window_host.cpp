// Host build of the progress window's rule (nabo_amd/csrc/l2c_window.h) for tests/test_wave_window_cpu.py: four threads
// walk the tiles of one stream as the four waves of a workgroup do in l2c_topk.hip -- publish at the top of a pair of tiles,
// ask for the slots every `check` tiles, look at them behind the pair's first tile, sleep while too far ahead, publish
// L2C_WIN_DONE before leaving -- with seeded random delays per tile.  A program of its own (it also builds with
// -fsanitize=thread); one line of name=value pairs on stdout.
//     window_host WINDOW_OPT CHECK_OPT TILES SEED MODE POLLS_MAX
// MODE: 0 all four run; 1 wave 0 leaves at once (an all-padding wave); 2 waves 0..2 leave at once; 3 wave 1 stops
// publishing half way and does not move again until the others have ended (only the give-up bound releases them).
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>

#include "l2c_window.h"

using namespace nabo;

static std::atomic<int32_t> slot[L2C_WIN_SLOTS];
static std::atomic<int> arrived{0}, gave_up{0}, others_ended{0};
static int window, check, tiles, mode, polls_max;
static unsigned seed;

struct Result {
    bool ended = false;
    int32_t max_ahead = 0;          // largest (own tile - slowest live slot) seen at a publish while nobody had given up
    long waits = 0, polls = 0;
    bool gave_up = false;
};
static Result res[L2C_WIN_SLOTS];

static int32_t slowest()
{
    return l2c_win_min(slot[0].load(), slot[1].load(), slot[2].load(), slot[3].load());
}

static void tile_work(std::mt19937 &rng, int w)
{
    // a wave's pace: its own factor (the waves of a workgroup differ by their rows), now and then a long tile (a drain)
    const unsigned r = rng();
    unsigned spin = (r & 63u) * (unsigned)(1 + w);
    if ((r >> 8) % 97u == 0) spin += 4000u;
    volatile unsigned sink = 0;
    for (unsigned i = 0; i < spin; ++i) sink = sink + i;
    if ((r >> 20) % 257u == 0) std::this_thread::yield();
}

static void wave(int w)
{
    Result &R = res[w];
    std::mt19937 rng(seed * 4u + (unsigned)w);
    const bool dead = (mode == 1 && w == 0) || (mode == 2 && w < 3);
    // every slot is written before any wave polls: the barrier stands ahead of the early return
    slot[w].store(dead ? L2C_WIN_DONE : 0);
    arrived.fetch_add(1);
    while (arrived.load() < L2C_WIN_SLOTS) std::this_thread::yield();
    if (dead) {
        R.ended = true;
        return;
    }
    const bool staller = mode == 3 && w == 1;
    bool sync = window > 0;
    int next = 0;
    for (int t = 0; t < tiles; t += 2) {
        if (staller && t >= tiles / 2) {            // silent from here on, and still until the others are out
            while (others_ended.load() < L2C_WIN_SLOTS - 1) std::this_thread::yield();
            break;
        }
        slot[w].store(t);
        int32_t seen = 0;
        const bool due = sync && t >= next;
        if (due) seen = slowest();
        if (window > 0) {
            const int32_t ahead = t - slowest();
            if (gave_up.load() == 0 && ahead > R.max_ahead) R.max_ahead = ahead;
        }
        tile_work(rng, w);
        if (due) {
            next = t + check;
            bool waited = false;
            for (int polls = 0;; ++polls) {
                const L2cWinVerdict v = l2c_win_verdict(t, seen, window, polls, polls_max);
                if (v == L2C_WIN_GO) break;
                if (v == L2C_WIN_GIVE_UP) {
                    sync = false;
                    R.gave_up = true;
                    gave_up.fetch_add(1);
                    break;
                }
                waited = true;
                ++R.polls;
                std::this_thread::yield();
                seen = slowest();
            }
            R.waits += waited;
        }
        tile_work(rng, w);
    }
    slot[w].store(L2C_WIN_DONE);
    if (!staller) others_ended.fetch_add(1);
    R.ended = true;
}

int main(int argc, char **argv)
{
    if (argc != 7) return 2;
    window = l2c_win_window(atoi(argv[1]));
    check = l2c_win_check(atoi(argv[2]));
    tiles = atoi(argv[3]);
    seed = (unsigned)atoi(argv[4]);
    mode = atoi(argv[5]);
    polls_max = atoi(argv[6]);
    // the rule on its own: a finished wave is no minimum anybody waits for
    const bool done_passes = l2c_win_verdict(1 << 30, l2c_win_min(L2C_WIN_DONE, L2C_WIN_DONE, 1 << 30, L2C_WIN_DONE), 1, 0) == L2C_WIN_GO &&
                             l2c_win_verdict(100, l2c_win_min(L2C_WIN_DONE, 100, 98, L2C_WIN_DONE), 1, 0) == L2C_WIN_WAIT &&
                             l2c_win_verdict(100, 98, 1, L2C_WIN_POLLS) == L2C_WIN_GIVE_UP && l2c_win_verdict(100, 99, 1, L2C_WIN_POLLS) == L2C_WIN_GO;
    std::thread th[L2C_WIN_SLOTS];
    for (int w = 0; w < L2C_WIN_SLOTS; ++w) th[w] = std::thread(wave, w);
    for (auto &t : th) t.join();
    int ended = 0, ahead = 0, given = 0;
    long waits = 0, polls = 0;
    for (const Result &r : res) {
        ended += r.ended;
        ahead = r.max_ahead > ahead ? r.max_ahead : ahead;
        given += r.gave_up;
        waits += r.waits;
        polls += r.polls;
    }
    printf("window=%d check=%d ended=%d max_ahead=%d gave_up=%d waits=%ld polls=%ld done_passes=%d\n", window, check, ended, ahead,
           given, waits, polls, (int)done_passes);
    return 0;
}

// The layout rules of the local tournament seeds (nabo_amd/csrc/local_seeds.h) compiled for the host: what the layout
// kernel computes on the device, callable from tests/test_local_seeds_cpu.py.
#include "local_seeds.h"

using namespace nabo;

extern "C" void lseed_tournament_host(int lkeep, int T, int *pt, int *gt) { lseed_tournament(lkeep, T, pt, gt); }

extern "C" int64_t lseed_columns_host(int64_t rows, int C) { return lseed_columns(rows, C); }

// lay = base [C + 1] | padb [C + 1] | pade [C + 1]; ranges [n_cols][4] (query side only)
extern "C" void lseed_layout_host(int C, const uint32_t *ref_cnt, const uint32_t *row_cnt, int cap, int lkeep, int tile0,
                                  const int *rest, int64_t n_cols, int64_t *lay, int *ranges)
{
    lseed_layout(C, ref_cnt, row_cnt, cap, lkeep, tile0, lay, lay + (C + 1), lay + 2 * (C + 1));
    if (!row_cnt || !ranges) return;
    for (int64_t i = 0; i < 4 * n_cols; ++i) ranges[i] = 0;
    const LseedRange r = {rest[0], rest[1], rest[2], rest[3]};
    for (int b = 0; b <= C; ++b)
        lseed_fill_columns(b, C, ref_cnt, cap, lkeep, tile0, r, lay, lay + 2 * (C + 1), reinterpret_cast<LseedRange *>(ranges), n_cols);
}

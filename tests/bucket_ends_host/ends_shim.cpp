// Host build of the bucket-end table's rule (nabo_amd/csrc/local_seeds.h) for tests/test_bucket_ends_cpu.py: the layout of
// the full ordered copy and the ends the filter's mode control walks, as the device computes them.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "local_seeds.h"

extern "C" {

// ref_cnt [C] -> end [C]; returns the tiles the ordered stream runs over for `ref_tiles` reference tiles
int64_t lseed_bucket_ends_host(int C, const uint32_t *ref_cnt, int64_t ref_tiles, int32_t *end)
{
    std::vector<int64_t> lay(3 * (std::size_t)(C + 1));
    int64_t *base = lay.data(), *padb = base + (C + 1), *pade = padb + (C + 1);
    nabo::lseed_layout_full(C, ref_cnt, base, padb, pade);
    nabo::lseed_bucket_ends(C, pade, end);
    return nabo::lseed_ordered_tiles(ref_tiles, C);
}

}

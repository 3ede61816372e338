// The sub-order's key rule (nabo_amd/csrc/local_seeds.h) compiled for the host: the choice of sub-anchors, their ranking,
// the nearest sub-anchor and the positions inside the buckets, callable from tests/test_sub_order_cpu.py.
#include "local_seeds.h"

using namespace nabo;

extern "C" int lseed_sub_count_host(int option) { return lseed_sub_count(option); }
extern "C" int lseed_sub_default_host() { return LSEED_SUB_DEFAULT; }
extern "C" int lseed_sub_max_host() { return LSEED_MAX_SUB; }

extern "C" void lseed_sub_ranks_host(int S, int dim, const float *pts, int by_index, uint8_t *rank)
{
    lseed_sub_ranks(S, dim, pts, by_index != 0, rank);
}

extern "C" void lseed_sub_positions_host(int C, int S, int64_t n, int dim, const float *cells, const int32_t *bucket, int by_index,
                                         int64_t *pos)
{
    lseed_sub_positions(C, S, n, dim, cells, bucket, by_index != 0, pos);
}

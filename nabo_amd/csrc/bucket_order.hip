// bucket_order.hip -- the one sequence that sorts packed cells into bucket order (bucket_order.h), for the references' runs,
// their full ordered copy and a launch's rows alike: ensure_local_seeds (set_ref.hip) and local_seeds (query.hip) say what
// differs.  The only caller of the sort, layout and move launches of local_seeds.hip.
#include "index.h"
#include "local_seeds.h"

namespace nabo {

int bucket_sort(nabo_index *ix, const BucketSort &use)
{
    const IndexShape &sh = ix->shape;
    BucketRefs &refs = ix->ref.l2.buckets;
    BucketScratch &ws = ix->ws.buckets;
    hipStream_t st = ix->stream;
    const int C = refs.buckets, S = refs.sub_count, kc = use.kc;
    const bool two_level = ix->ref.l2.slots2;
    int rc;
    if ((rc = ws.keys.reserve(lseed_key_bytes(use.ncell))) || (rc = ws.block_counts.reserve(lseed_blockcnt_bytes(use.ncell, C))) ||
        (use.rows && (rc = ws.totals.reserve((size_t)C * sizeof(uint32_t)))) || (rc = ws.layout.reserve(lseed_layout_bytes(C))))
        return rc;
    uint32_t *key = ws.keys.as<uint32_t>(), *block = ws.block_counts.as<uint32_t>(), *ref_count = refs.bucket_count.as<uint32_t>();
    int64_t *lay = ws.layout.as<int64_t>();
    if (use.assign)
        HIP_TRY(lseed_sort_launch(kc, !use.rows, use.cells, use.ncell, sh.g, refs.anchors.p, C, key, block,
                                  use.rows ? ws.totals.as<uint32_t>() : ref_count, st, two_level));
    HIP_TRY(lseed_layout_launch(C, ref_count, use.rows ? ws.totals.as<uint32_t>() : nullptr, use.cap, use.lkeep, use.tile0, use.rest, lay,
                                use.column_ranges, use.columns, st));
    if (use.bucket_ends) HIP_TRY(lseed_ends_launch(C, lay, use.bucket_ends, st));
    // (every row is moved: the cap is the references' -- of a row's bucket only the run's length matters, to the layout)
    const int move_cap = use.rows ? 0 : use.cap;
    if (use.sub == BucketSort::CALLER_ORDER) {
        HIP_TRY(lseed_move_launch(kc, use.cells, use.ncell, key, block, C, lay, move_cap, use.pad_cell, use.dst, use.dst_map, st));
        return NABO_OK;
    }
    // The sub-order (local_seeds.h): the bucket-ordered copy goes to scratch first -- for the references its buckets in caller
    // order are where the sub-anchors are drawn from --, a second sort inside the buckets makes the copy the stream reads.
    const int64_t npos = use.positions;
    if ((rc = ws.unsorted_copy.reserve((size_t)(npos / 32) * kc * 1024 + 128)) || (rc = ws.unsorted_map.reserve((size_t)npos * sizeof(uint32_t))) ||
        (use.sub == BucketSort::BUILD_SUB_ANCHORS && (rc = ws.sub_floats.reserve(lseed_sub_float_bytes(kc, C, S)))) ||
        (rc = ws.sub_keys.reserve(lseed_key_bytes(npos))) || (rc = ws.sub_block_counts.reserve(lseed_blockcnt_bytes(npos, C * S))) ||
        (rc = ws.sub_totals.reserve((size_t)C * S * sizeof(uint32_t))) || (rc = ws.sub_layout.reserve((size_t)C * S * sizeof(int64_t))))
        return rc;
    unsigned char *copy1 = ws.unsorted_copy.as<unsigned char>();
    uint32_t *map1 = ws.unsorted_map.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(map1, 0xFF, (size_t)npos * sizeof(uint32_t), st));
    HIP_TRY(lseed_move_launch(kc, use.cells, use.ncell, key, block, C, lay, 0, use.pad_cell, copy1, map1, st));
    if (use.sub == BucketSort::BUILD_SUB_ANCHORS)
        HIP_TRY(lseed_sub_build_launch(kc, copy1, lay, ref_count, sh.g, C, S, refs.sub_rank_rule != 0, refs.sub_anchors.p,
                                       ws.sub_floats.as<float>(), refs.sub_ranks.as<uint8_t>(), refs.sub_norms.as<float>(), st, two_level));
    HIP_TRY(lseed_sub_sort_launch(kc, !use.rows, copy1, npos, map1, key, refs.sub_anchors.p, refs.sub_norms.as<float>(),
                                  refs.sub_ranks.as<uint8_t>(), ref_count, C, S, lay, ws.sub_keys.as<uint32_t>(),
                                  ws.sub_block_counts.as<uint32_t>(), ws.sub_totals.as<uint32_t>(), ws.sub_layout.as<int64_t>(), st));
    HIP_TRY(lseed_sub_move_launch(kc, copy1, npos, map1, ws.sub_keys.as<uint32_t>(), ws.sub_block_counts.as<uint32_t>(),
                                  ws.sub_layout.as<int64_t>(), use.cells, use.pad_cell, C, lay, use.dst, use.dst_map, st));
    return NABO_OK;
}

}  // namespace nabo

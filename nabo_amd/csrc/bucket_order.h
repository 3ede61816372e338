// bucket_order.h -- the bucket order of the one-product pass, host side: the state an index keeps of it and the ONE sequence
// that sorts cells into it (bucket_order.hip; the kernels: local_seeds.hip, the layout rules: local_seeds.h).
//
// The references are cut into buckets (nearest of C anchor cells).  Three copies are made in bucket order: the references'
// capped RUNS behind the one-product operands (the local tournament seeds), ALL references (the ordered copy the two-level
// stream reads, cells inside a bucket by sub-anchor), and a launch's ROWS (sorted by the same anchors and sub-anchors).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "host_common.h"

struct nabo_index;

namespace nabo {

// The REFERENCE side (nabo_index::Refs::L2): everything built from the references, by ensure_local_seeds for the index's
// options of the moment.  Stale after every repack (ensure_packed clears the two built flags); the queries read it.
struct BucketRefs {
    // anchors and the unmasked references per bucket; built for `buckets` anchors and `cap` references kept per run
    DevBuf anchors, bucket_count;
    int buckets = 0, cap = 0;
    // the runs live BEHIND the one-product operands in ycpk1, from tile ref_tiles_alloc on (runs_room tiles, set when the
    // operands are packed: one address space for l2c_pre_kernel's tile ranges)
    int64_t runs_room = 0;
    bool runs_built = false;
    // the ordered copy: ALL unmasked references in bucket order, ordered_tiles tiles and two all-padding tiles behind them;
    // ordered_map [position] = reference index (0xFFFFFFFF: a padding cell); bucket_ends [buckets] (int32): the buckets'
    // ends in tiles of the copy (lseed_bucket_ends), the mode control's table -- kept apart because the layout it is taken
    // from is scratch, and the queries' sorts overwrite it.  Not built while the verdict is no (two_level_verdict.h).
    DevBuf ordered, ordered_map, bucket_ends;
    int64_t ordered_tiles = 0;
    bool ordered_built = false;
    // the sub-order of the ordered copy (local_seeds.h): built for sub_count sub-anchors per bucket (1: none) ranked by rule
    // sub_rank_rule; their component slots [buckets][sub_count] as chunks, their norms and ranks -- the queries sort their
    // rows with the same tables
    DevBuf sub_anchors, sub_norms, sub_ranks;
    int sub_count = 1, sub_rank_rule = 0;
    // what a workgroup of the ordered main launch skips by (bucket_skip.h), built behind the ordered copy and with it:
    // the groups of the stream -- sub-bucket r of bucket b is group b * sub_count + r -- as first position, size and tiles
    // [skip_groups] int32 each; the buckets' means [buckets][g] and the unit directions between them, by_from [b][g][b'] and
    // by_to [b'][g][b], float64; ymin [buckets][skip_groups] floats
    DevBuf skip_first, skip_count, skip_t0, skip_t1, skip_mean_parts, skip_means, skip_by_from, skip_by_to, skip_ymin;
    int skip_groups = 0;
    bool skip_built = false;
};

// The SCRATCH side (nabo_index::Workspace).  The reference build and the queries use the SAME scratch, on the same stream:
// a sort's keys, block counts and layout are dead once its last move is enqueued -- except that the references' full copy
// is laid out from the keys and block counts their runs were sorted with (BucketSort::assign).
struct BucketScratch {
    DevBuf keys, block_counts, totals, layout;                 // the counting sort by bucket (totals: of a launch's rows)
    DevBuf unsorted_copy, unsorted_map;                        // the sub-order: the bucket-ordered copy before it, and its map
    DevBuf sub_keys, sub_block_counts, sub_totals, sub_layout;  // ... the second sort, by (bucket, sub-rank)
    DevBuf sub_floats;                                         // ... the sub-anchors as floats (scratch of their ranking)
    // What the sort of a launch's rows HANDS OVER to the filter launches behind it (query.hip: local_seeds writes, the
    // tournament, the probe and the ordered main launch read; nabo_index_stream_order reads the map afterwards):
    struct Rows {
        DevBuf ordered, map, column_ranges;      // the bucket-ordered target tiles, [position] = row, the columns' tile ranges
        DevBuf tile_counters;                    // the two-level launch's tile counters [4] (l2c_topk.hip)
        DevBuf runs;                             // the run lists of the main launch's workgroups (bucket_skip.h), where it skips
        bool streamed = false;                   // the last first pass ran the ordered main launch ...
        int64_t positions = 0;                   // ... over this many positions of `ordered`
    } rows;
};

// One use of bucket_sort: what differs between the references' runs, their full copy and a launch's rows.
struct BucketSort {
    // the cells are a launch's rows: assigned to the references' anchors, counted in BucketScratch::totals, laid out in whole
    // columns behind their buckets' runs.  false: the references -- counted in BucketRefs::bucket_count, fixed slots
    bool rows = false;
    // false: the keys and block counts of the sort before stand (the references' full copy follows their runs)
    bool assign = true;
    int kc = 0;                                  // operand steps of the packed cells
    const unsigned char *cells = nullptr;        // the packed cells in caller order ...
    int64_t ncell = 0;
    int64_t pad_cell = 0;                        // ... and the cell among them that padding positions copy
    int cap = 0;                                 // references kept per bucket (0: all -- the full copy, buckets in whole tiles)
    // rows only: kept list entries, first tile of the runs, the stream-prefix tournament of the rest class, the columns' ranges
    int lkeep = 1, tile0 = 0, rest[4] = {0, 0, 0, 0};
    int *column_ranges = nullptr;
    int64_t columns = 0;
    int32_t *bucket_ends = nullptr;              // where the buckets' ends in tiles are kept (null: not wanted)
    // the order inside a bucket: caller order, by the references' sub-anchors, or by sub-anchors that this sort draws from
    // its own bucket-ordered cells first (the references' full copy)
    enum Sub { CALLER_ORDER, USE_SUB_ANCHORS, BUILD_SUB_ANCHORS } sub = CALLER_ORDER;
    int64_t positions = 0;                       // positions of the destination the sub-order sorts (whole tiles)
    unsigned char *dst = nullptr;                // the bucket-ordered copy, and [position] = cell (null: no map; the caller
    uint32_t *dst_map = nullptr;                 //   fills the map with 0xFFFFFFFF, and whatever no bucket reaches of dst)
};

// bucket_order.hip: sort into buckets -> layout -> optional sub-order -> move to the destination with its map, enqueued on
// the index's stream.  Reserves the scratch it needs; the reference side's tables are the caller's to reserve.
int bucket_sort(nabo_index *ix, const BucketSort &use);

}  // namespace nabo

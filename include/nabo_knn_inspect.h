/* nabo_knn_inspect.h -- a look into an index of include/nabo_knn.h, for tests and tools: nothing a caller of the k-NN needs. */
#ifndef NABO_KNN_INSPECT_H
#define NABO_KNN_INSPECT_H

#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The order the two-level stream of the one-product pass read its two sides in, as of the last query that took it
 * (NABO_E_INVALID if the last query did not).  row_map [*n_row_pos]: the target row at every position of the bucket-ordered
 * copy of the targets, 0xFFFFFFFF for a padding position; ref_map [*n_ref_pos]: the reference at every position of the
 * ordered copy of the references, likewise.  Either array may be NULL: the call then returns the two lengths only.  Waits
 * for the index's stream. */
int nabo_index_stream_order(nabo_index *ix, uint32_t *row_map, int64_t *n_row_pos, uint32_t *ref_map, int64_t *n_ref_pos);

#ifdef __cplusplus
}
#endif
#endif

/* include/nabo_umap_transform.h through a plain C99 compiler, linked against libnabo_knn.so: takes the address of every
 * entry point, prints how many there are, and checks that bad arguments are refused before any device is touched. */
#include <stdio.h>

#include "nabo_umap_transform.h"

int main(void)
{
    void *fns[] = {(void *)nabo_umap_transform_create,        (void *)nabo_umap_transform_destroy,
                   (void *)nabo_umap_transform_set_params,    (void *)nabo_umap_transform_set_embedding,
                   (void *)nabo_umap_transform_set_cells,     (void *)nabo_umap_transform_query,
                   (void *)nabo_umap_transform_set_knn,       (void *)nabo_umap_transform_set_graph,
                   (void *)nabo_umap_transform_get_graph,     (void *)nabo_umap_transform_set_positions,
                   (void *)nabo_umap_transform_get_positions, (void *)nabo_umap_transform_run,
                   (void *)nabo_umap_transform_rewind,        (void *)nabo_umap_transform_last_run_counts,
                   (void *)nabo_umap_transform_last_ms,       (void *)nabo_umap_transform_geometry};
    int n = 0;
    for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) n += fns[i] != NULL;
    nabo_umap_transform *T = NULL;
    int32_t group = 0;
    /* one reference cell */
    int rc = nabo_umap_transform_create(&T, 0, 1, 2);
    /* four dimensions */
    int rc2 = nabo_umap_transform_create(&T, 0, 100, 4);
    /* no handle */
    int rc3 = nabo_umap_transform_set_params(NULL, 100, 5, 1.0, 1.5, 0.9, 0);
    int rc4 = nabo_umap_transform_run(NULL, 1, NULL);
    int rc5 = nabo_umap_transform_geometry(&group);
    printf("%d entry points; 1 reference cell -> %d, 4 dims -> %d, no handle -> %d %d (%s); %d lanes per target\n", n, rc, rc2, rc3,
           rc4, nabo_last_error(), (int)group);
    return rc == NABO_E_INVALID && rc2 == NABO_E_INVALID && rc3 == NABO_E_INVALID && rc4 == NABO_E_INVALID && rc5 == NABO_OK &&
                   T == NULL && group >= 1 && group <= 64
               ? 0
               : 1;
}

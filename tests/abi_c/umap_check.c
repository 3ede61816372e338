/* include/nabo_umap.h through a plain C99 compiler, linked against libnabo_knn.so: takes the address of every entry
 * point, prints how many there are, and checks that bad arguments are refused before any device is touched. */
#include <stdio.h>

#include "nabo_umap.h"

int main(void)
{
    void *fns[] = {(void *)nabo_umap_create,        (void *)nabo_umap_destroy,       (void *)nabo_umap_set_params,
                   (void *)nabo_umap_set_knn,       (void *)nabo_umap_fit_knn,       (void *)nabo_umap_graph_size,
                   (void *)nabo_umap_get_graph,     (void *)nabo_umap_set_embedding, (void *)nabo_umap_get_embedding,
                   (void *)nabo_umap_run,           (void *)nabo_umap_rewind,        (void *)nabo_umap_last_epoch_counts,
                   (void *)nabo_umap_last_ms,       (void *)nabo_umap_geometry,      (void *)nabo_umap_set_graph};
    int n = 0;
    for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) n += fns[i] != NULL;
    nabo_umap *U = NULL;
    int32_t group = 0;
    /* two cells */
    int rc = nabo_umap_create(&U, 0, 2, 2);
    /* four dimensions */
    int rc2 = nabo_umap_create(&U, 0, 100, 4);
    /* no handle */
    int rc3 = nabo_umap_set_params(NULL, 200, 5, 1.0, 1.5, 0.9, 0);
    int rc4 = nabo_umap_run(NULL, 1, NULL);
    int rc5 = nabo_umap_geometry(&group);
    printf("%d entry points; 2 cells -> %d, 4 dims -> %d, no handle -> %d %d (%s); %d lanes per node\n", n, rc, rc2, rc3, rc4,
           nabo_last_error(), (int)group);
    return rc == NABO_E_INVALID && rc2 == NABO_E_INVALID && rc3 == NABO_E_INVALID && rc4 == NABO_E_INVALID && rc5 == NABO_OK &&
                   U == NULL && group >= 1 && group <= 64
               ? 0
               : 1;
}

/* include/nabo_community.h through a plain C99 compiler, linked against libnabo_knn.so: takes the address of every entry
 * point, prints how many there are, and checks that bad arguments are refused before any device is touched. */
#include <stdio.h>

#include "nabo_community.h"

int main(void)
{
    void *fns[] = {(void *)nabo_community_create,     (void *)nabo_community_destroy,   (void *)nabo_community_set_params,
                   (void *)nabo_community_run,        (void *)nabo_community_labels,    (void *)nabo_community_history,
                   (void *)nabo_community_modularity, (void *)nabo_community_split,     (void *)nabo_community_level_size,
                   (void *)nabo_community_get_level,  (void *)nabo_community_set_comm,  (void *)nabo_community_get_comm,
                   (void *)nabo_community_sweep,      (void *)nabo_community_aggregate, (void *)nabo_community_rewind,
                   (void *)nabo_community_last_ms,    (void *)nabo_community_geometry};
    int n = 0;
    for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) n += fns[i] != NULL;
    nabo_community *H = NULL;
    const int64_t ptr[3] = {0, 1, 2}, nbr[2] = {1, 0}, bad_nbr[2] = {1, 2};
    const double w[2] = {0.5, 0.5}, neg[2] = {0.5, -0.5};
    int32_t group = 0, thr = 0, cap = 0;
    /* no node */
    int rc = nabo_community_create(&H, 0, 0, ptr, nbr, w, 10000.0);
    /* a neighbour that is no node, a negative weight, a scale of zero */
    int rc2 = nabo_community_create(&H, 0, 2, ptr, bad_nbr, w, 10000.0);
    int rc3 = nabo_community_create(&H, 0, 2, ptr, nbr, neg, 10000.0);
    int rc4 = nabo_community_create(&H, 0, 2, ptr, nbr, w, 0.0);
    /* no handle */
    int rc5 = nabo_community_run(NULL);
    int rc6 = nabo_community_sweep(NULL, 0, 0, NULL, NULL);
    int rc7 = nabo_community_geometry(&group, &thr, &cap);
    printf("%d entry points; no node -> %d, bad graph -> %d %d %d, no handle -> %d %d (%s); %d lanes per row, long above %d, table of %d\n",
           n, rc, rc2, rc3, rc4, rc5, rc6, nabo_last_error(), (int)group, (int)thr, (int)cap);
    return rc == NABO_E_INVALID && rc2 == NABO_E_INVALID && rc3 == NABO_E_INVALID && rc4 == NABO_E_INVALID &&
                   rc5 == NABO_E_INVALID && rc6 == NABO_E_INVALID && rc7 == NABO_OK && H == NULL && group >= 1 && group <= 64 &&
                   thr >= group && cap > thr
               ? 0
               : 1;
}

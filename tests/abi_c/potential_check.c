/* include/nabo_potential.h through a plain C99 compiler, linked against libnabo_knn.so: takes the address of every entry
 * point, prints how many there are, and checks that bad arguments are refused before any device is touched. */
#include <stdio.h>

#include "nabo_potential.h"

int main(void)
{
    void *fns[] = {(void *)nabo_potential_create,    (void *)nabo_potential_destroy,      (void *)nabo_potential_set_params,
                   (void *)nabo_potential_graph_size, (void *)nabo_potential_prepare,     (void *)nabo_potential_get_prepared,
                   (void *)nabo_potential_iterate,   (void *)nabo_potential_get_state,    (void *)nabo_potential_set_state,
                   (void *)nabo_potential_finish,    (void *)nabo_potential_solve,        (void *)nabo_potential_info,
                   (void *)nabo_potential_last_ms,   (void *)nabo_potential_geometry};
    int n = 0;
    for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) n += fns[i] != NULL;
    nabo_potential *H = NULL;
    const int64_t ptr[4] = {0, 1, 2, 2}, nbr[2] = {1, 0}, bad_nbr[2] = {1, 3};
    int32_t group = 0, thr = 0, rows = 0, done = 0;
    double V[3];
    /* no node */
    int rc = nabo_potential_create(&H, 0, 0, ptr, nbr);
    /* a neighbour that is no node; node 2 has no edge */
    int rc2 = nabo_potential_create(&H, 0, 2, ptr, bad_nbr);
    int rc3 = nabo_potential_create(&H, 0, 3, ptr, nbr);
    /* no handle */
    int rc4 = nabo_potential_solve(NULL, NULL, V);
    int rc5 = nabo_potential_iterate(NULL, 1, &done);
    int rc6 = nabo_potential_set_params(NULL, 1e-10, 10);
    int rc7 = nabo_potential_geometry(&group, &thr, &rows);
    printf("%d entry points; no node -> %d, bad graph -> %d %d, no handle -> %d %d %d (%s); %d lanes per row, long above %d, %d rows per workgroup\n",
           n, rc, rc2, rc3, rc4, rc5, rc6, nabo_last_error(), (int)group, (int)thr, (int)rows);
    return rc == NABO_E_INVALID && rc2 == NABO_E_INVALID && rc3 == NABO_E_INVALID && rc4 == NABO_E_INVALID && rc5 == NABO_E_INVALID &&
                   rc6 == NABO_E_INVALID && rc7 == NABO_OK && H == NULL && group >= 1 && group <= 64 && thr >= group && rows >= 256 &&
                   NABO_POTENTIAL_CONVERGED == 1
               ? 0
               : 1;
}

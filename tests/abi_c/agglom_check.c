/* include/nabo_agglom.h through a plain C99 compiler, linked against libnabo_knn.so: takes the address of every entry
 * point, prints how many there are, and checks that a missing handle is refused before any device is touched. */
#include <stdio.h>

#include "nabo_agglom.h"

int main(void)
{
    void *fns[] = {(void *)nabo_community_agglomerate, (void *)nabo_community_dendrogram, (void *)nabo_community_agglom_info,
                   (void *)nabo_community_cut,         (void *)nabo_community_match_pass, (void *)nabo_community_match,
                   (void *)nabo_community_agglom_ms};
    int n = 0;
    for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) n += fns[i] != NULL;
    int64_t m = 0, info[4];
    double ms[4];
    int rc = nabo_community_agglomerate(NULL, 1);
    int rc2 = nabo_community_dendrogram(NULL, &m, 0, NULL, NULL);
    int rc3 = nabo_community_agglom_info(NULL, info);
    int rc4 = nabo_community_cut(NULL, 0, NULL, NULL, NULL);
    int rc5 = nabo_community_match_pass(NULL, NULL, NULL, NULL, NULL);
    int rc6 = nabo_community_match(NULL, NULL, NULL, NULL);
    int rc7 = nabo_community_agglom_ms(NULL, ms);
    printf("%d entry points; no handle -> %d %d %d %d %d %d %d (%s)\n", n, rc, rc2, rc3, rc4, rc5, rc6, rc7, nabo_last_error());
    return rc == NABO_E_INVALID && rc2 == NABO_E_INVALID && rc3 == NABO_E_INVALID && rc4 == NABO_E_INVALID && rc5 == NABO_E_INVALID &&
                   rc6 == NABO_E_INVALID && rc7 == NABO_E_INVALID
               ? 0
               : 1;
}

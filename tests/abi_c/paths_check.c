/* include/nabo_graph.h through a plain C99 compiler, linked against libnabo_knn.so: takes the address of every
 * entry point and prints how many there are. */
#include <stdio.h>

#include "nabo_graph.h"
#include "nabo_knn.h"

int main(void)
{
    void *fns[] = {
        (void *)nabo_refgraph_create, (void *)nabo_refgraph_destroy, (void *)nabo_refgraph_set_option,
        (void *)nabo_refgraph_group_hops, (void *)nabo_refgraph_last_stats, (void *)nabo_refgraph_last_local_nodes,
    };
    int n = 0;
    for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) n += fns[i] != NULL;
    nabo_refgraph *g = NULL;
    const int64_t ptr[2] = {1, 0};
    int rc = nabo_refgraph_create(&g, 0, 1, ptr, NULL);     /* ptr[0] != 0: refused before any device is touched */
    printf("%d entry points; bad CSR -> %d (%s)\n", n, rc, nabo_last_error());
    return rc == NABO_E_INVALID && g == NULL ? 0 : 1;
}

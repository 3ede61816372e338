/* include/nabo_cluster.h through a plain C99 compiler, linked against libnabo_knn.so: takes the address of every
 * entry point, prints how many there are, and checks that bad arguments are refused before any device is touched.
 * `cluster_check run` also classifies the rows of the tests' hand-built graph on the device and prints the answers:
 *     cluster_check run < rows        (n_ref n_clusters n_targets weight_frac min_degree min_weight,
 *                                      ref_cluster[n_ref], ptr[n_targets + 1], then nbr w per edge) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nabo_cluster.h"
#include "nabo_knn.h"

static int run(void)
{
    long long n_ref, n_targets, min_degree;
    int n_clusters;
    double weight_frac, min_weight;
    if (scanf("%lld %d %lld %lf %lld %lf", &n_ref, &n_clusters, &n_targets, &weight_frac, &min_degree, &min_weight) != 6) return 2;
    int32_t *rc = malloc(sizeof(int32_t) * (size_t)(n_ref + 1));
    int64_t *ptr = malloc(sizeof(int64_t) * (size_t)(n_targets + 1));
    for (long long i = 0; i < n_ref; ++i) {
        int v;
        if (scanf("%d", &v) != 1) return 2;
        rc[i] = v;
    }
    for (long long i = 0; i <= n_targets; ++i) {
        long long v;
        if (scanf("%lld", &v) != 1) return 2;
        ptr[i] = v;
    }
    const long long E = ptr[n_targets];
    int64_t *nbr = malloc(sizeof(int64_t) * (size_t)(E + 1));
    double *w = malloc(sizeof(double) * (size_t)(E + 1));
    for (long long e = 0; e < E; ++e) {
        long long v;
        if (scanf("%lld %lf", &v, &w[e]) != 2) return 2;
        nbr[e] = v;
    }
    int32_t *label = malloc(sizeof(int32_t) * (size_t)(n_targets + 1));
    double *best = malloc(sizeof(double) * (size_t)(n_targets + 1)), *total = malloc(sizeof(double) * (size_t)(n_targets + 1));
    int64_t *counts = malloc(sizeof(int64_t) * (size_t)(n_clusters + 1));
    int st = nabo_classify_targets(0, n_ref, rc, n_clusters, n_targets, ptr, nbr, w, weight_frac, min_degree, min_weight, label,
                                   best, total, counts);
    if (st != NABO_OK) {
        printf("error %d: %s\n", st, nabo_last_error());
        return 1;
    }
    for (long long i = 0; i < n_targets; ++i) printf("row %lld %d %.17g %.17g\n", i, (int)label[i], best[i], total[i]);
    for (int c = 0; c <= n_clusters; ++c) printf("count %d %lld\n", c, (long long)counts[c]);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "run")) return run();
    void *fns[] = {(void *)nabo_classify_targets, (void *)nabo_refgraph_set_levels, (void *)nabo_cluster_last_device_ms};
    int n = 0;
    for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) n += fns[i] != NULL;
    const int64_t ptr[2] = {1, 0};
    int32_t label[1];
    int rc = nabo_classify_targets(0, 0, NULL, 1, 1, ptr, NULL, NULL, 0.5, 2, 0.1, label, NULL, NULL, NULL); /* ptr[0] != 0 */
    int rc2 = nabo_refgraph_set_levels(NULL, 0, ptr, NULL, -1, NULL);                                          /* no graph */
    printf("%d entry points; bad rows -> %d, no graph -> %d (%s)\n", n, rc, rc2, nabo_last_error());
    return rc == NABO_E_INVALID && rc2 == NABO_E_INVALID ? 0 : 1;
}

/* include/nabo_de.h through a plain C99 compiler, linked against libnabo_knn.so: takes the address of every entry
 * point, prints how many there are, and checks that bad arguments are refused before any device is touched.
 * `de_check run` also tests the genes of a small matrix on the device and prints the per-pair answers:
 *     de_check run < input     (n_genes n_cells n_sets exp_frac_thresh log2_fc_thresh, gene_ptr[n_genes + 1],
 *                               then cell val per nonzero, sf[n_cells], set_ptr[n_sets + 1], members) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nabo_de.h"

static int run(void)
{
    long long n_genes, n_cells, n_sets, v;
    double ef, lfc;
    if (scanf("%lld %lld %lld %lf %lf", &n_genes, &n_cells, &n_sets, &ef, &lfc) != 5) return 2;
    int64_t *gene_ptr = malloc(sizeof(int64_t) * (size_t)(n_genes + 1));
    for (long long i = 0; i <= n_genes; ++i) {
        if (scanf("%lld", &v) != 1) return 2;
        gene_ptr[i] = v;
    }
    const long long nnz = gene_ptr[n_genes];
    int32_t *cell = malloc(sizeof(int32_t) * (size_t)(nnz + 1));
    float *val = malloc(sizeof(float) * (size_t)(nnz + 1)), *sf = malloc(sizeof(float) * (size_t)(n_cells + 1));
    for (long long e = 0; e < nnz; ++e) {
        if (scanf("%lld %f", &v, &val[e]) != 2) return 2;
        cell[e] = (int32_t)v;
    }
    for (long long i = 0; i < n_cells; ++i)
        if (scanf("%f", &sf[i]) != 1) return 2;
    int64_t *set_ptr = malloc(sizeof(int64_t) * (size_t)(n_sets + 1));
    for (long long i = 0; i <= n_sets; ++i) {
        if (scanf("%lld", &v) != 1) return 2;
        set_ptr[i] = v;
    }
    int64_t *members = malloc(sizeof(int64_t) * (size_t)(set_ptr[n_sets] + 1));
    for (long long i = 0; i < set_ptr[n_sets]; ++i) {
        if (scanf("%lld", &v) != 1) return 2;
        members[i] = v;
    }
    const size_t n_out = (size_t)(n_genes * (n_sets - 1)) + 1;
    int32_t *status = malloc(sizeof(int32_t) * n_out);
    int64_t *i64 = malloc(sizeof(int64_t) * n_out * 5);
    double *f64 = malloc(sizeof(double) * n_out * 4);
    int st = nabo_de_test(0, n_genes, n_cells, gene_ptr, cell, val, sf, 0, NULL, NULL, NULL, NULL, n_sets, set_ptr, members, 0, NULL,
                          NULL, ef, lfc, 0, status, i64, i64 + n_out, i64 + 2 * n_out, i64 + 3 * n_out, i64 + 4 * n_out, f64,
                          f64 + n_out, f64 + 2 * n_out, f64 + 3 * n_out);
    if (st != NABO_OK) {
        printf("error %d: %s\n", st, nabo_last_error());
        return 1;
    }
    for (size_t i = 0; i + 1 < n_out; ++i)
        printf("pair %zu %d %lld %lld %lld %lld %lld %.17g %.17g %.17g %.17g\n", i, (int)status[i], (long long)i64[i],
               (long long)i64[n_out + i], (long long)i64[2 * n_out + i], (long long)i64[3 * n_out + i], (long long)i64[4 * n_out + i],
               f64[i], f64[n_out + i], f64[2 * n_out + i], f64[3 * n_out + i]);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "run")) return run();
    void *fns[] = {(void *)nabo_de_test, (void *)nabo_de_last_device_ms};
    int n = 0;
    for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) n += fns[i] != NULL;
    const int64_t gene_ptr[2] = {0, 0}, bad_ptr[2] = {1, 0}, set_ptr[3] = {0, 0, 0};
    int32_t status[1];
    int64_t i64[5];
    double f64[4];
    /* the test set is empty */
    int rc = nabo_de_test(0, 1, 0, gene_ptr, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL, 2, set_ptr, NULL, 0, NULL, NULL, 0.25, 1.0, 0,
                          status, i64, i64 + 1, i64 + 2, i64 + 3, i64 + 4, f64, f64 + 1, f64 + 2, f64 + 3);
    /* gene_ptr[0] != 0 */
    int rc2 = nabo_de_test(0, 1, 0, bad_ptr, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL, 2, set_ptr, NULL, 0, NULL, NULL, 0.25, 1.0, 0,
                           status, i64, i64 + 1, i64 + 2, i64 + 3, i64 + 4, f64, f64 + 1, f64 + 2, f64 + 3);
    printf("%d entry points; empty test set -> %d, bad gene_ptr -> %d (%s)\n", n, rc, rc2, nabo_last_error());
    return rc == NABO_E_INVALID && rc2 == NABO_E_INVALID && nabo_de_last_device_ms(NULL, NULL) == NABO_E_INVALID ? 0 : 1;
}

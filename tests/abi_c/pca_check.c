/* include/nabo_pca.h through a plain C99 compiler, linked against libnabo_knn.so: takes the address of every entry
 * point, prints how many there are, and checks that bad arguments are refused before any device is touched.
 * `pca_check run` also projects the rows of a small matrix on the device and prints Z:
 *     pca_check run < input     (n_cells n_raw_genes G C n_rows, cell_ptr[n_cells + 1], then gene val per entry,
 *                               sf[n_cells], gene_pos[n_raw_genes], mu[G], sigma[G], mean[G], components[C * G],
 *                               rows[n_rows]) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nabo_pca.h"

static int read_doubles(double *a, long long n)
{
    for (long long i = 0; i < n; ++i)
        if (scanf("%lf", &a[i]) != 1) return 1;
    return 0;
}

static int run(void)
{
    long long n_cells, n_raw, G, C, n_rows, v;
    if (scanf("%lld %lld %lld %lld %lld", &n_cells, &n_raw, &G, &C, &n_rows) != 5) return 2;
    int64_t *cell_ptr = malloc(sizeof(int64_t) * (size_t)(n_cells + 1));
    for (long long i = 0; i <= n_cells; ++i) {
        if (scanf("%lld", &v) != 1) return 2;
        cell_ptr[i] = v;
    }
    const long long nnz = cell_ptr[n_cells];
    int32_t *gene = malloc(sizeof(int32_t) * (size_t)(nnz + 1)), *gene_pos = malloc(sizeof(int32_t) * (size_t)(n_raw + 1));
    float *val = malloc(sizeof(float) * (size_t)(nnz + 1)), *sf = malloc(sizeof(float) * (size_t)(n_cells + 1));
    for (long long e = 0; e < nnz; ++e) {
        if (scanf("%lld %f", &v, &val[e]) != 2) return 2;
        gene[e] = (int32_t)v;
    }
    for (long long i = 0; i < n_cells; ++i)
        if (scanf("%f", &sf[i]) != 1) return 2;
    for (long long i = 0; i < n_raw; ++i) {
        if (scanf("%lld", &v) != 1) return 2;
        gene_pos[i] = (int32_t)v;
    }
    double *mu = malloc(sizeof(double) * (size_t)(3 * G + C * G)), *sigma = mu + G, *mean = mu + 2 * G, *comp = mu + 3 * G;
    if (read_doubles(mu, 3 * G + C * G)) return 2;
    int64_t *rows = malloc(sizeof(int64_t) * (size_t)(n_rows + 1));
    for (long long i = 0; i < n_rows; ++i) {
        if (scanf("%lld", &v) != 1) return 2;
        rows[i] = v;
    }
    double *Z = malloc(sizeof(double) * (size_t)(n_rows * C + 1));
    int st = nabo_pca_project(0, n_cells, n_raw, cell_ptr, gene, val, sf, gene_pos, G, mu, sigma, mean, (int32_t)C, comp, n_rows, rows, 0, Z);
    if (st != NABO_OK) {
        printf("error %d: %s\n", st, nabo_last_error());
        return 1;
    }
    for (long long r = 0; r < n_rows; ++r) {
        printf("row %lld", r);
        for (long long c = 0; c < C; ++c) printf(" %.17g", Z[r * C + c]);
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "run")) return run();
    void *fns[] = {(void *)nabo_pca_project, (void *)nabo_gene_stats, (void *)nabo_pca_last_device_ms};
    int n = 0;
    for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) n += fns[i] != NULL;
    const int64_t ptr[2] = {0, 1}, bad_ptr[2] = {1, 1};
    const int32_t gene[1] = {0}, pos[1] = {0};
    const float val[1] = {1.0f}, sf[1] = {1.0f};
    const double mu[1] = {0.0}, sigma[1] = {1.0}, zero[1] = {0.0}, comp[1] = {1.0};
    double z[1];
    int64_t nc[1];
    uint8_t valid[1];
    /* sigma = 0 */
    int rc = nabo_pca_project(0, 1, 1, ptr, gene, val, sf, pos, 1, mu, zero, zero, 1, comp, 0, NULL, 0, z);
    /* cell_ptr[0] != 0 */
    int rc2 = nabo_pca_project(0, 1, 1, bad_ptr, gene, val, sf, pos, 1, mu, sigma, zero, 1, comp, 0, NULL, 0, z);
    /* gene_ptr[0] != 0 */
    int rc3 = nabo_gene_stats(0, 1, 1, bad_ptr, gene, val, sf, 0, NULL, NULL, nc, valid, z, z, z);
    printf("%d entry points; sigma 0 -> %d, bad cell_ptr -> %d, bad gene_ptr -> %d (%s)\n", n, rc, rc2, rc3, nabo_last_error());
    return rc == NABO_E_INVALID && rc2 == NABO_E_INVALID && rc3 == NABO_E_INVALID && nabo_pca_last_device_ms(NULL, NULL) == NABO_E_INVALID ? 0 : 1;
}

/* include/nabo_qc.h through a plain C99 compiler, linked against libnabo_knn.so: takes the address of every entry point,
 * prints how many there are, and checks that bad arguments are refused before any device is touched.
 * `qc_check run` also sums the rows of a small matrix on the device and prints them:
 *     qc_check run < input      (n_cells n_raw_genes n_classes n_rows, cell_ptr[n_cells + 1], then gene val per entry,
 *                               gene_class[n_raw_genes], rows[n_rows]) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nabo_qc.h"

static int run(void)
{
    long long n_cells, n_raw, n_classes, n_rows, v;
    if (scanf("%lld %lld %lld %lld", &n_cells, &n_raw, &n_classes, &n_rows) != 4) return 2;
    int64_t *cell_ptr = malloc(sizeof(int64_t) * (size_t)(n_cells + 1));
    for (long long i = 0; i <= n_cells; ++i) {
        if (scanf("%lld", &v) != 1) return 2;
        cell_ptr[i] = v;
    }
    const long long nnz = cell_ptr[n_cells];
    int32_t *gene = malloc(sizeof(int32_t) * (size_t)(nnz + 1));
    float *val = malloc(sizeof(float) * (size_t)(nnz + 1));
    for (long long e = 0; e < nnz; ++e) {
        if (scanf("%lld %f", &v, &val[e]) != 2) return 2;
        gene[e] = (int32_t)v;
    }
    uint8_t *cls = malloc((size_t)(n_raw + 1));
    for (long long i = 0; i < n_raw; ++i) {
        if (scanf("%lld", &v) != 1) return 2;
        cls[i] = (uint8_t)v;
    }
    int64_t *rows = malloc(sizeof(int64_t) * (size_t)(n_rows + 1)), *n_ent = malloc(sizeof(int64_t) * (size_t)(n_rows + 1));
    for (long long i = 0; i < n_rows; ++i) {
        if (scanf("%lld", &v) != 1) return 2;
        rows[i] = v;
    }
    double *sums = malloc(sizeof(double) * (size_t)(n_rows * (1 + n_classes) + 1));
    int st = nabo_cell_qc(0, n_cells, n_raw, cell_ptr, gene, val, (int32_t)n_classes, cls, n_rows, rows, 0, n_ent, sums);
    if (st != NABO_OK) {
        printf("error %d: %s\n", st, nabo_last_error());
        return 1;
    }
    for (long long r = 0; r < n_rows; ++r) {
        printf("row %lld %lld", r, (long long)n_ent[r]);
        for (long long c = 0; c <= n_classes; ++c) printf(" %.17g", sums[r * (1 + n_classes) + c]);
        printf("\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "run")) return run();
    void *fns[] = {(void *)nabo_cell_qc, (void *)nabo_qc_last_device_ms};
    int n = 0;
    for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) n += fns[i] != NULL;
    const int64_t ptr[2] = {0, 1}, bad_ptr[2] = {1, 1};
    const int32_t gene[1] = {0};
    const float val[1] = {1.0f}, neg[1] = {-1.0f};
    const uint8_t cls[1] = {1};
    int64_t n_ent[1];
    double sums[2];
    /* nine classes */
    int rc = nabo_cell_qc(0, 1, 1, ptr, gene, val, 9, cls, 0, NULL, 0, n_ent, sums);
    /* cell_ptr[0] != 0 */
    int rc2 = nabo_cell_qc(0, 1, 1, bad_ptr, gene, val, 1, cls, 0, NULL, 0, n_ent, sums);
    /* a negative value */
    int rc3 = nabo_cell_qc(0, 1, 1, ptr, gene, neg, 1, cls, 0, NULL, 0, n_ent, sums);
    printf("%d entry points; 9 classes -> %d, bad cell_ptr -> %d, negative value -> %d (%s)\n", n, rc, rc2, rc3, nabo_last_error());
    return rc == NABO_E_INVALID && rc2 == NABO_E_INVALID && rc3 == NABO_E_INVALID && nabo_qc_last_device_ms(NULL, NULL) == NABO_E_INVALID ? 0 : 1;
}

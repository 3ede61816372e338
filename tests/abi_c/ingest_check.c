/* include/nabo_ingest.h through a plain C99 compiler, linked against libnabo_knn.so: takes the address of every entry
 * point, prints how many there are, and checks that bad arguments are refused before any device is touched.
 * `ingest_check run CHUNK < matrix.mtx` also reads the file on the device, CHUNK bytes per feed, and prints both indexes:
 *     size n_genes n_cells nnz / cell_ptr ... / gene ... / val ... / gene_ptr ... / cell ... / gene_val ... */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nabo_ingest.h"

static void print64(const char *name, const int64_t *a, int64_t n)
{
    printf("%s", name);
    for (int64_t i = 0; i < n; ++i) printf(" %lld", (long long)a[i]);
    printf("\n");
}

static void print32(const char *name, const uint32_t *a, int64_t n)
{
    printf("%s", name);
    for (int64_t i = 0; i < n; ++i) printf(" %lu", (unsigned long)a[i]);
    printf("\n");
}

static int run(long long chunk)
{
    size_t cap = 1 << 16, n = 0, got;
    char *file = malloc(cap);
    while ((got = fread(file + n, 1, cap - n, stdin)) > 0) {
        n += got;
        if (n == cap) file = realloc(file, cap *= 2);
    }
    nabo_mtx *h = NULL;
    int st = nabo_mtx_create(0, 0, 0, &h);
    for (size_t at = 0; st == NABO_OK && at < n; at += (size_t)chunk)
        st = nabo_mtx_feed(h, file + at, (int64_t)(n - at < (size_t)chunk ? n - at : (size_t)chunk));
    int64_t n_genes = 0, n_cells = 0, nnz = 0;
    if (st == NABO_OK) st = nabo_mtx_finish(h, &n_genes, &n_cells, &nnz);
    if (st != NABO_OK) {
        printf("error %d: %s\n", st, nabo_last_error());
        nabo_mtx_free(h);
        return 1;
    }
    int64_t *cell_ptr = malloc(sizeof(int64_t) * (size_t)(n_cells + 1)), *gene_ptr = malloc(sizeof(int64_t) * (size_t)(n_genes + 1));
    int32_t *gene = malloc(4 * (size_t)(nnz + 1)), *cell = malloc(4 * (size_t)(nnz + 1));
    uint32_t *val = malloc(4 * (size_t)(nnz + 1)), *gval = malloc(4 * (size_t)(nnz + 1));
    st = nabo_mtx_get_csr(h, cell_ptr, gene, val);
    if (st == NABO_OK) st = nabo_mtx_get_csc(h, gene_ptr, cell, gval);
    nabo_mtx_free(h);
    if (st != NABO_OK) {
        printf("error %d: %s\n", st, nabo_last_error());
        return 1;
    }
    printf("size %lld %lld %lld\n", (long long)n_genes, (long long)n_cells, (long long)nnz);
    print64("cell_ptr", cell_ptr, n_cells + 1);
    print32("gene", (const uint32_t *)gene, nnz);
    print32("val", val, nnz);
    print64("gene_ptr", gene_ptr, n_genes + 1);
    print32("cell", (const uint32_t *)cell, nnz);
    print32("gene_val", gval, nnz);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 2 && !strcmp(argv[1], "run")) return run(atoll(argv[2]) > 0 ? atoll(argv[2]) : 1 << 20);
    void *fns[] = {(void *)nabo_mtx_create, (void *)nabo_mtx_feed,     (void *)nabo_mtx_finish,   (void *)nabo_mtx_get_csr,        (void *)nabo_mtx_get_csc,
                   (void *)nabo_mtx_free,   (void *)nabo_mtx_geometry, (void *)nabo_mtx_last_device_ms, (void *)nabo_csr_transpose};
    int n = 0;
    for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) n += fns[i] != NULL;
    int32_t tile = 0, max_line = 0;
    const int64_t ptr[2] = {0, 2}, bad_ptr[2] = {1, 2};
    const int32_t idx[2] = {0, 1}, same[2] = {1, 1};
    const float val[2] = {1.0f, 2.0f};
    int64_t out_ptr[3];
    int32_t out_idx[2];
    float out_val[2];
    /* ptr[0] != 0 */
    int rc = nabo_csr_transpose(0, 1, 2, bad_ptr, idx, val, out_ptr, out_idx, out_val);
    /* a row that is not strictly increasing */
    int rc2 = nabo_csr_transpose(0, 1, 2, ptr, same, val, out_ptr, out_idx, out_val);
    /* no reader */
    int rc3 = nabo_mtx_feed(NULL, "x", 1);
    int rc4 = nabo_mtx_geometry(&tile, &max_line);
    printf("%d entry points; bad ptr -> %d, repeated index -> %d, NULL reader -> %d (%s); tile_bytes %d max_line %d\n", n, rc, rc2, rc3,
           nabo_last_error(), (int)tile, (int)max_line);
    nabo_mtx_free(NULL);
    return rc == NABO_E_INVALID && rc2 == NABO_E_INVALID && rc3 == NABO_E_INVALID && rc4 == NABO_OK && tile > 0 && max_line > 0 &&
                   nabo_mtx_geometry(NULL, NULL) == NABO_E_INVALID && nabo_mtx_last_device_ms(NULL, NULL, NULL) == NABO_E_INVALID
               ? 0
               : 1;
}

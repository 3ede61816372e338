/* include/nabo_counts.h through a plain C99 compiler, linked against libnabo_knn.so: takes the address of every entry
 * point, prints how many there are, and checks that bad arguments are refused before any device is touched.
 * `counts_check run CAP BLANK < blob` also writes a matrix on the device and prints its text, read CAP bytes at a time;
 * blob: int64 n_genes, n_cells, then cell_ptr int64[n_cells + 1], gene int32[nnz], val uint32[nnz]. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nabo_counts.h"

static int run(long long cap, int blank)
{
    size_t room = 1 << 16, n = 0, got;
    char *blob = malloc(room);
    while ((got = fread(blob + n, 1, room - n, stdin)) > 0) {
        n += got;
        if (n == room) blob = realloc(blob, room *= 2);
    }
    int64_t dims[2];
    if (n < sizeof dims) return 2;
    memcpy(dims, blob, sizeof dims);
    const int64_t *ptr = (const int64_t *)(blob + 16);
    const int64_t nnz = ptr[dims[1]];
    const int32_t *gene = (const int32_t *)(blob + 16 + 8 * (dims[1] + 1));
    const uint32_t *val = (const uint32_t *)(gene + nnz);
    nabo_mtxw *h = NULL;
    int64_t total = 0, done = 0, k = 0;
    int st = nabo_mtxw_create(0, dims[0], dims[1], ptr, gene, val, "% plain C\n", blank, 64, 0, &h, &total);
    char *buf = malloc((size_t)cap);
    while (st == NABO_OK && (st = nabo_mtxw_read(h, buf, cap, &k)) == NABO_OK && k > 0) {
        fwrite(buf, 1, (size_t)k, stdout);
        done += k;
    }
    nabo_mtxw_free(h);
    if (st != NABO_OK) {
        printf("error %d: %s\n", st, nabo_last_error());
        return 1;
    }
    return done == total ? 0 : 3;
}

int main(int argc, char **argv)
{
    if (argc > 3 && !strcmp(argv[1], "run")) return run(atoll(argv[2]) > 0 ? atoll(argv[2]) : 4096, atoi(argv[3]));
    void *fns[] = {(void *)nabo_mtxw_create,   (void *)nabo_mtxw_read,   (void *)nabo_mtxw_last_device_ms,
                   (void *)nabo_mtxw_free,     (void *)nabo_mtxw_geometry, (void *)nabo_counts_remap};
    int n = 0;
    for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) n += fns[i] != NULL;
    const int64_t ptr[2] = {0, 2}, bad_ptr[2] = {1, 2}, src[1] = {0}, bad_src[1] = {1};
    const int32_t idx[2] = {0, 1}, same[2] = {1, 1}, map[2] = {1, 0}, bad_map[2] = {0, 2};
    const uint32_t val[2] = {1, 2};
    nabo_mtxw *h = NULL;
    int64_t total = 0, nnz = 0, out_ptr[2];
    int32_t out_idx[2];
    uint32_t out_val[2];
    /* ptr[0] != 0; a cell that is not strictly increasing; comments that are no lines */
    int rc = nabo_mtxw_create(0, 2, 1, bad_ptr, idx, val, NULL, 0, 0, 0, &h, &total);
    int rc2 = nabo_mtxw_create(0, 2, 1, ptr, same, val, NULL, 0, 0, 0, &h, &total);
    int rc3 = nabo_mtxw_create(0, 2, 1, ptr, idx, val, "no percent\n", 0, 0, 0, &h, &total);
    /* a source row and a target column out of range */
    int rc4 = nabo_counts_remap(0, 1, 2, ptr, idx, val, 1, bad_src, 2, map, &nnz, out_ptr, out_idx, out_val, NULL, NULL, NULL);
    int rc5 = nabo_counts_remap(0, 1, 2, ptr, idx, val, 1, src, 2, bad_map, &nnz, out_ptr, out_idx, out_val, NULL, NULL, NULL);
    int rc6 = nabo_mtxw_read(NULL, out_val, 1, &total);
    int32_t g[4] = {0, 0, 0, 0};
    int rc7 = nabo_mtxw_geometry(&g[0], &g[1], &g[2], &g[3]);
    printf("%d entry points; bad ptr -> %d, repeated gene -> %d, bad comments -> %d, bad row_src -> %d, bad col_map -> %d, NULL writer -> %d (%s); "
           "tile_bytes %d min_chunk %d long_cell %d max_line %d\n",
           n, rc, rc2, rc3, rc4, rc5, rc6, nabo_last_error(), (int)g[0], (int)g[1], (int)g[2], (int)g[3]);
    nabo_mtxw_free(NULL);
    return rc == NABO_E_INVALID && rc2 == NABO_E_INVALID && rc3 == NABO_E_INVALID && rc4 == NABO_E_INVALID && rc5 == NABO_E_INVALID &&
                   rc6 == NABO_E_INVALID && rc7 == NABO_OK && h == NULL && g[0] > 0 && g[1] > 0 && g[2] > 0 && g[3] == 33 &&
                   nabo_mtxw_geometry(NULL, NULL, NULL, NULL) == NABO_E_INVALID && nabo_mtxw_last_device_ms(NULL, NULL, NULL) == NABO_E_INVALID
               ? 0
               : 1;
}

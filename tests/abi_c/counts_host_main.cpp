// The host half of the Matrix Market writer and of the remap (nabo_amd/csrc/counts_host.h) as a program of its own, for
// a build under the address and undefined-behaviour sanitizers (tests/test_counts_cpu.py):
//     counts_host_main BLANK CAP CHUNK COMMENTS < blob
// blob: int64 n_genes, n_cells, n_out_rows, n_out_cols, n_map, then cell_ptr int64[n_cells + 1], gene int32[nnz], val
// uint32[nnz], row_src int64[n_out_rows], col_map int32[n_map] (the remap's plan reads the matrix as n_cells rows over n_map
// columns).
// stdout: the whole text, served as nabo_mtxw_read serves it -- reads of CAP bytes, the body refilled CHUNK bytes at a time
// from the host's statement of it.  stderr, one line each: `comments OK`, `chunk CLAMPED`, `idx CODE MAJOR ENTRY`,
// `long N LONGEST`, `plan CODE AT BOUND MONOTONE`, `digits OK` (digits10 and put_digits against snprintf at every power
// of ten and its neighbours).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../nabo_amd/csrc/counts_host.h"

namespace cnt = nabo::counts;

template <class T> static std::vector<T> take(const std::vector<uint8_t> &blob, size_t *at, size_t n)
{
    std::vector<T> out(n);
    if (*at + n * sizeof(T) > blob.size()) exit(4);
    if (n) memcpy(out.data(), blob.data() + *at, n * sizeof(T));
    *at += n * sizeof(T);
    return out;
}

static bool digits_agree()
{
    std::vector<uint32_t> vs = {0u, 1u, 0xFFFFFFFFu, 0xFFFFFFFEu, 0x80000000u, 0x7FFFFFFFu};
    for (uint64_t p = 10; p <= 1000000000ull; p *= 10)
        for (int d = -1; d <= 1; ++d) vs.push_back((uint32_t)((int64_t)p + d));
    for (uint32_t v : vs) {
        char want[16], got[16];
        const int n = snprintf(want, sizeof want, "%lu", (unsigned long)v);
        if (cnt::digits10(v) != n || cnt::put_digits(got + n, v) != got || memcmp(want, got, (size_t)n) != 0) return false;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    const bool blank = atoi(argv[1]) != 0;
    const long long cap = atoll(argv[2]), chunk_arg = atoll(argv[3]);
    const char *comments = argv[4][0] ? argv[4] : nullptr;
    std::vector<uint8_t> blob;
    uint8_t tmp[4096];
    size_t got;
    while ((got = fread(tmp, 1, sizeof tmp, stdin)) > 0) blob.insert(blob.end(), tmp, tmp + got);
    size_t at = 0;
    const std::vector<int64_t> dims = take<int64_t>(blob, &at, 5);
    const int64_t n_genes = dims[0], n_cells = dims[1], n_out_rows = dims[2], n_out_cols = dims[3], n_map = dims[4];
    const std::vector<int64_t> ptr = take<int64_t>(blob, &at, (size_t)n_cells + 1);
    const int64_t nnz = std::max<int64_t>(ptr[(size_t)n_cells], 0);
    const std::vector<int32_t> gene = take<int32_t>(blob, &at, (size_t)nnz);
    const std::vector<uint32_t> val = take<uint32_t>(blob, &at, (size_t)nnz);
    const std::vector<int64_t> row_src = take<int64_t>(blob, &at, (size_t)n_out_rows);
    const std::vector<int32_t> col_map = take<int32_t>(blob, &at, (size_t)n_map);

    const int64_t chunk = cnt::clamp_chunk(chunk_arg);
    fprintf(stderr, "comments %d\nchunk %lld\n", (int)cnt::comments_ok(comments), (long long)chunk);
    const cnt::IdxVerdict v = cnt::check_indices(n_cells, n_genes, ptr.data(), gene.data(), val.data());
    fprintf(stderr, "idx %d %lld %lld\n", v.code, (long long)v.major, (long long)v.entry);
    std::vector<int32_t> longs;
    const int64_t longest = cnt::long_cells(n_cells, ptr.data(), &longs);
    fprintf(stderr, "long %zu %lld\n", longs.size(), (long long)longest);
    const cnt::RemapPlan plan = cnt::plan_remap(n_cells, n_map, ptr.data(), n_out_rows, row_src.data(), n_out_cols, col_map.data());
    fprintf(stderr, "plan %d %lld %lld %d\n", plan.code, (long long)plan.at, (long long)plan.bound, (int)plan.monotone);
    fprintf(stderr, "digits %d\n", (int)digits_agree());
    if (v.code || !cnt::comments_ok(comments)) return 0;

    const std::string body = cnt::body_text(n_cells, ptr.data(), gene.data(), val.data(), blank);
    cnt::Server srv;
    srv.head = cnt::head_text(comments, n_genes, n_cells, nnz);
    srv.body_bytes = (int64_t)body.size();
    std::vector<uint8_t> chunk_buf((size_t)chunk), out((size_t)std::max<long long>(cap, 1));
    srv.chunk = chunk_buf.data();
    int64_t total = 0;
    for (;;) {
        int64_t n = 0;
        while (n < cap) {
            if (srv.need_chunk()) {
                const int64_t from = srv.body_pos(), len = std::min<int64_t>(chunk, srv.body_bytes - from);
                memcpy(chunk_buf.data(), body.data() + from, (size_t)len);
                srv.chunk_at = from;
                srv.chunk_len = len;
            }
            const int64_t took = srv.take(out.data() + n, cap - n);
            if (took == 0) break;
            n += took;
        }
        if (n == 0) break;
        fwrite(out.data(), 1, (size_t)n, stdout);
        total += n;
    }
    return total == srv.total() ? 0 : 3;
}

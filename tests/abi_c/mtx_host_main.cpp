// The host half of the Matrix Market reader (nabo_amd/csrc/mtx_host.h) as a program of its own, for a build under the
// address and undefined-behaviour sanitizers (tests/test_ingest_cpu.py):
//     mtx_host_main SPLIT CHUNK < file
// feeds the file SPLIT bytes at a time (0: all at once) through HeaderParser and a LineBuffer of CHUNK bytes, as
// nabo_mtx_feed and nabo_mtx_finish do, and prints `header n_genes n_cells nnz header_lines real` (or `refused STATUS
// message`) and then the pieces it would upload, concatenated: the body, with a `\n` after a last line that lacks one.
// Every piece must be whole lines; `too long` ends the output when a line outgrows the buffer.  The verdict of parse_line
// on every line of the body follows on stderr, one number per line.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../nabo_amd/csrc/mtx_host.h"

namespace mtx = nabo::mtx;

static int emit(const mtx::LineBuffer &lb, int64_t len, std::vector<uint8_t> *body)
{
    if (len > 0 && lb.buf[len - 1] != '\n') return 1;
    body->insert(body->end(), lb.buf, lb.buf + len);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const long long split = atoll(argv[1]), chunk = atoll(argv[2]);
    std::vector<uint8_t> file, body;
    uint8_t tmp[4096];
    size_t got;
    while ((got = fread(tmp, 1, sizeof tmp, stdin)) > 0) file.insert(file.end(), tmp, tmp + got);
    mtx::HeaderParser head;
    mtx::LineBuffer lb;
    lb.chunk = mtx::LineBuffer::clamp_chunk(chunk);
    std::vector<uint8_t> store((size_t)lb.max_piece());
    lb.buf = store.data();
    bool too_long = false;
    const int64_t step = split > 0 ? split : (int64_t)file.size() + 1;
    for (int64_t at = 0; at < (int64_t)file.size() && !head.status && !too_long; at += step) {
        const uint8_t *p = file.data() + at;
        int64_t n = std::min<int64_t>(step, (int64_t)file.size() - at);
        if (!head.done) {
            const int64_t took = head.feed(p, n);
            p += took, n -= took;
        }
        while (n > 0 && head.done && !too_long) {
            const int64_t took = lb.push(p, n);
            p += took, n -= took;
            if (!lb.ready()) continue;
            const int64_t len = lb.piece();
            if (len == 0) {
                too_long = lb.too_long();
                continue;
            }
            if (emit(lb, len, &body)) return 3;
            lb.drop(len);
        }
    }
    if (!head.done) head.finish();
    if (head.status) {
        printf("refused %d %s\n", head.status, head.message.c_str());
        return 0;
    }
    printf("header %lld %lld %lld %lld %d\n", (long long)head.n_genes, (long long)head.n_cells, (long long)head.nnz, (long long)head.lines, (int)head.real);
    if (!too_long && emit(lb, lb.close(), &body)) return 3;
    if (!body.empty()) fwrite(body.data(), 1, body.size(), stdout);
    if (too_long) printf("too long\n");
    size_t pos = 0;
    while (pos < body.size()) {
        const uint8_t *nl = static_cast<const uint8_t *>(memchr(body.data() + pos, '\n', body.size() - pos));
        const size_t end = nl ? (size_t)(nl - body.data()) : body.size();
        uint64_t f[3];
        fprintf(stderr, "%d\n", mtx::parse_line(body.data() + pos, (int64_t)(end - pos), head.n_genes, head.n_cells, f));
        pos = end + 1;
    }
    return 0;
}

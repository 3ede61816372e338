// The host half of the CSV reader (nabo_amd/csrc/csv_host.h) and the number routine it shares with the kernel
// (nabo_amd/csrc/csv_number.h) as a program of their own, for a build under the address and undefined-behaviour sanitizers
// (tests/test_csv_cpu.py):
//     csv_host_main fields KIND < fields      one field per line of stdin (its `\n` not part of it): prints `CODE BITS` per
//                                             field, CODE the verdict of convert_field (0 converted, -1 deferred, > 0 an
//                                             error) and BITS the 8 bytes in hex -- for a deferred field those host_convert
//                                             gives, with `!N` appended when host_convert refuses with code N
//     csv_host_main table                     the 651 powers of five, `q high low` in hex
//     csv_host_main feed SPLIT CHUNK SEP < x  feeds stdin SPLIT bytes at a time (0: all at once) through a FieldBuffer of
//                                             CHUNK bytes with the separator byte SEP (a number) as nabo_csv_feed and
//                                             nabo_csv_finish do, and prints the pieces it would upload, concatenated; every
//                                             piece must end with a separator or a `\n`; `too long` ends the output when a
//                                             field outgrows the buffer.  stderr, per piece: the carried column, the piece's
//                                             length, and `line field` of the byte in its middle (locate).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../nabo_amd/csrc/csv_host.h"

namespace csv = nabo::csv;

static std::vector<uint8_t> read_all()
{
    std::vector<uint8_t> file;
    uint8_t tmp[4096];
    size_t got;
    while ((got = fread(tmp, 1, sizeof tmp, stdin)) > 0) file.insert(file.end(), tmp, tmp + got);
    return file;
}

static int run_fields(int kind)
{
    std::vector<uint64_t> pow5((size_t)csv::POW5_WORDS);
    csv::build_pow5(pow5.data());
    const std::vector<uint8_t> file = read_all();
    size_t pos = 0;
    while (pos < file.size()) {
        const uint8_t *nl = static_cast<const uint8_t *>(memchr(file.data() + pos, '\n', file.size() - pos));
        const size_t end = nl ? (size_t)(nl - file.data()) : file.size();
        // a copy of its own size, so that a read past the field is a read past an allocation
        std::vector<uint8_t> f(file.begin() + (long)pos, file.begin() + (long)end);
        uint64_t bits = 0;
        int code = f.size() > (size_t)csv::MAX_FIELD ? (int)csv::DEFER : csv::convert_field(f.data(), (int)f.size(), false, kind, pow5.data(), &bits);
        int refused = 0;
        if (code == csv::DEFER) refused = csv::host_convert(f.data(), (int64_t)f.size(), false, kind, &bits);
        if (code > 0) bits = 0;
        printf("%d %016llx", code, (unsigned long long)bits);
        if (refused) printf(" !%d", refused);
        printf("\n");
        pos = end + 1;
    }
    return 0;
}

static int run_table()
{
    std::vector<uint64_t> pow5((size_t)csv::POW5_WORDS);
    csv::build_pow5(pow5.data());
    for (int q = csv::POW5_MIN; q <= csv::POW5_MAX; ++q)
        printf("%d %016llx %016llx\n", q, (unsigned long long)pow5[(size_t)(2 * (q - csv::POW5_MIN))], (unsigned long long)pow5[(size_t)(2 * (q - csv::POW5_MIN) + 1)]);
    return 0;
}

static int emit(const csv::FieldBuffer &fb, int64_t len, int64_t *col, std::vector<uint8_t> *body)
{
    if (len == 0) return 0;
    if (fb.buf[len - 1] != '\n' && fb.buf[len - 1] != fb.sep) return 1;
    const csv::Place mid = csv::locate(fb.buf, len / 2, fb.sep, *col), end = csv::locate(fb.buf, len, fb.sep, *col);
    fprintf(stderr, "%lld %lld %lld %lld\n", (long long)*col, (long long)len, (long long)mid.line, (long long)mid.field);
    *col = end.field;
    body->insert(body->end(), fb.buf, fb.buf + len);
    return 0;
}

static int run_feed(long long split, long long chunk, int sep)
{
    const std::vector<uint8_t> file = read_all();
    std::vector<uint8_t> body;
    csv::FieldBuffer fb;
    fb.sep = (uint8_t)sep;
    fb.chunk = csv::FieldBuffer::clamp_chunk(chunk);
    std::vector<uint8_t> store((size_t)fb.max_piece());
    fb.buf = store.data();
    bool too_long = false;
    int64_t col = 0;
    const int64_t step = split > 0 ? split : (int64_t)file.size() + 1;
    for (int64_t at = 0; at < (int64_t)file.size() && !too_long; at += step) {
        const uint8_t *p = file.data() + at;
        int64_t n = std::min<int64_t>(step, (int64_t)file.size() - at);
        while (n > 0 && !too_long) {
            const int64_t took = fb.push(p, n);
            p += took, n -= took;
            if (!fb.ready()) continue;
            const int64_t len = fb.piece();
            if (len == 0) {
                too_long = fb.too_long();
                continue;
            }
            if (emit(fb, len, &col, &body)) return 3;
            fb.drop(len);
        }
    }
    if (!too_long && emit(fb, fb.close(), &col, &body)) return 3;
    if (!body.empty()) fwrite(body.data(), 1, body.size(), stdout);
    if (too_long) printf("too long\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && std::string(argv[1]) == "fields") return run_fields(atoi(argv[2]));
    if (argc == 2 && std::string(argv[1]) == "table") return run_table();
    if (argc == 5 && std::string(argv[1]) == "feed") return run_feed(atoll(argv[2]), atoll(argv[3]), atoi(argv[4]));
    return 2;
}

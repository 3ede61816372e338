// mtx_host.h -- the host half of the Matrix Market reader (include/nabo_ingest.h), without a single HIP call: the
// geometry, the error codes the parse kernel and the host share, the header parser, the host's statement of one body
// line, and the buffer that turns bytes fed in any split into pieces of whole lines.  mtx_ingest.hip includes it; the
// tests compile it with a small main (tests/abi_c/mtx_host_main.cpp) under the address and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/nabo_knn.h"

namespace nabo {
namespace mtx {

constexpr int TILE_BYTES = 16384, MAX_LINE = 1024;
constexpr int64_t DEFAULT_CHUNK = (int64_t)64 << 20, MIN_CHUNK = 64, MAX_CHUNK = (int64_t)1 << 30;

// what is wrong with a body line, in the order the header states: the length, the first offending byte, the number of
// fields, the ranges.  LINE_EXCESS is the host's: an entry line beyond the nnz the size line announced.
enum LineCode { LINE_ENTRY = 0, LINE_LONG = 1, LINE_SYNTAX = 2, LINE_REAL = 3, LINE_FIELDS = 4, LINE_GENE = 5, LINE_CELL = 6, LINE_VALUE = 7, LINE_EXCESS = 8, LINE_SKIP = -1 };

inline const char *code_text(int code)
{
    switch (code) {
    case LINE_LONG: return "the line is longer than max_line bytes";
    case LINE_SYNTAX: return "expected three unsigned integers `gene cell value` (no signs, nothing else on the line)";
    case LINE_REAL: return "real values are not supported: write counts as unsigned integers";
    case LINE_FIELDS: return "expected exactly three fields `gene cell value`";
    case LINE_GENE: return "gene is not in [1, n_genes]";
    case LINE_CELL: return "cell is not in [1, n_cells]";
    case LINE_VALUE: return "value is not in [0, 4294967295]";
    case LINE_EXCESS: return "more entry lines than the size line announced";
    }
    return "?";
}

// One body line s[0 .. len), its `\n` not included: LINE_ENTRY with the 1-based gene and cell and the value,
// LINE_SKIP, or what is wrong with it.  The parse kernel's mtx_parse_line is the same function over LDS.
inline int parse_line(const uint8_t *s, int64_t len, int64_t n_genes, int64_t n_cells, uint64_t f[3])
{
    if (len > MAX_LINE) return LINE_LONG;
    int nf = 0, nd = 0, bad = 0;
    unsigned over = 0;
    bool indig = false, seen = false;
    uint64_t v = 0;
    f[0] = f[1] = f[2] = 0;
    for (int64_t i = 0; i < len && !bad; ++i) {
        const uint8_t c = s[i];
        if (c == ' ' || c == '\t' || (c == '\r' && i + 1 == len)) {
            if (indig) {
                f[nf] = v;
                over |= (unsigned)(nd > 19) << nf;
                ++nf;
                indig = false;
            }
            continue;
        }
        if (!seen) {
            seen = true;
            if (c == '%') return LINE_SKIP;
        }
        const unsigned d = (unsigned)c - '0';
        if (d <= 9) {
            if (!indig) {
                if (nf == 3) {
                    bad = LINE_FIELDS;
                    continue;
                }
                indig = true;
                v = 0;
                nd = 0;
            }
            if (nd > 0 || d > 0)
                if (++nd <= 19) v = v * 10 + d;
        } else
            bad = (c == '.' || ((c == 'e' || c == 'E') && indig)) ? LINE_REAL : LINE_SYNTAX;
    }
    if (bad) return bad;
    if (indig) {
        f[nf] = v;
        over |= (unsigned)(nd > 19) << nf;
        ++nf;
    }
    if (!seen) return LINE_SKIP;
    if (nf != 3) return LINE_FIELDS;
    if ((over & 1) || f[0] < 1 || f[0] > (uint64_t)n_genes) return LINE_GENE;
    if ((over & 2) || f[1] < 1 || f[1] > (uint64_t)n_cells) return LINE_CELL;
    if ((over & 4) || f[2] > 0xFFFFFFFFull) return LINE_VALUE;
    return LINE_ENTRY;
}

// The header: banner, comments, size line.  feed() consumes bytes up to and including the `\n` of the size line and
// says how many it took; done is set then.  status < 0 with a message after a refusal.
struct HeaderParser {
    std::string line, message;
    int64_t lines = 0, n_genes = 0, n_cells = 0, nnz = 0;
    bool banner = false, real = false, done = false;
    int status = 0;

    int fail(int code, const std::string &what)
    {
        message = "line " + std::to_string((long long)lines + 1) + ": " + what;
        return status = code;
    }

    static std::string lower(std::string s)
    {
        for (char &c : s)
            if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
        return s;
    }

    // the words of a line, split at blanks
    static int words(const std::string &s, std::string out[], int max)
    {
        int n = 0;
        size_t i = 0;
        while (i < s.size()) {
            while (i < s.size() && (s[i] == ' ' || s[i] == '\t')) ++i;
            if (i == s.size()) break;
            size_t j = i;
            while (j < s.size() && s[j] != ' ' && s[j] != '\t') ++j;
            if (n < max) out[n] = s.substr(i, j - i);
            ++n;
            i = j;
        }
        return n;
    }

    int take_line()
    {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (!banner) {
            static const char tag[] = "%%MatrixMarket";
            if (line.compare(0, sizeof tag - 1, tag) != 0) return fail(NABO_E_INVALID, "the file does not start with %%MatrixMarket");
            std::string w[5];
            const int n = words(line.substr(sizeof tag - 1), w, 5);
            for (std::string &x : w) x = lower(x);
            if (n != 4 || w[0] != "matrix" || w[1] != "coordinate" || (w[2] != "integer" && w[2] != "real") || w[3] != "general")
                return fail(NABO_E_INVALID, "the banner must read `matrix coordinate integer general` (or `real`)");
            real = w[2] == "real";
            banner = true;
            return 0;
        }
        if (!line.empty() && line[0] == '%') return 0;
        std::string w[4];
        if (words(line, w, 4) != 3) return fail(NABO_E_INVALID, "the size line must hold three unsigned integers `n_genes n_cells nnz`");
        uint64_t v[3];
        for (int k = 0; k < 3; ++k) {
            size_t z = 0;
            while (z < w[k].size() && w[k][z] == '0') ++z;
            v[k] = 0;
            for (size_t i = 0; i < w[k].size(); ++i) {
                if (w[k][i] < '0' || w[k][i] > '9') return fail(NABO_E_INVALID, "the size line must hold three unsigned integers `n_genes n_cells nnz`");
                if (i >= z && i - z < 19) v[k] = v[k] * 10 + (uint64_t)(w[k][i] - '0');
            }
            if (w[k].size() - z > 19) v[k] = ~(uint64_t)0;
        }
        if (v[0] >= ((uint64_t)1 << 31) || v[1] >= ((uint64_t)1 << 31)) return fail(NABO_E_UNSUPPORTED, "n_genes and n_cells must be below 2^31");
        if (v[2] >= 0xFFFFFFFFull) return fail(NABO_E_UNSUPPORTED, "nnz must be below 2^32 - 1");
        n_genes = (int64_t)v[0], n_cells = (int64_t)v[1], nnz = (int64_t)v[2];
        done = true;
        return 0;
    }

    int64_t feed(const uint8_t *p, int64_t n)
    {
        int64_t i = 0;
        while (i < n && !done && !status) {
            const uint8_t c = p[i++];
            if (c != '\n') {
                line.push_back((char)c);
                continue;
            }
            if (take_line() == 0) ++lines;
            line.clear();
        }
        return i;
    }

    // the stream ended inside the header: a size line without its `\n` still counts
    int finish()
    {
        if (!done && !status && !line.empty()) {
            if (take_line() == 0) ++lines;
            line.clear();
        }
        if (!done && !status) fail(NABO_E_INVALID, banner ? "the file ends before its size line" : "the file does not start with %%MatrixMarket");
        return status;
    }
};

// The body's bytes, fed in any split, as pieces of whole lines.  buf has room for max_piece() bytes (the caller's: pinned
// memory in the library, a vector in the tests).  push() appends as much as fits; once size >= chunk, piece() is the
// length through the last `\n` (0: none yet, and the unfinished line is too long when size > MAX_LINE); drop(len)
// carries the rest to the front.  close() ends the stream: a last line without `\n` gets one, so that a `\r` at the end
// of the stream stands in front of a `\n` like any other.
struct LineBuffer {
    uint8_t *buf = nullptr;
    int64_t chunk = 0, size = 0;

    static int64_t clamp_chunk(int64_t c) { return c <= 0 ? DEFAULT_CHUNK : c < MIN_CHUNK ? MIN_CHUNK : c > MAX_CHUNK ? MAX_CHUNK : c; }
    int64_t fill() const { return chunk > MAX_LINE + 1 ? chunk : MAX_LINE + 1; }
    // the bytes a piece can have, and the buffer must hold: a full buffer and the `\n` of close()
    int64_t max_piece() const { return fill() + 1; }

    int64_t push(const uint8_t *p, int64_t n)
    {
        const int64_t take = n < fill() - size ? n : fill() - size;
        memcpy(buf + size, p, (size_t)take);
        size += take;
        return take;
    }
    bool ready() const { return size >= chunk; }
    int64_t piece() const
    {
        for (int64_t i = size; i > 0; --i)
            if (buf[i - 1] == '\n') return i;
        return 0;
    }
    bool too_long() const { return size > MAX_LINE; }
    void drop(int64_t len)
    {
        memmove(buf, buf + len, (size_t)(size - len));
        size -= len;
    }
    int64_t close()
    {
        if (size > 0 && buf[size - 1] != '\n') buf[size++] = '\n';
        return size;
    }
};

}  // namespace mtx
}  // namespace nabo

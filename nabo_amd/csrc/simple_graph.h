// simple_graph.h -- the simple graph the layout, the clustering and the differentiation potential start from, built once
// here on the host: tests/test_simple_graph_cpu.py compiles this header alone and checks it without a GPU.
//
// The input is a CSR that may list a pair in either direction, more than once, and self-loops.  The simple graph keeps
// each unordered pair once; the weight of a pair is that of its LAST occurrence, the one at the highest CSR position across
// all rows.  Its rows are symmetric and free of loops, in ascending neighbour.  Self-loops stay in the pair list, for the
// per-node sums of the steps that count them.  Node ids are below 2^31 (every caller checks), so a pair is one 64-bit key.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace nabo {

struct SimpleGraph {
    bool weighted = false;
    std::vector<uint64_t> pairs;       // the distinct pairs a <= b as (a << 32 | b), strictly ascending: (a, b) order
    std::vector<int64_t> last;         // weighted only: the CSR position of each pair's last occurrence
    std::vector<int64_t> rptr;         // [n + 1]
    std::vector<int32_t> rnbr;         // [rptr[n]]
    std::vector<int64_t> slot_pair;    // weighted only: the pair each slot of rnbr came from (a per-arc array is one pass over it)
    static int64_t lo(uint64_t key) { return (int64_t)(key >> 32); }
    static int64_t hi(uint64_t key) { return (int64_t)(key & 0xFFFFFFFFull); }
};

// One entry per arc of the input, made by make(key, position), in ascending order.  The entries are first bucketed by the
// pair's lower node (a counting sort) and each bucket, the few pairs of one node, is then sorted on its own: the order of
// one sort over all arcs at a fraction of its time.
template <class T, class Make> std::vector<T> sorted_arcs(int64_t n, const int64_t *ptr, const int64_t *nbr, Make make)
{
    std::vector<int64_t> at((size_t)n + 2, 0);   // at[a + 1]: where the next entry of bucket a goes; afterwards its end
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) ++at[(size_t)std::min(i, nbr[e]) + 2];
    for (int64_t a = 0; a < n; ++a) at[(size_t)a + 2] += at[(size_t)a + 1];
    std::vector<T> v((size_t)ptr[n]);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
            const int64_t a = std::min(i, nbr[e]), b = std::max(i, nbr[e]);
            v[(size_t)at[(size_t)a + 1]++] = make(((uint64_t)a << 32) | (uint64_t)b, e);
        }
    for (int64_t a = 0; a < n; ++a) std::sort(v.begin() + at[(size_t)a], v.begin() + at[(size_t)a + 1]);
    return v;
}

// Step 1, the pairs.  A weight-less graph sorts bare keys; a weighted one carries each arc's position to find the last.
inline void simple_pairs(SimpleGraph &g, int64_t n, const int64_t *ptr, const int64_t *nbr, bool weighted)
{
    g.weighted = weighted;
    if (!weighted) {
        g.pairs = sorted_arcs<uint64_t>(n, ptr, nbr, [](uint64_t key, int64_t) { return key; });
        g.pairs.erase(std::unique(g.pairs.begin(), g.pairs.end()), g.pairs.end());
        return;
    }
    struct Occ {
        uint64_t key;
        int64_t pos;
        bool operator<(const Occ &o) const { return key != o.key ? key < o.key : pos < o.pos; }
    };
    const std::vector<Occ> occ = sorted_arcs<Occ>(n, ptr, nbr, [](uint64_t key, int64_t pos) { return Occ{key, pos}; });
    g.pairs.reserve(occ.size());
    g.last.reserve(occ.size());
    for (size_t e = 0; e < occ.size(); ++e)
        if (e + 1 == occ.size() || occ[e + 1].key != occ[e].key) {
            g.pairs.push_back(occ[e].key);
            g.last.push_back(occ[e].pos);
        }
}

// Step 2, the rows of the pairs p with keep(p).  Within a row come first the lower-numbered partners (the pairs are in
// (a, b) order: ascending a for a fixed b), then the higher-numbered ones.  visit(p, a, b) sees every kept pair, self-loops
// included, in (a, b) order during the counting pass: what a step adds up per pair costs no pass of its own.
template <class Keep, class Visit> void simple_rows(SimpleGraph &g, int64_t n, Keep keep, Visit visit)
{
    const size_t P = g.pairs.size();
    g.rptr.assign((size_t)n + 1, 0);
    for (size_t p = 0; p < P; ++p) {
        const int64_t a = SimpleGraph::lo(g.pairs[p]), b = SimpleGraph::hi(g.pairs[p]);
        if (!keep(p)) continue;
        visit(p, a, b);
        if (a != b) {
            ++g.rptr[(size_t)a + 1];
            ++g.rptr[(size_t)b + 1];
        }
    }
    for (int64_t i = 0; i < n; ++i) g.rptr[(size_t)i + 1] += g.rptr[(size_t)i];
    const size_t A = (size_t)g.rptr[(size_t)n];
    g.rnbr.resize(A);
    g.slot_pair.resize(g.weighted ? A : 0);
    std::vector<int64_t> fill(g.rptr.begin(), g.rptr.end() - 1);
    for (int upper = 0; upper < 2; ++upper)
        for (size_t p = 0; p < P; ++p) {
            const int64_t a = SimpleGraph::lo(g.pairs[p]), b = SimpleGraph::hi(g.pairs[p]);
            if (a == b || !keep(p)) continue;
            const size_t at = (size_t)fill[(size_t)(upper ? a : b)]++;
            g.rnbr[at] = (int32_t)(upper ? b : a);
            if (g.weighted) g.slot_pair[at] = (int64_t)p;
        }
}

template <class Visit> void simple_graph(SimpleGraph &g, int64_t n, const int64_t *ptr, const int64_t *nbr, bool weighted, Visit visit)
{
    simple_pairs(g, n, ptr, nbr, weighted);
    simple_rows(g, n, [](size_t) { return true; }, visit);
}

// the rows of more than `threshold` arcs, ascending
inline std::vector<int32_t> long_rows(const std::vector<int64_t> &rptr, int64_t threshold)
{
    std::vector<int32_t> rows;
    for (size_t i = 0; i + 1 < rptr.size(); ++i)
        if (rptr[i + 1] - rptr[i] > threshold) rows.push_back((int32_t)i);
    return rows;
}

}  // namespace nabo

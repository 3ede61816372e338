// The simple-graph builder (nabo_amd/csrc/simple_graph.h) compiled for the host alone, callable from
// tests/test_simple_graph_cpu.py: the two steps as the library's callers take them, and long_rows.
#include "simple_graph.h"

#include <cstring>

using namespace nabo;

namespace {
struct Shim : SimpleGraph {
    std::vector<int64_t> visited;   // the pairs the counting pass showed its visitor, in that order
};
}  // namespace

extern "C" {

void *sg_pairs(int64_t n, const int64_t *ptr, const int64_t *nbr, int weighted)
{
    Shim *g = new Shim;
    simple_pairs(*g, n, ptr, nbr, weighted != 0);
    return g;
}

// keep: one byte per pair, NULL = every pair
void sg_rows(void *h, int64_t n, const uint8_t *keep)
{
    Shim *g = static_cast<Shim *>(h);
    const auto visit = [g](size_t p, int64_t a, int64_t b) {
        if (a == SimpleGraph::lo(g->pairs[p]) && b == SimpleGraph::hi(g->pairs[p])) g->visited.push_back((int64_t)p);
    };
    g->visited.clear();
    if (keep) simple_rows(*g, n, [keep](size_t p) { return keep[p] != 0; }, visit);
    else simple_rows(*g, n, [](size_t) { return true; }, visit);
}

// sizes: pairs, last, rptr, rnbr, slot_pair, visited
void sg_sizes(void *h, int64_t sizes[6])
{
    const Shim *g = static_cast<Shim *>(h);
    const size_t s[6] = {g->pairs.size(), g->last.size(), g->rptr.size(), g->rnbr.size(), g->slot_pair.size(), g->visited.size()};
    for (int i = 0; i < 6; ++i) sizes[i] = (int64_t)s[i];
}

void sg_get(void *h, uint64_t *pairs, int64_t *last, int64_t *rptr, int32_t *rnbr, int64_t *slot_pair, int64_t *visited)
{
    const Shim *g = static_cast<Shim *>(h);
    const auto copy = [](void *to, const auto &v) {
        if (to && !v.empty()) memcpy(to, v.data(), v.size() * sizeof v[0]);
    };
    copy(pairs, g->pairs);
    copy(last, g->last);
    copy(rptr, g->rptr);
    copy(rnbr, g->rnbr);
    copy(slot_pair, g->slot_pair);
    copy(visited, g->visited);
}

void sg_free(void *h) { delete static_cast<Shim *>(h); }

// out: room for n rows; returns how many are long
int64_t sg_long_rows(int64_t n, const int64_t *rptr, int64_t threshold, int32_t *out)
{
    const std::vector<int32_t> rows = long_rows(std::vector<int64_t>(rptr, rptr + n + 1), threshold);
    if (!rows.empty()) memcpy(out, rows.data(), rows.size() * 4);
    return (int64_t)rows.size();
}

}  // extern "C"

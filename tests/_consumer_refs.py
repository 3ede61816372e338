"""Plain references and fixed, seeded cases for the kernels that CONSUME the k-NN lists (tests/test_consumers_gpu.py):
the permutation null (score_null.hip, csr_build.hip), the shard merge and the SNN counts (canberra.hip).

Every reference here is plain Python / numpy written from the definitions in include/nabo_knn.h; nothing in this file
calls into nabo_amd.  tests/test_consumer_refs_cpu.py checks the references against the oracle wherever the oracle
defines the operation, and checks the error bound of the null's mean and sd on every case below."""
import numpy as np

U = 2.0 ** -53            # unit roundoff of float64


# ---- permutation null: mean and sd of the permuted scores ------------------------------------------------------------
def null_stats_ld(scores):
    """Two-pass mean and population sd of scores [n_ref, n_perm] in np.longdouble (the reference the device is held to)."""
    s = np.asarray(scores, dtype=np.longdouble)
    mean = s.sum(axis=1) / np.longdouble(s.shape[1])
    dev = s - mean[:, None]
    sd = np.sqrt((dev * dev).sum(axis=1) / np.longdouble(s.shape[1]))
    return mean, sd


def null_bounds(scores):
    """(bound on |mean - ref|, bound on |sd - ref|) per reference node.  With u = 2^-53, M = max_p |S_p| and
    gamma = (n_perm + 8) u: a float64 mean of n_perm terms summed in ANY order is within gamma M of the true mean; a
    two-pass sd taken around a mean that is off by delta is off by at most |delta| + gamma sd."""
    s = np.asarray(scores, dtype=np.float64)
    gamma = (s.shape[1] + 8) * U
    big = np.abs(s).max(axis=1)
    _, sd = null_stats_ld(s)
    return gamma * big, gamma * (big + sd.astype(np.float64))


def _stripe_tree(v):
    """The device's summation order (null_score_kernel): thread q of 256 adds entries q, q+256, ... in turn, then a
    pairwise tree over the 256 partial sums (offsets 128, 64, .., 1).  v [n_ref, n_perm] float64."""
    n_ref, P = v.shape
    part = np.zeros((n_ref, 256))
    for i in range((P + 255) // 256):
        blk = v[:, 256 * i:256 * (i + 1)]
        part[:, :blk.shape[1]] = part[:, :blk.shape[1]] + blk
    o = 128
    while o > 0:
        part[:, :o] = part[:, :o] + part[:, o:2 * o]
        o >>= 1
    return part[:, 0].copy()


def null_stats_device_order(scores, two_pass):
    """float64 restatement of the kernel's mean / sd: two_pass=True is sqrt(sum (s - mean)^2 / P); False is the earlier
    one-pass sqrt(max(0, sum s^2 / P - mean^2))."""
    s = np.asarray(scores, dtype=np.float64)
    P = s.shape[1]
    mean = _stripe_tree(s) / float(P)
    if two_pass:
        d = s - mean[:, None]
        return mean, np.sqrt(_stripe_tree(d * d) / float(P))
    var = _stripe_tree(s * s) / float(P) - mean * mean
    return mean, np.sqrt(np.maximum(var, 0.0))


N_REF, N_T = 40, 300                               # the small graph: the oracle's Python loop over edges stays cheap
SNN_W = np.round(np.arange(1, 11) / (20.0 - np.arange(1, 11)), 2)       # the ten weights a k = 11 mapping produces


def _null_graph(seed, n_ref=N_REF, n_t=N_T, k=4):
    rng = np.random.default_rng(seed)
    edge_t = np.repeat(np.arange(n_t, dtype=np.int64), k)
    edge_r = rng.integers(0, n_ref, n_t * k)
    w = rng.choice(SNN_W, n_t * k)
    sh = rng.permutation(n_t * k)                  # any order: the device sorts, stably, by reference node
    group = (rng.random(n_t) < 0.3).astype(np.uint8)
    group[:3] = 1
    return edge_t[sh], edge_r[sh], w[sh], group


def _null_rows_graph(seed, equal_w=0.9):
    """Row extremes: node 0 has no edge, node 1 exactly one, node 2 an edge from EVERY pooled cell with weights spanning
    1e-8 .. 1e8 (n_ge is then bit-equal only if the sums run in the caller's order), node 3 an edge of the SAME weight
    from every pooled cell (the narrow null: every permuted score is the same up to rounding), the rest as usual."""
    rng = np.random.default_rng(seed)
    edge_t, edge_r, w, group = _null_graph(seed)
    edge_r = np.where(edge_r < 4, edge_r + 4, edge_r)                   # nodes 0..3 are placed by hand
    cells = np.arange(N_T, dtype=np.int64)
    wide = 10.0 ** rng.uniform(-8, 8, N_T)
    wide[:4] = [1e8, 1e-8, 3e7, 7e-8]
    edge_t = np.concatenate([edge_t, [17], cells, cells])
    edge_r = np.concatenate([edge_r, [1], np.full(N_T, 2), np.full(N_T, 3)])
    w = np.concatenate([w, [0.37], wide, np.full(N_T, equal_w)])
    sh = rng.permutation(edge_t.shape[0])
    return edge_t[sh], edge_r[sh], w[sh], group


def _case(graph, n_perm, key_bits=64, multiplier=1000.0, seed=12345, group=None):
    edge_t, edge_r, w, grp = graph
    return {"edge_t": edge_t, "edge_r": edge_r, "w": w, "group": grp if group is None else group, "n_ref": N_REF,
            "n_perm": n_perm, "key_bits": key_bits, "multiplier": multiplier, "seed": seed}


NULL_N_PERM = [1, 31, 32, 33, 255, 256, 257, 1023, 1024, 2047, 2048, 4095, 4096]
NULL_KEY_BITS = [8, 16, 24, 32, 40, 48, 56, 64]
NARROW = "rows-mult1e6-bits8"      # equal weights from every cell, multiplier 1e6, realised group sizes vary


def nacc_of(n_perm):
    """the null_score_kernel<NACC> instantiation a permutation count runs (null_score_launch)"""
    need = (n_perm + 1 + 255) // 256
    return next(n for n in (1, 2, 4, 8, 17) if need <= n)


def null_cases():
    """{id: case}: every oracle-checked case of the permutation null.  < 5000 edges each."""
    cases = {}
    for P in NULL_N_PERM:
        cases["nperm-%d" % P] = _case(_null_graph(100 + P), P)
    for b in NULL_KEY_BITS:
        cases["bits-%d" % b] = _case(_null_graph(200 + b), 96, key_bits=b, seed=777 + b)
    g = _null_graph(301)
    cases["group-all"] = _case(g, 257, group=np.ones(N_T, dtype=np.uint8))
    one = np.zeros(N_T, dtype=np.uint8)
    one[123] = 1
    cases["group-one"] = _case(g, 257, group=one)
    for mult, name in ((1.0, "1"), (1000.0, "1000"), (1e6, "1e6")):
        cases["rows-mult%s" % name] = _case(_null_rows_graph(400), 300, multiplier=mult)
    cases[NARROW] = _case(_null_rows_graph(401), 257, key_bits=8, multiplier=1e6)
    cases["rows-mult1e6-b"] = _case(_null_rows_graph(401), 300, multiplier=1e6)      # 64-bit keys: that node's sd is 0
    cases["rows-mult1e6-nperm4096"] = _case(_null_rows_graph(402), 4096, multiplier=1e6)
    return cases


def csr_from_edges(edge_r, n_ref):
    """(order, row_ptr): the CSR by reference node a stable host sort gives"""
    edge_r = np.asarray(edge_r, dtype=np.int64)
    order = np.argsort(edge_r, kind="stable")
    rp = np.zeros(n_ref + 1, dtype=np.int64)
    np.cumsum(np.bincount(edge_r, minlength=n_ref), out=rp[1:])
    return order, rp


CSR_N_REF = [1, 2, 3, 255, 256, 257, 65536, 65537]


def csr_edge_lists(n_ref, n_t=500):
    """{style: (edge_t, edge_r, w)} for one n_ref: shuffled over all nodes; every edge on the LAST node; and, where there
    is room, two used nodes with a run of > 1000 empty rows between them (and empty rows before and after)."""
    rng = np.random.default_rng(9000 + n_ref)
    E = 3000
    out = {}
    et = rng.integers(0, n_t, E)
    w = rng.choice(SNN_W, E) * 10.0 ** rng.integers(-3, 4, E)           # order of summation shows in the low bits
    out["shuffled"] = (et, rng.integers(0, n_ref, E), w)
    out["last-node"] = (et, np.full(E, n_ref - 1, dtype=np.int64), w)
    if n_ref > 3000:
        lo, hi = 7, n_ref - 2                                           # rows 8 .. n_ref-3 are empty
        out["gap"] = (et, np.where(rng.random(E) < 0.5, lo, hi).astype(np.int64), w)
    return out


def csr_big_edge_list():
    """>= 300k edges (the radix sort runs several blocks), a few rows with >= 50 edges each among mostly short rows"""
    rng = np.random.default_rng(31337)
    n_ref, n_t, E = 70001, 20000, 320000
    er = rng.integers(0, n_ref, E)
    heavy = np.array([0, 4095, 4096, 65535, 65536, n_ref - 1])
    hit = rng.choice(E, 6 * 80, replace=False)
    er[hit] = np.repeat(heavy, 80)
    et = rng.integers(0, n_t, E)
    w = rng.choice(SNN_W, E) * 10.0 ** rng.integers(-3, 4, E)
    group = (rng.random(n_t) < 0.4).astype(np.uint8)
    group[0] = 1
    assert (np.bincount(er, minlength=n_ref)[heavy] >= 50).all()
    return n_ref, n_t, et, er, w, group


# ---- shard merge ------------------------------------------------------------------------------------------------------
def merge_ref(parts_idx, parts_dist, k, drop_first):
    """nabo_merge_topk from its definition: per row the (dist, idx) pairs with idx >= 0 of all parts, sorted by
    (dist, idx), the positional drop, the first k; positions past the real entries hold idx -1 / dist NaN."""
    parts_idx, parts_dist = np.asarray(parts_idx), np.asarray(parts_dist)
    n_parts, m, kp = parts_idx.shape
    out_i = np.full((m, k), -1, dtype=np.int64)
    out_d = np.full((m, k), np.nan)
    for row in range(m):
        pairs = sorted((float(parts_dist[p, row, s]), int(parts_idx[p, row, s]))
                       for p in range(n_parts) for s in range(kp) if parts_idx[p, row, s] >= 0)
        pairs = pairs[(1 if drop_first else 0):][:k]
        for o, (d, j) in enumerate(pairs):
            out_i[row, o], out_d[row, o] = j, d
    return out_i, out_d


MAX_IDX = 0xFFFFFFFE              # the largest global index the merge carries (0xFFFFFFFF is its "absent")

# (n_parts, kp, m, k, drop_first): n_parts*kp lands in every merge_kernel width (<= 64, 65..128, 129..256, 257..512,
# 513..1024; exactly 64, 65 and 1024 among them), n_parts = 1, kp = 1, k + drop == n_parts*kp, every m of the issue
MERGE_CASES = [
    (1, 1, 1, 1, False), (1, 64, 2, 64, False), (4, 16, 3, 63, True), (3, 7, 777, 11, True),
    (5, 13, 5, 64, True), (65, 1, 3, 30, False), (8, 16, 777, 50, True),
    (3, 56, 5, 56, False), (8, 32, 2, 256, False),
    (9, 32, 3, 287, True), (16, 32, 777, 11, True),
    (17, 32, 5, 57, False), (32, 32, 3, 1023, True), (1024, 1, 1, 1024, False), (1, 1024, 2, 5, True),
]


def merge_width(n_parts, kp):
    """the merge_kernel<NCL, true> instantiation a shape runs (merge_dispatch)"""
    need = (n_parts * kp + 63) // 64
    return next(n for n in (1, 2, 4, 8, 16) if need <= n)


def merge_case(n_parts, kp, m, k, drop_first, seed=0):
    """parts_idx / parts_dist [n_parts, m, kp]: rows sorted in the canonical order, distances from a small lattice (exact
    ties across parts, the tied entries then order by global index), tails of -1 / +inf, parts that are entirely absent,
    global indices up to MAX_IDX.  Row 0 is complete and its smallest distance is shared by two entries (what the
    positional drop then removes is the smaller INDEX); the last row has at most two real entries."""
    rng = np.random.default_rng(seed + 7919 * n_parts + 31 * kp + m)
    total = n_parts * kp
    pi = np.full((n_parts, m, kp), -1, dtype=np.int64)
    pd = np.full((n_parts, m, kp), np.inf)
    for row in range(m):
        pool = np.unique(np.concatenate([rng.integers(0, MAX_IDX + 1, 2 * total + 8, dtype=np.int64),
                                         [MAX_IDX, MAX_IDX - 1, 0]]))
        idx = rng.permutation(pool)[:total]
        if row % 2 == 0 and MAX_IDX not in idx:
            idx[rng.integers(0, total)] = MAX_IDX                       # an index next to the sentinel
        dist = rng.integers(1, max(4, total // 6), total) * 0.25
        if row == 0:
            dist[0] = dist[total - 1] = 0.0                             # first place tied (across parts if n_parts > 1)
        idx, dist = idx.reshape(n_parts, kp), dist.reshape(n_parts, kp)
        for p in range(n_parts):
            if row == 0:
                nreal = kp
            elif row == m - 1:
                nreal = min(kp, 2) if p == n_parts - 1 else 0
            else:
                nreal = [kp, int(rng.integers(0, kp + 1)), 0][int(rng.choice(3, p=[0.5, 0.35, 0.15]))]
            o = np.lexsort((idx[p, :nreal], dist[p, :nreal]))
            pi[p, row, :nreal] = idx[p, :nreal][o]
            pd[p, row, :nreal] = dist[p, :nreal][o]
    return pi, pd


# ---- SNN counts -------------------------------------------------------------------------------------------------------
def snn_ref(t_idx, r_idx, k):
    """out[t, s] = | set(t_idx[t]) & set(r_idx[j]) | for j = t_idx[t, s], entries < 0 removed from both sets first;
    0 when j < 0 or j >= n.  Literal Python sets."""
    t_idx, r_idx = np.asarray(t_idx)[:, :k], np.asarray(r_idx)[:, :k]
    m, n = t_idx.shape[0], r_idx.shape[0]
    rs = [set(int(v) for v in r_idx[j] if v >= 0) for j in range(n)]
    out = np.zeros((m, k), dtype=np.int32)
    for t in range(m):
        a = set(int(v) for v in t_idx[t] if v >= 0)
        for s in range(k):
            j = int(t_idx[t, s])
            if 0 <= j < n:
                out[t, s] = len(a & rs[j])
    return out


SNN_SHAPES = [(10, 700, 11), (2000, 50, 5), (300, 300, 1), (64, 5000, 2), (257, 1000, 50), (33, 400, 100)]
SNN_ABSENT = ["none", "t", "r", "both", "oob"]


def _window_rows(rng, centres, n, k):
    """rows of k DISTINCT indices (drawn without replacement) from a window around each centre, so that the sets of
    nearby rows overlap as k-NN lists do"""
    half = min(max(k + k // 2, 3), n // 2)
    span = np.arange(-half, half)[:n]
    return np.stack([(c + rng.choice(span, k, replace=False)) % n for c in centres]).astype(np.int64)


def snn_case(m, n, k, absent="none", seed=0):
    rng = np.random.default_rng(seed + 1000003 * m + 1009 * n + k)
    r_idx = _window_rows(rng, np.arange(n), n, k)
    t_idx = _window_rows(rng, rng.integers(0, n, m), n, k)

    def cut(a):                                      # every other row ends in 1 .. k entries of -1 (tail lengths cycle)
        a = a.copy()
        for i in range(0, a.shape[0], 2):
            a[i, k - (1 + (i // 2) % k):] = -1
        return a
    if absent in ("t", "both"):
        t_idx = cut(t_idx)
    if absent in ("r", "both"):
        r_idx = cut(r_idx)
    if absent == "oob":                              # target entries past the reference rows: the slot counts nothing
        t_idx = cut(t_idx)
        t_idx[1::2, 0] = n
        t_idx[1::4, k - 1] = n + 5
    return t_idx, r_idx

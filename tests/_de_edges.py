"""Named edge cases of the Mann-Whitney DE step (nabo_de_test, nabo_amd/csrc/de_rank.hip), shared by test_de_cpu.py (the
dense reference against the restatement) and test_de_edges_gpu.py (the device against both).  Every case is fixed and
seeded, and as small as the edge it reaches allows.

A case is a dict: "n_genes", "m1", "m2" (_csc tuples, m2 or None), "set_ptr", "members", "pair_test", "pair_ctrl",
"exp_frac_thresh", "log2_fc_thresh"; `args(case)` gives the device step's arguments.  Optional keys: "default_pairs" (the
pairs are the ABI's default ones: also call it with pair_test NULL), "exact_threshold" (log2_fc sits ON the threshold by
design), "budgets" ({budget in bytes: gene chunks it must give}), "refused" (a word of the error message; the call must
fail and the next one work).

Families (FAMILIES[family] lists the case names):
  runs    la / lb over {0, 1, 2, 63, 64, 65, 127, 128, 129, 200}^2 with heavy ties and with distinct values; tie groups of
          2 .. 70 values that start at sorted positions 60 .. 66 and 126 .. 130 of the test run, of the control run, in
          one run only and in both with different multiplicities; every value equal
  trunc   the n2 largest control values: a cut inside a group of equal values, at a group's edge, an all-zero control
          set, ng < n1, ng = n1, n1 = 1
  zeros   stored 0.0 and -0.0, products that underflow to +0 and -0, subnormal products, a column of stored zeros only,
          an absent column; in the test set, the control set and both
  sets    repeated members, a cell in 3 and in 5 sets, a set in both roles, a set in no pair, an empty control set,
          one set against itself, the default pairs
  two     two matrices of different cell counts, columns empty on one side, the both-roles refusal
  chunks  12 genes with empty ones first, last and in the middle under budgets that give 1 chunk, 1 gene per chunk and
          something between, with one and two matrices; (genes of a chunk) * n_sets at 1, 2, 8, 9, 16, 17
  thresh  exp_frac exactly on its threshold, an all-zero test set, thresholds beyond every value, log2_fc exactly on its
          threshold
  limit   n1 = n2 = 2^20 - 1: the zero block's t^3 just under 2^63; n1 + n2 = 2^21 refused
  exact   the exact p: every 1 <= n2 <= n1 <= 8 at five values of U, n2 = 8 and 7 against large n1 up to the last
          binomial below 2^127, the first one beyond it refused
"""
import math

import numpy as np

LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
NEG_INF = -math.inf


def csc(n_cells, columns, sf=None):
    """_csc tuple of `columns`, a list of {cell: stored value}"""
    ptr, cells, vals = [0], [], []
    for col in columns:
        for c in sorted(col):
            cells.append(c)
            vals.append(col[c])
        ptr.append(len(cells))
    sf = np.ones(n_cells, dtype=np.float32) if sf is None else np.asarray(sf, dtype=np.float32)
    assert sf.shape[0] == n_cells
    return (n_cells, np.array(ptr, dtype=np.int64), np.array(cells, dtype=np.int32), np.array(vals, dtype=np.float32), sf)


def flatten(sets):
    ptr = np.zeros(len(sets) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sets], out=ptr[1:])
    return ptr, np.concatenate([np.asarray(s, dtype=np.int64) for s in sets] + [np.zeros(0, dtype=np.int64)])


def make(m1, sets, pairs, eft, lft, m2=None, **extra):
    set_ptr, members = flatten(sets)
    case = {"n_genes": m1[1].shape[0] - 1, "m1": m1, "m2": m2, "set_ptr": set_ptr, "members": members,
            "pair_test": np.array([p[0] for p in pairs], dtype=np.int32), "pair_ctrl": np.array([p[1] for p in pairs], dtype=np.int32),
            "exp_frac_thresh": eft, "log2_fc_thresh": lft}
    case.update(extra)
    return case


def args(case):
    return (case["n_genes"], case["m1"], case["m2"], case["set_ptr"], case["members"], case["pair_test"], case["pair_ctrl"],
            case["exp_frac_thresh"], case["log2_fc_thresh"])


def two_sets(n1, ng, genes, eft, lft, seed, **extra):
    """test set = cells [0, n1), control set = cells [n1, n1 + ng), one pair; genes: [(stored test values, stored control
    values)], scattered over the set's cells"""
    rng = np.random.default_rng(seed)
    cols = []
    for tv, cv in genes:
        assert len(tv) <= n1 and len(cv) <= ng
        col = {int(c): v for c, v in zip(rng.permutation(n1)[:len(tv)], tv)}
        col.update({n1 + int(c): v for c, v in zip(rng.permutation(ng)[:len(cv)], cv)})
        cols.append(col)
    sets = [rng.permutation(n1).tolist(), (n1 + rng.permutation(ng)).tolist()]
    return make(csc(n1 + ng, cols), sets, [(0, 1)], eft, lft, **extra)


# ---- runs -------------------------------------------------------------------------------------------------------------
def _runs():
    out = {}
    rng = np.random.default_rng(11)
    out["runs_grid_ties"] = two_sets(200, 200, [(rng.integers(1, 6, la).tolist(), rng.integers(2, 8, lb).tolist()) for la in LENS for lb in LENS],
                                     0.0, NEG_INF, 12)
    genes = []
    for la in LENS:
        for lb in LENS:
            v = rng.permutation(400)[:la + lb] + 1
            genes.append((v[:la].tolist(), v[la:].tolist()))
    out["runs_grid_distinct"] = two_sets(200, 200, genes, 0.0, NEG_INF, 13)

    def with_group(start, length, mode):
        """a run of distinct values 1 .. start, then `length` copies of V, then three larger values; the other run: values
        between the integers, and V not at all ("alone") or 3 times ("both")"""
        V = start + 1
        run = list(range(1, start + 1)) + [V] * length + [V + 1, V + 2, V + 3]
        other = [0.5, 1.5, 1.5, start - 0.5, V + 0.5, V + 2.5] + ([V] * 3 if mode == "both" else [])
        return run, other
    starts, lengths = (60, 61, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130), (2, 7, 64, 70)
    a, b = [], []
    for k, s in enumerate(starts):
        for j, ln in enumerate(lengths):
            run, other = with_group(s, ln, "both" if (k + j) % 2 else "alone")
            a.append((run, other))
            b.append((other, run))
    out["runs_groups_in_test"] = two_sets(210, 210, a, 0.0, NEG_INF, 14)
    out["runs_groups_in_control"] = two_sets(210, 210, b, 0.0, NEG_INF, 15)
    # every value equal: with no zero in the pool the variance term is exactly 0
    out["runs_all_equal"] = two_sets(130, 130, [([3.0] * 130, [3.0] * 130), ([3.0] * 64, [3.0] * 65), ([3.0] * 129, [3.0] * 130),
                                               ([3.0] * 130, [])], 0.0, NEG_INF, 16)
    return out


# ---- trunc ------------------------------------------------------------------------------------------------------------
def _trunc():
    out = {}
    test = [2, 2, 3, 5, 5, 7]
    ctrl = [[2] * 6 + [3] * 4 + [5] * 3,            # 13 nonzeros, 10 kept: the cut falls inside the six 2s
            [1] * 3 + [2] * 4 + [3] * 3 + [5] * 3,   # the cut falls at the edge between the 1s and the 2s
            [],                                      # all zeros: control mean 0, log2_fc +inf
            [0.0, 0.0, 0.0],                         # the same with stored zeros
            [2, 3, 3, 9],                            # fewer nonzeros than n2: zeros fill up
            [1, 2, 2, 3, 3, 3, 5, 5, 5, 8],          # exactly n2 nonzeros
            [5] * 25,                                # one group, cut in its middle
            [1] * 15 + [2] * 10]                     # the kept values are exactly the last group
    out["trunc_ng_gt_n1"] = two_sets(10, 25, [(test, c) for c in ctrl] + [([], ctrl[0]), ([4] * 10, ctrl[0])], 0.0, NEG_INF, 21)
    out["trunc_ng_lt_n1"] = two_sets(25, 10, [(test * 3, [2, 3, 3, 9]), (test, [5] * 10), ([1] * 25, []), (test, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10])],
                                     0.0, NEG_INF, 22)
    out["trunc_ng_eq_n1"] = two_sets(12, 12, [(test, [2, 3, 3, 9]), (test * 2, [5] * 12), (test, [2, 2, 3])], 0.0, NEG_INF, 23)
    # n1 = 1 against ng = 1 and ng = 5: cells 0 | 1 | 2 .. 6
    cols = [{0: 3.0, 1: 1.0, 2: 1.0, 3: 5.0, 4: 2.0}, {0: 3.0, 1: 3.0, 3: 3.0, 5: 4.0}, {1: 2.0, 6: 1.0}, {0: 2.0},
            {0: 1.0, 1: 4.0, 2: 4.0, 3: 4.0, 4: 5.0, 5: 6.0, 6: 7.0}]
    out["trunc_n1_is_1"] = make(csc(7, cols), [[0], [1], [4, 2, 6, 3, 5]], [(0, 1), (0, 2)], 0.0, NEG_INF)
    return out


# ---- zeros ------------------------------------------------------------------------------------------------------------
# stored value and the size factor of the cell that holds it; the float32 product is the cell's value
KINDS = {"pos_zero": (0.0, 1.0), "neg_zero": (-0.0, 1.0), "underflow": (1e-30, 1e-30), "neg_underflow": (-1e-30, 1e-30),
         "subnormal": (1e-20, 1e-20), "subnormal_b": (3e-20, 1e-20)}
_SF_OF_CELL = [1.0] * 6 + [1e-20] * 3 + [1e-30] * 3            # the 12 cells of a set


def _zeros():
    def column(test_kinds, ctrl_kinds, normals=(1.0, 2.0, 2.0, 3.0)):
        """the normal values on sf = 1 cells of both sets, then each kind on a cell with its size factor"""
        col = {}
        for base, kinds in ((0, test_kinds), (12, ctrl_kinds)):
            free = {sf: [base + i for i, s in enumerate(_SF_OF_CELL) if s == sf] for sf in set(_SF_OF_CELL)}
            for v in normals:
                col[free[1.0].pop()] = v
            for k in kinds:
                val, sf = KINDS[k]
                col[free[sf].pop()] = val
        return col
    cols = []
    for k in ("pos_zero", "neg_zero", "underflow", "neg_underflow", "subnormal"):
        cols += [column([k], []), column([], [k]), column([k], [k])]
    cols += [column(["subnormal", "subnormal", "subnormal_b"], ["subnormal", "subnormal_b", "neg_zero"]),     # ties among subnormals
             column(["subnormal", "subnormal", "subnormal_b", "underflow"], [], normals=()),             # subnormals against zeros
             column(["pos_zero", "neg_zero", "underflow", "neg_underflow"], ["neg_zero", "pos_zero", "neg_underflow", "underflow"], normals=()),
             {}]                                                                                         # an absent column
    cols.append({c: (1.1754944e-38 if c % 2 else 1e-20) for c in (0, 1, 6, 7, 12, 13, 18, 19)})          # the smallest normal next to subnormals
    sf = np.array(_SF_OF_CELL * 2, dtype=np.float32)
    sets = [[5, 0, 11, 3, 8, 1, 9, 2, 10, 4, 6, 7], list(range(23, 11, -1))]
    m = csc(24, cols, sf)
    return {"zeros_ranked": make(m, sets, [(0, 1), (1, 0)], 0.0, NEG_INF),
            # 3 subnormals of 12 cells are exactly the expressed fraction 0.25: flushed to zero, the gene would be skipped
            "zeros_counted": make(m, sets, [(0, 1), (1, 0)], 0.25, NEG_INF)}


# ---- sets -------------------------------------------------------------------------------------------------------------
def _random_columns(rng, n_cells, n_genes, density=0.5, hi=5):
    return [{int(c): float(rng.integers(1, hi)) for c in np.nonzero(rng.random(n_cells) < density)[0]} for _ in range(n_genes)]


def _sets():
    out = {}
    rng = np.random.default_rng(31)
    m = csc(30, _random_columns(rng, 30, 4))
    sets = [[0, 3, 1, 2, 3, 4, 5, 6, 3, 7, 8, 5, 9],           # cell 3 three times, cell 5 twice
            [14, 5, 6, 7, 8, 9, 10, 11, 12, 13],
            [],                                                # an empty control set between non-empty ones
            [3, 5, 20, 21, 22, 23, 24, 25],
            [27, 3, 5, 9, 26],
            [5, 28, 29, 12],                                   # cell 5 is in sets 0, 1, 3, 4, 5; cell 3 in 0, 3, 4
            [1, 2, 3]]                                         # named in no pair
    out["sets_memberships"] = make(m, sets, [(0, 1), (0, 2), (0, 3), (1, 0), (3, 4), (4, 5), (5, 2), (1, 3), (4, 4)], 0.0, NEG_INF)
    out["sets_one_set_against_itself"] = make(csc(9, _random_columns(rng, 9, 3, 0.7)), [[0, 1, 2, 3, 4, 5, 6, 7, 8, 4]], [(0, 0)], 0.0, NEG_INF)
    sets = [[0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11, 12], [], [13, 14, 15, 16, 17, 18, 19, 20, 21, 0]]
    out["sets_default_pairs"] = make(csc(22, _random_columns(rng, 22, 5)), sets, [(0, 1), (0, 2), (0, 3)], 0.0, NEG_INF, default_pairs=True)
    out["sets_one_set_default_pairs"] = make(csc(4, _random_columns(rng, 4, 2, 0.7)), [[0, 1, 2, 3]], [], 0.0, NEG_INF, default_pairs=True)
    return out


# ---- two matrices -----------------------------------------------------------------------------------------------------
def _two():
    rng = np.random.default_rng(41)
    a, b = _random_columns(rng, 20, 6, 0.6), _random_columns(rng, 33, 6, 0.6)
    b[1], a[2], a[3], b[3] = {}, {}, {}, {}                    # control column empty, test column empty, both empty
    m1, m2 = csc(20, a), csc(33, b, 0.5 + 0.25 * rng.integers(0, 5, 33))
    sets = [list(range(0, 12)), [32, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20, 19, 3], [19, 18, 17, 16, 15, 14, 13, 3, 3],
            list(range(0, 20)), []]
    good = make(m1, sets, [(0, 1), (0, 3), (2, 1), (2, 3), (2, 4)], 0.0, NEG_INF, m2=m2)
    bad = make(m1, sets, [(0, 1), (1, 2)], 0.0, NEG_INF, m2=m2, refused="test in one pair and control in another")
    return {"two_matrices": good, "two_both_roles_refused": bad}


# ---- chunks -----------------------------------------------------------------------------------------------------------
def gene_bytes(case):
    """the device bytes include/nabo_de.h counts for each gene: 16 per nonzero and 24 per (nonzero, set membership) of
    either matrix, the gene's segment pointers and results"""
    n_sets, n_pairs = case["set_ptr"].shape[0] - 1, case["pair_test"].shape[0]
    two = case["m2"] is not None
    fixed = n_sets * 8 + n_pairs * (4 + 5 * 8 + 3 * 8) + 16
    out = np.full(case["n_genes"], fixed, dtype=np.int64)
    for m, roles in ((case["m1"], (case["pair_test"],) if two else (case["pair_test"], case["pair_ctrl"])), (case["m2"], (case["pair_ctrl"],))):
        if m is None:
            continue
        used = set(int(s) for r in roles for s in r)
        per_cell = np.zeros(m[0], dtype=np.int64)
        for s in used:
            np.add.at(per_cell, case["members"][case["set_ptr"][s]:case["set_ptr"][s + 1]], 1)
        for g in range(case["n_genes"]):
            cells = m[2][m[1][g]:m[1][g + 1]]
            out[g] += 16 * cells.shape[0] + 24 * int(per_cell[cells].sum())
    return out


def chunks_under(budget, sizes):
    """how many chunks a greedy fill of the genes, in order, gives"""
    n, used = 0, None
    for b in sizes.tolist():
        if used is None or used + b > budget:
            n, used = n + 1, 0
        used += b
    return n


def _chunks():
    out = {}
    rng = np.random.default_rng(51)
    empty = (0, 5, 11)

    def columns(n_cells, n_listed, skip):
        """every non-empty gene lists the same cells with other values: the genes need the same bytes, so that a budget
        of one gene's bytes puts every gene, the empty ones too, in a chunk of its own"""
        cells = rng.permutation(n_cells)[:n_listed]
        return [{int(c): float(rng.integers(1, 5)) for c in (cells if g not in skip else [])} for g in range(12)]
    sets1 = [list(range(0, 20)), list(range(10, 32)), list(range(25, 40)) + [0, 1]]
    one = make(csc(40, columns(40, 27, empty)), sets1, [(0, 1), (0, 2), (1, 2), (2, 0)], 0.0, NEG_INF)
    # two matrices: gene 3 has keys in matrix 1 only, gene 8 in matrix 2 only, genes 0, 5, 11 in neither
    sets2 = [list(range(0, 20)), list(range(10, 32)), list(range(0, 25)), list(range(20, 50)) + [3, 3]]
    two = make(csc(40, columns(40, 27, empty + (8,))), sets2, [(0, 2), (0, 3), (1, 2), (1, 3)], 0.0, NEG_INF,
               m2=csc(50, columns(50, 31, empty + (3,))))
    for name, case in (("chunks_one_matrix", one), ("chunks_two_matrices", two)):
        sizes = gene_bytes(case)
        big = int(sizes.max())
        case["budgets"] = {1 << 30: 1, big: chunks_under(big, sizes), 5 * big // 2: chunks_under(5 * big // 2, sizes)}
        assert case["budgets"][big] == 12 and 1 < case["budgets"][5 * big // 2] < 12, case["budgets"]
        out[name] = case
    # (genes of a chunk) * n_sets = 1, 2, 8, 9, 16 and 17: the sort's key width at and around a power of two
    for n_seg, n_genes, n_sets in ((1, 1, 1), (2, 1, 2), (2, 2, 1), (8, 4, 2), (9, 3, 3), (16, 4, 4), (17, 17, 1)):
        n_cells = 12 * n_sets
        sets = [list(range(12 * s, 12 * s + 12)) for s in range(n_sets)]
        pairs = [(s, (s + 1) % n_sets) for s in range(n_sets)]
        out["chunks_nseg_%d_%dx%d" % (n_seg, n_genes, n_sets)] = make(csc(n_cells, _random_columns(rng, n_cells, n_genes, 0.6)), sets, pairs, 0.0, NEG_INF)
    return out


# ---- thresholds -------------------------------------------------------------------------------------------------------
def _thresh():
    out = {}
    genes = [([1, 2, 2, 3, 4], [1, 2, 4]), ([1, 2, 2, 3], [1, 2, 4]), ([], [1, 2, 4]), ([], []), ([3] * 20, [1, 1])]
    out["thresh_frac_on_threshold"] = two_sets(20, 20, genes, 0.25, NEG_INF, 61)          # 5 / 20 is tested, 4 / 20 skipped
    out["thresh_all_zero_test_ranked"] = two_sets(20, 20, genes, 0.0, NEG_INF, 61)        # log2_fc -inf and +inf, both ranked
    out["thresh_all_zero_test_skipped"] = two_sets(20, 20, genes, 0.0, 1.0, 61)           # -inf < 1 is skipped, +inf is not
    out["thresh_frac_above_one"] = two_sets(20, 20, genes, 1.5, NEG_INF, 61)
    out["thresh_log2_fc_beyond_all"] = two_sets(20, 20, genes, 0.0, 1e300, 61)            # only +inf passes
    # means exactly 4 and 2: log2_fc is exactly 1.0 and 1.0 < 1.0 is false, so every gene is tested
    genes = [([4, 4, 4, 4], [2, 2, 2, 2]), ([8, 4, 4], [1, 3, 2, 2]), ([16], [8]), ([1, 2, 3, 10], [1, 1, 1, 5])]
    out["thresh_log2_fc_on_threshold"] = two_sets(4, 4, genes, 0.0, 1.0, 62, exact_threshold=True)
    return out


# ---- the int64 limit --------------------------------------------------------------------------------------------------
def _limit():
    n = 1 << 20
    # 7 nonzeros in each set, 6 of them in shared cells: the zero block holds 2 * (2^20 - 8) values, t^3 = 2^63 - 3 * 2^46 + ...
    col = {0: 2.0, 5: 1.0, 77: 2.0, 4096: 3.0, 65535: 3.0, n - 70: 5.0, n - 2: 1.0, n - 1: 4.0}
    m = csc(n, [col])
    near = make(m, [np.arange(0, n - 1), np.arange(1, n)], [(0, 1), (1, 0)], 0.0, NEG_INF)
    at = make(m, [np.arange(0, n), np.arange(0, n)], [(0, 1)], 0.0, NEG_INF, refused="pools 2097152 values")
    return {"limit_just_below": near, "limit_reached_refused": at}


# ---- the exact p ------------------------------------------------------------------------------------------------------
def arrangement(n1, n2, u1):
    """(test ranks, control ranks), together 1 .. n1 + n2, with #{(test, control): test > control} = u1"""
    assert 0 <= u1 <= n1 * n2
    full, rem = divmod(u1, n2)
    below = [0] * (n1 - full - (1 if rem else 0)) + ([rem] if rem else []) + [n2] * full      # controls below each test value
    test, ctrl, pos = [], [], 0
    for b in below:
        while len(ctrl) < b:
            pos += 1
            ctrl.append(pos)
        pos += 1
        test.append(pos)
    while len(ctrl) < n2:
        pos += 1
        ctrl.append(pos)
    return test, ctrl


def _exact_case(combos, levels_of, seed, zero_of=lambda k: k % 2 == 1):
    """one pair of disjoint sets per (n1, n2); gene j puts pair k at U1 = levels_of(n1, n2)[j].  With zero_of(k) the
    lowest rank is a cell the column does not list: the one zero of the pool"""
    rng = np.random.default_rng(seed)
    sets, pairs, base = [], [], 0
    for n1, n2 in combos:
        sets += [base + rng.permutation(n1), base + n1 + rng.permutation(n2)]
        pairs.append((len(sets) - 2, len(sets) - 1))
        base += n1 + n2
    n_genes = len(levels_of(*combos[0]))
    cols = [dict() for _ in range(n_genes)]
    for k, (n1, n2) in enumerate(combos):
        for j, u1 in enumerate(levels_of(n1, n2)):
            test, ctrl = arrangement(n1, n2, u1)
            shift = 1 if zero_of(k) else 0
            for cells, ranks in ((sets[2 * k], test), (sets[2 * k + 1], ctrl)):
                for c, r in zip(cells.tolist(), ranks):
                    if r - shift:
                        cols[j][c] = float(r - shift)
    return make(csc(base, cols), sets, pairs, 0.0, NEG_INF)


def _exact():
    small = [(n1, n2) for n1 in range(1, 9) for n2 in range(1, n1 + 1)]
    out = {"exact_sweep_to_8": _exact_case(small, lambda a, b: (0, a * b, a * b // 2, a * b // 4, a * b - max(1, a * b // 3)), 71)}
    big = [(9, 8), (1000, 8), (174439, 8), (174440, 8), (226220, 8), (300000, 7)]
    out["exact_large_n1"] = _exact_case(big, lambda a, b: (a * b - 3, 17), 72)
    out["exact_binomial_beyond_refused"] = _exact_case([(226221, 8)], lambda a, b: (a * b - 3,), 73, zero_of=lambda k: False)
    out["exact_binomial_beyond_refused"]["refused"] = "226221 and 8"
    return out


FAMILY_BUILDERS = {"runs": _runs, "trunc": _trunc, "zeros": _zeros, "sets": _sets, "two": _two, "chunks": _chunks, "thresh": _thresh,
                   "limit": _limit, "exact": _exact}
# the names are fixed here so that collecting the tests builds nothing
FAMILIES = {
    "runs": ["runs_grid_ties", "runs_grid_distinct", "runs_groups_in_test", "runs_groups_in_control", "runs_all_equal"],
    "trunc": ["trunc_ng_gt_n1", "trunc_ng_lt_n1", "trunc_ng_eq_n1", "trunc_n1_is_1"],
    "zeros": ["zeros_ranked", "zeros_counted"],
    "sets": ["sets_memberships", "sets_one_set_against_itself", "sets_default_pairs", "sets_one_set_default_pairs"],
    "two": ["two_matrices", "two_both_roles_refused"],
    "chunks": ["chunks_one_matrix", "chunks_two_matrices", "chunks_nseg_1_1x1", "chunks_nseg_2_1x2", "chunks_nseg_2_2x1", "chunks_nseg_8_4x2",
               "chunks_nseg_9_3x3", "chunks_nseg_16_4x4", "chunks_nseg_17_17x1"],
    "thresh": ["thresh_frac_on_threshold", "thresh_all_zero_test_ranked", "thresh_all_zero_test_skipped", "thresh_frac_above_one",
               "thresh_log2_fc_beyond_all", "thresh_log2_fc_on_threshold"],
    "limit": ["limit_just_below", "limit_reached_refused"],
    "exact": ["exact_sweep_to_8", "exact_large_n1", "exact_binomial_beyond_refused"],
}
_built = {}


def family_of(name):
    return [f for f, names in FAMILIES.items() if name in names][0]


def case(name):
    """the case `name`; a family is built once, on first use"""
    fam = family_of(name)
    if fam not in _built:
        _built[fam] = FAMILY_BUILDERS[fam]()
        assert sorted(_built[fam]) == sorted(FAMILIES[fam]), fam
    return _built[fam][name]


def all_names(refused=False):
    """the cases that compute (refused = False) or the ones the library must refuse"""
    return [n for names in FAMILIES.values() for n in names if n.endswith("_refused") == refused]

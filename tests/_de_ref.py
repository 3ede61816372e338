"""Plain numpy restatement of the Mann-Whitney DE step (include/nabo_de.h; nabo/_marker.py:69-102 with scipy >= 1.7's
mannwhitneyu), the tests' stand-in for the device: no scipy, no GPU.  It is checked against the reference's own tables
(tests/golden/de.npz, tools/gen_golden_de.py) in test_de_cpu.py, and the device against it in test_de_gpu.py.

It works on a gene's dense float32 vector, as the reference does, and ranks with numpy's sort / searchsorted / unique;
the device never builds that vector."""
import json
import math

import numpy as np

SKIP_GENE, SKIP_PAIR, ASYMPTOTIC, EXACT, EMPTY = 0, 1, 2, 3, 4
FIELDS = (("status", np.int32), ("nonzero_test", np.int64), ("n1", np.int64), ("n2", np.int64), ("u2", np.int64), ("tie", np.int64),
          ("log2_fc", np.float64), ("z", np.float64), ("pval", np.float64), ("rbc", np.float64))
SQRTH = 0.7071067811865476


def exact_p(n1, n2, u2):
    """2 * P(U >= max(U1, U2)) for samples without ties, clipped to 1: the number of arrangements with U = k is the
    coefficient of q^k in prod_{i=1..m} (1 - q^(n+i)) / (1 - q^i); Python integers, so exact"""
    m, n = min(n1, n2), max(n1, n2)
    K = m * n - max(u2, 2 * m * n - u2) // 2
    f = [0] * (K + 1)
    f[0] = 1
    for i in range(1, m + 1):
        for k in range(K, n + i - 1, -1):
            f[k] -= f[k - n - i]
        for k in range(i, K + 1):
            f[k] += f[k - i]
    return min(1.0, 2.0 * (sum(f) / math.comb(m + n, m)))


def z_of(n1, n2, u2, tie):
    """scipy's _get_mwu_z with continuity correction, operation by operation, for U = max(U1, U2)"""
    n1n2 = float(n1 * n2)
    u1 = u2 / 2.0
    u = max(u1, n1n2 - u1)
    mu = n1n2 / 2.0
    n = n1 + n2
    s = math.sqrt(n1n2 / 12.0 * (float(n + 1) - float(np.float64(np.int64(tie))) / float(n * (n - 1))))
    num = u - mu
    num -= 0.5
    with np.errstate(divide="ignore"):
        return float(np.float64(num) / np.float64(s))


def p_of(z):
    return min(1.0, math.erfc(z * SQRTH))


def dense_column(m, g):
    n_cells, gene_ptr, cell, val, sf = m
    a = np.zeros(n_cells, dtype=np.float32)
    e0, e1 = int(gene_ptr[g]), int(gene_ptr[g + 1])
    a[cell[e0:e1]] = val[e0:e1]
    return a * sf


def de_step(n_genes, m1, m2, set_ptr, members, pair_test, pair_ctrl, exp_frac_thresh, log2_fc_thresh):
    """the device step's contract: m1 / m2 are (n_cells, gene_ptr, cell, val float32, sf float32), m2 or None"""
    n_pairs = len(pair_test)
    out = {k: np.zeros((n_genes, n_pairs), dtype=t) for k, t in FIELDS}
    sets = [np.asarray(members[int(set_ptr[s]):int(set_ptr[s + 1])], dtype=np.int64) for s in range(len(set_ptr) - 1)]
    for g in range(n_genes):
        col1 = dense_column(m1, g)
        col2 = col1 if m2 is None else dense_column(m2, g)
        runs = {}

        def run(s, col, tag):
            if (s, tag) not in runs:
                x = col[sets[s]]
                runs[(s, tag)] = np.sort(x[x != 0])
            return runs[(s, tag)]
        for p in range(n_pairs):
            ts, cs = int(pair_test[p]), int(pair_ctrl[p])
            A = run(ts, col1, 1)
            n1, ng = len(sets[ts]), len(sets[cs])
            n2 = min(n1, ng)
            o = {"nonzero_test": len(A), "n1": n1, "n2": n2}
            if len(A) / n1 < exp_frac_thresh:
                o["status"] = SKIP_GENE
            elif ng == 0:
                o["status"], o["log2_fc"] = EMPTY, np.nan
            else:
                B = run(cs, col2, 2)
                B = B[len(B) - min(len(B), n2):]
                z1, zc = n1 - len(A), n2 - len(B)
                mean_a, mean_b = A.astype(np.float64).sum() / n1, B.astype(np.float64).sum() / n2
                with np.errstate(divide="ignore"):
                    lfc = np.inf if mean_b == 0 else float(np.log2(mean_a) - np.log2(mean_b))
                o["log2_fc"] = lfc
                if lfc < log2_fc_thresh:
                    o["status"] = SKIP_PAIR
                else:
                    lo, hi = np.searchsorted(B, A, "left"), np.searchsorted(B, A, "right")
                    u2 = int((2 * (zc + lo) + (hi - lo)).sum()) + z1 * zc
                    t = [int(x) for x in np.unique(np.concatenate([A, B]), return_counts=True)[1]] + [z1 + zc]
                    tie = sum(x ** 3 - x for x in t)
                    o["u2"], o["tie"] = u2, tie
                    o["z"] = z_of(n1, n2, u2, tie)
                    o["rbc"] = 1 - u2 / (n1 * n2)
                    if (n1 <= 8 or n2 <= 8) and tie == 0:
                        o["status"], o["pval"] = EXACT, exact_p(n1, n2, u2)
                    else:
                        o["status"], o["pval"] = ASYMPTOTIC, p_of(o["z"])
            for k, v in o.items():
                out[k][g, p] = v
    return out


def csc_of(d, prefix):
    """the _csc tuple of a matrix stored in de.npz under `prefix`"""
    sf = np.asarray(d[prefix + "_sf"], dtype=np.float32)
    return (sf.shape[0], np.asarray(d[prefix + "_gene_ptr"], dtype=np.int64), np.asarray(d[prefix + "_cell"], dtype=np.int32),
            np.asarray(d[prefix + "_val"], dtype=np.float32), sf)


def golden_cases(d):
    return json.loads(str(d["cases"]))


def table_rows(table):
    """{(gene, versus_group): (exp_frac, rbc, log2_fc, pval, qval)} of a dict of columns or a DataFrame"""
    cols = {k: list(table[k]) for k in ("gene", "versus_group", "test_group", "exp_frac", "rbc", "log2_fc", "pval", "qval")}
    keys = list(zip(cols["gene"], cols["test_group"], cols["versus_group"]))
    assert len(set(keys)) == len(keys)
    return {k: tuple(float(cols[c][i]) for c in ("exp_frac", "rbc", "log2_fc", "pval", "qval")) for i, k in enumerate(keys)}


def same(a, b, tol_abs=0.0, tol_rel=0.0):
    """equal, NaN and inf included, within the tolerance"""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= tol_abs + tol_rel * abs(b)


def compare_tables(got, want, log2fc_tol, p_rel):
    """differences between a table of this build and the reference's: the row set, exp_frac and rbc exactly, log2_fc
    within log2fc_tol absolute, pval and qval within p_rel relative; and this build's order by (qval, emission)"""
    g, w = table_rows(got), table_rows(want)
    bad = []
    if set(g) != set(w):
        return ["row sets differ: %d extra, %d missing" % (len(set(g) - set(w)), len(set(w) - set(g)))]
    for k in w:
        (ef, rbc, lfc, p, q), (ef_, rbc_, lfc_, p_, q_) = g[k], w[k]
        if ef != ef_ or not same(rbc, rbc_):
            bad.append((k, "exp_frac / rbc", g[k], w[k]))
        elif not same(lfc, lfc_, tol_abs=log2fc_tol):
            bad.append((k, "log2_fc", lfc, lfc_))
        elif not same(p, p_, tol_rel=p_rel) or not same(q, q_, tol_rel=p_rel):
            bad.append((k, "pval / qval", (p, q), (p_, q_)))
    q, tg = [float(x) for x in got["qval"]], list(got["test_group"])
    if any(b < a and s == t for a, b, s, t in zip(q, q[1:], tg, tg[1:])):
        bad.append("a test group's rows are not sorted by qval")
    return bad


def valid_genes(d, prefix, prefix2):
    """the genes run_de_test loops over: the kept genes of the first dataset, with a second one only those it names"""
    names = [str(x) for x in d[prefix + "_genes"]]
    other = None if prefix2 is None else set(str(x) for x in d[prefix2 + "_genes"])
    out = {}
    for i in d[prefix + "_keep"].tolist():
        if other is None or names[i] in other:
            out[names[i]] = None
    return list(out)


def select_columns(d, prefix, genes):
    """the _csc tuple of the columns `genes` (names, in that order) of the matrix stored under `prefix`"""
    n_cells, ptr, cell, val, sf = csc_of(d, prefix)
    names = [str(x) for x in d[prefix + "_genes"]]
    sel = [names.index(g) for g in genes]
    gp = np.concatenate([[0], np.cumsum([ptr[j + 1] - ptr[j] for j in sel])]).astype(np.int64)
    return (n_cells, gp, np.concatenate([cell[ptr[j]:ptr[j + 1]] for j in sel] + [np.zeros(0, np.int32)]),
            np.concatenate([val[ptr[j]:ptr[j + 1]] for j in sel] + [np.zeros(0, np.float32)]), sf)


def case_inputs(d, case):
    """(genes, m1, m2, test cell indices, control index groups) of a golden case; an unknown cell raises KeyError"""
    ci_a = {str(x): i for i, x in enumerate(d[case["d1"] + "_cells"])}
    ci_b = ci_a if case["d2"] is None else {str(x): i for i, x in enumerate(d[case["d2"] + "_cells"])}
    genes = valid_genes(d, case["d1"], case["d2"])
    m1 = select_columns(d, case["d1"], genes)
    m2 = None if case["d2"] is None else select_columns(d, case["d2"], genes)
    return genes, m1, m2, [ci_a[x] for x in case["test_cells"]], [[ci_b[x] for x in grp] for grp in case["control_cells"]]


def check_cases(d, step, log2fc_tol, p_rel):
    """every golden run_de_test case through nabo_amd's host logic with `step` as the device step; returns the number of
    reference rows matched"""
    from nabo_amd import _de
    rows = 0
    for case in golden_cases(d):
        try:
            genes, m1, m2, test_idx, groups = case_inputs(d, case)
            got = _de._de_from_csc(genes, m1, m2, test_idx, groups, case["test_label"], case["labels"], case["exp_frac_thresh"],
                                   case["log2_fc_thresh"], 2, step)
            res = "ok"
        except (ZeroDivisionError, KeyError) as e:
            res = type(e).__name__
        assert res == case["result"], (case["name"], res, case["result"])
        if res == "ok":
            bad = compare_tables(got, case["table"], log2fc_tol, p_rel)
            assert not bad, (case["name"], bad[:5])
            assert got["log2_fc"].dtype == np.float32 and got["qval"].dtype == np.float64
            rows += len(case["table"]["gene"])
    return rows


def check_markers(d, step, log2fc_tol, p_rel):
    from nabo_amd import _de
    rows = 0
    genes = valid_genes(d, "d1", None)
    m1 = select_columns(d, "d1", genes)
    ci = {str(x): i for i, x in enumerate(d["d1_cells"])}
    for key in ("markers", "markers_clamped"):
        c = json.loads(str(d[key]))
        calls = []

        def counted(*a):
            calls.append(len(a[5]))
            return step(*a)
        table, de_genes = _de._markers_from_csc(c["clusters"], genes, m1, c["de_frequency"], c["exp_frac_thresh"], c["log2_fc_thresh"],
                                                c["qval_thresh"], ci, counted)
        assert calls == [12], calls                              # ONE device step: 4 clusters, each against the 3 others
        bad = compare_tables(table, c["table"], log2fc_tol, p_rel)
        assert not bad, (key, bad[:5])
        assert {str(k): sorted(v) for k, v in de_genes.items()} == {k: sorted(v) for k, v in c["de_genes"].items()}, key
        assert list(de_genes) == sorted(de_genes)
        # the per-cluster tables follow each other in sorted cluster order
        groups = [x for i, x in enumerate(table["test_group"]) if i == 0 or table["test_group"][i - 1] != x]
        assert groups == sorted(set(c["table"]["test_group"]), key=groups.index) and len(groups) == len(set(groups))
        rows += len(c["table"]["gene"])
    return rows

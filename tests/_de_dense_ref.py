"""The Mann-Whitney DE step (include/nabo_de.h) from its definition, for the edge suite: numpy, Python integers and
`decimal`; no scipy, no GPU.

tests/_de_ref.py::de_step is the kernel's own decomposition (drop the zeros, sort, search one run in the other, add the
zero blocks).  This one never separates zeros from the rest.  Per gene and pair it builds the dense float32 column
`a * sf`, indexes it with the set's members (repeats included), keeps the min(n1, ng) largest control values by
sorting the dense control vector, pools the two samples and ranks the pool: a value with `less` pooled values below it
in a tie group of t has the doubled tie-averaged rank 2 * less + t + 1.  Then

    u2  = 2 * R1 - n1 * (n1 + 1)        R1 the rank sum of the test sample
    tie = sum of t^3 - t                over np.unique's counts of the pooled dense vector, zeros inside it

in Python integers.  nonzero_test counts `x != 0` (a subnormal is nonzero, -0.0 is not), and the statuses follow the
header.

z.  The header's formula is evaluated in `decimal` at 50 digits from the exact integers.  What the float64 operations of
the header can lose against it, u = 2^-53, first order: n1 n2, u2 / 2, max(U1, U2), n1 n2 / 2, their difference and the
- 0.5 are exact (half-integers below 2^53), and so is n (n - 1).  That leaves
    q = fl(fl(tie) / (n (n - 1)))                    conversion and quotient: 2u relative to q
    d = fl((n + 1) - q)                              q's error grows by q / d = kappa - 1, the subtraction adds u
    s = sqrt(fl(fl(n1 n2 / 12) * d))                 quotient u, product u; the root halves what came before, adds u
    z = fl(num / s)                                  u
with kappa = (n + 1) / ((n + 1) - tie / (n (n - 1))): in all ((kappa - 1) 2u + 3u) / 2 + 2u = (kappa + 2.5) u.  The
bound asked of the kernel is (kappa + 4) u: the remainder covers the second-order terms.  When the variance term is
exactly 0 (every pooled value equal, tie = n^3 - n) the kernel must return z = -inf and p = 1.

p.  For an asymptotic pair min(1, math.erfc(z * SQRTH)) of the z THE KERNEL RETURNED, within the p bound of
test_de_cpu.tolerances (the host's libm erfc on both sides).  For an exact pair _de_ref.exact_p (Python integers, one
correctly rounded division) within 4u: the C code converts two 128-bit integers to double (u each) and divides (u).

log2_fc.  log2 of the math.fsum means (correctly rounded sums), within the log2_fc bound of test_de_cpu.tolerances.
"""
import decimal
import math

import numpy as np

import _de_ref as dref

U = 2.0 ** -53
P_EXACT_REL = 4 * U
CTX = decimal.Context(prec=50)


def z_exact(n1, n2, u2, tie):
    """(z as a Decimal or None when the variance term is exactly 0, kappa as a float or inf)"""
    D = decimal.Decimal
    n = n1 + n2
    n1n2 = D(n1 * n2)
    u = max(D(u2) / 2, n1n2 - D(u2) / 2)
    var = CTX.subtract(D(n + 1), CTX.divide(D(tie), D(n * (n - 1))))
    if var == 0:
        return None, math.inf
    kappa = float(CTX.divide(D(n + 1), var))
    s = CTX.sqrt(CTX.multiply(CTX.divide(n1n2, D(12)), var))
    return CTX.divide(u - n1n2 / 2 - D("0.5"), s), kappa


def z_bound(kappa):
    return (kappa + 4) * U


def log2_fc_of(x, y):
    """log2(mean x) - log2(mean y) from correctly rounded sums; +inf when the control mean is 0"""
    ma = math.fsum(float(v) for v in x) / len(x)
    mb = math.fsum(float(v) for v in y) / len(y)
    if mb == 0:
        return math.inf
    if ma == 0:
        return -math.inf
    return math.log2(ma) - math.log2(mb)


def dense_pair(x, y_all, exp_frac_thresh, log2_fc_thresh):
    """one (gene, pair): x the test sample, y_all the whole control set, dense float32 vectors.  Returns a dict with
    Python values; "z" is a Decimal (None: must be -inf) and "kappa" its amplification"""
    n1, ng = len(x), len(y_all)
    n2 = min(n1, ng)
    o = {"nonzero_test": int(np.count_nonzero(x != 0)), "n1": n1, "n2": n2, "status": None}
    if o["nonzero_test"] / n1 < exp_frac_thresh:
        o["status"] = dref.SKIP_GENE
        return o
    if ng == 0:
        o["status"], o["log2_fc"] = dref.EMPTY, math.nan
        return o
    y = np.sort(y_all, kind="stable")[ng - n2:]                 # the n2 largest of the dense control vector
    o["log2_fc"] = log2_fc_of(x, y)
    if o["log2_fc"] < log2_fc_thresh:
        o["status"] = dref.SKIP_PAIR
        return o
    pooled = np.concatenate([x, y])
    _, inv, counts = np.unique(pooled, return_inverse=True, return_counts=True)
    counts = [int(c) for c in counts]
    rank2, less = [], 0
    for t in counts:                                             # doubled tie-averaged rank of each tie group
        rank2.append(2 * less + t + 1)
        less += t
    r1 = sum(rank2[j] for j in np.asarray(inv).reshape(-1)[:n1].tolist())
    o["u2"] = r1 - n1 * (n1 + 1)
    o["tie"] = sum(t ** 3 - t for t in counts)
    o["z"], o["kappa"] = z_exact(n1, n2, o["u2"], o["tie"])
    o["rbc"] = 1 - o["u2"] / (n1 * n2)
    o["status"] = dref.EXACT if (n1 <= 8 or n2 <= 8) and o["tie"] == 0 else dref.ASYMPTOTIC
    return o


def dense_step(n_genes, m1, m2, set_ptr, members, pair_test, pair_ctrl, exp_frac_thresh, log2_fc_thresh):
    """[gene][pair] -> dense_pair's dict, for the arguments of the device step"""
    sets = [np.asarray(members[int(set_ptr[s]):int(set_ptr[s + 1])], dtype=np.int64) for s in range(len(set_ptr) - 1)]
    out = []
    for g in range(n_genes):
        col1 = dref.dense_column(m1, g)
        col2 = col1 if m2 is None else dref.dense_column(m2, g)
        out.append([dense_pair(col1[sets[int(t)]], col2[sets[int(c)]], exp_frac_thresh, log2_fc_thresh)
                    for t, c in zip(pair_test, pair_ctrl)])
    return out


def check_against_dense(got, want, log2fc_tol, p_rel, what, exact_p_of=dref.exact_p):
    """a step's arrays `got` (the device's, or the restatement's) against dense_step's `want`: status and integers
    exactly, rbc exactly, z within its bound (or -inf), p and log2_fc as the module's docstring says; entries a status
    leaves out are 0.  Returns the largest z error in units of its bound."""
    worst = 0.0
    for g, row in enumerate(want):
        for p, w in enumerate(row):
            at = (what, g, p)
            st = int(got["status"][g, p])
            assert st == w["status"], (at, "status", st, w["status"])
            for k in ("nonzero_test", "n1", "n2"):
                assert int(got[k][g, p]) == w[k], (at, k, int(got[k][g, p]), w[k])
            lfc, z, pv = float(got["log2_fc"][g, p]), float(got["z"][g, p]), float(got["pval"][g, p])
            if st in (dref.SKIP_GENE, dref.SKIP_PAIR, dref.EMPTY):
                for k in ("u2", "tie", "z", "pval", "rbc"):
                    assert got[k][g, p] == 0, (at, k, "must be 0 for status %d" % st)
                if st == dref.SKIP_GENE:
                    assert lfc == 0.0, at
                elif st == dref.EMPTY:
                    assert math.isnan(lfc), at
                else:
                    assert dref.same(lfc, w["log2_fc"], tol_abs=log2fc_tol), (at, "log2_fc", lfc, w["log2_fc"])
                continue
            assert int(got["u2"][g, p]) == w["u2"] and int(got["tie"][g, p]) == w["tie"], \
                (at, "u2 / tie", int(got["u2"][g, p]), w["u2"], int(got["tie"][g, p]), w["tie"])
            assert float(got["rbc"][g, p]) == w["rbc"], (at, "rbc")
            assert dref.same(lfc, w["log2_fc"], tol_abs=log2fc_tol), (at, "log2_fc", lfc, w["log2_fc"])
            if w["z"] is None:
                assert z == -math.inf and pv == 1.0, (at, "zero variance", z, pv)
            else:
                assert math.isfinite(z), (at, "z", z)
                err = abs(CTX.subtract(decimal.Decimal(z), w["z"]))
                bound = decimal.Decimal(z_bound(w["kappa"])) * abs(w["z"])
                assert err <= bound, (at, "z", z, str(w["z"]), w["kappa"])
                if bound > 0:
                    worst = max(worst, float(err / bound))
            if st == dref.ASYMPTOTIC:
                q = dref.p_of(z)
                assert abs(pv - q) <= p_rel * q, (at, "pval", pv, q)
            else:
                q = exact_p_of(w["n1"], w["n2"], w["u2"])
                assert abs(pv - q) <= P_EXACT_REL * q, (at, "exact pval", pv, q)
    return worst

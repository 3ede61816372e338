"""Plain numpy / Python restatement of the contract of nabo_amd/csrc/refine.hip, one function per launcher with the
launcher's own arguments, and the builder of the cases tests/test_refine_gpu.py runs (tests/test_refine_ref_cpu.py checks
both on the CPU).

Distances come from oracle.pairwise (the literal float64 restatement; the device must match it bit for bit), order is
(distance, index).  Every verdict is restated in the kernel's operation order on Python floats: IEEE float64, one
rounding per operation, no FMA.  Thresholds are float32 (np.float32), as the filter hands them over.

Every verdict carries a `margin`: the relative distance of the two sides of the comparison that decided it, 0 where the
comparison is between exactly representable values (counts, indices, +inf, a distance against the plateau value g).
The cases keep every inexact comparison at least MARGIN away from equality, so the device has no excuse to differ.
"""
import functools
import math
import types

import numpy as np

import oracle

PAD = 0xFFFFFFFF
INF = float("inf")
F32 = np.float32
MARGIN = 1e-9
TAU_SCALE = 2.0 ** -6


# ---- float32 helpers ---------------------------------------------------------------------------------------------
def f32_up(v):
    """smallest float32 >= v"""
    f = F32(v)
    return f if float(f) >= v else np.nextafter(f, F32(np.inf))


def f32_down(v):
    """largest float32 <= v"""
    f = F32(v)
    return f if float(f) <= v else np.nextafter(f, F32(-np.inf))


def f32_step(f, n):
    """n float32 steps up (n > 0) or down (n < 0)"""
    f = F32(f)
    for _ in range(abs(n)):
        f = np.nextafter(f, F32(np.inf if n > 0 else -np.inf))
    return f


def ulp32(f):
    f = abs(F32(f))
    return float(np.nextafter(f, F32(np.inf))) - float(f)


def rel(a, b):
    if a == b:
        return 0.0
    if math.isinf(a) or math.isinf(b) or a != a or b != b:
        return INF
    return abs(a - b) / max(abs(a), abs(b))


def pairwise(X, Y, metric, f=0.25):
    X, Y = np.atleast_2d(X), np.atleast_2d(Y)
    if X.shape[0] == 0 or Y.shape[0] == 0:
        return np.zeros((X.shape[0], Y.shape[0]))
    return oracle.pairwise(X, Y, metric, f)


def err_coef_one_product(g):
    """rounding-error coefficient of l2_refine (nabo_amd/csrc/query.hip) for the one-product pass at g components"""
    kc = 2 * ((g + 3 + 31) // 32)
    return 1.05 * ((16.0 * kc + 8.0) * 2.0 ** -24 + 2.0 ** -20 + 2.0 ** -21)


def cb_constants(g):
    """cbf_constants (nabo_amd/csrc/canberra_f32.hip) in float32 arithmetic: (slack, plateau)"""
    s = F32(g) * (F32(g) + F32(2.0)) * F32(5.9604644775390625e-08)
    return s, F32(g) - s


# ---- the verdict of one row ----------------------------------------------------------------------------------------
def verdict(metric, nreal, kk, dk, ie, taus, last, n_valid_total, xn, err_coef, ymax_sqrt, tau_scale, g, plateau):
    """(certified, branch, margin) of a row with nreal real candidates, k'-th exact distance dk at index ie (None when
    nreal < k'), thresholds taus (float32 [S]) and `last` = entry L - 1 of every list (uint32 [S])."""
    if nreal < kk:
        ok = nreal >= n_valid_total
        return ok, "short_ok" if ok else "short_fail", 0.0
    tmin = F32(np.min(np.asarray(taus, dtype=F32)))
    if tmin == F32(np.inf):
        ok = nreal >= n_valid_total
        return ok, "inf_ok" if ok else "inf_fail", 0.0
    if metric == 1:
        t = float(tmin)
        if t > dk:
            return True, "plateau_near" if tmin == plateau else "cert", rel(t, dk)
        if tmin != plateau:
            return False, "fail", rel(t, dk)
        if dk < float(g):
            return True, "plateau_near", rel(dk, float(g))
        pmin = PAD
        for s in range(len(taus)):
            if F32(taus[s]) == plateau:
                pmin = min(pmin, int(last[s]))
        ok = int(ie) <= pmin
        return ok, "plateau_le" if ok else "plateau_gt", 0.0
    sx = math.sqrt(xn) if xn == xn else xn
    E = err_coef * (sx + ymax_sqrt) * (sx + ymax_sqrt)
    bound = (float(tmin) * tau_scale + xn - E) * (1.0 - 1e-12)
    if metric == 2:
        lhs, rhs = 0.5 * bound - 2e-13, dk
    else:
        lhs, rhs = bound, dk * dk * (1.0 + 1e-12)
    ok = lhs > rhs
    return ok, "cert" if ok else "fail", rel(lhs, rhs)


def lower_seed(seed, dk, tau_scale):
    """a fail_seed lowered by max(16 float32 ulps, 1e-9 dk^2 / tau_scale): must no longer certify its row"""
    return f32_down(float(seed) - max(16.0 * ulp32(seed), 1e-9 * dk * dk / tau_scale))


def _sorted_candidates(cand_row, drow):
    c = np.asarray(cand_row, dtype=np.uint32)
    real = c[c != PAD].astype(np.int64)
    d = drow[real]
    o = np.lexsort((real, d))
    return real[o], d[o]


def _tail(oi, od, drow, masked_list, n_masked_list, n_valid, k, drop, base):
    """positions n_valid .. k' - 1 of the order row: the masked references in index order with their true distances,
    then -1 / NaN"""
    for p in range(n_valid, k + drop):
        o, q = p - drop, p - n_valid
        if o < 0:
            continue
        if q < n_masked_list:
            j = int(masked_list[q])
            oi[o], od[o] = base + j, drow[j]
        else:
            oi[o], od[o] = -1, np.nan


def refine(X, row0, m, Y, g, cand_idx, cand_tau, S, L, xnorm, err_coef, ymax_sqrt, tau_scale, k, drop, base,
           n_valid_total, masked_list, n_masked_list, metric, cb_f=0.25, cb_plateau=F32(0.0), D=None, want_seed=True):
    """refine_launch.  cand_idx [m - row0][S * L], cand_tau [m - row0][S] are local to the launch; xnorm is indexed by
    the row itself.  Returns per local row: certified, branch, margin, dk, idx / dist (k outputs, meaningful where
    certified) and seed_lo: for a Euclidean / cosine row that failed with nreal >= k' and a finite threshold, the
    smallest float32 threshold that certifies it (the device's fail_seed is admissible in [seed_lo, any value whose
    lower_seed() lies below seed_lo]); +inf otherwise."""
    rows = m - row0
    if D is None:
        D = pairwise(X[row0:m], Y, metric, cb_f)
    kk = k + drop
    cand_idx = np.asarray(cand_idx, dtype=np.uint32).reshape(rows, S * L)
    cand_tau = np.asarray(cand_tau, dtype=F32).reshape(rows, S)
    out = types.SimpleNamespace(certified=np.zeros(rows, dtype=bool), branch=[None] * rows, margin=np.zeros(rows),
                                dk=np.full(rows, np.nan), idx=np.full((rows, k), -7, dtype=np.int64),
                                dist=np.full((rows, k), -7.0), seed_lo=np.full(rows, np.inf, dtype=F32))
    for r in range(rows):
        ci, cd = _sorted_candidates(cand_idx[r], D[r])
        nreal = ci.shape[0]
        dk = float(cd[kk - 1]) if nreal >= kk else None
        ie = int(ci[kk - 1]) if nreal >= kk else None
        xn = float(xnorm[row0 + r]) if xnorm is not None else None
        last = cand_idx[r].reshape(S, L)[:, L - 1]
        args = (last, n_valid_total, xn, err_coef, ymax_sqrt, tau_scale, g, cb_plateau)
        ok, branch, margin = verdict(metric, nreal, kk, dk, ie, cand_tau[r], *args)
        out.certified[r], out.branch[r], out.margin[r] = ok, branch, margin
        if dk is not None:
            out.dk[r] = dk
        if ok:
            for e in range(drop, min(kk, nreal)):
                out.idx[r, e - drop], out.dist[r, e - drop] = base + ci[e], cd[e]
            if nreal < kk:
                _tail(out.idx[r], out.dist[r], D[r], masked_list, n_masked_list, nreal, k, drop, base)
        elif want_seed and branch == "fail" and metric != 1:
            cert = lambda T: verdict(metric, nreal, kk, dk, ie, [T], *args)[0]
            sx = math.sqrt(xn)
            E = err_coef * (sx + ymax_sqrt) * (sx + ymax_sqrt)
            T = f32_up(((dk * dk if metric == 0 else 2.0 * dk) - xn + E) / tau_scale)
            for _ in range(4096):
                if cert(T):
                    break
                T = f32_step(T, 1)
            while cert(f32_step(T, -1)):
                T = f32_step(T, -1)
            out.seed_lo[r] = T
    return out


def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return min(a, b)


def refine_cand(X, row0, m, Y, g, cand_idx, cand_tau, S, L, xnorm, err_coef, ymax_sqrt, tau_scale, kout, base,
                n_valid_total, metric, D=None):
    """refine_cand_launch: (idx [rows][kout], dist, bound [rows])"""
    rows = m - row0
    if D is None:
        D = pairwise(X[row0:m], Y, metric, 0.0)
    cand_idx = np.asarray(cand_idx, dtype=np.uint32).reshape(rows, S * L)
    cand_tau = np.asarray(cand_tau, dtype=F32).reshape(rows, S)
    idx = np.full((rows, kout), -1, dtype=np.int64)
    dist = np.full((rows, kout), np.inf)
    bound = np.empty(rows)
    for r in range(rows):
        ci, cd = _sorted_candidates(cand_idx[r], D[r])
        nreal = ci.shape[0]
        nout = min(kout, nreal)
        idx[r, :nout], dist[r, :nout] = base + ci[:nout], cd[:nout]
        tmin = F32(np.min(cand_tau[r]))
        xn = float(xnorm[row0 + r])
        b = INF
        if tmin != F32(np.inf):
            sx = math.sqrt(xn) if xn == xn else xn
            E = err_coef * (sx + ymax_sqrt) * (sx + ymax_sqrt)
            b = (float(tmin) * tau_scale + xn - E) * (1.0 - 1e-12)
            if metric == 2:
                c = 0.5 * b - 2e-13
                b = c * c * (1.0 - 1e-12) if c > 0.0 else -INF
        elif nreal < n_valid_total:
            b = -INF
        if nreal > kout:
            dn = float(cd[kout])
            b = _fmin(b, dn * dn * (1.0 - 1e-12))
        if xn != xn:
            b = -INF
        bound[r] = b
    return idx, dist, bound


def merge_lists(cand_idx, cand_key, cand_tau, rows, S, L, lkeep, Lout):
    """merge_lists_launch: the union of a row's S lists sorted by (float32 key, index), the first lkeep kept in rows of
    Lout; out_tau = min(every tau, the key of the first entry cut).
    The device sorts keys by bit pattern, so -0.0 would order before +0.0 where numpy ties them: the keys of the cases
    never hold -0.0 (cases assert it)."""
    cand_idx = np.asarray(cand_idx, dtype=np.uint32).reshape(rows, S * L)
    cand_key = np.asarray(cand_key, dtype=F32).reshape(rows, S * L)
    cand_tau = np.asarray(cand_tau, dtype=F32).reshape(rows, S)
    out_idx = np.full((rows, Lout), PAD, dtype=np.uint32)
    out_tau = np.empty(rows, dtype=F32)
    for r in range(rows):
        real = cand_idx[r] != PAD
        ci, ck = cand_idx[r][real], cand_key[r][real]
        o = np.lexsort((ci, ck))
        ci, ck = ci[o], ck[o]
        keep = min(lkeep, ci.shape[0])
        out_idx[r, :keep] = ci[:keep]
        t = F32(np.min(cand_tau[r]))
        if ci.shape[0] > lkeep:
            t = min(t, ck[lkeep])
        out_tau[r] = t
    return out_idx, out_tau


def exact_rows(X, Y, n, g, metric, f, mask, rows, nrows, k, drop, base, masked_list, n_masked_list):
    """exact_rows_launch with oracle.knn's semantics (masked last, positional drop, base), the masked tail truncated at
    n_masked_list: (idx [nrows][k], dist) for the flagged rows in the order of `rows`"""
    rows = np.asarray(rows[:nrows], dtype=np.int64)
    D = pairwise(X[rows], Y[:n], metric, f)
    valid = np.flatnonzero(np.asarray(mask[:n]) == 0) if mask is not None else np.arange(n)
    kk = k + drop
    idx = np.full((nrows, k), -7, dtype=np.int64)
    dist = np.full((nrows, k), -7.0)
    for b in range(nrows):
        d = D[b, valid]
        o = np.lexsort((valid, d))
        found = min(kk, valid.shape[0])
        for p in range(drop, found):
            idx[b, p - drop], dist[b, p - drop] = base + valid[o[p]], d[o[p]]
        if found < kk:
            _tail(idx[b], dist[b], D[b], masked_list, n_masked_list, found, k, drop, base)
    return idx, dist


def masked_tail(X, m, Y, g, metric, f, masked_list, n_masked_list, n_valid, k, drop, base):
    """masked_tail_launch: (idx [m][k], dist, written [k]) -- only the outputs flagged in `written` are touched"""
    D = pairwise(X[:m], Y, metric, f)
    idx = np.full((m, k), -7, dtype=np.int64)
    dist = np.full((m, k), -7.0)
    written = np.zeros(k, dtype=bool)
    for p in range(n_valid, k + drop):
        if p - drop >= 0:
            written[p - drop] = True
    for r in range(m):
        _tail(idx[r], dist[r], D[r], masked_list, n_masked_list, n_valid, k, drop, base)
    return idx, dist, written


def normalise_rows(X):
    """normalise_rows_launch: ascending sums of rounded products, one sqrt, one divide per component; zero rows stay zero"""
    X = np.asarray(X, dtype=np.float64)
    nx = np.zeros(X.shape[0])
    for c in range(X.shape[1]):
        nx = nx + X[:, c] * X[:, c]
    s = np.sqrt(nx)
    with np.errstate(all="ignore"):
        return np.where((nx == 0.0)[:, None], 0.0, X / s[:, None])


# ---- sound lists, the way a filter would make them ---------------------------------------------------------------------
def build_lists(key, valid, S, L, lkeep):
    """key [rows][n] float32 filter scores, valid [n] bool.  References are dealt to S splits by index range; each list
    keeps its lkeep smallest (score, index) in a row of length L with pads behind; tau = the split's first dropped score
    or +inf.  Returns (cand_idx [rows][S * L] uint32, cand_key, cand_tau [rows][S])."""
    rows, n = key.shape
    chunk = (n + S - 1) // S if n else 1
    cand_idx = np.full((rows, S, L), PAD, dtype=np.uint32)
    cand_key = np.full((rows, S, L), np.inf, dtype=F32)
    cand_tau = np.full((rows, S), np.inf, dtype=F32)
    for s in range(S):
        js = np.arange(s * chunk, min(n, (s + 1) * chunk))
        js = js[valid[js]] if js.shape[0] else js
        if js.shape[0] == 0:
            continue
        sc = key[:, js]
        o = np.argsort(sc, axis=1, kind="stable")              # js ascending: (score, index) order
        keep = min(lkeep, js.shape[0])
        cand_idx[:, s, :keep] = js[o[:, :keep]]
        cand_key[:, s, :keep] = np.take_along_axis(sc, o[:, :keep], axis=1)
        if js.shape[0] > lkeep:
            cand_tau[:, s] = np.take_along_axis(sc, o[:, lkeep:lkeep + 1], axis=1)[:, 0]
    return cand_idx.reshape(rows, S * L), cand_key.reshape(rows, S * L), cand_tau


def _remove_candidate(case, r, j):
    """reference j leaves row r's lists (pads stay behind)"""
    S, L = case.S, case.L
    ci = case.cand_idx[r].reshape(S, L)
    ck = case.cand_key[r].reshape(S, L)
    for s in range(S):
        hit = np.flatnonzero(ci[s] == j)
        if hit.shape[0]:
            p = int(hit[0])
            ci[s, p:L - 1], ck[s, p:L - 1] = ci[s, p + 1:].copy(), ck[s, p + 1:].copy()
            ci[s, L - 1], ck[s, L - 1] = PAD, np.inf
            return s
    raise AssertionError("reference %d is not a candidate of row %d" % (j, r))


def canberra_key(D, g, plateau):
    """a float32 lower bound of the exact distance, strictly below it; the plateau for a distance of exactly g"""
    lo = D.astype(F32)
    lo = np.where(lo.astype(np.float64) >= D, np.nextafter(lo, F32(-np.inf)), lo)
    lo = np.nextafter(lo, F32(-np.inf))                       # (one more: a tie's threshold stays a float32 step off d_k')
    lo = np.minimum(lo, np.nextafter(plateau, F32(-np.inf)))
    return np.where(D == float(g), plateau, lo).astype(F32)


KINDS_L2 = ["plain", "hair_cert", "hair_fail", "e_only", "tie", "dup_in", "plain", "plain"]
KINDS_CB = ["plain", "hair_cert", "hair_fail", "tie", "dup_in", "plateau_near", "plateau_le", "plateau_gt"]
NROWS = 131

# (S, L, lkeep, lvalid, g, k, drop, base, row0, masked); Canberra lists are full (lkeep = L)
MAIN = [
    (1, 32, 32, 0, 7, 15, 0, 0, 0, False),
    (1, 32, 32, 32, 64, 15, 1, 1000, 5, True),        # staged gather, g at its limit
    (1, 32, 32, 0, 65, 1, 0, 0, 0, False),            # beyond it
    (1, 64, 40, 40, 50, 15, 0, 0, 5, True),           # 40 staged rows: 4 * 40 * 51 * 8 = 65280 bytes
    (1, 64, 41, 41, 50, 15, 1, 1000, 0, False),       # 41: beyond the 64 KB, not staged
    (1, 64, 40, 24, 50, 31, 1, 0, 0, False),          # more valid entries than staged rows: slots >= 24 read global memory
    (1, 64, 64, 0, 1, 15, 0, 0, 5, False),
    (3, 32, 23, 23, 100, 15, 1, 0, 0, True),          # S * L no multiple of 64
    (2, 64, 40, 40, 50, 31, 1, 1000, 5, False),
    (4, 64, 40, 40, 7, 15, 0, 0, 0, True),
    (8, 64, 23, 23, 50, 15, 1, 0, 5, False),
    (16, 64, 23, 23, 65, 15, 0, 1000, 0, False),
    (32, 32, 23, 23, 50, 31, 1, 0, 5, True),
]
SHAPES = [(1, 32), (1, 64), (3, 32), (2, 64), (4, 64), (8, 64), (16, 64), (32, 32)]


def case_names():
    names = ["main%d" % i for i in range(len(MAIN))]
    for S, L in SHAPES:
        names += ["inf_%dx%d" % (S, L), "short_%dx%d" % (S, L)]
    return names


def _params(name, metric):
    if name.startswith("main"):
        S, L, lkeep, lvalid, g, k, drop, base, row0, masked = MAIN[int(name[4:])]
        size = "main"
    else:
        size, shape = name.split("_")
        S, L = (int(v) for v in shape.split("x"))
        _, _, lkeep, lvalid, g, k, drop, base, row0, masked = next(c for c in MAIN if c[:2] == (S, L))
        if size == "short":
            k, drop = 15, 1
    if metric == 1:
        lkeep = L
    if size == "inf" and k + drop + 1 > S * lkeep:
        k, drop = 15, 0
    return size, S, L, lkeep, lvalid, g, k, drop, base, row0, masked


@functools.lru_cache(maxsize=None)
def make_case(name, metric):
    """One launch of refine_launch: data, sound lists, and rows whose thresholds were LOWERED (never raised: the lists
    stay sound) to sit on each side of the certificate.  case.kind[r] says what row r was built to probe."""
    size, S, L, lkeep, lvalid, g, k, drop, base, row0, masked = _params(name, metric)
    kk = k + drop
    rng = np.random.default_rng(7919 * (case_names().index(name) + 1) + metric)
    c = types.SimpleNamespace(name=name, metric=metric, S=S, L=L, lkeep=lkeep, lvalid=lvalid, g=g, k=k, drop=drop, base=base,
                              row0=row0, cb_f=0.25, tau_scale=TAU_SCALE, err_coef=err_coef_one_product(g))
    _, c.plateau = cb_constants(g)
    if metric != 1:
        c.plateau = F32(0.0)
    rows = NROWS if size == "main" else 23
    m = c.m = row0 + rows
    kinds = KINDS_CB if metric == 1 else KINDS_L2
    kind = [kinds[r % 8] if size == "main" else "plain" for r in range(rows)]
    if size == "main":
        n0 = max(1200, S * (lkeep + 30))
        n_masked = n0 // 10 if masked else 0
    elif size == "inf":
        n_valid = min(S * lkeep, kk + 11)
        n_masked = min(5, S * lkeep - n_valid)
        n0 = n_valid + n_masked
    else:
        n_valid, n_masked = min(9, kk - 1), 12
        n0 = n_valid + n_masked
    draw = (lambda *s: rng.uniform(1.0, 2.0, size=s)) if metric == 1 else (lambda *s: rng.standard_normal(s))
    X, Y0 = draw(m, g), draw(n0, g)
    if metric != 1:
        X *= 0.9
    mask0 = np.zeros(n0, dtype=np.uint8)
    mask0[rng.choice(n0, n_masked, replace=False)] = 1
    extra = []
    c1 = 10.0 + rng.uniform(0.0, 1.0, size=g)
    c2 = 30.0 + rng.uniform(0.0, 1.0, size=g)
    if size == "main":
        if metric == 1:
            for r in range(rows):
                if kind[r] == "plateau_near":
                    X[row0 + r] = c1 * (1.0 + 0.01 * rng.uniform(-1, 1, size=g))
                elif kind[r] in ("plateau_le", "plateau_gt"):
                    X[row0 + r] = c2 * (1.0 + 0.01 * rng.uniform(-1, 1, size=g))
        # a duplicate of the k'-th nearest reference of every `tie` / `dup_in` row goes behind the others
        D0 = pairwise(X[row0:m], Y0, metric, c.cb_f)
        valid0 = np.flatnonzero(mask0 == 0)
        star = {}
        for r in range(rows):
            if kind[r] in ("tie", "dup_in"):              # (the duplicates made so far count: they are references too)
                ids = np.concatenate([valid0, n0 + np.arange(len(extra))])
                dr = D0[r, valid0]
                if extra:
                    dr = np.concatenate([dr, pairwise(X[row0 + r], np.asarray(extra), metric, c.cb_f)[0]])
                star[r] = int(ids[np.lexsort((ids, dr))[kk - 1]])
                extra.append(Y0[star[r]] if star[r] < n0 else extra[star[r] - n0])
        if metric == 1:                                   # references near the two far centres: k' of one, k' - 2 of the other
            extra += [c1 * (1.0 + 0.01 * rng.uniform(-1, 1, size=g)) for _ in range(kk)]
            extra += [c2 * (1.0 + 0.01 * rng.uniform(-1, 1, size=g)) for _ in range(max(kk - 2, 0))]
    Y = np.vstack([Y0] + [np.asarray(extra).reshape(-1, g)]) if extra else Y0
    n = c.n = Y.shape[0]
    mask = np.concatenate([mask0, np.zeros(n - n0, dtype=np.uint8)])
    c.X, c.Y, c.mask = X, Y, mask
    valid = mask == 0
    c.n_valid_total = int(valid.sum())
    ml = np.flatnonzero(mask != 0).astype(np.uint32)
    c.n_masked_list = min(ml.shape[0], 4 if size == "short" else 8)
    c.masked_list = ml[:max(c.n_masked_list, 1)] if ml.shape[0] else np.zeros(1, dtype=np.uint32)
    D = c.D = pairwise(X[row0:m], Y, metric, c.cb_f)
    # the filter's scores
    if metric == 1:
        c.xnorm, c.ymax_sqrt = None, 0.0
        key = canberra_key(D, g, c.plateau)
    else:
        if metric == 2:
            Xn, Yn = normalise_rows(X), normalise_rows(Y)
            d2 = pairwise(Xn[row0:m], Yn, 0) ** 2
        else:
            Xn, Yn, d2 = X, Y, D * D
        c.xnorm = (Xn * Xn).sum(axis=1)
        c.ymax_sqrt = math.sqrt(float((Yn * Yn).sum(axis=1).max()))
        key = ((d2 - c.xnorm[row0:m, None]) / c.tau_scale).astype(F32)
    chunk = (n + S - 1) // S
    if metric == 1 and size == "main":
        # plateau_gt: all but one of list 0's entries are references at distance g whose score stayed BELOW the plateau
        # (a component on the window's edge is not provably outside) and they carry split 0's highest indices
        sub = F32(g - 0.5)
        for r in range(rows):
            if kind[r] == "plateau_gt":
                far = np.flatnonzero((D[r, :chunk] == float(g)) & valid[:chunk] & (np.arange(chunk) < n0))
                near0 = int(((D[r, :chunk] != float(g)) & valid[:chunk]).sum())
                a = lkeep - near0 - 1
                if kk < 2 or a < 1 or far.shape[0] < a + 2:
                    kind[r] = "plateau_le"
                else:
                    key[r, far[-a:]] = sub
    c.key = key
    c.cand_idx, c.cand_key, c.cand_tau = build_lists(key, valid, S, L, lkeep)
    assert not np.any(np.signbit(c.cand_key) & (c.cand_key == 0))          # no -0.0 (merge_lists)
    c.kind = kind
    if size != "main":
        # a reference whose score was not finite vanished from every third row's lists without a trace
        for r in range(rows):
            if r % 3 == 1 and c.n_valid_total > 0:
                real = c.cand_idx[r][c.cand_idx[r] != PAD]
                _remove_candidate(c, r, int(real[r % real.shape[0]]))
                kind[r] = "vanished"
        return c
    # thresholds lowered from the natural ones, in ONE list of the row (the minimum over the lists decides)
    nat = refine(X, row0, m, Y, g, c.cand_idx, c.cand_tau, S, L, c.xnorm, c.err_coef, c.ymax_sqrt, c.tau_scale, k, drop, base,
                 c.n_valid_total, c.masked_list, c.n_masked_list, metric, c.cb_f, c.plateau, D=D, want_seed=False)
    for r in range(rows):
        kd = kind[r]
        if kd in ("plain",) or kd.startswith("plateau"):
            continue
        if not (nat.certified[r] and nat.branch[r] == "cert" and nat.margin[r] >= 1e-5):
            kind[r] = "plain"
            continue
        dk = float(nat.dk[r])
        s = r % S
        if kd in ("tie", "dup_in"):
            j = n0 + sorted(star).index(r)
            ci, cd = _sorted_candidates(c.cand_idx[r], D[r])
            if not (ci.shape[0] > kk and ci[kk - 1] == star[r] and ci[kk] == j):
                kind[r] = "plain"
            elif kd == "tie":
                s = _remove_candidate(c, r, j)
                c.cand_tau[r, s] = min(c.cand_tau[r, s], key[r, j])
            continue
        if metric == 1:
            T = f32_step(f32_up(dk), 2) if kd == "hair_cert" else f32_step(f32_down(dk), -2)
        else:
            xn = float(c.xnorm[row0 + r])
            sx = math.sqrt(xn)
            E = c.err_coef * (sx + c.ymax_sqrt) * (sx + c.ymax_sqrt)
            t2 = dk * dk if metric == 0 else 2.0 * dk
            if kd == "hair_cert":
                T = f32_up((t2 * (1.0 + 1e-7) + 1e-12 - xn + E) / c.tau_scale)
            elif kd == "hair_fail":
                T = f32_down((t2 * (1.0 - 1e-7) - 1e-12 - xn + E) / c.tau_scale)
            else:                                             # e_only: above d_k'^2 without E, below it with E
                T = F32((t2 + 0.5 * E - xn) / c.tau_scale)
        if not T < c.cand_tau[r, s]:
            kind[r] = "plain"
            continue
        c.cand_tau[r, s] = T
    return c


def run_refine(c, cand_idx=None, cand_tau=None, S=None, L=None, err_coef=None, want_seed=True):
    """the restatement on a case (optionally other lists / thresholds of the same rows)"""
    return refine(c.X, c.row0, c.m, c.Y, c.g, c.cand_idx if cand_idx is None else cand_idx,
                  c.cand_tau if cand_tau is None else cand_tau, S or c.S, L or c.L, c.xnorm,
                  c.err_coef if err_coef is None else err_coef, c.ymax_sqrt, c.tau_scale, c.k, c.drop, c.base,
                  c.n_valid_total, c.masked_list, c.n_masked_list, c.metric, c.cb_f, c.plateau, D=c.D, want_seed=want_seed)


def merged_shape(c):
    """(lkeep, Lout) of the merge the product would put in front of this case's refine"""
    lkeep = min(c.lkeep, 64)
    return lkeep, 32 if lkeep <= 32 else 64


@functools.lru_cache(maxsize=None)
def canberra_exact_case():
    """Canberra verdicts between representable values, g = 7, k = 4, three lists of 32 over 120 references:
      references 0..39: every component 100 (F);  40..75: the target (2, .., 2) but components 0 and 1 at 100 (W, at
      distance exactly 2.0 of it);  76..79: F;  80, 81: (2, .., 2);  82..85: (3, .., 3);  86, 87: (5, .., 5);  88..119: F.
      row 0  target 2: the 4th entry is a W at 2.0, list 1 dropped W 72.. at score 2.0f: tau == d_k', not certified
      row 1  the same with that tau one float32 up (the one raised threshold of the suite): certified
      row 2  target 5: two entries at 0, then distance g by index; every tau the plateau, 4th entry index 1 <= 31: certified
      row 3  target 5, references 9..39 scored below the plateau: list 0 is [9..39, 0], 4th entry 9 > 0: not certified
      row 4  target 3: four entries at 0, every tau the plateau: certified by the plain rule (d_k' < g)
      row 5  row 2 with list 2's tau below the plateau: the plain rule decides, tau > g is false: not certified
      row 6  target 5, references 10..39 scored below the plateau: list 0 is [10..39, 0, 1], 4th entry 1 == 1: certified"""
    g, S, L = 7, 3, 32
    _, plateau = cb_constants(g)
    c = types.SimpleNamespace(name="canberra_exact", metric=1, S=S, L=L, lkeep=L, lvalid=0, g=g, k=4, drop=0, base=0, row0=0,
                              m=7, cb_f=0.25, tau_scale=1.0, err_coef=0.0, ymax_sqrt=0.0, xnorm=None, plateau=plateau)
    Y = np.full((120, g), 100.0)
    Y[40:76, 2:] = 2.0
    Y[80:82], Y[82:86], Y[86:88] = 2.0, 3.0, 5.0
    X = np.array([[2.0] * g, [2.0] * g, [5.0] * g, [5.0] * g, [3.0] * g, [5.0] * g, [5.0] * g])
    c.X, c.Y, c.n, c.mask, c.n_valid_total = X, Y, 120, np.zeros(120, dtype=np.uint8), 120
    c.masked_list, c.n_masked_list = np.zeros(1, dtype=np.uint32), 0
    c.D = pairwise(X, Y, 1, 0.25)
    key = np.where(c.D == float(g), plateau, c.D.astype(F32)).astype(F32)
    key[3, 9:40] = F32(g - 0.5)
    key[6, 10:40] = F32(g - 0.5)
    c.key = key
    c.cand_idx, c.cand_key, c.cand_tau = build_lists(key, c.mask == 0, S, L, L)
    c.cand_tau[1, 1] = f32_step(c.cand_tau[1, 1], 1)
    c.cand_tau[5, 2] = plateau - F32(1.0)
    c.kind = ["tau_eq_dk", "tau_above_dk", "plateau_le", "plateau_gt", "plateau_near", "plateau_mixed", "plateau_eq"]
    c.expect = [(False, "fail"), (True, "cert"), (True, "plateau_le"), (False, "plateau_gt"), (True, "plateau_near"),
                (False, "fail"), (True, "plateau_le")]
    return c

"""The kernels of nabo_amd/csrc/refine.hip, one by one, against the restatement of their contract (tests/_refine_ref.py, itself
checked by hand and case by case in tests/test_refine_ref_cpu.py): the float64 re-evaluation and the per-row certificate
(refine_launch), the shard-mode variant and its bound (refine_cand_launch), the merge of a row's lists by their filter keys
(merge_lists_launch), the exact fallback (exact_rows_launch, masked_tail_launch) and normalise_rows_launch.  Everything is
asserted by equality: verdicts, indices, and the bits of distances, bounds and thresholds.  No case holds a row within 1e-9
of a certificate's threshold (the CPU test proves it), so nothing is excused.

The C ABI reaches these kernels only through whole queries, so they are driven through the launchers the library already
exports for its own translation units, by their mangled names (declared in nabo_amd/csrc/launch.h), on buffers from
nabo_dev_malloc and the NULL stream: no new entry point.  rperm / tperm are always NULL, as in the product.
"""
import ctypes as C

import numpy as np
import pytest

import oracle

import _refine_ref as rr

pytestmark = pytest.mark.gpu

REFINE = "_ZN4nabo13refine_launchEPKdllS1_iPKjPKfiiS1_dddiillS3_iPlPdPjS8_P12ihipStream_tidfiS3_S3_Pf"
REFINE_CAND = "_ZN4nabo18refine_cand_launchEPKdllS1_iPKjPKfiiS1_dddillPlPdS7_P12ihipStream_tiiS3_S3_"
MERGE = "_ZN4nabo18merge_lists_launchEPKjPKfS3_liiiiPjPfP12ihipStream_t"
EXACT = "_ZN4nabo17exact_rows_launchEPKdS1_liidPKhPKjjiilS5_iPlPdS7_jP12ihipStream_t"
TAIL = "_ZN4nabo18masked_tail_launchEPKdlS1_iidPKjiiiilPlPdP12ihipStream_t"
NORMALISE = "_ZN4nabo21normalise_rows_launchEPKdliPdP12ihipStream_t"
CBF_CONSTANTS = "_ZN4nabo13cbf_constantsEiPfS0_"
vp, i32, i64, u32, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_uint, C.c_double
ARGS = {
    REFINE: [vp, i64, i64, vp, i32, vp, vp, i32, i32, vp, dbl, dbl, dbl, i32, i32, i64, i64, vp, i32, vp, vp, vp, vp, vp, i32, dbl,
             C.c_float, i32, vp, vp, vp],
    REFINE_CAND: [vp, i64, i64, vp, i32, vp, vp, i32, i32, vp, dbl, dbl, dbl, i32, i64, i64, vp, vp, vp, vp, i32, i32, vp, vp],
    MERGE: [vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, vp],
    EXACT: [vp, vp, i64, i32, i32, dbl, vp, vp, u32, i32, i32, i64, vp, i32, vp, vp, vp, u32, vp],
    TAIL: [vp, i64, vp, i32, i32, dbl, vp, i32, i32, i32, i32, i64, vp, vp, vp],
    NORMALISE: [vp, i64, i32, vp, vp],
    CBF_CONSTANTS: [i32, C.POINTER(C.c_float), C.POINTER(C.c_float)],
}
HIP_INVALID_VALUE = 1
PAD = rr.PAD
F32 = np.float32
SENT = 0x5A                                                   # outputs are filled with this byte before every launch


def _fn(name):
    from nabo_amd import _lib
    try:
        f = getattr(_lib.lib(), name)
    except AttributeError:
        pytest.fail("the library does not export %s" % name)
    f.argtypes = ARGS[name]
    f.restype = None if name == CBF_CONSTANTS else C.c_int
    return f


def _plateau(g):
    s, p = C.c_float(), C.c_float()
    _fn(CBF_CONSTANTS)(g, C.byref(s), C.byref(p))
    assert F32(p.value) == rr.cb_constants(g)[1]
    return F32(p.value)


class Dev:
    """device buffers of one test, freed together"""

    def __init__(self):
        self.bufs = []

    def new(self, nbytes, fill=None):
        from nabo_amd import _knn
        b = _knn.DeviceBuffer(max(int(nbytes), 8))
        self.bufs.append(b)
        if fill is not None:
            b.upload(np.full(max(int(nbytes), 8), fill, dtype=np.uint8))
        return b

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        b = self.new(arr.nbytes)
        if arr.nbytes:
            b.upload(arr)
        return b

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def _sync():
    from nabo_amd import _lib
    _lib.check(_lib.lib().nabo_dev_synchronize(0))


@pytest.fixture
def dev(gpu_lib):
    d = Dev()
    yield d
    d.free()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _sentinel(shape, dtype):
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, SENT, dtype=np.uint8).view(dtype).reshape(shape)


class RefineRun:
    """one case's constant inputs on the device; launch() runs refine_launch on given lists / thresholds"""

    def __init__(self, dev, c):
        self.dev, self.c = dev, c
        self.dX, self.dY = dev.up(c.X), dev.up(c.Y)
        self.dxn = dev.up(c.xnorm) if c.xnorm is not None else None
        self.dml = dev.up(c.masked_list)
        self.doi, self.dod = dev.new(c.m * c.k * 8), dev.new(c.m * c.k * 8)
        self.dfr, self.dfs, self.dfc = dev.new(c.m * 4), dev.new(c.m * 4), dev.new(4)
        self.plateau = _plateau(c.g) if c.metric == 1 else F32(0.0)

    def launch(self, cand_idx=None, cand_tau=None, S=None, L=None, lvalid=None, seeds=True):
        c, dev = self.c, self.dev
        cand_idx = c.cand_idx if cand_idx is None else cand_idx
        cand_tau = c.cand_tau if cand_tau is None else cand_tau
        S, L = S or c.S, L or c.L
        rows = c.m - c.row0
        assert cand_idx.shape == (rows, S * L) and cand_idx.dtype == np.uint32
        assert cand_tau.shape == (rows, S) and cand_tau.dtype == F32
        real = cand_idx[cand_idx != PAD]
        assert real.size == 0 or real.max() < c.n                   # nothing the kernel could read out of range
        dci, dct = dev.up(cand_idx), dev.up(cand_tau)
        for b in (self.doi, self.dod, self.dfr, self.dfs):
            b.upload(np.full(b.nbytes, SENT, dtype=np.uint8))
        self.dfc.upload(np.zeros(1, dtype=np.uint32))
        rc = _fn(REFINE)(self.dX.ptr, c.row0, c.m, self.dY.ptr, c.g, dci.ptr, dct.ptr, S, L,
                         self.dxn.ptr if self.dxn else None, c.err_coef, c.ymax_sqrt, c.tau_scale, c.k, c.drop, c.base,
                         c.n_valid_total, self.dml.ptr, c.n_masked_list, self.doi.ptr, self.dod.ptr, self.dfr.ptr, self.dfc.ptr,
                         None, c.metric, c.cb_f, float(self.plateau), c.lvalid if lvalid is None else lvalid, None, None,
                         self.dfs.ptr if seeds else None)
        assert rc == 0
        _sync()
        nf = int(self.dfc.download((1,), np.uint32)[0])
        assert nf <= rows
        fr = self.dfr.download((c.m,), np.uint32)
        fs = self.dfs.download((c.m,), F32)
        assert (fr[nf:] == _sentinel((c.m - nf,), np.uint32)).all()
        if not seeds:
            assert (fs.view(np.uint32) == _sentinel((c.m,), np.uint32)).all()
        failed = fr[:nf].astype(np.int64) - c.row0
        assert len(set(failed.tolist())) == nf and (failed >= 0).all() and (failed < rows).all()
        seed = np.full(rows, np.nan, dtype=F32)
        seed[failed] = fs[:nf]
        return set(failed.tolist()), seed, self.doi.download((c.m, c.k), np.int64), self.dod.download((c.m, c.k), np.float64)


def _check_against(c, exp, got, what, seeds=True):
    """verdicts, outputs and seeds of one launch against the restatement `exp`"""
    failed, seed, oi, od = got
    rows = c.m - c.row0
    exp_failed = set(np.flatnonzero(~exp.certified).tolist())
    assert failed == exp_failed, "%s: rows only the device fails %s, only the restatement fails %s" % (
        what, sorted(failed - exp_failed)[:8], sorted(exp_failed - failed)[:8])
    si, sd = _sentinel((c.k,), np.int64), _sentinel((c.k,), np.uint64)
    for row in range(c.row0):
        assert (oi[row] == si).all() and (_bits(od[row]) == sd).all(), "%s: row %d below row0 was written" % (what, row)
    for r in range(rows):
        row = c.row0 + r
        if exp.certified[r]:
            assert np.array_equal(oi[row], exp.idx[r]), "%s row %d (%s): %s != %s" % (what, r, exp.branch[r], oi[row], exp.idx[r])
            assert np.array_equal(_bits(od[row]), _bits(exp.dist[r])), "%s row %d (%s): distance bits" % (what, r, exp.branch[r])
            continue
        assert (oi[row] == si).all() and (_bits(od[row]) == sd).all(), "%s: failed row %d was written" % (what, r)
        if not seeds:
            continue
        if exp.branch[r] == "fail" and c.metric != 1:
            assert np.isfinite(seed[r]) and seed[r] >= exp.seed_lo[r], "%s row %d: seed %r below %r" % (what, r, seed[r], exp.seed_lo[r])
            assert rr.lower_seed(seed[r], exp.dk[r], c.tau_scale) < exp.seed_lo[r], "%s row %d: seed %r far above %r" % (
                what, r, seed[r], exp.seed_lo[r])
        else:
            assert seed[r] == F32(np.inf), "%s row %d (%s): seed %r" % (what, r, exp.branch[r], seed[r])


@pytest.mark.parametrize("name", rr.case_names())
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_refine_verdicts_outputs_and_seeds(dev, metric, name):
    c = rr.make_case(name, metric)
    exp = rr.run_refine(c)
    run = RefineRun(dev, c)
    what = "%s metric %d" % (name, metric)
    got = run.launch()
    _check_against(c, exp, got, what)
    rows = c.m - c.row0
    for r in range(rows):                           # (restated on their own: what the rows were built for)
        if c.kind[r] == "tie":
            assert r in got[0], "%s row %d: a tie across k' with the duplicate outside the lists was certified" % (what, r)
        if c.kind[r] == "dup_in":
            assert r not in got[0] and (np.diff(got[3][c.row0 + r]) >= 0).all()
    # without fail_seed: same verdicts, same outputs
    _check_against(c, exp, run.launch(seeds=False), what + " fail_seed=NULL", seeds=False)
    seeded = [r for r in range(rows) if exp.branch[r] == "fail" and metric != 1]
    if not seeded:
        return
    # the row's thresholds replaced by its seed certify it; the seed lowered by max(16 ulps, 1e-9 d^2 / tau_scale) does not
    seed = got[1]
    tau_s, tau_l = c.cand_tau.copy(), c.cand_tau.copy()
    for r in seeded:
        tau_s[r, :] = seed[r]
        tau_l[r, :] = rr.lower_seed(seed[r], exp.dk[r], c.tau_scale)
    got_s = run.launch(cand_tau=tau_s)
    assert not (got_s[0] & set(seeded)), "%s: rows not certified by their own seed: %s" % (what, sorted(got_s[0] & set(seeded))[:8])
    assert got_s[0] == got[0] - set(seeded), what + ": other rows' verdicts moved"
    got_l = run.launch(cand_tau=tau_l)
    assert set(seeded) <= got_l[0], "%s: rows certified below their seed: %s" % (what, sorted(set(seeded) - got_l[0])[:8])


def test_canberra_between_representable_values(dev):
    """tau == d_k' exactly (2.0 against 2.0f) does not certify, one float32 above does; the plateau rule three ways and with a
    list below the plateau; the plateau is the library's own (cbf_constants), xnorm is NULL as query.hip passes it."""
    c = rr.canberra_exact_case()
    run = RefineRun(dev, c)
    assert run.plateau == c.plateau and c.xnorm is None
    exp = rr.run_refine(c)
    got = run.launch()
    assert [r not in got[0] for r in range(c.m)] == [e[0] for e in c.expect], "certified %s, built as %s" % (
        [r not in got[0] for r in range(c.m)], c.kind)
    _check_against(c, exp, got, "canberra_exact")


CAND_CASES = ["main1", "main5", "main6", "main7", "main9", "main12", "inf_1x32", "inf_4x64", "short_3x32"]


@pytest.mark.parametrize("kout", [1, 9, 32, 64])
@pytest.mark.parametrize("name", CAND_CASES)
@pytest.mark.parametrize("metric", [0, 2])
def test_refine_cand_lists_and_bound(dev, metric, name, kout):
    c = rr.make_case(name, metric)
    rows = c.m - c.row0
    xn = c.xnorm.copy()
    xn[c.row0 + 2] = np.nan                                   # a target outside the filter's range
    exp_i, exp_d, exp_b = rr.refine_cand(c.X, c.row0, c.m, c.Y, c.g, c.cand_idx, c.cand_tau, c.S, c.L, xn, c.err_coef, c.ymax_sqrt,
                                         c.tau_scale, kout, c.base, c.n_valid_total, metric, D=c.D)
    dX, dY, dxn, dci, dct = dev.up(c.X), dev.up(c.Y), dev.up(xn), dev.up(c.cand_idx), dev.up(c.cand_tau)
    doi, dod, dob = dev.new(c.m * kout * 8, SENT), dev.new(c.m * kout * 8, SENT), dev.new(c.m * 8, SENT)
    rc = _fn(REFINE_CAND)(dX.ptr, c.row0, c.m, dY.ptr, c.g, dci.ptr, dct.ptr, c.S, c.L, dxn.ptr, c.err_coef, c.ymax_sqrt,
                          c.tau_scale, kout, c.base, c.n_valid_total, doi.ptr, dod.ptr, dob.ptr, None, metric, c.lvalid, None, None)
    assert rc == 0
    _sync()
    oi, od, ob = doi.download((c.m, kout), np.int64), dod.download((c.m, kout), np.float64), dob.download((c.m,), np.float64)
    what = "%s metric %d kout %d" % (name, metric, kout)
    assert (oi[:c.row0] == _sentinel((c.row0, kout), np.int64)).all() and (_bits(ob[:c.row0]) == _sentinel((c.row0,), np.uint64)).all()
    bad = np.flatnonzero((oi[c.row0:] != exp_i).any(axis=1) | (_bits(od[c.row0:]) != _bits(exp_d)).any(axis=1))
    assert bad.size == 0, "%s: lists of rows %s differ" % (what, bad[:8])
    bad = np.flatnonzero(_bits(ob[c.row0:]) != _bits(exp_b))
    assert bad.size == 0, "%s: bound of rows %s: %s != %s" % (what, bad[:8], ob[c.row0:][bad[:8]], exp_b[bad[:8]])
    # the cases reach what they are here for
    nreal = (c.cand_idx != PAD).sum(axis=1)
    assert exp_b[2] == -np.inf
    if name.startswith("main"):
        assert kout >= 32 or (nreal > kout).any()
        assert metric == 2 or np.isfinite(np.delete(exp_b, 2)).all()
    if name.startswith("inf") and kout == 64:
        assert (exp_b == np.inf).any() and (np.delete(exp_b, 2) == -np.inf).any() and (nreal < kout).all()


MERGE_SHAPES = [(23, 32), (32, 32), (64, 64), (128, 128), (5, 64)]


def _merge_inputs(name, variant):
    c = rr.make_case(name, 0)
    idx, key, tau = c.cand_idx.copy(), c.cand_key.copy(), c.cand_tau.copy()
    if variant == "tied":                                    # coarse keys: ties across every cut (+ 0.0: no -0.0)
        key = (np.round(key / F32(256.0)) * F32(256.0) + F32(0.0)).astype(F32)
        key[idx == PAD] = np.inf
    elif variant == "one_list":                              # every list but the last is all pads
        idx.reshape(-1, c.S, c.L)[:, :-1, :] = PAD
        tau[:, :-1] = np.inf
    assert not (np.signbit(key) & (key == 0)).any()
    return c, idx, key, tau


@pytest.mark.parametrize("variant", ["plain", "tied", "one_list"])
@pytest.mark.parametrize("name", ["main0", "main4", "main7", "main8", "main9", "main10", "main11", "main12", "inf_3x32"])
def test_merge_lists(dev, name, variant):
    c, idx, key, tau = _merge_inputs(name, variant)
    rows = c.m - c.row0
    ncl = (c.S * c.L + 63) // 64
    di, dk, dt = dev.up(idx), dev.up(key), dev.up(tau)
    done = 0
    for lkeep, Lout in MERGE_SHAPES:
        if Lout > 64 * ncl:
            continue
        done += 1
        doi, dot = dev.new(rows * Lout * 4, SENT), dev.new(rows * 4, SENT)
        rc = _fn(MERGE)(di.ptr, dk.ptr, dt.ptr, rows, c.S, c.L, lkeep, Lout, doi.ptr, dot.ptr, None)
        assert rc == 0
        _sync()
        oi, ot = doi.download((rows, Lout), np.uint32), dot.download((rows,), F32)
        ei, et = rr.merge_lists(idx, key, tau, rows, c.S, c.L, lkeep, Lout)
        what = "%s %s lkeep %d Lout %d" % (name, variant, lkeep, Lout)
        bad = np.flatnonzero((oi != ei).any(axis=1) | (ot.view(np.uint32) != et.view(np.uint32)))
        assert bad.size == 0, "%s: rows %s differ; first: tau %r != %r" % (what, bad[:8], ot[bad[0]], et[bad[0]])
        # soundness, on its own: whatever is not in the merged list scores >= out_tau, and out_tau <= every tau
        assert (ot[:, None] <= tau).all(), what
        cut_ties = cut_rows = 0
        for r in range(rows):
            gone = (idx[r] != PAD) & ~np.isin(idx[r], oi[r][oi[r] != PAD])
            assert (key[r][gone] >= ot[r]).all(), "%s row %d: a candidate below out_tau left the list" % (what, r)
            kept_max = key[r][(idx[r] != PAD) & ~gone].max() if (~gone & (idx[r] != PAD)).any() else -np.inf
            cut_rows += int(gone.any())
            cut_ties += int(gone.any() and key[r][gone].min() == kept_max)
        if variant == "tied" and name.startswith("main") and cut_rows:
            assert cut_ties > 0, what + ": no row with equal keys on both sides of the cut"
        if variant == "plain" and name in ("main0", "main9"):        # (g = 7: many references score below ||x||^2)
            assert (key[idx != PAD] < 0).sum() > 1000
    assert done >= 4


@pytest.mark.parametrize("S,L,lkeep,Lout", [(4, 64, 64, 129), (4, 64, 33, 32), (17, 64, 32, 32), (2, 32, 0, 32)])
def test_merge_lists_refuses_what_it_cannot_do(dev, S, L, lkeep, Lout):
    rows = 5
    idx = np.arange(rows * S * L, dtype=np.uint32).reshape(rows, S * L) % 1000
    di, dk, dt = dev.up(idx), dev.up(np.ones((rows, S * L), dtype=F32)), dev.up(np.ones((rows, S), dtype=F32))
    doi, dot = dev.new(rows * max(Lout, 128) * 4, SENT), dev.new(rows * 4, SENT)
    rc = _fn(MERGE)(di.ptr, dk.ptr, dt.ptr, rows, S, L, lkeep, Lout, doi.ptr, dot.ptr, None)
    assert rc == HIP_INVALID_VALUE
    _sync()
    assert (doi.download((rows * max(Lout, 128),), np.uint32) == _sentinel((1,), np.uint32)[0]).all()
    assert (dot.download((rows,), np.uint32) == _sentinel((1,), np.uint32)[0]).all()


MERGED = ["main8", "main9", "main10", "main11", "main12"]


@pytest.mark.parametrize("name", MERGED)
@pytest.mark.parametrize("metric", [0, 2])
def test_merge_then_refine_is_no_more_lenient(dev, metric, name):
    """The product's own sequence: the S lists merged, then the merged list refined (S = 1, L = Lout, lvalid = lkeep).  A row
    the merged list certifies is certified unmerged too, with the same bits.  (Euclidean and cosine: query.hip merges no
    Canberra lists.)"""
    c = rr.make_case(name, metric)
    rows = c.m - c.row0
    lkeep, Lout = rr.merged_shape(c)
    di, dk, dt = dev.up(c.cand_idx), dev.up(c.cand_key), dev.up(c.cand_tau)
    dmi, dmt = dev.new(rows * Lout * 4, SENT), dev.new(rows * 4, SENT)
    assert _fn(MERGE)(di.ptr, dk.ptr, dt.ptr, rows, c.S, c.L, lkeep, Lout, dmi.ptr, dmt.ptr, None) == 0
    _sync()
    mi, mt = dmi.download((rows, Lout), np.uint32), dmt.download((rows, 1), F32)
    ei, et = rr.merge_lists(c.cand_idx, c.cand_key, c.cand_tau, rows, c.S, c.L, lkeep, Lout)
    assert np.array_equal(mi, ei) and np.array_equal(mt[:, 0].view(np.uint32), et.view(np.uint32))
    run = RefineRun(dev, c)
    what = "%s metric %d" % (name, metric)
    merged = run.launch(cand_idx=mi, cand_tau=mt, S=1, L=Lout, lvalid=lkeep)
    exp_m = rr.run_refine(c, cand_idx=mi, cand_tau=mt, S=1, L=Lout)
    _check_against(c, exp_m, merged, what + " merged")
    plain = run.launch()
    exp_u = rr.run_refine(c)
    assert plain[0] <= merged[0], "%s: rows certified merged but not unmerged: %s" % (what, sorted(plain[0] - merged[0])[:8])
    sure = [r for r in range(rows) if r not in merged[0]]
    assert sure or c.k + c.drop > lkeep, what
    for r in sure:
        row = c.row0 + r
        assert np.array_equal(merged[2][row], exp_u.idx[r]) and np.array_equal(_bits(merged[3][row]), _bits(exp_u.dist[r])), (what, r)


# n, mask fraction, duplicates, k, drop, base, nrows, d_rows, masked-list length (None: all of them)
EXACT_CASES = [
    (1, 0.0, False, 1, 0, 0, 1, 8, None),
    (255, 0.2, False, 15, 1, 1000, 7, 3, None),
    (256, 0.0, True, 15, 0, 0, 8, 8, None),
    (257, 0.3, True, 31, 1, 0, 9, 3, None),
    (1000, 0.1, True, 15, 1, 1000, 20, 8, None),
    (1000, 0.0, False, 1, 0, 0, 20, 3, None),
    (40, 0.9, False, 15, 1, 1000, 9, 8, 6),          # fewer valid references than k': the masked tail, cut at 6, then -1 / NaN
    (40, 0.9, False, 15, 0, 0, 7, 3, None),
]


@pytest.mark.parametrize("case", range(len(EXACT_CASES)))
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_exact_rows(dev, metric, case):
    n, mfrac, dup, k, drop, base, nrows, d_rows, nml = EXACT_CASES[case]
    g, m = (50 if case == 4 else 7), 37
    rng = np.random.default_rng(100 * case + metric)
    draw = (lambda *s: rng.uniform(1.0, 2.0, size=s)) if metric == 1 else (lambda *s: rng.standard_normal(s))
    X, Y = draw(m, g), draw(n, g)
    if dup:
        Y[n // 2:n // 2 + 40] = Y[:40]                          # ties: index order decides
        X[:4] = Y[:4]
    mask = (rng.random(n) < mfrac).astype(np.uint8)
    if mfrac >= 0.9:
        mask[:] = 1
        mask[rng.choice(n, 5, replace=False)] = 0
    ml_all = np.flatnonzero(mask).astype(np.uint32)
    nml = ml_all.shape[0] if nml is None else nml
    rows = rng.choice(m, nrows, replace=False).astype(np.uint32)
    exp_i, exp_d = rr.exact_rows(X, Y, n, g, metric, 0.25, mask if mfrac else None, rows, nrows, k, drop, base, ml_all, nml)
    if k + drop <= n and nml == ml_all.shape[0]:                 # where the oracle itself can say it
        ki, kd = oracle.knn(X[rows], Y, k, metric=metric, ref_mask=mask if mfrac else None, drop_first=bool(drop))
        assert np.array_equal(exp_i, ki + base) and np.array_equal(_bits(exp_d), _bits(kd))
    dX, dY, dM, dR, dML = dev.up(X), dev.up(Y), dev.up(mask), dev.up(rows), dev.up(ml_all if ml_all.size else np.zeros(1, np.uint32))
    doi, dod, dD = dev.new(m * k * 8, SENT), dev.new(m * k * 8, SENT), dev.new(d_rows * n * 8)
    rc = _fn(EXACT)(dX.ptr, dY.ptr, n, g, metric, 0.25, dM.ptr if mfrac else None, dR.ptr, nrows, k, drop, base, dML.ptr, nml,
                    doi.ptr, dod.ptr, dD.ptr, d_rows, None)
    assert rc == 0
    _sync()
    oi, od = doi.download((m, k), np.int64), dod.download((m, k), np.float64)
    for b, row in enumerate(rows):
        assert np.array_equal(oi[row], exp_i[b]), "case %d metric %d row %d: %s != %s" % (case, metric, row, oi[row], exp_i[b])
        assert np.array_equal(_bits(od[row]), _bits(exp_d[b])), "case %d metric %d row %d: distance bits" % (case, metric, row)
    rest = np.setdiff1d(np.arange(m), rows)
    assert (oi[rest] == _sentinel((1,), np.int64)[0]).all() and (_bits(od[rest]) == _sentinel((1,), np.uint64)[0]).all()
    if mfrac >= 0.9:
        assert (exp_i == -1).any() == (nml == 6)


@pytest.mark.parametrize("drop", [0, 1])
@pytest.mark.parametrize("k", [5, 15])
@pytest.mark.parametrize("n_valid", [0, 3])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_masked_tail(dev, metric, n_valid, k, drop):
    g, m, n, nml = 7, 9, 30, 4                                   # (4 listed: shorter than the gap up to k')
    rng = np.random.default_rng(10 * n_valid + k + drop)
    X, Y = rng.uniform(1.0, 2.0, size=(m, g)), rng.uniform(1.0, 2.0, size=(n, g))
    ml = np.sort(rng.choice(n, 12, replace=False)).astype(np.uint32)
    exp_i, exp_d, written = rr.masked_tail(X, m, Y, g, metric, 0.25, ml, nml, n_valid, k, drop, 1000)
    dX, dY, dML = dev.up(X), dev.up(Y), dev.up(ml)
    doi, dod = dev.new(m * k * 8, SENT), dev.new(m * k * 8, SENT)
    rc = _fn(TAIL)(dX.ptr, m, dY.ptr, g, metric, 0.25, dML.ptr, nml, n_valid, k, drop, 1000, doi.ptr, dod.ptr, None)
    assert rc == 0
    _sync()
    oi, od = doi.download((m, k), np.int64), dod.download((m, k), np.float64)
    assert written.any() and (exp_i[:, written] >= 1000).any() and ((exp_i[:, written] == -1).any() == (k + drop - n_valid > nml))
    assert np.array_equal(oi[:, written], exp_i[:, written]) and np.array_equal(_bits(od[:, written]), _bits(exp_d[:, written]))
    assert (oi[:, ~written] == _sentinel((1,), np.int64)[0]).all() and (_bits(od[:, ~written]) == _sentinel((1,), np.uint64)[0]).all()


@pytest.mark.parametrize("g", [1, 7, 50, 100])
def test_normalise_rows(dev, g):
    m = 515
    rng = np.random.default_rng(g)
    X = rng.standard_normal((m, g)) * rng.uniform(1e-3, 1e3, size=(m, 1))
    X[[0, 255, 256, m - 1]] = 0.0
    X[7] = 1e-160                                               # squares underflow to subnormals, not to zero
    dX, dO = dev.up(X), dev.new(m * g * 8, SENT)
    assert _fn(NORMALISE)(dX.ptr, m, g, dO.ptr, None) == 0
    _sync()
    got, exp = dO.download((m, g), np.float64), rr.normalise_rows(X)
    assert (exp[[0, 255, 256, m - 1]] == 0.0).all() and not np.signbit(exp[0]).any()
    bad = np.argwhere(_bits(got) != _bits(exp))
    assert bad.shape[0] == 0, "g=%d: %d values differ, first at %s: %r != %r" % (g, bad.shape[0], bad[0], got[tuple(bad[0])], exp[tuple(bad[0])])

"""The f16 operand packer (pack_ctiles_kernel, nabo_amd/csrc/pack.hip) byte for byte against the numpy restatement of its
rule (tests/_pack_ref.py, itself checked by hand in tests/test_pack_ref_cpu.py): every byte of every tile, norm64 and the
running norm maximum.  The C ABI hands no packed buffer back, so the kernels are driven through the launchers the library
already exports for its own translation units (nabo::pack_cref_launch / nabo::pack_cquery_launch, by their mangled names;
declared in nabo_amd/csrc/launch.h) on buffers from nabo_dev_malloc: no new entry point.

Cases: g in {1, 7, 8, 31, 50, 61, 64, 100, 125} x cells in {1, 31, 32, 33, 95, 1000, 4097} -- last tiles with padding
cells, and three all-padding tiles behind them (the library allocates such split padding), so a block of several tiles is
partly empty -- each as references and as targets, one-product operands (NSEG 1) in both register layouts and the f16x3
split (NSEG 3, g < 64: the library has no f16x3 filter beyond), references with and without a mask and with a row
permutation; from 31 cells on, rows that hold NaN, +inf, -inf and a value beyond the f16 range.
"""
import ctypes as C

import numpy as np
import pytest

import _pack_ref as pr

pytestmark = pytest.mark.gpu

CREF = "_ZN4nabo16pack_cref_launchEPKdliS1_dilPKhPhPjbP12ihipStream_tPKji"
CQUERY = "_ZN4nabo18pack_cquery_launchEPKdliS1_dilPhPdbP12ihipStream_tPKji"
GS = [1, 7, 8, 31, 50, 61, 64, 100, 125]
CELLS = [1, 31, 32, 33, 95, 1000, 4097]


def _launchers():
    from nabo_amd import _lib
    L = _lib.lib()
    vp, i32, i64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
    cref, cquery = getattr(L, CREF), getattr(L, CQUERY)
    cref.argtypes = [vp, i64, i32, vp, dbl, i32, i64, vp, vp, vp, C.c_bool, vp, vp, i32]
    cquery.argtypes = [vp, i64, i32, vp, dbl, i32, i64, vp, vp, C.c_bool, vp, vp, i32]
    cref.restype = cquery.restype = C.c_int
    return cref, cquery


def _inputs(g, n):
    rng = np.random.default_rng(1000 * g + n)
    V = rng.standard_normal((n, g)) * rng.uniform(0.2, 3.0, size=g)[None, :] + rng.uniform(-5, 5, size=g)[None, :]
    centre = V.mean(axis=0) + rng.uniform(0.05, 0.1, size=g)        # (never a row itself: one cell, one component)
    amax = np.abs(V - centre).max()
    scale = 2.0 ** (12 - int(np.ceil(np.log2(amax))))          # as the library scales: max |v| in (2^11, 2^12]
    if n >= 31:
        V[3, g // 2] = np.nan
        V[n - 1, 0] = np.inf                                    # in the padded last tile
        V[17, g - 1] = -np.inf
        V[n // 2, g // 3] = centre[g // 3] + 40000.0 / scale    # finite, beyond the f16 range once scaled
        V[5, 0] = centre[0] + 30000.0 / scale                   # the last value inside it
    mask = (rng.random(n) < 0.3).astype(np.uint8)
    perm = rng.permutation(n).astype(np.uint32)
    return V, centre, scale, mask, perm


@pytest.mark.parametrize("n", CELLS)
@pytest.mark.parametrize("g", GS)
def test_packed_bytes_equal_reference(gpu_lib, g, n):
    from nabo_amd import _knn, _lib
    cref, cquery = _launchers()
    V, centre, scale, mask, perm = _inputs(g, n)
    ntiles = (n + 31) // 32 + 3
    kc_max = pr.pick_kc(g, 3 if g < 64 else 1)
    dV = _knn.DeviceBuffer(V.nbytes).upload(V)
    dC = _knn.DeviceBuffer(centre.nbytes).upload(centre)
    dM = _knn.DeviceBuffer(n).upload(mask)
    dP = _knn.DeviceBuffer(4 * n).upload(perm)
    dOut = _knn.DeviceBuffer(ntiles * kc_max * 1024)
    dNorm = _knn.DeviceBuffer(8 * n)
    dMax = _knn.DeviceBuffer(4)
    sync = lambda: _lib.check(_lib.lib().nabo_dev_synchronize(0))
    try:
        for nseg in ((1, 3) if g < 64 else (1,)):
            kc = pr.pick_kc(g, nseg)
            for layout16 in (True, False):
                for is_ref in (True, False):
                    variants = [(None, None)]
                    if is_ref:
                        variants.append((mask, None))
                    if layout16:
                        variants.append((mask if is_ref else None, perm))
                    for mk, pm in variants:
                        what = "g=%d n=%d nseg=%d layout16=%s %s mask=%s perm=%s" % (
                            g, n, nseg, layout16, "ref" if is_ref else "target", mk is not None, pm is not None)
                        dOut.upload(np.full(ntiles * kc * 1024, 0xA5, dtype=np.uint8))       # every byte must be written
                        dNorm.upload(np.full(n, -7.0))
                        dMax.upload(np.zeros(1, dtype=np.uint32))
                        if is_ref:
                            rc = cref(dV.ptr, n, g, dC.ptr, scale, kc, ntiles, dM.ptr if mk is not None else None, dOut.ptr,
                                      dMax.ptr, layout16, None, dP.ptr if pm is not None else None, nseg)
                        else:
                            rc = cquery(dV.ptr, n, g, dC.ptr, scale, kc, ntiles, dOut.ptr, dNorm.ptr, layout16, None,
                                        dP.ptr if pm is not None else None, nseg)
                        assert rc == 0, what
                        sync()
                        got = dOut.download((ntiles, kc, 64, 8), np.uint16)
                        exp, norm64, nmax = pr.pack_reference(V, centre, scale, kc, ntiles, is_ref, layout16, nseg, mk, pm)
                        diff = np.argwhere(got != exp)
                        assert diff.shape[0] == 0, "%s: %d f16 words differ, first at (tile, register, lane, j) = %s: %#06x != %#06x" % (
                            what, diff.shape[0], diff[0].tolist(), got[tuple(diff[0])], exp[tuple(diff[0])])
                        if is_ref:
                            assert int(dMax.download((1,), np.uint32)[0]) == nmax, what
                        else:
                            assert np.array_equal(dNorm.download((n,), np.uint64), norm64.view(np.uint64)), what
    finally:
        for b in (dV, dC, dM, dP, dOut, dNorm, dMax):
            b.free()


def test_norm_maximum_survives_the_deferred_read(gpu_lib):
    """The largest reference norm reaches the refine's certificate whether or not the host waited for it behind the pack:
    set_ref, set_mask and a second set_ref in a row (each invalidates the read before it), then queries -- same lists as
    an index that is queried straight away, and every row certified by the same pass."""
    import nabo_amd
    rng = np.random.default_rng(77)
    Y1, Y2 = rng.standard_normal((4000, 50)), 3.0 * rng.standard_normal((4000, 50)) + 1.0
    X = rng.standard_normal((1500, 50))
    mask = (rng.random(4000) < 0.2).astype(np.uint8)
    a = nabo_amd.KnnIndex(4000, 50, metric=nabo_amd.EUCLIDEAN)
    a.set_ref(Y1)
    a.set_mask(mask)
    a.set_ref(Y2)
    ia, da = a.query(X, 15)
    pa = a.last_row_pass(1500)
    b = nabo_amd.KnnIndex(4000, 50, metric=nabo_amd.EUCLIDEAN)
    b.set_ref(Y2)
    ib, db = b.query(X, 15)
    assert np.array_equal(ia, ib) and np.array_equal(da, db) and np.array_equal(pa, b.last_row_pass(1500))
    d2 = ((X[:200, None, :] - Y2[None, :, :]) ** 2).sum(axis=2)
    assert np.array_equal(np.sort(ia[:200], axis=1), np.sort(np.argsort(d2, axis=1, kind="stable")[:, :15], axis=1))
    a.close()
    b.close()

"""A plain numpy restatement of the f16 operand packing (pack_ctiles_kernel, nabo_amd/csrc/pack.hip): what every byte of
a packed tile, norm64 and the running norm maximum must be.  Written from the rule in the kernel's comment block, not
from its code: centre, scale by a power of two, round to fp32, split into f16 hi + lo, the norm / error slots, and the two
register layouts.  tests/test_pack_ref_cpu.py checks it against cases worked out by hand."""
import numpy as np

F16_LIMIT = np.float32(30000.0)          # a component beyond it (or NaN / inf) takes the cell out of the filter
TWO_M15 = np.float32(2.0 ** -15)
ER_FLOOR = np.float32(2.0 ** -13)
ER_REF = 1.002 * 1.001953125             # ey = f16(1.002 ||rep_y||), rounded up by (1 + 2^-9)
ER_TGT = 0.001953125 * 1.01 * 1.001953125        # tx = f16(2^-9 1.01 ||rep_x||), likewise


def slots_needed(g, nseg):
    return g + 3 if nseg == 1 else 3 * (g + 1)


def pick_kc(g, nseg):
    """steps of 16 slots, an even number of them (the 16x16x32 layout takes them in pairs)"""
    return 2 * ((slots_needed(g, nseg) + 31) // 32)


def cell_values(V, centre, scale, is_ref, nseg, mask=None):
    """Per cell: hi, lo (float32 arrays [n][g], the f16 values), bad, ss (float64, SCALED units) and the three norm slots
    nh, nl, er (float32) of a LIVE cell."""
    V = np.asarray(V, dtype=np.float64)
    n, g = V.shape
    with np.errstate(all="ignore"):
        f = ((V - np.asarray(centre, dtype=np.float64)[None, :]) * np.float64(scale)).astype(np.float32)
        bad = ~(np.abs(f) <= F16_LIMIT).all(axis=1)
        hi = f.astype(np.float16).astype(np.float32)
        lo = (f - hi).astype(np.float16).astype(np.float32)
        rep = hi.astype(np.float64) + lo.astype(np.float64)
        ss = np.zeros(n, dtype=np.float64)
        for e in range(g):                                   # sequential, in component order
            ss = ss + rep[:, e] * rep[:, e]
        nh = np.zeros(n, dtype=np.float32)
        nl = np.zeros(n, dtype=np.float32)
        er = np.zeros(n, dtype=np.float32)
        if is_ref:
            masked = np.zeros(n, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
            fin = ~bad & ~masked
            nf = np.full(n, np.inf, dtype=np.float32)
            nf[fin] = ss[fin].astype(np.float32) * TWO_M15
            nh = nf.astype(np.float16).astype(np.float32)
            nl[fin] = (nf[fin] - nh[fin]).astype(np.float16).astype(np.float32)
            if nseg == 1:
                er[fin] = np.maximum((np.sqrt(ss[fin]) * ER_REF).astype(np.float32), ER_FLOOR)
        else:
            fin = ~bad
            nh[:] = 32768.0
            nl[:] = 32768.0
            if nseg == 1:
                er[fin] = -np.maximum((np.sqrt(ss[fin]) * ER_TGT).astype(np.float32), ER_FLOOR)
    return hi, lo, bad, ss, nh, nl, er, fin


def pack_reference(V, centre, scale, kc, ntiles, is_ref, layout16, nseg, mask=None, perm=None):
    """-> (tile bytes as uint16 [ntiles][kc][64][8], norm64 [n] (targets) or None, norm maximum bits (references) or None).
    perm: packed position i holds row perm[i] (the mask is indexed by ROW, norm64 by POSITION)."""
    V = np.asarray(V, dtype=np.float64)
    if perm is not None:
        V = V[perm]
        mask = None if mask is None else np.asarray(mask)[perm]
    n, g = V.shape
    hi, lo, bad, ss, nh, nl, er, fin = cell_values(V, centre, scale, is_ref, nseg, mask)
    nslots = 16 * kc
    assert slots_needed(g, nseg) <= nslots and (not layout16 or kc % 2 == 0)
    ncp = 32 * ntiles
    assert ncp >= n
    # slot values per padded cell [ncp][nslots], float32, before the final rounding to f16
    S = np.zeros((ncp, nslots), dtype=np.float32)
    ok = ~bad
    sgn = np.float32(1.0 if is_ref else -2.0)
    pad_nh = np.float32(np.inf) if is_ref else np.float32(32768.0 if nseg == 1 else 0.0)
    pad_nl = np.float32(0.0) if is_ref else pad_nh
    NH = np.full(ncp, pad_nh, dtype=np.float32); NH[:n] = nh
    NL = np.full(ncp, pad_nl, dtype=np.float32); NL[:n] = nl
    ER = np.zeros(ncp, dtype=np.float32); ER[:n] = er
    H = np.zeros((ncp, g), dtype=np.float32); H[:n][ok] = hi[ok] * sgn
    Lo = np.zeros((ncp, g), dtype=np.float32); Lo[:n][ok] = lo[ok] * sgn
    if nseg == 1:
        S[:, :g] = H
        S[:, g], S[:, g + 1], S[:, g + 2] = NH, NL, ER
    else:
        g1 = g + 1
        segs = (H, Lo, H) if is_ref else (H, H, Lo)
        for s in range(3):
            S[:, s * g1:s * g1 + g] = segs[s]
        S[:, g], S[:, g1 + g] = NH, NL
    with np.errstate(all="ignore"):
        S16 = S.astype(np.float16).reshape(ntiles, 32, nslots)
    out = np.zeros((ntiles, kc, 64, 8), dtype=np.float16)
    lane = np.arange(64)
    if layout16:
        ks = kc // 2
        for h in range(2):
            for s in range(ks):
                cells = 16 * h + (lane & 15)
                p0 = 32 * s + 8 * (lane >> 4)
                for j in range(8):
                    out[:, h * ks + s, :, j] = S16[:, cells, p0 + j]
    else:
        for s in range(kc):
            cells = lane & 31
            p0 = 16 * s + 8 * (lane >> 5)
            for j in range(8):
                out[:, s, :, j] = S16[:, cells, p0 + j]
    if is_ref:
        bits = ss[fin].astype(np.float32).view(np.uint32)
        return out.view(np.uint16), None, int(bits.max()) if bits.size else 0
    with np.errstate(all="ignore"):
        norm64 = np.where(bad, np.nan, ss / (np.float64(scale) * np.float64(scale)))
    return out.view(np.uint16), norm64, None

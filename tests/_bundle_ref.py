"""The yardstick of edge bundling: include/nabo_bundle.h restated in float64 numpy, one function per step, every sum in the
header's order (numpy contracts nothing into an fma; np.cumsum adds sequentially).  The blur weights come from the
library's own host function, as the header prescribes, so that no `exp` can differ.

`margins`, where a function takes it, is a dict that collects how close the step's integer decisions came to their
thresholds: "m" |L / tl - nearest integer| (L > 0, below the P_MAX clamp), "pixel" |q * A - nearest integer| (q exactly 0
or 1 left out: such a value is a copied end point or a clamp's constant, the same bits on every device), "j"
|c_j - t_i| over every interior sample and every c_j.  tests/test_bundle_cpu.py demands all of them above 1e-9 on the
GPU tests' inputs: a condition on the inputs, which lets the GPU tests ask for equal integers everywhere.
"""
import numpy as np

P_MAX = 256
DEFAULTS = {"initial_bandwidth": 0.05, "decay": 0.7, "iterations": 4, "accuracy": 500, "advect_iterations": 50,
            "resample_every": 2, "min_segment_length": 0.008, "max_segment_length": 0.016, "tension": 0.3, "smooth_passes": 10}


def _note(margins, key, value):
    if margins is not None:
        margins[key] = min(margins.get(key, np.inf), float(value))


def target_length(p):
    return (p["min_segment_length"] + p["max_segment_length"]) / 2


def normalise(pos):
    pos = np.asarray(pos, dtype=np.float64)
    lo, span = pos.min(axis=0), pos.max(axis=0) - pos.min(axis=0)
    q = np.zeros_like(pos)
    for a in range(2):
        if span[a] != 0:
            q[:, a] = (pos[:, a] - lo[a]) / span[a]
    return q, lo, span


def straight(q, src, dst):
    E = len(src)
    pts = np.empty((2 * E, 2))
    pts[0::2], pts[1::2] = q[src], q[dst]
    return 2 * np.arange(E + 1, dtype=np.int64), pts


def resample_one(P, tl, margins=None):
    p = P.shape[0]
    d = P[1:] - P[:-1]
    seg = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    c = np.concatenate([[0.0], np.cumsum(seg)])
    L = c[p - 1]
    if L == 0:
        return np.stack([P[0], P[p - 1]])
    r = L / tl
    m = int(min(max(np.ceil(r) + 1, 2), P_MAX))
    if np.ceil(r) + 1 < P_MAX + 8:
        _note(margins, "m", abs(r - np.rint(r)))
    Q = np.empty((m, 2))
    Q[0], Q[m - 1] = P[0], P[p - 1]
    if m > 2:
        t = np.arange(1, m - 1, dtype=np.float64) * (L / (m - 1))
        if margins is not None:
            _note(margins, "j", np.abs(c[None, :] - t[:, None]).min())
        j = np.minimum(np.searchsorted(c, t, side="right") - 1, p - 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(seg[j] == 0, 0.0, (t - c[j]) / seg[j])
        Q[1:m - 1] = P[j] + (P[j + 1] - P[j]) * f[:, None]
    return Q


def resample(off, pts, tl, margins=None):
    out = [resample_one(pts[off[e]:off[e + 1]], tl, margins) for e in range(len(off) - 1)]
    noff = np.concatenate([[0], np.cumsum([len(x) for x in out])]).astype(np.int64)
    return noff, np.concatenate(out)


def pixel(q, A, margins=None):
    v = q * float(A)
    if margins is not None:
        inner = v[(q != 0.0) & (q != 1.0)]
        if inner.size:
            _note(margins, "pixel", np.abs(inner - np.rint(inner)).min())
    return np.clip(np.trunc(v).astype(np.int64), 0, A)


def density(pts, A, margins=None):
    u, v = pixel(pts[:, 0], A, margins), pixel(pts[:, 1], A, margins)
    return np.bincount(u * (A + 1) + v, minlength=(A + 1) * (A + 1)).astype(np.uint32).reshape(A + 1, A + 1)


def blur_weights(b):
    from nabo_amd import _bundle
    return _bundle.blur_weights(b)


def blur_axis(img, w, axis):
    R = (len(w) - 1) // 2
    n = img.shape[axis]
    acc = np.zeros(img.shape, dtype=np.float64)
    for t in range(-R, R + 1):
        if abs(t) >= n:
            continue
        term = np.zeros(img.shape, dtype=np.float64)      # term[u] = w_t * img[u + t], 0 outside the image
        dst = [slice(None)] * 2
        src = [slice(None)] * 2
        dst[axis] = slice(max(0, -t), n - max(0, t))
        src[axis] = slice(max(0, t), n - max(0, -t))
        term[tuple(dst)] = w[t + R] * img[tuple(src)]
        acc = acc + term
    return acc


def field(img, b):
    """(blurred, GX, GY) of a count image for a bandwidth of b pixels"""
    w = blur_weights(b)
    B = blur_axis(blur_axis(img.astype(np.float64), w, 0), w, 1)
    D = B / B.max()
    A = img.shape[0] - 1
    ip, im = np.minimum(np.arange(A + 1) + 1, A), np.maximum(np.arange(A + 1) - 1, 0)
    gx, gy = D[ip, :] - D[im, :], D[:, ip] - D[:, im]
    mag = np.sqrt(gx * gx + gy * gy) + 1e-5
    return B, gx / mag, gy / mag


def interior(off, n):
    m = np.ones(n, dtype=bool)
    m[off[:-1]] = False
    m[off[1:] - 1] = False
    return m


def advect_step(off, pts, GX, GY, A, margins=None):
    i = np.flatnonzero(interior(off, len(pts)))
    out = pts.copy()
    u, v = pixel(pts[i, 0], A, margins), pixel(pts[i, 1], A, margins)
    out[i, 0] = np.minimum(np.maximum(pts[i, 0] + GX[u, v] / float(A), 0.0), 1.0)
    out[i, 1] = np.minimum(np.maximum(pts[i, 1] + GY[u, v] / float(A), 0.0), 1.0)
    return out


def advect(off, pts, GX, GY, A, n_steps, resample_every, tl, margins=None):
    """one round of n_steps steps"""
    for s in range(1, n_steps + 1):
        pts = advect_step(off, pts, GX, GY, A, margins)
        if s % resample_every == 0 or s == n_steps:
            off, pts = resample(off, pts, tl, margins)
    return off, pts


def smooth(off, pts, tension, passes):
    i = np.flatnonzero(interior(off, len(pts)))
    keep, half = 1.0 - tension, tension * 0.5
    for _ in range(passes):
        new = pts.copy()
        new[i] = (keep * pts[i]) + (half * (pts[i - 1] + pts[i + 1]))
        pts = new
    return pts


def run_normalised(q, src, dst, margins=None, **params):
    p = dict(DEFAULTS, **params)
    A, tl = p["accuracy"], target_length(p)
    off, pts = straight(q, src, dst)
    off, pts = resample(off, pts, tl, margins)
    d = p["decay"]
    for _ in range(p["iterations"]):
        b = (p["initial_bandwidth"] * d) * float(A)
        d = d * p["decay"]
        if b < 2:
            break
        _, GX, GY = field(density(pts, A, margins), b)
        if p["advect_iterations"]:
            off, pts = advect(off, pts, GX, GY, A, p["advect_iterations"], p["resample_every"], tl, margins)
    return off, smooth(off, pts, p["tension"], p["smooth_passes"])


def with_nan_rows(off, pts):
    E = len(off) - 1
    out = np.full((len(pts) + E, 2), np.nan)
    at = np.arange(len(pts)) + (np.searchsorted(off, np.arange(len(pts)), side="right") - 1)
    out[at] = pts
    return out


def run(pos, src, dst, margins=None, **params):
    """(points with a NaN row after each edge, offsets): what nabo_amd.hammer_bundle returns"""
    q, lo, span = normalise(pos)
    off, pts = run_normalised(q, np.asarray(src), np.asarray(dst), margins, **params)
    return with_nan_rows(off, pts * span + lo), off


def figures(points, off, edges, pos, src, dst):
    """(mean distance from an edge's midpoint, by arc length, to the nearest other midpoint; mean ratio of the polyline's
    length to the straight edge's) over `edges` of a result with NaN rows"""
    mids, ratio = [], []
    for e in edges:
        P = points[off[e] + e:off[e + 1] + e]
        seg = np.sqrt(((P[1:] - P[:-1]) ** 2).sum(axis=1))
        c = np.concatenate([[0.0], np.cumsum(seg)])
        j = min(int(np.searchsorted(c, c[-1] / 2, side="right")) - 1, len(P) - 2)
        f = 0.0 if seg[j] == 0 else (c[-1] / 2 - c[j]) / seg[j]
        mids.append(P[j] + (P[j + 1] - P[j]) * f)
        ratio.append(c[-1] / np.sqrt(((pos[src[e]] - pos[dst[e]]) ** 2).sum()))
    mids = np.array(mids)
    d = np.sqrt(((mids[:, None, :] - mids[None, :, :]) ** 2).sum(axis=2))
    np.fill_diagonal(d, np.inf)
    return float(d.min(axis=1).mean()), float(np.mean(ratio))

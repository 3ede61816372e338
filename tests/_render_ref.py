"""The yardstick of the rasteriser: include/nabo_render.h's definition in plain numpy, float64 for the coordinate-to-pixel
step and int64 after it.  The device's images must equal these byte for byte.  `margins`, where given, collects how far the
float64 step's results stay from the integers at which a floor would flip (tests/test_render_cpu.py asks 1e-9 of every
input the GPU tests use)."""
import numpy as np

CLAMP = float(2 ** 20)
R_MAX = 1024


def pixel_coord(c, c0, c1, n, margins=None):
    """px of the definition, clamped; one IEEE operation per step"""
    c = np.asarray(c, dtype=np.float64)
    p = ((c - np.float64(c0)) / (np.float64(c1) - np.float64(c0))) * np.float64(n)
    if margins is not None and p.size:
        q = p[np.abs(p) < 2 * CLAMP]   # (beyond that no rounding brings a point back under the clamp)
        for name, x in (("pixel", q), ("subpixel", q * 16)):
            if x.size:
                margins[name] = min(margins.get(name, np.inf), float(np.abs(x - np.round(x)).min()))
    return np.minimum(np.maximum(p, -CLAMP), CLAMP)


def point_pixels(pts, W, H, view, margins=None):
    """(u, v) int64 of points [n, 2]"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    px = pixel_coord(pts[:, 0], view[0], view[1], W, margins)
    py = pixel_coord(pts[:, 1], view[2], view[3], H, margins)
    return np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)


def segment_pixels(u0, v0, u1, v1):
    """the s pixels i = 0 .. s - 1 of one segment, then its end pixel: [(u, v)], s + 1 of them"""
    du, dv = u1 - u0, v1 - v0
    s = max(abs(du), abs(dv))
    out = [(u0 + (2 * i * du + s) // (2 * s), v0 + (2 * i * dv + s) // (2 * s)) for i in range(s)]
    return out + [(u1, v1)]


def _accumulate(img, u, v, W, H):
    ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    img += np.bincount(v[ok] * W + u[ok], minlength=W * H)


def edge_counts(off, pts, W, H, view, margins=None, batch=1 << 22):
    """uint32 [H, W] of the polylines pts[off[e]:off[e + 1]]"""
    off = np.asarray(off, dtype=np.int64)
    u, v = point_pixels(pts, W, H, view, margins)
    n = u.shape[0]
    img = np.zeros(W * H, dtype=np.int64)
    if n == 0:
        return img.reshape(H, W).astype(np.uint32)
    assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 2).all()
    last = np.zeros(n, dtype=bool)
    last[off[1:] - 1] = True
    nxt = np.minimum(np.arange(n) + 1, n - 1)
    du, dv = np.where(last, 0, u[nxt] - u), np.where(last, 0, v[nxt] - v)
    s = np.maximum(np.abs(du), np.abs(dv))
    steps = np.where(last, 1, s)            # a segment draws i = 0 .. s - 1, a last point its own pixel
    s = np.where(last, 1, s)                # (for a last point: du = dv = 0, floor(1 / 2) = 0)
    g0 = 0
    while g0 < n:
        g1, tot = g0, 0
        while g1 < n and (g1 == g0 or tot + steps[g1] <= batch):
            tot += steps[g1]
            g1 += 1
        k = np.repeat(np.arange(g0, g1), steps[g0:g1])
        start = np.concatenate([[0], np.cumsum(steps[g0:g1])])[:-1]
        i = np.arange(k.shape[0], dtype=np.int64) - np.repeat(start, steps[g0:g1])
        sk = np.maximum(s[k], 1)
        _accumulate(img, u[k] + (2 * i * du[k] + sk) // (2 * sk), v[k] + (2 * i * dv[k] + sk) // (2 * sk), W, H)
        g0 = g1
    assert img.max() < 2 ** 32
    return img.reshape(H, W).astype(np.uint32)


def straight(pos, src, dst):
    """(off, pts) of the straight edges as two-point polylines"""
    pos = np.asarray(pos, dtype=np.float64)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    pts = np.stack([pos[src], pos[dst]], axis=1).reshape(-1, 2)
    return 2 * np.arange(len(src) + 1, dtype=np.int64), pts


def disc_pixels(cx, cy, R):
    """the pixels (u, v) a node of centre (cx, cy) and radius R, all in 1/16 pixel, covers (canvas or not)"""
    pu, pv = cx >> 4, cy >> 4
    u = np.arange(min((cx - R - 8) >> 4, pu) - 1, max((cx + R) >> 4, pu) + 2)
    v = np.arange(min((cy - R - 8) >> 4, pv) - 1, max((cy + R) >> 4, pv) + 2)
    uu, vv = np.meshgrid(u, v)
    cov = ((16 * uu + 8 - cx) ** 2 + (16 * vv + 8 - cy) ** 2 <= R * R) | ((uu == pu) & (vv == pv))
    return sorted(zip(uu[cov].tolist(), vv[cov].tolist()))


def node_layers(pos, radius16, rgb, W, H, view, margins=None):
    """(count uint32 [H, W], sums uint32 [H, W, 3])"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    radius16 = np.broadcast_to(np.asarray(radius16, dtype=np.int64), (pos.shape[0],))
    rgb = np.broadcast_to(np.asarray(rgb, dtype=np.int64), (pos.shape[0], 3))
    assert radius16.min(initial=0) >= 0 and radius16.max(initial=0) <= R_MAX
    px = pixel_coord(pos[:, 0], view[0], view[1], W, margins)
    py = pixel_coord(pos[:, 1], view[2], view[3], H, margins)
    cx, cy = np.floor(px * 16).astype(np.int64), np.floor(py * 16).astype(np.int64)
    cnt, sums = np.zeros((H, W), dtype=np.int64), np.zeros((H, W, 3), dtype=np.int64)
    uu, vv = np.meshgrid(np.arange(W), np.arange(H))
    for k in range(pos.shape[0]):
        R, pu, pv = int(radius16[k]), int(cx[k]) >> 4, int(cy[k]) >> 4
        u0, u1 = max(min((int(cx[k]) - R - 8) >> 4, pu) - 1, 0), min(max((int(cx[k]) + R) >> 4, pu) + 1, W - 1)
        v0, v1 = max(min((int(cy[k]) - R - 8) >> 4, pv) - 1, 0), min(max((int(cy[k]) + R) >> 4, pv) + 1, H - 1)
        if u0 > u1 or v0 > v1:
            continue
        bu, bv = uu[v0:v1 + 1, u0:u1 + 1], vv[v0:v1 + 1, u0:u1 + 1]
        cov = ((16 * bu + 8 - cx[k]) ** 2 + (16 * bv + 8 - cy[k]) ** 2 <= R * R) | ((bu == pu) & (bv == pv))
        cnt[v0:v1 + 1, u0:u1 + 1] += cov
        sums[v0:v1 + 1, u0:u1 + 1] += cov[:, :, None] * rgb[k]
    assert sums.max(initial=0) < 2 ** 32
    return cnt.astype(np.uint32), sums.astype(np.uint32)


def alpha_lut(alpha, L):
    k = 1.0 - float(alpha)
    t, out = 1.0, np.empty(L, dtype=np.uint8)
    for c in range(L):
        out[c] = int(np.floor(255.0 * (1.0 - t) + 0.5))
        t = t * k
    return out


def compose(ce, cn, sums, edge_rgb, lut_e, lut_n):
    """uint8 [H, W, 4]"""
    ce, cn, sums = np.asarray(ce, dtype=np.int64), np.asarray(cn, dtype=np.int64), np.asarray(sums, dtype=np.int64)
    lut_e, lut_n = np.asarray(lut_e, dtype=np.int64), np.asarray(lut_n, dtype=np.int64)
    Ae, An = lut_e[np.minimum(ce, len(lut_e) - 1)], lut_n[np.minimum(cn, len(lut_n) - 1)]
    safe = np.maximum(cn, 1)
    Cn = np.where(cn[..., None] > 0, (sums + (cn // 2)[..., None]) // safe[..., None], 0)
    t = Ae * (255 - An)
    den = 255 * An + t
    dsafe = np.maximum(den, 1)[..., None]
    Ce = np.asarray(edge_rgb, dtype=np.int64).reshape(3)
    Ck = np.where(den[..., None] > 0, ((255 * An)[..., None] * Cn + t[..., None] * Ce + (den // 2)[..., None]) // dsafe, 0)
    out = np.concatenate([Ck, ((den + 127) // 255)[..., None]], axis=-1)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def default_viewport(pos):
    pos = np.asarray(pos, dtype=np.float64)
    out = []
    for a in range(2):
        lo, hi = float(pos[:, a].min()), float(pos[:, a].max())
        pad = (hi - lo) * 0.05 if hi > lo else 0.5
        out += [lo - pad, hi + pad]
    return tuple(out)


def picture(W, H, view, lines=None, nodes=None, edge_rgb=(0, 0, 0), e_alpha=0.1, v_alpha=0.6, L=65536, margins=None):
    """the whole picture: lines = (off, pts) or None, nodes = (pos, radius16, rgb uint8) or None"""
    ce = edge_counts(lines[0], lines[1], W, H, view, margins) if lines is not None else np.zeros((H, W), dtype=np.uint32)
    if nodes is not None:
        cn, sums = node_layers(nodes[0], nodes[1], nodes[2], W, H, view, margins)
    else:
        cn, sums = np.zeros((H, W), dtype=np.uint32), np.zeros((H, W, 3), dtype=np.uint32)
    return compose(ce, cn, sums, edge_rgb, alpha_lut(e_alpha, L), alpha_lut(v_alpha, L))

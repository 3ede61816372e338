"""The fixed-seed inputs of the rasteriser's tests, shared by tests/test_render_cpu.py (which checks on the yardstick alone
that no pixel coordinate of theirs sits on an integer) and tests/test_render_gpu.py.  Points are chosen in pixel space, a
fraction of a pixel away from every pixel and 1/16-pixel border, and carried into layout coordinates."""
import functools

import numpy as np

import _bundle_ref as br
import _render_ref as rr

SEED = 31
VIEW = (-3.7, 9.1, 2.2, 5.9)
CANVASES = ((37, 23), (1, 1), (64, 1), (257, 130))
LONG_CANVAS = (1024, 8)
E_COUNTS = (1, 63, 64, 65)
HOT = 100000
CLIPPED = ((37, 23, True), (257, 130, False), (1, 1, False))
BORDER_CANVASES = ((37, 23), (257, 130), LONG_CANVAS)


def _frac(rng, shape):
    """fractions of a pixel that are no multiple of 1/16 to within 1/160"""
    return (rng.integers(0, 16, size=shape) + 0.1 + 0.8 * rng.random(shape)) / 16


def to_layout(p, W, H, view=VIEW):
    """pixel coordinates [n, 2] -> layout coordinates"""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 2)
    return np.stack([view[0] + (p[:, 0] / W) * (view[1] - view[0]), view[2] + (p[:, 1] / H) * (view[3] - view[2])], axis=1)


def pack(lines):
    off = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.int64)
    return off, np.concatenate(lines).astype(np.float64)


def octants(W, H):
    """from one pixel to 16 directions -- every octant, horizontal, vertical, the exact diagonals -- both ways, and zero length"""
    rng = np.random.default_rng(SEED + W)
    c = np.array([W // 2, H // 2])
    lines = []
    for dx, dy in ((9, 0), (9, 4), (9, 9), (4, 9), (0, 9), (-4, 9), (-9, 9), (-9, 4), (-9, 0), (-9, -4), (-9, -9), (-4, -9), (0, -9),
                   (4, -9), (9, -9), (9, -4), (0, 0), (5, 2)):
        a, b = c + _frac(rng, 2), c + np.array([dx, dy]) + _frac(rng, 2)
        lines += [np.stack([a, b]), np.stack([b, a])]
    off, p = pack(lines)
    return off, to_layout(p, W, H)


def polylines(E, W, H, seed=0):
    """E polylines of 2, 3 or 9 .. 40 points (more than a short group's lanes), from a little outside the canvas"""
    rng = np.random.default_rng(SEED + 1000 * seed + E + W)
    lines = []
    for e in range(E):
        p = (2, 3, int(rng.integers(9, 41)))[e % 3]
        lines.append(np.floor(rng.uniform(-0.2, 1.2, size=(p, 2)) * [W, H]) + _frac(rng, (p, 2)))
    off, p = pack(lines)
    return off, to_layout(p, W, H)


def threshold_segments(short):
    """on the long canvas: two-point polylines of s = short - 1 .. short + 2 steps and a few times that, flat, steep and
    reversed; three-point ones whose first segment has exactly short and short + 1 steps"""
    W, H = LONG_CANVAS
    rng = np.random.default_rng(SEED + 5)
    lines = []
    for s in (short - 1, short, short + 1, short + 2, 3 * short + 1, 1000):
        for dy in (0, 3, -5):
            u0, v0 = int(rng.integers(2, W - s - 1)), int(rng.integers(5, 7)) if dy < 0 else 1
            a, b = np.array([u0, v0]) + _frac(rng, 2), np.array([u0 + s, v0 + dy]) + _frac(rng, 2)
            lines += [np.stack([a, b]), np.stack([b, a])]
    for s in (short, short + 1):
        a = np.array([3, 2]) + _frac(rng, 2)
        lines.append(np.stack([a, a + [s, 1], a + [s + 2, -1]]))
    off, p = pack(lines)
    return off, to_layout(p, W, H)


def clipped(W, H, clamp=True):
    """a zoomed viewport's segments: from inside to far outside, across with both ends outside, missing the canvas, and
    (clamp) with one or both ends beyond the +-2^20 clamp: up to 2^21 steps each, which the yardstick walks one by one"""
    rng = np.random.default_rng(SEED + 9 + W)
    far, beyond = 3000.0, 5.0e6
    inside = lambda: rng.uniform(0.1, 0.9, size=2) * [W, H]
    lines = []
    for ang in np.linspace(0.05, 2 * np.pi, 7, endpoint=False):
        d = np.array([np.cos(ang), np.sin(ang)])
        lines.append(np.stack([inside(), inside() + far * d]))                      # inside -> outside
        lines.append(np.stack([inside() - far * d, inside() + (far + 17) * d]))    # across
        lines.append(np.stack([inside() + far * d, inside() + far * d + [40.3, -25.7]]))   # misses
        if clamp:
            lines.append(np.stack([inside(), inside() + beyond * d]))                  # ends beyond the clamp
            lines.append(np.stack([inside() - beyond * d, inside() + beyond * d]))     # both ends beyond it
    if clamp:
        lines.append(np.stack([np.array([-beyond, 0.37 * H]), np.array([beyond, 0.61 * H])]))
        lines.append(np.stack([np.array([0.43 * W, beyond]), np.array([0.45 * W, -beyond]), inside()]))
    off, p = pack(lines)
    return off, to_layout(p, W, H)


def hot_pixel(W, H):
    """HOT two-point polylines inside pixel (W // 3, H // 2)"""
    rng = np.random.default_rng(SEED + 11)
    p = np.array([W // 3, H // 2]) + _frac(rng, (2 * HOT, 2))
    return 2 * np.arange(HOT + 1, dtype=np.int64), to_layout(p, W, H)


def node_radii(g):
    """radii in 1/16 pixel: 0, 1/16, around one pixel, around the small / large threshold, large, R_MAX"""
    t = g["node_small_r"]
    return np.array([0, 1, 8, 15, 16, 24, 40, t - 1, t, t + 1, t + 2, 100, 300, g["r_max"]], dtype=np.int64)


def nodes(n, W, H, g, seed=0):
    """(pos, radius16, rgb): n nodes from a little outside the canvas, radii cycling through node_radii"""
    rng = np.random.default_rng(SEED + 2000 * seed + n + W)
    p = np.floor(rng.uniform(-0.3, 1.3, size=(n, 2)) * [W, H]) + _frac(rng, (n, 2))
    return to_layout(p, W, H), node_radii(g)[np.arange(n) % 14], rng.integers(0, 256, size=(n, 3)).astype(np.uint8)


def border_nodes(W, H, g):
    """discs cut by each border and by each corner, and wholly outside, at radii of both paths"""
    rng = np.random.default_rng(SEED + 13 + W)
    t = g["node_small_r"]
    spots = [(0, H // 2), (W - 1, H // 2), (W // 2, 0), (W // 2, H - 1), (0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1),
             (-3, H // 2), (W + 2, -2), (-400, -300), (W + 90, H // 2)]
    pos, rad = [], []
    for s in spots:
        for R in (40, t, t + 1, 300):
            pos.append(np.array(s) + _frac(rng, 2))
            rad.append(R)
    return to_layout(np.array(pos), W, H), np.array(rad, dtype=np.int64), rng.integers(0, 256, size=(len(rad), 3)).astype(np.uint8)


def coincident_nodes(W, H):
    """1 000 nodes on one spot, of different colours"""
    rng = np.random.default_rng(SEED + 17)
    p = np.tile(np.array([W // 2, H // 3]) + _frac(rng, 2), (1000, 1))
    return to_layout(p, W, H), np.full(1000, 24, dtype=np.int64), rng.integers(0, 256, size=(1000, 3)).astype(np.uint8)


def stacked_lines(W, H, counts):
    """counts[j] two-point polylines inside pixel (2 + 3 j, 1)"""
    rng = np.random.default_rng(SEED + 19)
    p = [np.array([2 + 3 * j, 1]) + _frac(rng, (2 * c, 2)) for j, c in enumerate(counts) if c]
    p = np.concatenate(p)
    return 2 * np.arange(len(p) // 2 + 1, dtype=np.int64), to_layout(p, W, H)


def stacked_nodes(W, H, counts):
    """counts[j] nodes of radius 0 on pixel (2 + 3 j, 1) and on the pixel above it"""
    rng = np.random.default_rng(SEED + 23)
    p = [np.array([2 + 3 * j, 1 + up]) + _frac(rng, (c, 2)) for j, c in enumerate(counts) for up in (0, 1) if c]
    p = np.concatenate(p)
    return to_layout(p, W, H), np.zeros(len(p), dtype=np.int64), rng.integers(0, 256, size=(len(p), 3)).astype(np.uint8)


WHOLE = dict(width=257, height=130, e_alpha=0.3, v_alpha=0.6, edge_rgb=np.array([40, 90, 200], dtype=np.uint8))
WHOLE_BUNDLE = dict(accuracy=64)


def whole_graph():
    """300 nodes in 5 blobs, 4 nearest neighbours each and 150 long edges; radii in pixels and colours"""
    rng = np.random.default_rng(SEED + 29)
    centres = rng.random((5, 2)) * 10
    pos = centres[np.arange(300) % 5] + rng.normal(size=(300, 2)) * 0.7
    d = ((pos[:, None, :] - pos[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind="stable")[:, :4]
    a = rng.integers(0, 300, size=150)
    b = (a + 1 + rng.integers(0, 299, size=150)) % 300
    src, dst = np.concatenate([np.repeat(np.arange(300), 4), a]).astype(np.int64), np.concatenate([nn.reshape(-1), b]).astype(np.int64)
    radius = rng.integers(4, 60, size=300) / 16.0 + 1 / 64   # k/16 + 1/64 pixel: floor(r * 16 + 0.5) is k
    return pos, src, dst, radius, rng.integers(0, 256, size=(300, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def whole_bundled():
    """the yardstick's bundling of whole_graph: (off, pts without NaN rows, the bundling margins)"""
    pos, src, dst, _, _ = whole_graph()
    m = {}
    pts, off = br.run(pos, src, dst, m, **WHOLE_BUNDLE)
    keep = np.ones(len(pts), dtype=bool)
    keep[off[1:] + np.arange(len(src))] = False
    return off, pts[keep], m


def whole_picture(bundled, margins=None):
    pos, src, dst, radius, rgb = whole_graph()
    lines = whole_bundled()[:2] if bundled else rr.straight(pos, src, dst)
    return rr.picture(WHOLE["width"], WHOLE["height"], rr.default_viewport(pos), lines, (pos, np.floor(radius * 16 + 0.5).astype(np.int64), rgb),
                      WHOLE["edge_rgb"], WHOLE["e_alpha"], WHOLE["v_alpha"], margins=margins)

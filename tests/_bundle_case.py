"""The fixed-seed inputs of the bundling tests, shared by tests/test_bundle_cpu.py (which checks on the yardstick alone
that no integer decision of theirs sits on a threshold), tests/test_bundle_gpu.py and tools/gen_golden_bundle.py."""
import numpy as np

import _bundle_ref as br

SEED = 20
TL = 0.012
RESAMPLE_E = (1, 15, 16, 17, 63, 64, 65, 1000)
RUN_A = (64, 500)


def graph():
    """400 nodes in 6 blobs, the 5 nearest neighbours of every node and 300 random long edges: 2 300 edges, the last 300
    of them the long ones.  (pos [400, 2], src, dst)"""
    rng = np.random.default_rng(SEED)
    centres = rng.random((6, 2)) * 10
    pos = centres[np.arange(400) % 6] + rng.normal(size=(400, 2)) * 0.6
    d = ((pos[:, None, :] - pos[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind="stable")[:, :5]
    src, dst = np.repeat(np.arange(400), 5), nn.reshape(-1)
    a = rng.integers(0, 400, size=300)
    b = (a + 1 + rng.integers(0, 399, size=300)) % 400
    return pos, np.concatenate([src, a]).astype(np.int64), np.concatenate([dst, b]).astype(np.int64)


LONG = np.arange(2000, 2300)


def _walk(rng, p, step):
    """a polyline of p points inside [0.05, 0.95]^2"""
    P = np.empty((p, 2))
    P[0] = 0.2 + 0.6 * rng.random(2)
    for j in range(1, p):
        P[j] = np.clip(P[j - 1] + rng.normal(size=2) * step, 0.05, 0.95)
    return P


def pack(lines):
    off = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.int64)
    return off, np.concatenate(lines).astype(np.float64)


def polylines(E, seed=SEED):
    """E polylines of mixed kinds: two points a short or a long way apart (the second outgrows a short group's room), a
    few points, more points than a short group holds"""
    rng = np.random.default_rng(seed + E)
    lines = []
    for e in range(E):
        kind = rng.integers(0, 4)
        if kind == 0:
            P = _walk(rng, 2, 0.004)
        elif kind == 1:
            P = np.stack([0.05 + 0.9 * rng.random(2), 0.05 + 0.9 * rng.random(2)])
        elif kind == 2:
            P = _walk(rng, int(rng.integers(3, 17)), 0.01)
        else:
            P = _walk(rng, int(rng.integers(17, 120)), 0.006)
        lines.append(P)
    return pack(lines)


def special_polylines():
    """a zero-length edge; lengths just below and just above tl; a 300-point zigzag of length 5, which hits P_MAX; interior
    zero-length segments; two points that coincide with a third between them"""
    zig = np.empty((300, 2))
    zig[:, 0] = 0.3 + (np.arange(300) % 2) * (5.0 / 299)
    zig[:, 1] = 0.5
    rep = np.array([[0.2, 0.2], [0.2, 0.2], [0.25, 0.2], [0.25, 0.2], [0.25, 0.2], [0.25, 0.31], [0.25, 0.31]])
    return pack([np.array([[0.4, 0.6], [0.4, 0.6]]),
                 np.array([[0.1, 0.1], [0.1 + TL * (1 - 1e-6), 0.1]]),
                 np.array([[0.1, 0.2], [0.1 + TL * (1 + 1e-6), 0.2]]),
                 zig, rep,
                 np.array([[0.7, 0.7], [0.7, 0.7], [0.7, 0.7]])])


def density_points(kind, A):
    """two-point edges for the density test"""
    rng = np.random.default_rng(SEED + A)
    if kind == "one_pixel":       # 4 096 points in one pixel
        P = (np.array([3.0, 5.0]) + 0.1 + 0.8 * rng.random((4096, 2))) / A
    elif kind == "ones":          # coordinates exactly 1.0 (and 0.0)
        P = rng.random((64, 2))
        P[::4, 0], P[1::4, 1], P[2::8] = 1.0, 1.0, 0.0
    else:
        P = rng.random((3000, 2))
    return 2 * np.arange(len(P) // 2 + 1, dtype=np.int64), P


def advect_state(A):
    """three-point edges whose ends sit in the image's outermost rows and columns (pixel 0, and pixel A, which only the
    coordinate 1.0 reaches) and whose middle points sit just inside: the density falls off towards the inside, and the step
    therefore clamps at 0 and at 1; plus a scatter of longer polylines"""
    rng = np.random.default_rng(SEED + 7)
    lines = []
    for k in range(40):
        y = 0.1 + 0.8 * rng.random(3)
        edge = 0.15 / A if k % 2 == 0 else 1.0
        x = np.array([edge, edge + (0.1 / A if k % 2 == 0 else -0.25 / A), edge])
        P = np.stack([x, y], axis=1)
        lines.append(P if k % 4 < 2 else P[:, ::-1])
    for k in range(60):
        lines.append(_walk(rng, int(rng.integers(3, 40)), 0.01))
    return pack(lines)


def smooth_state():
    rng = np.random.default_rng(SEED + 9)
    lines = [_walk(rng, 2, 0.1), _walk(rng, 3, 0.05)] + [_walk(rng, int(rng.integers(2, 60)), 0.02) for _ in range(70)]
    return pack(lines)


def dummy_graph(E):
    """nodes and edges for a handle whose state set_points replaces"""
    return np.array([[0.0, 0.0], [1.0, 1.0]]), np.zeros(E, dtype=np.int64), np.ones(E, dtype=np.int64)

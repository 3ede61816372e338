"""Plain float64 numpy restatement of include/nabo_layout.h (ForceAtlas2, every pair summed) and the graphs the layout
tests run on.  Pair terms are float64 on the float32-rounded positions; every sum is numpy's.  Beside each force it
returns the sum of the absolute values of its terms, which is what the tests' error bounds scale with."""
import numpy as np

DEFAULTS = dict(outbound_attraction_distribution=True, edge_weight_influence=1.0, jitter_tolerance=1.0, scaling_ratio=1.0,
                strong_gravity_mode=False, gravity=1.0)
D2_MIN = 2.0 ** -100
N_STEPS = 24          # iterations every case is stepped through
MARGIN = 1e-3         # relative distance S/T keeps from 2 and S/(jt T) from 1, from the second iteration on


class Graph:
    """the simple graph of a CSR in either arc direction: a pair keeps its LAST weight, a self-loop counts towards the
    degree and is no row entry; rows in ascending neighbour"""

    def __init__(self, ptr, nbr, w):
        n = len(ptr) - 1
        pairs = {}
        for i in range(n):
            for e in range(int(ptr[i]), int(ptr[i + 1])):
                j = int(nbr[e])
                pairs[(min(i, j), max(i, j))] = float(w[e])
        deg = np.zeros(n)
        arcs = []
        for (a, b), x in pairs.items():
            deg[a] += 1
            if a != b:
                deg[b] += 1
                arcs += [(a, b, x), (b, a, x)]
        arcs.sort()
        self.n = n
        self.mass = 1.0 + deg
        self.src = np.array([a[0] for a in arcs], dtype=np.int64)
        self.dst = np.array([a[1] for a in arcs], dtype=np.int64)
        self.w = np.array([a[2] for a in arcs], dtype=np.float64)


def simple_graph(n, lo, hi, w):
    """the same Graph from pairs lo < hi that are distinct already, with numpy alone"""
    lo, hi, w = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64), np.asarray(w, dtype=np.float64)
    assert (lo < hi).all() and len(np.unique(lo * n + hi)) == len(lo)
    src, dst, ww = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([w, w])
    o = np.lexsort((dst, src))
    g = Graph.__new__(Graph)
    g.n, g.mass = n, 1.0 + np.bincount(src, minlength=n).astype(np.float64)
    g.src, g.dst, g.w = src[o], dst[o], ww[o]
    return g


def start_state(pos0):
    pos0 = np.asarray(pos0, dtype=np.float64)
    z = np.zeros(len(pos0))
    return dict(x=pos0[:, 0].copy(), y=pos0[:, 1].copy(), dx=z.copy(), dy=z.copy(), speed=1.0, eff=1.0)


def repulsion_rows(g, x, y, rows, scaling_ratio, chunk=None):
    """step 2 for the nodes `rows` alone, each against every j: (rep, rep_abs) [len(rows), 2], float64 pair terms on the
    float32-rounded positions, rep_abs the sums of the absolute terms.  Rows are independent, so a sample of them costs
    len(rows) * n; `chunk` rows are in flight at a time (all of them by default)"""
    rows = np.asarray(rows, dtype=np.int64)
    xf, yf = x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    rep, rep_abs = np.empty((len(rows), 2)), np.empty((len(rows), 2))
    step_ = len(rows) if not chunk else int(chunk)
    for a in range(0, len(rows), max(step_, 1)):
        r = rows[a:a + step_]
        ddx, ddy = xf[r, None] - xf[None, :], yf[r, None] - yf[None, :]
        c = (scaling_ratio * g.mass[r])[:, None] * g.mass[None, :] / np.maximum(ddx * ddx + ddy * ddy, D2_MIN)
        tx, ty = c * ddx, c * ddy
        rep[a:a + step_] = np.stack([tx.sum(axis=1), ty.sum(axis=1)], axis=1)
        rep_abs[a:a + step_] = np.stack([np.abs(tx).sum(axis=1), np.abs(ty).sum(axis=1)], axis=1)
    return rep, rep_abs


def local_forces(g, x, y, **params):
    """steps 3 and 4 for every node, O(n + arcs): (grav, attr, attr_abs) [n, 2]; |grav| is its own sum of absolute terms"""
    p = dict(DEFAULTS, **params)
    n, mass = g.n, g.mass
    sr, grav_c = float(p["scaling_ratio"]), float(p["gravity"])
    oad = bool(p["outbound_attraction_distribution"])
    comp = float(np.mean(mass)) if oad else 1.0
    # 3. gravity
    r = np.sqrt(x * x + y * y)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = sr * mass * grav_c if p["strong_gravity_mode"] else mass * grav_c / r
    f = np.where(r > 0, f, 0.0)
    grav = -np.stack([x * f, y * f], axis=1)
    # 4. attraction, in row order
    ewi = float(p["edge_weight_influence"])
    e = np.ones_like(g.w) if ewi == 0 else g.w if ewi == 1 else np.power(g.w, ewi)
    f = -comp * e
    if oad:
        f = f / mass[np.minimum(g.src, g.dst)]
    ax, ay = (x[g.src] - x[g.dst]) * f, (y[g.src] - y[g.dst]) * f
    attr, attr_abs = np.zeros((n, 2)), np.zeros((n, 2))
    np.add.at(attr[:, 0], g.src, ax)
    np.add.at(attr[:, 1], g.src, ay)
    np.add.at(attr_abs[:, 0], g.src, np.abs(ax))
    np.add.at(attr_abs[:, 1], g.src, np.abs(ay))
    return grav, attr, attr_abs


def speed_step(n, S, T, speed, eff, jitter_tolerance):
    """step 6 from S, T > 0: (speed, eff, m_half, m_jt, target), the margins m_half = |S/T - 2| / 2 and
    m_jt = |S / (jt T) - 1| of its two comparisons"""
    speed, eff, jtol = float(speed), float(eff), float(jitter_tolerance)
    est = 0.05 * np.sqrt(float(n))
    jt = jtol * max(np.sqrt(est), min(10.0, est * T / (float(n) * float(n))))
    m_half = abs(S / T - 2.0) / 2.0
    if S / T > 2.0:
        if eff > 0.05:
            eff *= 0.5
        jt = max(jt, jtol)
    target = jt * eff * T / S
    m_jt = abs(S / (jt * T) - 1.0) if jt * T != 0 else np.inf
    if S > jt * T:
        if eff > 0.05:
            eff *= 0.7
    elif speed < 1000:
        eff *= 1.3
    speed += min(target - speed, 0.5 * speed)
    return float(speed), float(eff), m_half, m_jt, float(target)


def step(g, s, **params):
    """One iteration from the state s (x, y, dx, dy, speed, eff); returns the new state plus
    rep, grav, attr [n, 2] with rep_abs, grav_abs, attr_abs (sums of |term|), S, T, swing, stopped, and the margins
    m_half = |S/T - 2| / 2 and m_jt = |S / (jt T) - 1| of step 6's two comparisons."""
    p = dict(DEFAULTS, **params)
    n, mass = g.n, g.mass
    x, y = s["x"], s["y"]
    sr = float(p["scaling_ratio"])
    old = np.stack([s["dx"], s["dy"]], axis=1)
    # 2. repulsion
    rep, rep_abs = repulsion_rows(g, x, y, np.arange(n), sr)
    # 3. gravity, 4. attraction
    grav, attr, attr_abs = local_forces(g, x, y, **p)
    d = (rep + grav) + attr
    # 5. sums
    swing = mass * np.sqrt(((old - d) ** 2).sum(axis=1))
    tract = 0.5 * mass * np.sqrt(((old + d) ** 2).sum(axis=1))
    S, T = float(swing.sum()), float(tract.sum())
    out = dict(rep=rep, rep_abs=rep_abs, grav=grav, grav_abs=np.abs(grav), attr=attr, attr_abs=attr_abs, S=S, T=T, swing=swing,
               dx=d[:, 0].copy(), dy=d[:, 1].copy(), x=x.copy(), y=y.copy(), speed=s["speed"], eff=s["eff"], stopped=False,
               m_half=np.inf, m_jt=np.inf)
    # 6. speed
    if S == 0 or T == 0:
        out["stopped"] = True
        return out
    speed, eff, out["m_half"], out["m_jt"], _ = speed_step(n, S, T, s["speed"], s["eff"], p["jitter_tolerance"])
    # 7. move
    f = speed / (1.0 + np.sqrt(speed * swing))
    out.update(x=x + d[:, 0] * f, y=y + d[:, 1] * f, speed=float(speed), eff=float(eff), move=np.abs(d) * f[:, None])
    return out


def state_of(o):
    return {k: o[k] for k in ("x", "y", "dx", "dy", "speed", "eff")}


def run(g, pos0, niter, **params):
    """(final state, per-iteration outputs) of niter free-running iterations"""
    s, outs = start_state(pos0), []
    for _ in range(niter):
        o = step(g, s, **params)
        outs.append(o)
        s = state_of(o)
        if o["stopped"]:
            break
    return s, outs


# ---- the graphs ---------------------------------------------------------------------------------------------------
def planted(n, seed, groups=4, k=5):
    """(ptr, nbr, w, group): node i in group i mod `groups` lists k random nodes of its group (fewer when the group is
    small; never itself), weights round(U(0.05, 1), 2)"""
    rng = np.random.default_rng(seed)
    group = np.arange(n) % groups
    ptr, nbr, w = [0], [], []
    for i in range(n):
        own = np.nonzero((group == group[i]) & (np.arange(n) != i))[0]
        pick = rng.choice(own, size=min(k, len(own)), replace=False) if len(own) else own
        nbr += pick.tolist()
        w += np.round(rng.uniform(0.05, 1.0, len(pick)), 2).tolist()
        ptr.append(len(nbr))
    return np.array(ptr, dtype=np.int64), np.array(nbr, dtype=np.int64), np.array(w, dtype=np.float64), group


def _edit(n, seed, what):
    ptr, nbr, w, _ = planted(n, seed)
    rows = [(nbr[ptr[i]:ptr[i + 1]].tolist(), w[ptr[i]:ptr[i + 1]].tolist()) for i in range(n)]
    if what == "isolated":                  # node 3 has no edges: mass 1, repulsion and gravity only
        rows[3] = ([], [])
        for i, (a, b) in enumerate(rows):
            keep = [t for t, j in enumerate(a) if j != 3]
            rows[i] = ([a[t] for t in keep], [b[t] for t in keep])
    elif what == "selfloop":                # node 5 lists itself: one more in its degree, no force
        rows[5] = (rows[5][0] + [5], rows[5][1] + [0.77])
    elif what == "twice":                   # the pair (2, 6) three times, from both ends: the last weight holds
        rows[2] = (rows[2][0] + [6], rows[2][1] + [0.11])
        rows[6] = (rows[6][0] + [2, 2], rows[6][1] + [0.93, 0.42])
    ptr = np.concatenate([[0], np.cumsum([len(a) for a, _ in rows])]).astype(np.int64)
    return ptr, np.array(sum((a for a, _ in rows), []), dtype=np.int64), np.array(sum((b for _, b in rows), []), dtype=np.float64)


def cases(i_block, j_tile):
    """{name: dict(ptr, nbr, w, pos0, params)}: the planted graph at n = 2, 65, 257, 700 and one below, at and one above
    the kernel's j tile and i block; then a node without edges, two coincident nodes, a self-loop, a pair listed several
    times, and every parameter that takes another branch.  Start positions default_rng(100 + seed).random((n, 2)).  A case
    whose margins come closer than MARGIN gets another seed here, never a skipped step."""
    out = {}
    sizes = [2, 65, 257, 700] + [j_tile - 1, j_tile, j_tile + 1, i_block - 1, i_block, i_block + 1]
    for k, n in enumerate(dict.fromkeys(sizes)):
        seed = 1 + k % 4
        ptr, nbr, w, _ = planted(n, seed)
        out["planted_%d" % n] = dict(ptr=ptr, nbr=nbr, w=w, seed=seed, params={})
    n = j_tile + 44        # more than one tile, a ragged last one
    for k, (name, what, params) in enumerate([
            ("isolated", "isolated", {}), ("coincident", None, {}), ("selfloop", "selfloop", {}), ("twice", "twice", {}),
            ("no_oad", None, {"outbound_attraction_distribution": False}), ("ewi_0", None, {"edge_weight_influence": 0.0}),
            ("ewi_half", None, {"edge_weight_influence": 0.5}), ("strong_gravity", None, {"strong_gravity_mode": True}),
            ("scaled", None, {"scaling_ratio": 2.5, "gravity": 0.3, "jitter_tolerance": 0.8})]):
        seed = 15 if name == "ewi_0" else 5 + k        # (seed 10 brings ewi_0 within 1.4e-4 of S/T = 2 at one step)
        ptr, nbr, w = _edit(n, seed, what)
        out[name] = dict(ptr=ptr, nbr=nbr, w=w, seed=seed, params=params)
    for name, c in out.items():
        n = len(c["ptr"]) - 1
        c["pos0"] = np.random.default_rng(100 + c["seed"]).random((n, 2))
        if name == "coincident":
            c["pos0"][9] = c["pos0"][4]        # nodes 4 and 9 start at the same point: the pair contributes exactly 0
    return out


# ---- the large graphs: the paths only more than 64 tiles, or more than 256 node blocks, take ---------------------------
LARGE_STEPS = 2        # iterations a large case is stepped through
START_SPACING = 8.0    # mean distance between neighbouring nodes of a large case's start
NODE_BLOCK = 256       # nodes per workgroup of the node kernel, and partial sums the speed kernel takes per pass


def ring_chords(n, seed, chords=3):
    """(ptr, nbr, w, Graph) with numpy alone: the ring i -- i + 1 plus `chords` seeded random partners per node, each
    distinct pair once, listed from its lower end; weights round(U(0.05, 1), 2).  The graph is not the subject: it
    gives every node a mass of its own and an attraction"""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    a = np.concatenate([i, np.repeat(i, chords)])
    b = np.concatenate([(i + 1) % n, rng.integers(0, n, size=n * chords)])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = np.unique((lo * n + hi)[lo != hi])
    lo, hi = key // n, key % n
    w = np.round(rng.uniform(0.05, 1.0, len(key)), 2)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(lo, minlength=n), out=ptr[1:])
    return ptr, hi, w, simple_graph(n, lo, hi, w)


def split_geometry(n, j_tile, n_splits):
    """(tiles, tiles per split, tiles of the last split) of the repulsion of n nodes in n_splits splits"""
    ntiles = -(-n // j_tile)
    per = -(-ntiles // n_splits)
    return ntiles, per, ntiles - per * (n_splits - 1)


def large_cases(j_tile):
    """{name: dict(ptr, nbr, w, graph, pos0, seed, params)}: one node more than 64 tiles -- the first n whose splits
    hold two tiles, the last split one tile of one node -- and one node more than NODE_BLOCK blocks of NODE_BLOCK nodes,
    where the speed kernel's loop over the block sums comes round a second time.  Kept apart from cases(), whose names
    tests/golden/layout.npz pins.  Start positions START_SPACING sqrt(n) default_rng(100 + seed).random((n, 2)): on the
    unit square so many nodes start so close that their first move throws them far apart, the second iteration's forces
    have nothing to do with the first's and S / T comes out as 2 (1 + 5e-4) at n = 65537 whatever the seed, inside MARGIN
    of step 6's threshold.  With a mean spacing of 8 the repulsion and the attraction are of one size, the second
    iteration has S / T near 0.1 and S / (jt T) stays 0.2 and more from 1 (measured with the float64 restatement of
    every pair; the GPU test asserts the margins from the device's S and T)."""
    out = {}
    for n, seed in ((64 * j_tile + 1, 21), (NODE_BLOCK * NODE_BLOCK + 1, 22)):
        ptr, nbr, w, g = ring_chords(n, seed)
        out["ring_%d" % n] = dict(ptr=ptr, nbr=nbr, w=w, graph=g, seed=seed, params={},
                                  pos0=START_SPACING * np.sqrt(float(n)) * np.random.default_rng(100 + seed).random((n, 2)))
    return out


def sample_rows(n, i_block, j_tile, seed, n_random=256):
    """the rows whose repulsion the large cases check: node 0, node n - 1, the first and last node of every i block and of
    every tile (a lane's four nodes lie a tile apart), every node of the last tile, and n_random seeded random ones;
    ascending"""
    rows = {0, n - 1}
    for width in (i_block, j_tile):
        for b in range(0, n, width):
            rows |= {b, min(b + width, n) - 1}
    rows |= set(range((n - 1) // j_tile * j_tile, n))
    rows |= set(np.random.default_rng(seed).choice(n, size=min(n_random, n), replace=False).tolist())
    return np.array(sorted(rows), dtype=np.int64)

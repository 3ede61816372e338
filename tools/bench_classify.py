"""Times the classification kernel and one 64-set nabo_refgraph_set_levels call on the GPU (reported, not gated).

    python tools/bench_classify.py [--n 1000000] [--edges 15] [--clusters 32] [--repeats 7] [--snn-n 1000000]

Device time comes from HIP events inside the library (nabo_cluster_last_device_ms: uploads and downloads left out),
after a warm-up call, as the median of the repeats.  Bytes are the algorithm's: per edge 8 B neighbour + 8 B weight +
4 B cluster gather, per row 8 B of ptr + 4 B label + 16 B best / total.  The plain restatement (tests/_classify_ref.py)
is timed on a sub-sample of the rows and extrapolated.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import nabo_amd  # noqa: E402
from nabo_amd import _lib  # noqa: E402


def device_ms():
    ms = (C.c_double * 2)()
    _lib.check(_lib.lib().nabo_cluster_last_device_ms(ms))
    return ms[0], ms[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--edges", type=int, default=15)
    ap.add_argument("--clusters", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--snn-n", type=int, default=1000000)
    ap.add_argument("--sample", type=int, default=20000)
    a = ap.parse_args()
    if nabo_amd.device_count() < 1:
        raise SystemExit("no HIP device: this benchmark has no CPU fallback")
    rng = np.random.default_rng(1)
    n, k = a.n, a.edges
    rc = rng.integers(0, a.clusters, n).astype(np.int32)
    ptr = np.arange(0, n * k + 1, k, dtype=np.int64)
    # neighbours near the row's own index, as an SNN mapping gives: a target's reference cells are close to each other
    nbr = (np.repeat(rng.integers(0, n, n), k) + rng.integers(-2000, 2000, n * k)) % n
    w = rng.choice([0.05, 0.11, 0.18, 0.25, 0.33, 0.43, 0.54, 0.67, 0.82, 1.0], n * k)
    times = []
    for i in range(a.repeats + 1):
        got = nabo_amd.classify_from_edges(rc, ptr, nbr, w, 0.5, 2, 0.1, n_clusters=a.clusters)
        if i:
            times.append(device_ms()[0])
    ms = float(np.median(times))
    nbytes = n * k * 20 + n * (8 + 4 + 16)
    import _classify_ref as cref
    m = min(a.sample, n)
    t0 = time.perf_counter()
    lab, best, tot, _, _ = cref.classify(rc, a.clusters, ptr[:m + 1], nbr[:m * k], w[:m * k], 0.5, 2, 0.1, details=True)
    host_s = time.perf_counter() - t0
    same = bool(np.array_equal(lab, got["label"][:m]) and np.array_equal(best, got["best"][:m]) and np.array_equal(tot, got["total"][:m]))
    out = {"classify": {"n_ref": n, "n_targets": n, "edges_per_row": k, "clusters": a.clusters, "device_ms_median": ms,
                        "device_ms_all": times, "bytes": nbytes, "GBps": nbytes / ms / 1e6,
                        "restatement_rows": m, "restatement_s": host_s, "restatement_s_extrapolated_to_n": host_s * n / m,
                        "sample_equal": same}}
    # one 64-set levels call on an SNN graph built by the product
    if a.snn_n > 0:
        from nabo_amd._mapping import snn_edges
        from nabo_amd._paths import _DeviceGraph
        from nabo_amd._synth import pca_like
        ns, kk = a.snn_n, 11
        ref = pca_like(ns, 30, seed=41)
        r_idx, _ = nabo_amd.knn(ref, ref, kk, metric=nabo_amd.EUCLIDEAN, drop_first=True)
        et, ej, _ = snn_edges(r_idx, r_idx, kk)
        gptr = np.zeros(ns + 1, dtype=np.int64)
        np.cumsum(np.bincount(et, minlength=ns), out=gptr[1:])
        gnbr = ej[np.argsort(et, kind="stable")]
        g = _DeviceGraph(gptr, gnbr, 0)
        try:
            sets = [rng.integers(0, ns, 100) for _ in range(64)]
            sp = np.arange(0, 6401, 100, dtype=np.int64)
            mem = np.concatenate(sets).astype(np.int64)
            times, levels = [], None
            for i in range(a.repeats + 1):
                levels = g.set_levels(sp, mem, -1)
                if i:
                    times.append(device_ms()[1])
        finally:
            g.close()
        ms2 = float(np.median(times))
        arcs = int(len(gnbr)) * 2
        depth = int(levels.max())
        # per sweep: every arc's column read once per level it is expanded at (>= once), 24 B of masks per node, and
        # the 64 x n level matrix written once
        lb = arcs * 4 + ns * 24 + 64 * ns * 4
        out["set_levels"] = {"n_nodes": ns, "arcs_both_directions_upper": arcs, "sets": 64, "members_per_set": 100,
                             "device_ms_median": ms2, "device_ms_all": times, "deepest_level": depth,
                             "reached_fraction": float((levels >= 0).mean()), "bytes_lower_bound": lb, "GBps_lower_bound": lb / ms2 / 1e6}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

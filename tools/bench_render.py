#!/usr/bin/env python3
"""Times the rasteriser (nabo_render_*: include/nabo_render.h) on the GPU.  No pass / fail threshold: the step has no earlier
version in this project.  The one kernel of this kind the project had before, bundle_density_kernel (one integer atomic
per sample point of the bundled edges), is timed on the same graph as a yardstick, not a target.

    python tools/bench_render.py [--quick] [--nodes 100000 [1000000 ...]] [--k 15] [--size 2048] [--append] [--out FILE]
    python tools/bench_render.py --matplotlib 100000 [--append]      # the reference figure: matplotlib on this host's CPU

The graph is tools/bench_bundle.py's: an SNN graph on a layout of 40 Gaussian blobs.  Default sizes: 100 000 and 1 000 000
nodes; --quick: 20 000.  Per size two JSON lines, one with the straight edges (add_edges) and one with the bundled edges
drawn from the resident bundle (add_bundle), each on a --size x --size canvas with node radii of 1 - 3 pixels: device ms
per phase of the second of two identical renderings (HIP events around the kernels, nabo_render_last_ms), pixel updates
(the sums of the count images) per second of the edge and of the node phase, and the wall time of that rendering from clear
to the picture on the host, uploads and download included.  The bundled line adds the bundling run's device ms and its
density phase's point rate (the points the run ends with, once per round, over the phase's ms).  --append adds the lines to
--out (default profiles/render_bench.jsonl).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.bench_bundle import blob_graph  # noqa: E402


def render(cv, pos, radius, rgb, edges):
    t0 = time.perf_counter()
    cv.clear()
    edges(cv)
    cv.add_nodes(pos, radius, rgb)
    img = cv.compose("k", 0.1, 0.6)
    return img, time.perf_counter() - t0


def line(kind, n, k, size, n_edges, cv, img, wall, extra):
    ms = cv.last_ms()
    e_upd, n_upd = int(cv.edge_counts().sum(dtype=np.int64)), int(cv.node_counts().sum(dtype=np.int64))
    from nabo_amd import _lib, _render
    out = {"bench": "render", "edges_drawn": kind, "nodes": n, "k": k, "edges": n_edges, "canvas": [size, size],
           "geometry": _render.geometry(), "device_ms": ms, "wall_seconds": wall,
           "edge_pixel_updates": e_upd, "node_pixel_updates": n_upd,
           "edge_pixel_updates_per_second": e_upd / (ms["edges"] * 1e-3) if ms["edges"] > 0 else None,
           "node_pixel_updates_per_second": n_upd / (ms["nodes"] * 1e-3) if ms["nodes"] > 0 else None,
           "pixels_not_transparent": int((img[..., 3] > 0).sum()), "so": _lib.so_digest()}
    out.update(extra)
    return out


def bench(n, k, size):
    from nabo_amd import _bundle, _render
    pos, src, dst = blob_graph(n, k)
    rng = np.random.default_rng(5)
    radius, rgb = rng.uniform(1.0, 3.0, size=n), rng.integers(0, 256, size=(n, 3)).astype(np.uint8)
    out = []
    with _render.Canvas(size, size, _render.default_viewport(pos)) as cv:
        straight = lambda c: c.add_edges(pos, src, dst)
        render(cv, pos, radius, rgb, straight)          # warm-up: first launches, the buffers' first allocation
        img, wall = render(cv, pos, radius, rgb, straight)
        out.append(line("straight", n, k, size, int(len(src)), cv, img, wall, {"points": 2 * int(len(src))}))
        with _bundle.Bundle(pos, src, dst) as B:
            B.resample()
            t0 = time.perf_counter()
            B.run()
            b_wall = time.perf_counter() - t0
            b_ms = B.last_ms()
            off, _ = B.get_points()
            p = B.params
            rounds, d = 0, p["decay"]
            for _ in range(p["iterations"]):
                if (p["initial_bandwidth"] * d) * p["accuracy"] < 2:
                    break
                rounds, d = rounds + 1, d * p["decay"]
            bundled = lambda c: c.add_bundle(B)
            render(cv, pos, radius, rgb, bundled)
            img, wall = render(cv, pos, radius, rgb, bundled)
            dens = float(off[-1]) * rounds
            out.append(line("bundled", n, k, size, int(len(src)), cv, img, wall,
                            {"points": int(off[-1]), "bundle_device_ms": b_ms, "bundle_wall_seconds": b_wall, "bundle_rounds": rounds,
                             "bundle_density_points": dens,
                             "bundle_density_points_per_second": dens / (b_ms["density"] * 1e-3) if b_ms["density"] > 0 else None}))
    return out


def matplotlib_seconds(n, k, size):
    """a reference figure: matplotlib (Agg, one CPU core of this host) drawing the straight edges and the nodes of the same
    graph into size x size pixels -- a LineCollection and a scatter, as GraphPlot does"""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from matplotlib.collections import LineCollection
    pos, src, dst = blob_graph(n, k)
    rng = np.random.default_rng(5)
    radius, rgb = rng.uniform(1.0, 3.0, size=n), rng.integers(0, 256, size=(n, 3)) / 255.0
    t0 = time.perf_counter()
    fig = plt.figure(figsize=(size / 100.0, size / 100.0), dpi=100)
    ax = fig.add_axes([0, 0, 1, 1])
    ax.add_collection(LineCollection(np.stack([pos[src], pos[dst]], axis=1), colors="k", linewidths=0.72, alpha=0.1, zorder=1))
    ax.scatter(pos[:, 0], pos[:, 1], s=np.pi * (radius * 0.72) ** 2, c=rgb, lw=0, alpha=0.6, zorder=2)   # 0.72 points per pixel
    ax.autoscale_view()
    fig.canvas.draw()
    img = np.asarray(fig.canvas.buffer_rgba())
    wall = time.perf_counter() - t0
    plt.close(fig)
    return {"bench": "render_matplotlib_reference", "nodes": n, "k": k, "edges": int(len(src)), "canvas": [int(img.shape[1]), int(img.shape[0])],
            "wall_seconds": wall, "matplotlib": matplotlib.__version__}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--nodes", type=int, nargs="*", default=None)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_bench.jsonl"))
    ap.add_argument("--matplotlib", type=int, default=0, metavar="NODES",
                    help="instead: time matplotlib on this host's CPU for the straight-edge picture of a graph of NODES nodes")
    a = ap.parse_args()
    sizes = a.nodes or ([20000] if a.quick else [100000, 1000000])
    for n in ([a.matplotlib] if a.matplotlib else sizes):
        for rec in ([matplotlib_seconds(n, a.k, a.size)] if a.matplotlib else bench(n, a.k, a.size)):
            text = json.dumps(rec)
            print(text, flush=True)
            if a.append:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(text + "\n")


if __name__ == "__main__":
    sys.exit(main())

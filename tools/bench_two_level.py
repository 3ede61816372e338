"""The headline step (set_ref + query on resident device arrays, as bench.py times it) under the two-level stream's options, all
in one process on one GPU -- on bench.py's clustered data or on ONE broad Gaussian cloud, which bench.py cannot generate and
where the stream gains nothing: the mode control has to keep its cost to the probes.
    python tools/bench_two_level.py [steps] [m n g k] [--cloud] [name=value,...;name=value,...;...]
Configurations are separated by ';' and run in the order given, the first one again at the end (the spread).  The mode
control's knobs are index options like any other: "two_level_burst=3,two_level_share=25" is the per-bucket control with that
account, "two_level_stretch=64" the control before it, "bucket_skip=1" the stream without the skip of unreachable sub-buckets
(DESIGN.md 4.1f).  Tile counters: one-step, refetched, two-step, skipped; ms_pack holds the reference-side build."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nabo_amd import _knn, _lib  # noqa: E402
from nabo_amd._synth import pca_like  # noqa: E402

TILE_KEYS = ("two_level_one_step_tiles", "two_level_refetched_tiles", "two_level_two_step_tiles", "two_level_skipped_tiles")
cloud = "--cloud" in sys.argv
if cloud:
    sys.argv.remove("--cloud")
cfgs = None
for a in [a for a in sys.argv[1:] if "=" in a]:
    sys.argv.remove(a)
    cfgs = [{kv.split("=")[0]: int(kv.split("=")[1]) for kv in c.split(",") if kv} for c in a.split(";")]
if cfgs is None:
    cfgs = [{"two_level": 0}, {"two_level": 1}]
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
m, n, g, k = (int(a) for a in (sys.argv[2:6] if len(sys.argv) > 5 else (1000000, 1000000, 50, 15)))
if cloud:
    lam = np.sqrt(30.0 - 29.0 * np.arange(g) / max(g - 1, 1))          # pca_like's component scales, no clusters
    Y = np.random.default_rng(1003).standard_normal((n, g)) * lam
    X = np.random.default_rng(2003).standard_normal((m, g)) * lam
else:
    Y, X = pca_like(n, g, seed=1003), pca_like(m, g, seed=2003)
dx, dy = _knn.DeviceBuffer(X.nbytes).upload(X), _knn.DeviceBuffer(Y.nbytes).upload(Y)
di, dd = _knn.DeviceBuffer(m * k * 8), _knn.DeviceBuffer(m * k * 8)
for opts in cfgs + cfgs[:1]:
    ix = _knn.KnnIndex(n, g, metric=0, options=opts)
    st = []
    for it in range(steps + 1):
        if it == 1:
            _lib.check(_lib.lib().nabo_dev_synchronize(0))
            t0 = time.perf_counter()
        ix.set_ref(y_device_ptr=dy.ptr)
        ix.query_device(dx.ptr, m, k, False, di.ptr, dd.ptr)
        st.append(ix.last_stats())
    _lib.check(_lib.lib().nabo_dev_synchronize(0))
    ms = (time.perf_counter() - t0) * 1e3 / steps
    mean = lambda key: sum(s[key] for s in st[1:]) / len(st[1:])      # noqa: E731
    print(json.dumps({"data": "cloud" if cloud else "pca_like", "options": opts, "ms_per_step": round(ms, 3),
                      "ms_pack": round(mean("ms_pack"), 3), "ms_topk": round(mean("ms_topk"), 3), "ms_refine": round(mean("ms_refine"), 3),
                      "seeded_pass_rows": st[-1]["seeded_pass_rows"],
                      "tiles_first_step": [st[0][a] for a in TILE_KEYS],
                      "tiles_last_step": [st[-1][a] for a in TILE_KEYS]}),
          flush=True)
    ix.close()

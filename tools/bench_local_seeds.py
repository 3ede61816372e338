"""The headline step (set_ref + query on resident device arrays, as bench.py times it) under index options, all in one
process on one GPU: local tournament seeds off / on, anchors and cap swept.
    python tools/bench_local_seeds.py [steps] [m n g k] [name=value,...;name=value,...;...]
Configurations are separated by ';' and run in the order given, the first one again at the end (the spread)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nabo_amd import _knn, _lib  # noqa: E402
from nabo_amd._synth import pca_like  # noqa: E402

cfgs = None
for a in [a for a in sys.argv[1:] if "=" in a or a == "-"]:
    sys.argv.remove(a)
    cfgs = [{kv.split("=")[0]: int(kv.split("=")[1]) for kv in c.split(",") if kv} for c in a.split(";")]
if cfgs is None:
    cfgs = [{"local_seeds": 0}] + [{"local_anchors": c, "local_cap": cap} for c in (64, 256) for cap in (8192, 16384, 32768)]
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
m, n, g, k = (int(a) for a in (sys.argv[2:6] if len(sys.argv) > 5 else (1000000, 1000000, 50, 15)))
Y = pca_like(n, g, seed=1003)
X = pca_like(m, g, seed=2003)
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
        if it:
            st.append(ix.last_stats())
    _lib.check(_lib.lib().nabo_dev_synchronize(0))
    ms = (time.perf_counter() - t0) * 1e3 / steps
    mean = lambda key: sum(s[key] for s in st) / len(st)      # noqa: E731
    print(json.dumps({"options": opts, "ms_per_step": round(ms, 3), "ms_pack": round(mean("ms_pack"), 3), "ms_topk": round(mean("ms_topk"), 3),
                      "ms_refine": round(mean("ms_refine"), 3), "seeded_pass_rows": st[-1]["seeded_pass_rows"],
                      "plan_buckets": _knn.query_plan(n, g, m, k, options=opts)["local_seed_buckets"]}), flush=True)
    ix.close()

"""File-level hop-distance functions (nabo_amd.get_mapping_specificity / get_ref_specificity / calc_contiguous_spl /
RefGraph) on the `mapping_small` mapping file in both graph layouts, against what the reference's Graph returned
(tests/golden/paths.npz).  Needs h5py and a GPU: run by test_paths_gpu.py under an interpreter with h5py."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _graph_case import GOLD, build_file  # noqa: E402

import nabo_amd  # noqa: E402


def same(a, b):
    return list(a) == list(b) and np.array_equal(np.array(list(a.values()), dtype=np.float64),
                                                 np.array(list(b.values()), dtype=np.float64), equal_nan=True)


def main():
    gold = np.load(os.path.join(GOLD, "mapping_small.npz"))
    d = np.load(os.path.join(GOLD, "paths.npz"))
    ref = [str(x) for x in d["small_ref_nodes"]]
    out = {"checked": 0, "differ": []}
    with tempfile.TemporaryDirectory() as td:
        for layout in ("per_node", "columnar"):
            fn, _, _ = build_file(td, gold, graph_layout=layout, tag=layout)
            for t in ("ME", "IG"):
                p = "small_" + t
                nodes = [str(x) for x in d[p + "_t_nodes"]]
                for fill, key in ((True, "_spec_fill"), (False, "_spec_nofill")):
                    got = nabo_amd.get_mapping_specificity(fn, "WT", t, fill_na=fill)
                    out["checked"] += 1
                    if not same(got, dict(zip(nodes, d[p + key].tolist()))):
                        out["differ"].append((layout, t, "spec", fill))
                vals = dict(zip(nodes, d[p + "_spec_fill"].tolist()))
                for incl, q in ((False, "_refspec"), (True, "_refspec_incl")):
                    got = nabo_amd.get_ref_specificity(fn, "WT", t, vals, incl_unmapped=incl)
                    out["checked"] += 1
                    if not same(got, dict(zip([str(x) for x in d[p + q + "_nodes"]], d[p + q + "_vals"].tolist()))):
                        out["differ"].append((layout, t, "refspec", incl))
                with nabo_amd.RefGraph(fn, "WT") as g:
                    for lst, v in zip(json.loads(str(d[p + "_cspl_lists"])), d[p + "_cspl_vals"].tolist()):
                        got = g.contiguous_spl([ref[i] for i in lst])
                        out["checked"] += 1
                        if not (got == v or (got != got and v != v)):
                            out["differ"].append((layout, t, "cspl", len(lst)))
                lst = json.loads(str(d[p + "_cspl_lists"]))[0]
                got = nabo_amd.calc_contiguous_spl(fn, "WT", [ref[i] for i in lst])
                out["checked"] += 1
                if got != float(d[p + "_cspl_vals"][0]):
                    out["differ"].append((layout, t, "calc_contiguous_spl"))
            try:
                nabo_amd.get_mapping_specificity(fn, "WT", "missing")
                out["differ"].append((layout, "unknown target accepted"))
            except KeyError:
                out["checked"] += 1
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()

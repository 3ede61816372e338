"""File-level classification / DE-group functions (nabo_amd.classify_target, get_k_path_neighbours, get_de_groups,
get_mapped_cells, RefGraph) on the `mapping_small` mapping file in both graph layouts, against what the reference's
Graph returned (tests/golden/classify.npz).  Needs h5py and a GPU: run by test_classify_gpu.py under an interpreter
with h5py."""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _graph_case import GOLD, build_file  # noqa: E402

import nabo_amd  # noqa: E402


def main():
    gold = np.load(os.path.join(GOLD, "mapping_small.npz"))
    d = np.load(os.path.join(GOLD, "classify.npz"))
    ref = [str(x) for x in np.load(os.path.join(GOLD, "paths.npz"))["small_ref_nodes"]]
    lab, unnamed = d["small_clusters"], d["small_unnamed"]
    variants = {"full": {n: int(lab[i]) for i, n in enumerate(ref)},
                "partial": {n: int(lab[i]) for i, n in enumerate(ref) if not unnamed[i]}}
    out = {"checked": 0, "differ": []}
    answers = {}

    def note(key, ok, got):
        out["checked"] += 1
        if not ok:
            out["differ"].append(key)
        answers.setdefault(key[1:], {}).setdefault(key[0], []).append(repr(got))

    with tempfile.TemporaryDirectory() as td:
        for layout in ("per_node", "columnar"):
            fn, _, _ = build_file(td, gold, graph_layout=layout, tag=layout)
            for c in json.loads(str(d["cases"])):
                if c["tag"] != "small" or d[c["key"] + "_tied"].size:
                    continue                                    # deciding ties: checked at array level
                kw = dict(weight_frac=c["weight_frac"], min_degree=c["min_degree"], min_weight=c["min_weight"])
                if c["form"] == "clusters":
                    kw["clusters"] = variants[c["variant"]]
                else:
                    kw.update(cluster_dict=variants[c["variant"]], na_label="unk")
                got = nabo_amd.classify_target(fn, "WT", c["target"], **kw)
                note((layout, c["key"]), [str(v) for v in got.values()] == [str(x) for x in d[c["key"] + "_labels"]], got)
                cnt = nabo_amd.classify_target(fn, "WT", c["target"], ret_counts=True, **kw)
                note((layout, c["key"], "counts"), {str(k): int(v) for k, v in cnt.items()} == c["counts"], dict(cnt))
            with nabo_amd.RefGraph(fn, "WT") as g:
                pos = {n: i for i, n in enumerate(ref)}
                for c in json.loads(str(d["rings"])):
                    if c["tag"] != "small":
                        continue
                    got = g.k_path_neighbours([ref[i] for i in c["nodes"]], c["k_dist"], c["full_trail"], c["trail_start"])
                    got = [pos[x] for x in got]
                    note((layout, "ring", c["target"], c["k_dist"], c["full_trail"], c["trail_start"]),
                         (got if c["as_given"] else sorted(got)) == c["result"], got)
                for i, c in enumerate(json.loads(str(d["de_groups"]))):
                    if c["tag"] != "small":
                        continue
                    with contextlib.redirect_stdout(io.StringIO()):
                        got = g.set_de_groups(c["target"], clusters=variants["full"], **c["kwargs"])
                    want = c["result"]
                    if want is None:
                        ok = got is None
                    else:
                        code = {"Other": 0, "Test": 1, "Control": 2}
                        ok = (list(got["de_group"]) == ref and [code[v] for v in got["de_group"].values()] == want["de_group"]
                              and got["deTestCells"] == want["deTestCells"] and sorted(got["deCtrlCells"]) == want["deCtrlCells"]
                              and g.deTestCells == got["deTestCells"])
                    note((layout, "de", i), ok, got)
            c = [x for x in json.loads(str(d["rings"]))
                 if x["tag"] == "small" and x["k_dist"] == 2 and x["full_trail"] and x["trail_start"] == 0][0]
            got = nabo_amd.get_k_path_neighbours(fn, "WT", [ref[i] for i in c["nodes"]], c["k_dist"], c["full_trail"], c["trail_start"])
            note((layout, "get_k_path_neighbours"), sorted(pos[x] for x in got) == sorted(c["result"]), got)
            c = [x for x in json.loads(str(d["de_groups"])) if x["tag"] == "small" and x["result"] is not None][0]
            with contextlib.redirect_stdout(io.StringIO()):
                got = nabo_amd.get_de_groups(fn, "WT", c["target"], clusters=variants["full"], **c["kwargs"])
            note((layout, "get_de_groups"), got["deTestCells"] == c["result"]["deTestCells"], got)
            for i, c in enumerate(json.loads(str(d["mapped_cells"]))):
                if c["tag"] == "small":
                    got = nabo_amd.get_mapped_cells(fn, "WT", c["target"], c["ref_cells"], c["remove_suffix"])
                    note((layout, "mapped", i), got == c["result"], got)
            for fn_, exc, args in ((nabo_amd.classify_target, KeyError, (fn, "WT", "missing")),
                                   (nabo_amd.get_mapped_cells, ValueError, (fn, "WT", "missing", ["R0"]))):
                try:
                    fn_(*args, **({"clusters": variants["full"]} if exc is KeyError else {}))
                    out["differ"].append((layout, "unknown target accepted"))
                except exc:
                    out["checked"] += 1
            for kw, exc in (({}, ValueError), ({"clusters": {n: 1 for n in ref}}, ValueError)):
                try:
                    nabo_amd.classify_target(fn, "WT", "ME", **kw)
                    out["differ"].append((layout, "bad clusters accepted"))
                except exc:
                    out["checked"] += 1
            try:
                with nabo_amd.RefGraph(fn, "WT") as g:
                    g.set_de_groups("ME", 0, 1, from_clusters="1", clusters=variants["full"])
                out["differ"].append((layout, "from_clusters str accepted"))
            except TypeError:
                out["checked"] += 1
    # both layouts gave the same answers
    for key, vals in answers.items():
        if len(vals) != 2 or vals["per_node"] != vals["columnar"]:
            out["differ"].append(("layouts differ",) + tuple(key))
    print("RESULT " + json.dumps(out, default=str))


if __name__ == "__main__":
    main()

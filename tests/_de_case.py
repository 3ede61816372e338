"""File-level DE functions (nabo_amd.run_de_test, find_cluster_markers) on Nabo-format dataset files written from
tests/golden/de.npz, against the reference's tables stored there.  Needs h5py and a GPU: run by test_de_gpu.py under an
interpreter with h5py."""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _de_ref as dref  # noqa: E402

import nabo_amd  # noqa: E402


def write_dataset(fn, d, prefix, with_processed, shuffle_columns=False):
    """names/{cells,genes}, gene_data/<GENE> as (idx, val) records, processed_data/{sf,keep_genes_idx}"""
    import h5py
    ptr, cell, val = d[prefix + "_gene_ptr"], d[prefix + "_cell"], d[prefix + "_val"]
    with h5py.File(fn, "w") as h5:
        g = h5.create_group("names")
        g.create_dataset("cells", data=np.array([str(x).encode() for x in d[prefix + "_cells"]]))
        g.create_dataset("genes", data=np.array([str(x).encode() for x in d[prefix + "_genes"]]))
        gd = h5.create_group("gene_data")
        for j, name in enumerate(d[prefix + "_genes"]):
            rec = np.zeros(int(ptr[j + 1] - ptr[j]), dtype=[("idx", np.uint32), ("val", np.float32)])
            rec["idx"], rec["val"] = cell[ptr[j]:ptr[j + 1]], val[ptr[j]:ptr[j + 1]]
            if shuffle_columns:                                  # the file may list a column's cells in any order
                rec = rec[np.random.default_rng(j).permutation(rec.shape[0])]
            gd.create_dataset(str(name), data=rec)
        if with_processed:
            p = h5.create_group("processed_data")
            p.create_dataset("sf", data=d[prefix + "_sf"])
            p.create_dataset("keep_genes_idx", data=d[prefix + "_keep"])


def main():
    d = np.load(os.path.join(HERE, "golden", "de.npz"))
    tol, p_rel = 4 * float(d["log2fc_dev"]), float(d["p_dev"]) + 2 * 2.0 ** -52
    out = {"checked": 0, "rows": 0, "differ": []}
    with tempfile.TemporaryDirectory() as td:
        fns = {"d1": os.path.join(td, "d1.h5"), "d2": os.path.join(td, "d2.h5"), "q": os.path.join(td, "q.h5")}
        write_dataset(fns["d1"], d, "d1", True, shuffle_columns=True)
        write_dataset(fns["d2"], d, "d2", True)
        write_dataset(fns["q"], d, "q", False)                   # no processed_data: every gene kept, size factors 1
        for case in dref.golden_cases(d):
            try:
                got = nabo_amd.run_de_test(fns[case["d1"]], None if case["d2"] is None else fns[case["d2"]], case["test_cells"],
                                           case["control_cells"], case["test_label"], case["labels"], case["exp_frac_thresh"],
                                           case["log2_fc_thresh"], qval_thresh=2)
                res = "ok"
            except (ZeroDivisionError, KeyError) as e:
                res = type(e).__name__
            out["checked"] += 1
            if res != case["result"]:
                out["differ"].append((case["name"], res, case["result"]))
            elif res == "ok":
                bad = dref.compare_tables(got, case["table"], tol, p_rel)
                if bad or list(got.keys() if isinstance(got, dict) else got.columns) != nabo_amd._de.COLUMNS:
                    out["differ"].append((case["name"], bad[:3]))
                out["rows"] += len(case["table"]["gene"])
        for key in ("markers", "markers_clamped"):
            c = json.loads(str(d[key]))
            with contextlib.redirect_stdout(io.StringIO()) as msg:
                table, de_genes = nabo_amd.find_cluster_markers(c["clusters"], fns["d1"], c["de_frequency"], c["exp_frac_thresh"],
                                                                c["log2_fc_thresh"], c["qval_thresh"])
            out["checked"] += 1
            bad = dref.compare_tables(table, c["table"], tol, p_rel)
            if bad or {str(k): sorted(v) for k, v in de_genes.items()} != {k: sorted(v) for k, v in c["de_genes"].items()}:
                out["differ"].append((key, bad[:3]))
            if (c["de_frequency"] >= 4) != ("WARNING" in msg.getvalue()):
                out["differ"].append((key, "de_frequency warning"))
            out["rows"] += len(c["table"]["gene"])
        # the defaults filter at qval < 0.05: a subset of the unfiltered golden rows, every one below the threshold
        case = dref.golden_cases(d)[0]
        got = nabo_amd.run_de_test(fns["d1"], None, case["test_cells"], case["control_cells"], exp_frac_thresh=case["exp_frac_thresh"],
                                   log2_fc_thresh=case["log2_fc_thresh"])
        want = [q for q in case["table"]["qval"] if q < 0.05]
        out["checked"] += 1
        if len(got["qval"]) != len(want) or not all(float(q) < 0.05 for q in got["qval"]):
            out["differ"].append(("default qval filter", len(got["qval"]), len(want)))
    print("RESULT " + json.dumps(out, default=str))


if __name__ == "__main__":
    main()

"""What the C ABI answers to a malformed expression matrix, through ctypes: the return code and the exact message that
names the fault, found before any device is asked for (so never NABO_E_NODEVICE, with or without a GPU).  The texts are
the contract of nabo_cell_qc, nabo_pca_project, nabo_pca_cov, nabo_gene_stats and nabo_de_test (either matrix).

The good input is two lists over three indices.  For the row steps (QC, projection, fit) the lists are cells and the
indices genes; for the column steps (gene statistics, DE) the lists are genes and the indices cells.  One fault at a time.

The steps differ in one rule, the value check: QC has no size factors and checks the raw value, the projection, the fit
and the gene statistics check the raw value and its product with the cell's size factor, DE checks the product alone.
The one GPU test here pins that difference."""
import ctypes as C

import numpy as np
import pytest

from nabo_amd import _lib, _pca

INF = float("inf")
GOOD = dict(ptr=[0, 2, 3], idx=[0, 2, 1], val=[1, 2, 3], sf="unit", rows=None, budget=0)
ROW_STEPS, COLUMN_STEPS = ("qc", "project", "cov"), ("stats", "de1", "de2")
STEPS = ROW_STEPS + COLUMN_STEPS
RESIDENT, ROW_FIXED = _pca.cov_resident_bytes(3)      # of the fit: a row of e entries needs ROW_FIXED + 8 e beside RESIDENT

RAW = "entry 1 (cell 0, gene 2): value %s must be finite and >= 0"
BOTH = "entry 1 (%s): value %s, scaled value %s: both must be finite and >= 0"
SCALED = "matrix %d: the scaled value of entry 1 (gene 0, cell 2) is %s: values must be finite and >= 0"


def _by_form(rows_text, cols_text):
    """the message of the row steps, of the gene statistics, and of DE with its prefix"""
    out = {s: rows_text for s in ROW_STEPS}
    out.update(stats=cols_text, de1="matrix 1: " + cols_text, de2="matrix 2: " + cols_text)
    return out


def _value(v):
    return dict(qc=RAW % v, project=BOTH % ("cell 0, gene 2", v, v), cov=BOTH % ("cell 0, gene 2", v, v),
                stats=BOTH % ("gene 0, cell 2", v, v), de1=SCALED % (1, v), de2=SCALED % (2, v))


# the fault -> (what is changed, the code, the message by step; a step that is not named does not take the case)
FAULTS = {
    # (a NULL pointer array of matrix 2 is no fault: it says that there is one matrix)
    "null_ptr": (dict(ptr=None), _lib.E_INVALID,
                 {k: v for k, v in _by_form("cell_ptr is NULL", "gene_ptr is NULL").items() if k != "de2"}),
    "ptr0_is_1": (dict(ptr=[1, 2, 3]), _lib.E_INVALID, _by_form("cell_ptr[0] = 1, must be 0", "gene_ptr[0] = 1, must be 0")),
    "ptr_falls": (dict(ptr=[0, 3, 2]), _lib.E_INVALID, _by_form("cell_ptr is not monotone at cell 1", "gene_ptr is not monotone at gene 1")),
    "null_idx": (dict(idx=None), _lib.E_INVALID, _by_form("gene or val is NULL", "cell or val is NULL")),
    "null_sf": (dict(sf=None), _lib.E_INVALID, {k: v for k, v in _by_form("sf is NULL", "sf is NULL").items() if k != "qc"}),
    "idx_is_n": (dict(idx=[0, 3, 1]), _lib.E_INVALID, _by_form("gene[1] = 3 is not a gene in [0, 3)", "cell[1] = 3 is not a cell in [0, 3)")),
    "idx_is_minus_1": (dict(idx=[0, -1, 1]), _lib.E_INVALID,
                       _by_form("gene[1] = -1 is not a gene in [0, 3)", "cell[1] = -1 is not a cell in [0, 3)")),
    "idx_not_increasing": (dict(idx=[2, 0, 1]), _lib.E_INVALID,
                           _by_form("the genes of cell 0 are not strictly increasing at entry 1",
                                    "the cells of gene 0 are not strictly increasing at entry 1")),
    "negative_value": (dict(val=[1, -2, 3]), _lib.E_INVALID, _value("-2")),
    "infinite_value": (dict(val=[1, INF, 3]), _lib.E_INVALID, _value("inf")),
    "row_is_n": (dict(rows=[0, 2]), _lib.E_INVALID, {s: "rows[1] = 2 is not a cell in [0, 2)" for s in ROW_STEPS}),
    # (the fit counts its rows first: one row is no covariance)
    "row_is_minus_1": (dict(rows=[-1]), _lib.E_INVALID,
                       dict(qc="rows[0] = -1 is not a cell in [0, 2)", project="rows[0] = -1 is not a cell in [0, 2)",
                            cov="n_rows=1: a covariance needs at least 2 rows")),
    "row_is_minus_1_of_two": (dict(rows=[-1, 0]), _lib.E_INVALID, {s: "rows[0] = -1 is not a cell in [0, 2)" for s in ROW_STEPS}),
    # row 0 holds two entries: 24 + 16 bytes for QC without classes, 20 + 16 for one component, ROW_FIXED + 16 for the fit
    "budget_below_row_0": (dict(budget=dict(qc=39, project=35, cov=RESIDENT + ROW_FIXED + 15)), _lib.E_NOMEM,
                           dict(qc="row 0 alone needs 40 bytes of device buffers, the budget is 39",
                                project="row 0 alone needs 36 bytes of device buffers, the budget is 35",
                                cov="row 0 alone needs %d bytes of device buffers beside %d resident ones, the budget is %d"
                                    % (ROW_FIXED + 16, RESIDENT, RESIDENT + ROW_FIXED + 15))),
}


def _matrix(a):
    """the arrays of one matrix (kept alive by the caller) and their addresses; a["sf"]: "unit", None or a list"""
    n_minor = 2 if a["step"] in ROW_STEPS else 3
    sf = [1.0] * n_minor if a["sf"] == "unit" else a["sf"]
    keep = [None if a["ptr"] is None else np.array(a["ptr"], dtype=np.int64), None if a["idx"] is None else np.array(a["idx"], dtype=np.int32),
            np.array(a["val"], dtype=np.float32), None if sf is None else np.array(sf, dtype=np.float32)]
    return keep, [None if x is None else x.ctypes.data for x in keep]


def _call(step, change, de_out=None):
    """the step's entry point on GOOD with `change`; de_out: the ten output arrays of nabo_de_test, made here if None"""
    a = dict(GOOD, step=step, **change)
    keep, (ptr, idx, val, sf) = _matrix(a)
    rows = None if a["rows"] is None else np.array(a["rows"], dtype=np.int64)
    n_rows, p_rows = (2, None) if rows is None else (rows.shape[0], rows.ctypes.data)
    budget = a["budget"][step] if isinstance(a["budget"], dict) else a["budget"]
    L = _lib.lib()
    pos = np.arange(3, dtype=np.int32)
    zeros, ones, out = np.zeros(3), np.ones(3), np.zeros(64)
    o = out.ctypes.data
    if step == "qc":
        rc = L.nabo_cell_qc(0, 2, 3, ptr, idx, val, 0, None, n_rows, p_rows, budget, o, o)
    elif step == "project":
        rc = L.nabo_pca_project(0, 2, 3, ptr, idx, val, sf, pos.ctypes.data, 3, zeros.ctypes.data, ones.ctypes.data, zeros.ctypes.data, 1,
                                ones.ctypes.data, n_rows, p_rows, budget, o)
    elif step == "cov":
        rc = L.nabo_pca_cov(0, 2, 3, ptr, idx, val, sf, pos.ctypes.data, 3, zeros.ctypes.data, ones.ctypes.data, n_rows, p_rows, budget, o, o)
    elif step == "stats":
        rc = L.nabo_gene_stats(0, 2, 3, ptr, idx, val, sf, 0, None, None, o, o, o, o, o)
    else:
        # set 0 = cells 0, 1 (test, read from matrix 1), set 1 = cell 2 (control, read from matrix 2 when there is one)
        good_keep, good = _matrix(dict(GOOD, step=step))
        m1, m2 = ([ptr, idx, val, sf], [None] * 4) if step == "de1" else (good, [ptr, idx, val, sf])
        if step == "de1" and a.get("two"):
            m2 = good
        set_ptr, members = np.array([0, 2, 3], dtype=np.int64), np.array([0, 1, 2], dtype=np.int64)
        outs = de_out if de_out is not None else [np.zeros(2, dtype=np.int64) for _ in range(10)]
        rc = L.nabo_de_test(0, 2, 3, *m1, 3, *m2, 2, set_ptr.ctypes.data, members.ctypes.data, 1, None, None, 0.0, -100.0, budget,
                            *[x.ctypes.data for x in outs])
        del good_keep
    text = L.nabo_last_error().decode("utf-8")
    del keep
    return rc, text


def _cases():
    for fault, (_, code, texts) in sorted(FAULTS.items()):
        for step in STEPS:
            if step in texts:
                yield pytest.param(step, fault, code, texts[step], id="%s-%s" % (step, fault))


@pytest.mark.parametrize("step,fault,code,want", list(_cases()))
def test_entry_point_names_the_fault_before_it_asks_for_a_device(step, fault, code, want):
    assert _call(step, FAULTS[fault][0]) == (code, want)


def test_every_step_takes_every_case_that_applies_to_it():
    """the table above leaves a case out only where the step has no such argument"""
    for fault, (_, _, texts) in FAULTS.items():
        missing = set(STEPS) - set(texts)
        if fault.startswith("row_") or fault == "budget_below_row_0":
            assert missing == set(COLUMN_STEPS)
        else:
            assert missing == {"null_ptr": {"de2"}, "null_sf": {"qc"}}.get(fault, set())


@pytest.mark.gpu
def test_a_negative_value_under_a_negative_size_factor():
    """val[1] = -2 with the size factor -1 for its cell: the product is 2.  The projection and the gene statistics refuse
    the raw value; DE reads the product alone, accepts it and gives what val[1] = 2 with the size factor 1 gives."""
    rows_form = dict(val=[1, -2, 3], sf=[-1.0, 1.0])              # entry 1 lies in cell 0, and so does entry 0: the first to fail
    cols_form = dict(val=[1, -2, 3], sf=[1.0, 1.0, -1.0])         # entry 1 is (gene 0, cell 2)
    assert _call("project", rows_form) == (_lib.E_INVALID, "entry 0 (cell 0, gene 0): value 1, scaled value -1: both must be finite and >= 0")
    assert _call("stats", cols_form) == (_lib.E_INVALID, "entry 1 (gene 0, cell 2): value -2, scaled value 2: both must be finite and >= 0")
    dtypes = [np.int32] + [np.int64] * 5 + [np.float64] * 4
    for step, extra in (("de1", {}), ("de1", {"two": True}), ("de2", {})):
        got, want = ([np.full(2, 7, dtype=t) for t in dtypes] for _ in range(2))      # (gene, pair) results: 2 genes, 1 pair
        assert _call(step, dict(cols_form, **extra), got)[0] == 0
        assert _call(step, dict(val=[1, 2, 3], **extra), want)[0] == 0
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
        assert (got[0] != 7).all()                                # the step wrote its status

"""The quality-control step (include/nabo_qc.h, nabo_amd/_qc.py) without a GPU: the C header and its symbols, argument
checks, the no-device failure, and the host logic -- cells and genes to keep, size factors, the variance correction with
its LOWESS, HVGs and LVGs -- against what the reference computed (tests/golden/qc.npz, tools/gen_golden_qc.py), with the
device step replaced by the tests' plain restatement (tests/_qc_ref.py)."""
import contextlib
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _lib, _qc

import _qc_ref as qref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_qc_check(tmp_path):
    exe = os.path.join(str(tmp_path), "qc_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "abi_c", "qc_check.c"), "-L" + os.path.join(REPO, "nabo_amd"), "-lnabo_knn",
           "-Wl,-rpath," + os.path.join(REPO, "nabo_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    return exe


def said(fn, *a, **k):
    """(what fn returned, what it printed)"""
    with contextlib.redirect_stdout(io.StringIO()) as out:
        r = fn(*a, **k)
    return r, out.getvalue()


@pytest.fixture(scope="module")
def gold(golden):
    return golden("qc")


def sample(d, s):
    return d["cell_ptr"], d["gene"], d[s + "_val"]


def test_header_is_plain_c_and_links(tmp_path):
    _lib.lib()
    exe = build_qc_check(tmp_path)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "%d entry points" % len(_lib.QC_SYMBOLS) in r.stdout, r.stdout


def test_library_exports_qc_symbols():
    src = open(os.path.join(REPO, "include", "nabo_qc.h")).read()
    assert '#include "nabo_knn.h"' in src
    assert "nabo_qc.h" not in open(os.path.join(REPO, "include", "nabo_knn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_lib.QC_SYMBOLS)
    others = _lib.SYMBOLS + _lib.GRAPH_SYMBOLS + _lib.CLUSTER_SYMBOLS + _lib.DE_SYMBOLS + _lib.PCA_SYMBOLS + _lib.PCA_FIT_SYMBOLS
    assert not set(_lib.QC_SYMBOLS) & set(others)
    L = _lib.lib()
    for n in _lib.QC_SYMBOLS:
        assert hasattr(L, n), n
    kernel = open(os.path.join(REPO, "nabo_amd", "csrc", "cell_qc.hip")).read()
    assert "QC_LDS_TABLE_GENES = %d;" % _qc.LDS_TABLE_GENES in kernel and "n_raw_genes <= %d" % _qc.LDS_TABLE_GENES in open(
        os.path.join(REPO, "include", "nabo_qc.h")).read()


def test_public_names():
    for n in ("cell_qc_csr", "filter_data", "set_sf", "qc_and_sf", "gene_stats", "correct_var", "find_hvgs", "get_lvgs", "dump_hvgs"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))


GOOD = dict(cell_ptr=[0, 2, 3], gene=[0, 2, 1], val=[1.0, 2.0, 3.0], gene_class=[1, 0, 3], n_classes=2)


@pytest.mark.parametrize("change", [
    {"cell_ptr": [0, 4, 3]},                                  # cell_ptr not monotone
    {"cell_ptr": [1, 2, 3]},                                  # cell_ptr[0] != 0
    {"cell_ptr": [0, 2, 4]},                                  # cell_ptr[-1] past the end of the entries
    {"cell_ptr": [[0, 2, 3]]},                                # not 1-D
    {"gene": [0, 3, 1]},                                      # gene out of range
    {"gene": [0, -1, 1]},                                     # negative gene
    {"gene": [2, 0, 1]},                                      # genes of a cell not increasing
    {"gene": [1, 1, 0]},                                      # a gene twice in a cell
    {"gene": [0, 2 ** 40, 1]},                                # does not fit 32 bits
    {"val": [1.0, np.nan, 3.0]},                              # NaN
    {"val": [1.0, np.inf, 3.0]},                              # infinite
    {"val": [1.0, -2.0, 3.0]},                                # a negative value
    {"val": [1.0, 2.0]},                                      # fewer values than genes
    {"n_classes": 9},
    {"n_classes": -1},
    {"gene_class": None},                                     # classes without a table
    {"gene_class": [[1, 0, 3]]},                              # not 1-D
    {"rows": [0, 2]},                                         # a row that is no cell
    {"rows": [-1]},
    {"rows": [[0]]},
])
def test_bad_arguments_raise_before_any_device(change):
    with pytest.raises(ValueError) as e:
        nabo_amd.cell_qc_csr(**dict(GOOD, **change))
    assert str(e.value).startswith("ERROR: ")


def test_no_device_is_a_loud_failure():
    if nabo_amd.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device path is covered on the CPU box")
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.cell_qc_csr(**GOOD)
    assert "no HIP device" in str(e.value)


def test_restatement_orders_and_float32_trap():
    """the header's order on a case a float32 accumulator gets wrong, and against exactly rounded sums"""
    n, s = qref.cell_qc([0, 3], [0, 1, 2], [16777216.0, 1.0, 1.0], [1, 0, 1], 1)
    assert n.tolist() == [3] and s.tolist() == [[16777218.0, 16777217.0]]
    assert np.float32(16777216.0) + np.float32(1.0) == np.float32(16777216.0)
    rng = np.random.default_rng(1)
    x = rng.random(1000).astype(np.float32)
    ptr = [0, 0, 1, 17, 1000]
    a, b = qref.cell_qc(ptr, np.arange(1000) % 50, x)[1], qref.cell_qc(ptr, np.arange(1000) % 50, x, exact=True)[1]
    assert a[0, 0] == 0 and a[1, 0] == float(x[0]) and (np.abs(a - b) <= 1000 * 2.0 ** -53 * b).all()


@pytest.mark.parametrize("n_classes", [0, 3, 8])
def test_restatement_for_many_cells_equals_the_plain_one(n_classes):
    """qref.cell_qc_many (short cells all at once) against qref.cell_qc bit for bit: cells of 0 .. 17 entries, the
    lengths of the geometry tests and an empty last cell, with no class, three and eight"""
    from test_qc_gpu import EDGE_LENGTHS, edge_cells            # (that module imports this one)
    lengths = EDGE_LENGTHS + list(range(18)) + [16, 1, 16, 0]
    cell_ptr, gene, val, cls = edge_cells(5000, lengths, seed=50 + n_classes)
    val[cell_ptr[18]:cell_ptr[19]] = 0                          # a cell of five stored zeros only
    want = qref.cell_qc(cell_ptr, gene, val, cls if n_classes else None, n_classes)
    got = qref.cell_qc_many(cell_ptr, gene, val, cls if n_classes else None, n_classes)
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]) and got[0].tolist() == lengths
    assert got[1].shape == (len(lengths), 1 + n_classes) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
    assert (got[1][:, 0] > 0).sum() > 25 and got[1][18, 0] == 0 and lengths[18] == 5
    for k in range(n_classes):                                  # every class holds some of a cell's sum, never all of every cell's
        assert (got[1][:, 1 + k] > 0).any() and (got[1][:, 1 + k] < got[1][:, 0]).any()


@pytest.mark.parametrize("s", ["A", "B"])
@pytest.mark.parametrize("pre", ["", "_pre"])
def test_filter_reproduces_the_reference(gold, s, pre):
    """keep lists, report counts and lines of both samples, with keep lists in the file beforehand and without; sample
    B's thresholds lie in gaps 1000 x the measured deviation wide, so its lists are equal too"""
    d = gold
    genes = [str(g) for g in d["genes"]]
    mp, rp = qref.patterns_of(d)
    thr = qref.thresholds_of(d, s)
    kc0 = d["pre_cells"] if pre else np.arange(len(d["cells"]))
    kg0 = d["pre_genes"] if pre else np.arange(len(genes))
    (kc, kg, counts), _ = said(_qc._filter_from_csr, genes, sample(d, s), d[s + "_abundance"], kc0, kg0, mp, rp, qref.step, **thr)
    assert kc.dtype == np.int64 and np.array_equal(kc, d[s + pre + "_keep_cells"]) and np.array_equal(kg, d[s + pre + "_keep_genes"])
    assert counts == d[s + pre + "_counts"].tolist() and min(counts) >= 1
    assert _qc._report(counts) == [str(x) for x in d[s + pre + "_report"]]
    meta = json.loads(str(d["meta"]))
    where = {g: i for i, g in enumerate(genes)}
    assert meta["empty_cell"] not in kc and meta["zero_gene"] not in kg and where["mt-x"] not in kg and where["mito_a"] not in kg
    # the one-pass form gives the same lists and the same size factors
    (kc2, kg2, counts2, sf), _ = said(_qc._qc_and_sf_from_csr, genes, sample(d, s), d[s + "_abundance"], kc0, kg0, mp, rp, 1000.0, False, qref.step, **thr)
    assert np.array_equal(kc2, kc) and np.array_equal(kg2, kg) and counts2 == counts
    if s == "A":
        assert np.array_equal(sf.view(np.int32), d[s + pre + "_sf"].view(np.int32))


def test_sums_and_percentages_of_the_reference(gold):
    """sample A: float32 of the restated sums is the reference's float32 sum, bit for bit; sample B: within the measured
    deviation (4 x: the project's margin)"""
    d = gold
    cls = qref.class_bits(d["genes"], *qref.patterns_of(d))
    for s in ("A", "B"):
        n_ent, sums = qref.cell_qc(*sample(d, s), cls, 2)
        ref = np.stack([d[s + "_tot"], d[s + "_cum_mito"], d[s + "_cum_ribo"]], axis=1)
        assert np.array_equal(n_ent, d[s + "_ngenes"].astype(np.int64))
        if s == "A":
            assert np.array_equal(sums.astype(np.float32), ref)
        else:
            rel = np.abs(sums - ref)[ref != 0] / ref[ref != 0]
            print("sample B: float64 sums against the reference's float32 ones %.3g (measured %.3g)" % (rel.max(), float(d["tot_dev"])))
            assert rel.max() <= 4 * float(d["tot_dev"]) and rel.max() > 0


@pytest.mark.parametrize("pre", ["", "_pre"])
def test_size_factors_bit_equal_on_sample_a(gold, pre):
    d = gold
    n_genes = len(d["genes"])
    m, kg = sample(d, "A"), d["A" + pre + "_keep_genes"]
    ones = np.ones(len(d["cells"]), np.float32)
    for name, kw in (("sf", {}), ("sf_all", {"all_genes": True}), ("sf_scale", {"size_scale": 1234.567})):
        sf = _qc._sf_from_csr(list(d["cells"]), n_genes, m, kg, ones, step=qref.step, **kw)
        assert sf.dtype == np.float32 and np.array_equal(sf.view(np.int32), d["A" + pre + "_" + name].view(np.int32)), name
    # an empty cell: its sum counts as 1
    assert sf[json.loads(str(d["meta"]))["empty_cell"]] == np.float32(1234.567)
    # not a float32 division
    s = np.array([3.0, 7.0, 1234.0])
    assert np.array_equal(_qc._sf_from_sums(s, 1234.567), (1234.567 / s).astype(np.float32))
    # a dict replaces the named cells' entries of the vector in use
    sf2 = _qc._sf_from_csr(["a", "b", "c"], 1, ([0, 0, 0, 0], [], []), [0], np.array([1, 2, 3], np.float32), sf={"c": 4.0, "a": 8.0}, size_scale=100.0)
    assert sf2.tolist() == [12.5, 2.0, 25.0]
    with pytest.raises(TypeError) as e:
        _qc._sf_from_csr(["a"], 1, ([0, 0], [], []), [0], ones[:1], size_scale=None)
    assert "size_scale parameter should have a float value" in str(e.value)


def test_negative_min_gene_abundance_is_reset(gold):
    d = gold
    n = len(d["cells"])
    z = np.zeros(n)
    (_, kg, _), text = said(_qc._filter_from_sums, z, z, z, z, d["A_abundance"], range(n), range(len(d["genes"])), [], [], min_gene_abundance=-3,
                            rm_mito=False, rm_ribo=False)
    assert text.splitlines() == ["'min_gene_abundance' should be greater than or equal to 0", "Resetting 'min_gene_abundance' to 0"]
    assert kg.shape[0] == len(d["genes"])


def test_class_columns_follow_the_upper_case_lookup():
    genes = ["MT-A", "mt-x", "mito_a", "MITO_A", "G1"]
    cls, mito_idx, ribo_idx = _qc._classes(genes, [4], ["^MT-", "^mt-", "^mito_"], ["^RP"])
    assert cls.tolist() == [1, 0, 0, 1, 4] and sorted(mito_idx) == [0, 1, 2] and ribo_idx == []
    assert np.array_equal(cls & 3, qref.class_bits(genes, ["^MT-", "^mt-", "^mito_"], ["^RP"]))
    with pytest.raises(ValueError):
        _qc._classes(["MT-A", "mt-a"], None, ["^MT-", "^mt-"], [])


def test_lowess_and_correct_var_within_the_measured_deviation(gold):
    d = gold
    for nb in (100, 30):
        tab, bins_min, cor = _qc.correct_var(qref.stats_of(d, "A"), nb)
        # the bins' genes are the reference's: their log means agree to the last places (numpy's log is within an ulp of
        # the exact one in either build, so two builds are within 2 ulp of each other; 4 allowed)
        want = d["A_bins_min_%d" % nb]
        assert bins_min.shape == want.shape and (np.abs(bins_min - want) <= 4 * np.spacing(np.abs(want))).all()
        ref = d["A_var_cor_%d" % nb]
        dev = (np.abs(cor - ref) / np.maximum(1.0, np.abs(ref))).max()
        fv, ref_fv = _qc._table(tab)[1]["fixed_var"], d["A_fixed_var_%d" % nb]
        fdev = (np.abs(fv - ref_fv) / ref_fv).max()
        print("n_bins %d: LOWESS %.3g (measured %.3g), fixed_var %.3g (measured %.3g)" % (nb, dev, float(d["lowess_dev"]), fdev, float(d["fixed_var_dev"])))
        assert dev <= 4 * float(d["lowess_dev"]) and fdev <= 4 * float(d["fixed_var_dev"])
        zero = json.loads(str(d["meta"]))["zero_gene"]
        assert fv[zero] == fv.min()
    # a straight line is its own LOWESS curve; the fit comes back in the caller's order
    x = np.linspace(0, 1, 40)
    y = 2 * x + 1
    assert np.allclose(_qc.lowess(y, x, 0.4, 3), y, atol=1e-12)
    y2 = y + np.sin(37 * x)
    y2[20] += 50
    assert np.array_equal(_qc.lowess(y2[::-1], x[::-1], 0.4, 100)[::-1], _qc.lowess(y2, x, 0.4, 100))


def test_hvgs_and_lvgs_equal_the_reference(gold):
    d = gold
    tab = qref.stats_of(d, "A", 100)
    explicit = json.loads(str(d["hvg_explicit_args"]))
    for name, kw in (("corrected", dict(use_corrected_var=True)), ("plain", {}), ("explicit", dict(use_corrected_var=True, **explicit))):
        hv, text = said(_qc.find_hvgs, tab, **kw)
        assert hv == [str(x) for x in d["A_hvg_" + name]] and len(hv) >= 5, name
        assert text == "%d highly variable genes found\n" % len(hv)
    for name, kw in json.loads(str(d["lvg_args"])).items():
        lv, text = said(_qc.get_lvgs, tab, hvgs=d["A_hvg_explicit"], **kw)
        assert lv == [str(x) for x in d["A_lvg_" + name]] and text == "", name
    # both forms of the table give the same answers
    pd = pytest.importorskip("pandas")
    frame = pd.DataFrame({k: v for k, v in tab.items() if k != "genes"}, index=tab["genes"])
    assert said(_qc.find_hvgs, frame, use_corrected_var=True)[0] == [str(x) for x in d["A_hvg_corrected"]]
    assert list(_qc.correct_var(frame, 30)[0]["fixed_var"].values) == list(_qc._table(_qc.correct_var(tab, 30)[0])[1]["fixed_var"])


def test_hvg_and_lvg_error_paths(gold):
    tab = qref.stats_of(gold, "A")
    with pytest.raises(ValueError) as e:
        _qc.find_hvgs(tab, use_corrected_var=True)
    assert 'run "correct_var" method first' in str(e.value)
    with pytest.raises(ValueError) as e:
        _qc.get_lvgs(tab, nzm_cutoff=1.0, use_corrected_var=True)
    assert '"use_fixed_var" parameter is set to True' in str(e.value)
    with pytest.raises(ValueError) as e:
        _qc.get_lvgs(tab, n=3)
    assert "either of the two parameters" in str(e.value)
    with pytest.raises(ValueError) as e:
        _qc.get_lvgs(tab, nzm_cutoff=1.0, log_nzm_cutoff=0.0, n=3)
    assert "only ONE" in str(e.value)
    lv, text = said(_qc.get_lvgs, tab, nzm_cutoff=1e9, n=3)
    assert lv == [] and text.startswith('WARNING: Number of LVGs is lower than "n"/HVGs')
    with pytest.raises(ValueError):
        said(_qc.find_hvgs, tab, update_cache=True)
    # ties in the LVG sort go to table order
    t = {"genes": list("abcd"), "valid_gene": np.ones(4, bool), "m": np.ones(4), "nzm": np.full(4, 2.0), "variance": np.array([3.0, 1.0, 3.0, 1.0]),
         "ncells": np.full(4, 5.0)}
    assert _qc.get_lvgs(t, nzm_cutoff=1.0, n=4) == ["b", "d", "a", "c"]


def test_statistics_table_fills_invalid_genes_with_the_minima(gold):
    st = {"valid": np.array([1, 0, 1], np.uint8), "ncells": np.array([4, 0, 2]), "m": np.array([2.0, 0.0, 0.5]), "nzm": np.array([3.0, 0.0, 4.0]),
          "variance": np.array([1.0, 0.0, 9.0])}
    names, cols = _qc._table(_qc._stats_table(["a", "b", "c"], st))
    assert names == ["a", "b", "c"] and cols["valid_gene"].tolist() == [True, False, True]
    assert cols["m"].tolist() == [2.0, 0.5, 0.5] and cols["nzm"].tolist() == [3.0, 3.0, 4.0] and cols["variance"].tolist() == [1.0, 1.0, 9.0]
    assert cols["ncells"].tolist() == [4.0, 0.0, 2.0]

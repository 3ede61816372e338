"""The PCA projection and the gene statistics (include/nabo_pca.h, nabo_amd/_pca.py) without a GPU: the C header and its
symbols, argument checks, the no-device failure, the tests' plain restatement against the reference's vectors and
statistics (tests/golden/pca.npz, tools/gen_golden_pca.py), and the host logic -- which genes are valid and in which
order, missing genes, the forms of scaling_params -- with the device step replaced by that restatement."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _lib, _pca

import _pca_ref as pref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_pca_check(tmp_path):
    exe = os.path.join(str(tmp_path), "pca_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "abi_c", "pca_check.c"), "-L" + os.path.join(REPO, "nabo_amd"), "-lnabo_knn",
           "-Wl,-rpath," + os.path.join(REPO, "nabo_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    return exe


def ref_project_step(m, gene_pos, mu, sigma, mean, components, rows):
    """the restatement in the place of _pca._device_project"""
    return pref.project(m[1], m[2], m[3], m[4], gene_pos, mu, sigma, mean, components, rows)


def ref_stats_step(m, keep_cells, keep_genes):
    """the restatement in the place of _pca._device_stats"""
    return pref.gene_stats(m[1], m[2], m[3], m[4], keep_cells, keep_genes)


def test_header_is_plain_c_and_links(tmp_path):
    _lib.lib()
    exe = build_pca_check(tmp_path)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "%d entry points" % len(_lib.PCA_SYMBOLS) in r.stdout, r.stdout


def test_library_exports_pca_symbols():
    src = open(os.path.join(REPO, "include", "nabo_pca.h")).read()
    assert '#include "nabo_knn.h"' in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_lib.PCA_SYMBOLS)
    assert not set(_lib.PCA_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.GRAPH_SYMBOLS) | set(_lib.CLUSTER_SYMBOLS) | set(_lib.DE_SYMBOLS))
    L = _lib.lib()
    for n in _lib.PCA_SYMBOLS:
        assert hasattr(L, n), n


def test_public_names():
    for n in ("pca_project_csr", "gene_stats_csc", "get_scaling_params", "transform_pca"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))


GOOD = dict(cell_ptr=[0, 2, 3], gene=[0, 2, 1], val=[1.0, 2.0, 3.0], sf=[1.0, 1.0], gene_pos=[0, 1, -1], mu=[0.5, 0.25], sigma=[1.0, 2.0],
            mean=[0.0, 0.1], components=[[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
GOOD_STATS = dict(gene_ptr=[0, 2, 3], cell=[0, 2, 1], val=[1.0, 2.0, 3.0], sf=[1.0, 1.0, 1.0])


@pytest.mark.parametrize("change", [
    {"cell_ptr": [0, 4, 3]},                                  # cell_ptr not monotone
    {"cell_ptr": [1, 2, 3]},                                  # cell_ptr[0] != 0
    {"cell_ptr": [0, 2, 4]},                                  # cell_ptr[-1] past the end of the entries
    {"cell_ptr": [0, 2, 3, 3]},                               # more cells than size factors
    {"gene": [0, 3, 1]},                                      # gene out of range
    {"gene": [0, -1, 1]},                                     # negative gene
    {"gene": [2, 0, 1]},                                      # genes of a cell not increasing
    {"gene": [1, 1, 0]},                                      # a gene twice in a cell
    {"gene": [0, 2 ** 40, 1]},                                # does not fit 32 bits
    {"val": [1.0, np.nan, 3.0]},                              # NaN
    {"val": [1.0, np.inf, 3.0]},                              # infinite
    {"val": [1.0, -2.0, 3.0]},                                # a negative value
    {"sf": [1.0, -1.0]},                                      # a negative scaled value
    {"sf": [np.nan, 1.0]},
    {"val": [1.0, 3e38, 3.0], "sf": [10.0, 1.0]},            # the float32 product overflows
    {"gene_pos": [0, 2, -1]},                                 # a position >= G
    {"gene_pos": [0, 0, -1]},                                 # a position twice
    {"gene_pos": [0, 1, -2]},                                 # neither -1 nor a position
    {"sigma": [1.0, 0.0]},                                    # sigma zero
    {"sigma": [1.0, -1.0]},                                   # negative
    {"sigma": [np.nan, 1.0]},                                 # NaN
    {"sigma": [1.0, np.inf]},                                 # infinite
    {"mu": [0.0, np.nan]},
    {"mean": [0.0, 0.0, 0.0]},                                # mean of another length
    {"mu": [0.0]},                                            # mu of another length
    {"components": [[1.0, 0.0, 0.0]]},                        # components over another number of genes
    {"components": [1.0, 0.0]},                               # components not 2-D
    {"components": [[1.0, np.inf]]},
    {"rows": [0, 2]},                                         # a row that is no cell
    {"rows": [-1]},
    {"rows": [[0, 1]]},                                       # rows not 1-D
])
def test_bad_arguments_are_refused_before_any_device(change):
    with pytest.raises(ValueError):
        nabo_amd.pca_project_csr(**dict(GOOD, **change))


@pytest.mark.parametrize("change", [
    {"keep_cells": [0, 0]},                                   # a kept cell twice
    {"keep_cells": [0, 3]},                                   # a kept cell that is no cell
    {"keep_cells": []},                                       # no cell kept
    {"keep_genes": [1]},                                      # a mask of another length
    {"gene_ptr": [0, 3, 2]},
    {"cell": [1, 1, 1]},
    {"val": [1.0, -2.0, 3.0]},
    {"val": [1.0, 3e38, 3.0], "sf": [1.0, 1.0, 10.0]},
])
def test_bad_statistics_arguments_are_refused_before_any_device(change):
    with pytest.raises(ValueError):
        nabo_amd.gene_stats_csc(**dict(GOOD_STATS, **change))


def test_null_outputs_are_refused():
    L = _lib.lib()
    m = _pca._csr((GOOD["cell_ptr"], GOOD["gene"], GOOD["val"], GOOD["sf"]))
    t = _pca._tables(GOOD["gene_pos"], GOOD["mu"], GOOD["sigma"], GOOD["mean"], GOOD["components"])
    st = L.nabo_pca_project(0, 2, 3, m[1].ctypes.data, m[2].ctypes.data, m[3].ctypes.data, m[4].ctypes.data, t[0].ctypes.data, 2,
                            t[1].ctypes.data, t[2].ctypes.data, t[3].ctypes.data, 3, t[4].ctypes.data, 0, None, 0, None)
    assert st == _lib.E_INVALID and b"output" in L.nabo_last_error()
    a = {k: np.ascontiguousarray(v, dtype=d) for (k, v), d in zip(GOOD_STATS.items(), (np.int64, np.int32, np.float32, np.float32))}
    st = L.nabo_gene_stats(0, 2, 3, a["gene_ptr"].ctypes.data, a["cell"].ctypes.data, a["val"].ctypes.data, a["sf"].ctypes.data, 0, None, None,
                           *[None] * 5)
    assert st == _lib.E_INVALID and b"output" in L.nabo_last_error()
    assert L.nabo_pca_last_device_ms(None, None) == _lib.E_INVALID


def test_first_offending_entry_is_named():
    with pytest.raises(ValueError) as e:
        nabo_amd.pca_project_csr(**dict(GOOD, gene=[0, 2, 5]))
    assert "gene[2] = 5" in str(e.value)
    with pytest.raises(ValueError) as e:
        nabo_amd.pca_project_csr(**dict(GOOD, sigma=[1.0, 0.0]))
    assert "sigma[1]" in str(e.value)


def test_no_device_is_a_loud_failure():
    if nabo_amd.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device path is covered on the CPU box")
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.pca_project_csr(**GOOD)
    assert "no HIP device" in str(e.value)
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.gene_stats_csc(**GOOD_STATS)
    assert "no HIP device" in str(e.value)


def test_restatement_reproduces_reference_projections(golden):
    """every vector the reference's transform_pca wrote, within 4 x the deviation the generator measured (the factor the
    DE tests use over a measured deviation); the generator asserted that deviation below 1e-9"""
    d = golden("pca")
    tol = 4 * float(d["proj_dev"])
    assert 0 < tol < 4e-9
    calls = pref.projection_calls(d)
    assert [c[0] for c in calls] == ["ref", "target"]
    for name, _, kw, Zref in calls:
        Z = pref.project(**kw)
        assert Z.shape == Zref.shape and Z.shape[0] >= 200 and Z.shape[1] == 8
        dev = pref.row_dev(Zref, Z)
        print("%s: deviation %.3g (allowed %.3g)" % (name, dev, tol))
        assert dev <= tol, name
    # the fixture holds what the issue asks of it: dropped cells and genes, invalid kept genes, missing selected genes
    assert len(d["r_keep_cells"]) < len(d["r_cells"]) and len(d["r_keep_genes"]) < len(d["r_genes"])
    assert ((d["r_stats_valid"] == 0) & (pref.keep_mask(d, "r") == 1)).sum() >= 1
    assert pref.meta(d)["n_missing"] >= 2 and pref.meta(d)["fill_missing_false"] == "KeyError"


def test_restatement_reproduces_reference_statistics(golden):
    d = golden("pca")
    got = pref.gene_stats(*pref.csc_of(d, "r"), keep_cells=d["r_keep_cells"], keep_genes=pref.keep_mask(d, "r"))
    want = pref.golden_stats(d)
    assert np.array_equal(got["ncells"], want["ncells"]) and np.array_equal(got["valid"], want["valid"])
    devs = pref.stats_devs(want, got)
    for k, dev, stored in zip(("m", "nzm", "variance"), devs, (d["m_dev"], d["nzm_dev"], d["var_dev"])):
        print("%s: deviation %.3g (allowed %.3g)" % (k, dev, 4 * float(stored)))
        assert dev <= 4 * float(stored), k
    for k in ("m", "nzm", "variance"):
        assert (got[k][want["valid"] == 0] == 0).all()


def _close(a, b, rel):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((np.abs(a - b) <= rel * np.abs(b)).all())


def test_get_scaling_params_host_logic_reproduces_reference(golden):
    """gene selection and order exactly; mu and sigma within 4 x the measured float32-vs-float64 deviations"""
    d = golden("pca")
    raw = [str(x) for x in d["r_genes"]]
    m = nabo_amd._de._csc(pref.csc_of(d, "r"), "golden")
    args = (raw, d["r_keep_genes"].tolist(), m, d["r_keep_cells"])
    m_tol, s_tol = 4 * float(d["m_dev"]), 4 * float(d["var_dev"])
    names, mu, sigma = _pca._scaling_from_csc(*args, step=ref_stats_step)
    assert names == [str(x) for x in d["r_params_genes"]] and len(names) > 90
    assert _close(mu, d["r_params_mu"], m_tol) and _close(sigma, d["r_params_sigma"], s_tol)
    asked = [str(x) for x in d["pca_asked"]]
    names, mu, sigma = _pca._scaling_from_csc(*args, genes=asked, step=ref_stats_step)
    assert names == [str(x) for x in d["pca_genes"]] and names != sorted(names, key=raw.index)      # the given order, not the file's
    assert _close(mu, d["pca_mu"], m_tol) and _close(sigma, d["pca_sigma"], s_tol)
    names, mu, sigma = _pca._scaling_from_csc(*args, only_valid=False, step=ref_stats_step)
    assert names == [str(x) for x in d["r_params_any_genes"]] == raw
    assert _close(mu, d["r_params_any_mu"], m_tol) and _close(sigma, d["r_params_any_sigma"], s_tol)
    with pytest.raises(ValueError) as e:
        _pca._scaling_from_csc(*args, genes=["G7", "G4", "nobody"], step=ref_stats_step)
    assert pref.meta(d)["none_valid"] == "ValueError: " + str(e.value)
    # both forms of the result
    p = _pca._as_params(["a", "b"], np.array([1.0, 2.0]), np.array([3.0, 4.0]))
    assert _pca._params(p)[0] == ["a", "b"] and _pca._params(p)[2].tolist() == [3.0, 4.0]
    assert _pca._params({"genes": ["a", "b"], "mu": [1.0, 2.0], "sigma": [3.0, 4.0]})[1].tolist() == [1.0, 2.0]
    try:
        import pandas  # noqa: F401
        assert list(p.columns) == ["mu", "sigma"] and list(p.index) == ["a", "b"]
    except ImportError:
        assert sorted(p) == ["genes", "mu", "sigma"]


def test_transform_pca_host_logic_reproduces_reference(golden, capsys):
    d = golden("pca")
    tol = 4 * float(d["proj_dev"])
    tr = types.SimpleNamespace(mean_=d["pca_mean"], components_=d["pca_components"], whiten=False)
    sp = {"genes": [str(x) for x in d["pca_genes"]], "mu": d["pca_mu"], "sigma": d["pca_sigma"]}
    forms = [sp, _pca._as_params(sp["genes"], sp["mu"], sp["sigma"])]
    mr, mt = _pca._csr(pref.csr_of(d, "r")), _pca._csr(pref.csr_of(d, "t"))
    raw_r, raw_t = [str(x) for x in d["r_genes"]], [str(x) for x in d["t_genes"]]
    for form in forms:
        capsys.readouterr()
        Z = _pca._project_from_csr(raw_r, mr, d["r_keep_cells"], tr, form, False, ref_project_step)
        assert capsys.readouterr().out == "" and pref.row_dev(d["r_Z"], Z) <= tol
        with pytest.raises(KeyError) as e:
            _pca._project_from_csr(raw_t, mt, d["t_keep_cells"], tr, form, False, ref_project_step)
        assert "not found" in str(e.value)
        Z = _pca._project_from_csr(raw_t, mt, d["t_keep_cells"], tr, form, True, ref_project_step)
        assert capsys.readouterr().out.strip() == pref.meta(d)["warning"]
        assert pref.row_dev(d["t_Z"], Z) <= tol
    # a cell without entries projects to the bias; the fixture's target holds one
    empty = np.nonzero(np.diff(d["t_cell_ptr"]) == 0)[0]
    assert empty.size >= 1
    assert np.array_equal(Z[empty[0]], pref.bias_of(sp["mu"], sp["sigma"], tr.mean_, tr.components_))
    args = (raw_r, mr, d["r_keep_cells"])
    for bad_tr, bad_sp in ((None, sp), (tr, None), (types.SimpleNamespace(mean_=tr.mean_, components_=tr.components_, whiten=True), sp),
                           (tr, dict(sp, genes=sp["genes"][:-1] + sp["genes"][:1])),
                           (types.SimpleNamespace(mean_=tr.mean_[:-1], components_=tr.components_[:, :-1]), sp),
                           (tr, dict(sp, sigma=np.where(np.arange(len(sp["genes"])) == 3, 0.0, sp["sigma"])))):
        with pytest.raises(ValueError):
            step = ref_project_step if bad_sp is None or np.all(np.asarray(bad_sp["sigma"]) > 0) else nabo_amd._pca._device_project
            _pca._project_from_csr(*args, bad_tr, bad_sp, False, step)


def test_dataset_reader_builds_rows_from_records():
    """an index listed twice keeps its last value, the indices come out increasing"""
    rec = np.zeros(4, dtype=[("idx", np.uint32), ("val", np.float32)])
    rec["idx"], rec["val"] = [5, 2, 5, 3], [1.0, 2.0, 3.0, 4.0]
    idx, val = nabo_amd._de._DatasetFile._record(rec)
    assert idx.tolist() == [2, 3, 5] and val.tolist() == [2.0, 4.0, 3.0]

"""The Mann-Whitney DE test on the MI355X (nabo_de_test, nabo_amd._de): parity through the C ABI with the tests' plain
restatement and with the reference's tables (tests/golden/de.npz) on the fixtures and the quirk cases, the file-level
functions on Nabo-format dataset files, a 200k-cell x 2k-gene x 16-cluster case in forced chunks, and the plain-C
consumer."""
import json
import os
import subprocess

import numpy as np
import pytest

import _de_ref as dref
from test_de_cpu import build_de_check, tolerances
from test_mapping import _interpreter

HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _compare_steps(got, want, log2fc_tol, p_rel, what):
    """status, counts, 2U and the tie term exact; rbc and z bit-equal; log2_fc and pval within the tolerances"""
    for k in ("status", "nonzero_test", "n1", "n2", "u2", "tie"):
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:5].tolist())
    for k in ("rbc", "z"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k, np.argwhere(_bits(got[k]) != _bits(want[k]))[:5].tolist())
    a, b = got["log2_fc"], want["log2_fc"]
    fin = np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[np.isinf(b)], b[np.isinf(b)]) and np.array_equal(np.isfinite(a), fin), what
    print("%s: largest log2_fc difference %.3g (allowed %.3g)" % (what, np.abs(a[fin] - b[fin]).max() if fin.any() else 0.0, log2fc_tol))
    assert (np.abs(a[fin] - b[fin]) <= log2fc_tol).all(), what
    p, q = got["pval"], want["pval"]
    print("%s: largest relative pval difference %.3g (allowed %.3g)" % (what, (np.abs(p - q) / np.where(q > 0, q, 1)).max() if q.size else 0.0, p_rel))
    assert (np.abs(p - q) <= p_rel * q).all(), what


def _gpu_step(budget=0):
    from nabo_amd._de import _device_de

    def step(*a):
        return _device_de(*a, mem_budget=budget)
    return step


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [0, 40000])
def test_fixture_and_quirk_parity_through_the_abi(gpu_lib, golden, budget):
    """every golden call: the device step against the restatement, array by array, and the host logic on the device's
    arrays against the reference's tables (row sets exactly); with a 40 kB budget the genes go in several chunks"""
    from nabo_amd import _de
    d = golden("de")
    tol, p_rel = tolerances(d)
    seen, chunks = set(), []

    def step(*a):
        got, want = _gpu_step(budget)(*a), dref.de_step(*a)
        chunks.append(_de.last_device_ms()[1])
        _compare_steps(got, want, tol, p_rel, "budget %d, call %d" % (budget, len(chunks)))
        seen.update(np.unique(got["status"]).tolist())
        return got
    assert dref.check_cases(d, step, tol, p_rel) >= 600
    assert dref.check_markers(d, step, tol, p_rel) >= 200
    assert seen == {dref.SKIP_GENE, dref.SKIP_PAIR, dref.ASYMPTOTIC, dref.EXACT, dref.EMPTY}
    assert max(chunks) > 1 if budget else max(chunks) == 1, chunks


@pytest.mark.gpu
def test_array_level_entry_point_and_budget_errors(gpu_lib, golden):
    import nabo_amd
    d = golden("de")
    case = dref.golden_cases(d)[0]
    genes, m1, m2, test_idx, groups = dref.case_inputs(d, case)
    sets = [test_idx] + groups
    sp = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    mem = [c for s in sets for c in s]
    got = nabo_amd.de_test_csc(m1[1], m1[2], m1[3], m1[4], sp, mem, exp_frac_thresh=0.25, log2_fc_thresh=1.0)
    want = dref.de_step(len(genes), m1, None, sp, np.array(mem), [0, 0, 0], [1, 2, 3], 0.25, 1.0)
    _compare_steps(got, want, *tolerances(d), "de_test_csc")
    # explicit pairs in another order, a set that is test and control, a set in no pair
    got = nabo_amd.de_test_csc(m1[1], m1[2], m1[3], m1[4], sp, mem, pair_test=[2, 0, 1], pair_ctrl=[0, 2, 1], exp_frac_thresh=0.1, log2_fc_thresh=-3.0)
    want = dref.de_step(len(genes), m1, None, sp, np.array(mem), [2, 0, 1], [0, 2, 1], 0.1, -3.0)
    _compare_steps(got, want, *tolerances(d), "explicit pairs")
    assert (got["status"] >= dref.ASYMPTOTIC).sum() > 20
    # a budget one gene does not fit in is refused, not exceeded
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.de_test_csc(m1[1], m1[2], m1[3], m1[4], sp, mem, mem_budget=64)
    assert "budget" in str(e.value)


@pytest.mark.gpu
def test_file_level_functions(gpu_lib):
    py = _interpreter()
    if py is None:
        pytest.skip("no interpreter with h5py in this image")
    r = subprocess.run([py, os.path.join(HERE, "_de_case.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["checked"] >= 20 and res["rows"] >= 800 and res["differ"] == [], res


def scale_case(n_cells, n_genes, n_clusters, seed):
    """single-cell-like sparsity: every gene at 3 % of the cells, every fourth one at 40 % of its home cluster with
    doubled counts; gene 5 has no nonzero, gene 6 is nonzero in every cell, with doubled counts in cluster 3"""
    rng = np.random.default_rng(seed)
    cluster = rng.integers(0, n_clusters, n_cells)
    sf = (0.5 + rng.random(n_cells)).astype(np.float32)
    ptr, cells, vals = [0], [], []
    for j in range(n_genes):
        p = np.full(n_cells, 0.03)
        if j % 4 == 0:
            p[cluster == j % n_clusters] = 0.4
        idx = np.nonzero(rng.random(n_cells) < (0.0 if j == 5 else 2.0 if j == 6 else p))[0]
        lam = np.where(cluster[idx] == (3 if j == 6 else j % n_clusters), 3.0, 1.5) if j % 4 == 0 or j == 6 else 1.5
        cells.append(idx.astype(np.int32))
        vals.append((rng.poisson(lam, idx.shape[0]) + 1).astype(np.float32))
        ptr.append(ptr[-1] + idx.shape[0])
    order = np.argsort(cluster, kind="stable")
    set_ptr = np.concatenate([[0], np.cumsum(np.bincount(cluster, minlength=n_clusters))]).astype(np.int64)
    return (n_cells, np.array(ptr, dtype=np.int64), np.concatenate(cells), np.concatenate(vals), sf), set_ptr, order.astype(np.int64)


@pytest.mark.gpu
def test_scale_200k_cells_2k_genes_16_clusters_in_chunks(gpu_lib):
    """every cluster against every other (240 pairs per gene) in ONE call, the genes forced into chunks by a 64 MiB
    budget; all 480 000 (gene, pair) results against the restatement"""
    from nabo_amd import _de
    n_cells, n_genes, k = 200000, 2000, 16
    m, set_ptr, members = scale_case(n_cells, n_genes, k, seed=77)
    pt = np.repeat(np.arange(k, dtype=np.int32), k - 1)
    pc = np.array([j for i in range(k) for j in range(k) if j != i], dtype=np.int32)
    got = _de._device_de(n_genes, m, None, set_ptr, members, pt, pc, 0.25, 0.5, mem_budget=64 << 20)
    ms, chunks = _de.last_device_ms()
    print("nnz %d, %d chunks, device ms %s" % (m[2].shape[0], chunks, ms))
    assert chunks > 4
    want = dref.de_step(n_genes, m, None, set_ptr, members, pt, pc, 0.25, 0.5)
    d = np.load(os.path.join(HERE, "golden", "de.npz"))
    _compare_steps(got, want, *tolerances(d), "scale")
    st = want["status"]
    assert (st[5] == dref.SKIP_GENE).all() and (want["nonzero_test"][6] == want["n1"][6]).all()
    assert (st[6] == dref.ASYMPTOTIC).sum() == k - 1 and (st[6] == dref.SKIP_PAIR).sum() == (k - 1) ** 2     # cluster 3 against the others
    assert (st == dref.ASYMPTOTIC).sum() > 5000 and (st == dref.SKIP_PAIR).sum() > 100 and (st == dref.SKIP_GENE).sum() > 100000
    # one chunk gives the same answers
    again = _de._device_de(n_genes, m, None, set_ptr, members, pt, pc, 0.25, 0.5, mem_budget=8 << 30)
    assert _de.last_device_ms()[1] == 1
    for key in got:
        assert np.array_equal(got[key].view(np.int64) if got[key].dtype == np.float64 else got[key],
                              again[key].view(np.int64) if again[key].dtype == np.float64 else again[key]), key


@pytest.mark.gpu
def test_plain_c_consumer_gets_the_quirk_answers(gpu_lib, golden, tmp_path):
    exe = build_de_check(tmp_path)
    d = golden("de")
    case = [c for c in dref.golden_cases(d) if c["name"] == "quirk_groups"][0]
    genes, m1, _, test_idx, groups = dref.case_inputs(d, case)
    sets = [test_idx] + groups
    sp = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    mem = np.array([c for s in sets for c in s], dtype=np.int64)
    n_cells, ptr, cell, val, sf = m1
    text = "%d %d %d %r %r\n" % (len(genes), n_cells, len(sets), case["exp_frac_thresh"], case["log2_fc_thresh"])
    text += " ".join(str(int(x)) for x in ptr) + "\n" + "\n".join("%d %r" % (int(c), float(v)) for c, v in zip(cell, val)) + "\n"
    text += " ".join(repr(float(x)) for x in sf) + "\n" + " ".join(str(int(x)) for x in sp) + "\n" + " ".join(str(int(x)) for x in mem) + "\n"
    r = subprocess.run([exe, "run"], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout
    n = len(groups)
    want = dref.de_step(len(genes), m1, None, sp, mem, np.zeros(n, np.int32), np.arange(1, n + 1, dtype=np.int32),
                        case["exp_frac_thresh"], case["log2_fc_thresh"])
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("pair ")]
    assert len(rows) == len(genes) * n
    got = {k: np.array([t(x[2 + i]) for x in rows]).reshape(len(genes), n).astype(dt)
           for i, ((k, dt), t) in enumerate(zip(dref.FIELDS[:6] + (dref.FIELDS[6], dref.FIELDS[7], dref.FIELDS[8], dref.FIELDS[9]),
                                                (int,) * 6 + (float,) * 4))}
    _compare_steps(got, want, *tolerances(d), "plain C")
    assert (got["status"] == dref.EMPTY).any() and (got["status"] == dref.EXACT).any()

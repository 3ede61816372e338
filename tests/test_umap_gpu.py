"""UMAP on the MI355X (nabo_umap_*, nabo_amd._umap) against the tests' float64 restatement of include/nabo_umap.h
(tests/_umap_ref.py).  umap-learn's own results and random stream are not pinned; the header is the specification.

  graph       from given lists: rho bit-equal, ptr and nbr equal, sigma bit-equal, |w_gpu - w_ref| <= W_TOL = 16 * 2^-53
              (tests/_umap_ref.py derives it from the two exp).  Rows whose sigma search came within 1e-12 of a threshold,
              and arcs within 2 W_TOL of the prune threshold, could be excused up to 1 % -- the cases hold none
              (tests/test_umap_cpu.py asserts it), so nothing is excused here: equality is demanded everywhere.
  one epoch   ONE EPOCH AT A TIME from the restatement's positions (the optimisation is chaotic: comparing after many
              free-running epochs would test nothing).  The counts of attractive terms and negative samples and the
              64-bit sum of the sampled indices must be EQUAL -- they are the integer decisions -- and the positions
              within tests/_umap_ref.position_bound: every term within TERM_ULPS = 32 ulp of the restatement's (two pow
              of at most 2 + 4 ulp each, five roundings on each side), at most 4 alpha per clipped term through the
              actual |term|, the node's sum reassociated at most once per addition, and the move's two roundings.
  determinism two runs give identical bits; run(120) then run(80) equals run(200).
  whole run   by a property: the share of a cell's 10 nearest embedded neighbours among its 30 nearest in the input,
              against what the restatement reached for the same seeds (tests/golden/umap.npz).
  end to end  umap_fit equals Umap fed with knn(X, X, k) of the public API, bit for bit; make_umap on a PCA file.
"""
import numpy as np
import pytest

from nabo_amd import _umap

import _umap_ref as ur

pytestmark = pytest.mark.gpu

GROUP = _umap.geometry()
CASES = dict(ur.graph_cases(), **ur.width_cases())          # (width_cases: every width of the graph kernels, full and one over)
AB = (1.5769436135065888, 0.8950607193577038)      # spread 1, min_dist 0.1; any positive pair would do here


@pytest.mark.parametrize("n_epochs", (ur.N_EPOCHS_PRUNING, ur.N_EPOCHS_KEEPING))
@pytest.mark.parametrize("name", list(CASES))
def test_graph_from_given_lists(gpu_lib, name, n_epochs):
    idx, dist = CASES[name]
    ref = ur.fuzzy_graph(idx, dist, n_epochs)
    assert not ref["flagged"].any() and not ref["near"].any(), "the case sits on a threshold: choose another"
    rho, sigma, ptr, nbr, w = gpu_lib.umap_fuzzy_graph(idx, dist, n_epochs)
    assert rho.tobytes() == ref["rho"].tobytes()
    assert sigma.tobytes() == ref["sigma"].tobytes(), np.nonzero(sigma != ref["sigma"])[0][:10]
    assert np.array_equal(ptr, ref["ptr"]) and np.array_equal(nbr, ref["nbr"])
    err = float(np.max(np.abs(w - ref["w"])))
    print("%s, n_epochs %d: %d arcs of %d, longest row %d, max |w - w_ref| = %.3g (bound %.3g)"
          % (name, n_epochs, len(w), ref["n_unpruned"], int(np.diff(ptr).max()), err, ur.W_TOL))
    assert err <= ur.W_TOL
    # symmetric bit for bit on the device too
    src = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    back = {(int(s), int(d)): x for s, d, x in zip(src, nbr, w)}
    assert all(back[(j, i)] == x for (i, j), x in back.items())
    if n_epochs == ur.N_EPOCHS_KEEPING:
        assert len(w) == ref["n_unpruned"]


# ---------------------------------------------------------------------------------------------------------------------
# one epoch at a time

N_EP = 50


def _start(kind, n, dims, g):
    y = np.random.default_rng(21).uniform(0.0, 10.0, size=(n, dims))
    if kind == "coincident":
        # neighbours on one spot (the attraction's d2 == 0) and a dozen nodes on another (so do some samples')
        for i in range(0, n, 7):
            if g["ptr"][i + 1] > g["ptr"][i]:
                y[i] = y[int(g["nbr"][g["ptr"][i]])]
        y[n // 2:n // 2 + 12] = y[n // 2]
    elif kind == "far":
        y = y * 1e3                                            # d2 up to 1e8 under both pow; every term is tiny
    elif kind == "crowded":
        y = y * 5e-3                                           # every pair closer than 0.1: the repulsion is clipped
    return y


def _check_epoch(U, ep, y, tag):
    """loads y, runs one epoch on the device and one in the restatement, compares; returns the restatement's result"""
    U.set_embedding(y)
    o = ep.step(y)
    assert U.run(1) == 1
    c, got = U.last_epoch_counts(), U.get_embedding()
    assert np.array_equal(c["n_attr"], o["n_attr"]) and np.array_equal(c["n_neg"], o["n_neg"]), tag
    assert np.array_equal(c["idx_sum"], o["idx_sum"]), tag
    bound = ur.position_bound(o, y)
    err = np.abs(got - o["y"])
    assert np.isfinite(got).all() and (err <= bound).all(), (tag, float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))
    o["err_over_bound"] = float((err / np.maximum(bound, 1e-300)).max())
    D = y[ep.src[o["fired"]]] - y[ep.nbr[o["fired"]]]
    o["zero_d2"] = int(((D * D).sum(axis=1) == 0).sum())   # attractions between coincident nodes
    return o


# The clip.  c * D of the attraction tends to -2 b / d for distant nodes and that of the repulsion to 0, so a start spread
# FAR apart clips nothing (measured: 0 of 315 829 terms); the clip acts where nodes are CLOSE, on the repulsion, which
# with 5 samples per firing is five terms in six.  Both starts are run: "far" for the large arguments of pow, "crowded"
# for a start in which the clip acts on most terms.
EPOCH_CASES = [("knn_333x15", 2, 5, "plain"), ("knn_333x15", 3, 1, "plain"), ("hub_600x4", 2, 5, "plain"), ("hub_600x4", 3, 5, "far"),
               ("knn_333x15", 2, 1, "coincident"), ("knn_333x15", 3, 5, "far"), ("knn_120x56", 3, 5, "coincident"),
               ("hub_600x4", 2, 5, "crowded"), ("knn_333x15", 3, 5, "crowded"),
               ("knn_250x32", 2, 5, "plain"), ("knn_250x32", 3, 5, "crowded")]      # rows of 32 arcs and more: two full rounds of the group


@pytest.mark.parametrize("name,dims,nsr,start", EPOCH_CASES)
def test_one_epoch_at_a_time(gpu_lib, name, dims, nsr, start):
    idx, dist = CASES[name]
    g = ur.fuzzy_graph(idx, dist, N_EP)
    n = len(g["ptr"]) - 1
    seed = 3
    ep = ur.Epochs(g["ptr"], g["nbr"], g["w"], g["wmax"], N_EP, nsr, 1.0, AB[0], AB[1], seed, GROUP)
    y0 = _start(start, n, dims, g)
    worst, self_hits, clipped, terms, zero_d2 = 0.0, 0, 0, 0, 0
    with _umap.Umap(n, dims, n_epochs=N_EP, negative_sample_rate=nsr, a=AB[0], b=AB[1], seed=seed) as U:
        U.set_graph(g["ptr"], g["nbr"], g["w"])
        for t in (0, N_EP // 2, N_EP - 1):                     # the first, a middle and the last epoch
            U.rewind()
            assert U.run(t) == t                               # the schedule does not depend on the positions
            ep.rewind()
            ep.advance(t)
            o = _check_epoch(U, ep, y0, (name, t))
            if t == 0:
                assert o["n_attr"].sum() == 0 and np.array_equal(U.get_embedding(), y0)   # next_e = eps_e >= 1: nothing fires
            else:
                assert o["n_attr"].sum() > 0 and o["n_neg"].sum() > 0
            zero_d2 += o["zero_d2"]
            worst, self_hits, clipped, terms = max(worst, o["err_over_bound"]), self_hits + o["self_hits"], clipped + o["clipped"], terms + o["terms"]
        clipped_at_start, terms_at_start = clipped, terms      # these three epochs ran from y0 itself
        assert U.run(5) == 0                                   # never past n_epochs
        # 20 epochs with the restatement stepping alongside; its positions are reloaded before each step
        U.rewind()
        ep.rewind()
        U.run(10)
        ep.advance(10)
        y = y0
        for t in range(10, 30):
            o = _check_epoch(U, ep, y, (name, t))
            y = o["y"]
            zero_d2 += o["zero_d2"]
            worst, self_hits, clipped, terms = max(worst, o["err_over_bound"]), self_hits + o["self_hits"], clipped + o["clipped"], terms + o["terms"]
    print("%s, %d dims, %d samples per firing, %s start: %d terms, %d clipped, %d samples on their own node, %d attractions at "
          "d2 == 0; largest error / bound %.3g" % (name, dims, nsr, start, terms, clipped, self_hits, zero_d2, worst))
    if start == "crowded":
        # (one epoch later the nodes have flown apart, so the 20 steps that follow clip little)
        assert clipped_at_start > terms_at_start // 2, "the crowded start was meant to clip most terms"
    if start == "coincident":
        assert zero_d2 > 0
    if name == "knn_120x56" or (name == "knn_333x15" and nsr == 5):
        assert self_hits > 0, "some sample was meant to name its own node"


# ---------------------------------------------------------------------------------------------------------------------
# determinism

@pytest.fixture(scope="module")
def cells_1000():
    from nabo_amd._synth import pca_like
    return pca_like(1000, 20, seed=5)


def test_two_runs_are_bit_identical(gpu_lib, cells_1000):
    a = gpu_lib.umap_fit(cells_1000, 15, n_epochs=200, seed=1)
    b = gpu_lib.umap_fit(cells_1000, 15, n_epochs=200, seed=1)
    assert a.tobytes() == b.tobytes() and np.isfinite(a).all() and a.shape == (1000, 2)
    c = gpu_lib.umap_fit(cells_1000, 15, n_epochs=200, seed=2)
    assert c.tobytes() != a.tobytes()                          # the seed reaches the samples
    y0 = _umap.start_positions("pca", cells_1000, 1000, 2, 1)
    with _umap.Umap(1000, 2, n_epochs=200, seed=1) as U:
        U.fit_knn(cells_1000, 15)
        U.set_embedding(y0)
        assert U.run(120) == 120 and U.run(80) == 80 and U.run(1) == 0
        split = U.get_embedding()
        ms = U.last_ms()
    assert split.tobytes() == a.tobytes()
    assert ms["n_timed"] == 0 and ms["graph"] > 0 and ms["knn"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# the whole run, by a property

@pytest.mark.parametrize("dims", (2, 3))
@pytest.mark.parametrize("start", ("pca", "random"))
def test_whole_run_keeps_neighbourhoods(gpu_lib, golden, start, dims):
    gold = golden("umap")
    X, grp = gold["blobs_X"], gold["blobs_group"]
    si, di = gold["starts"].tolist().index(start), gold["dims"].tolist().index(dims)
    want = gold["share"][si, di]
    assert gold["same_group"][si, di].all() and int(gold["group"]) == GROUP, "tests/golden/umap.npz: run tools/gen_golden_umap.py"
    floor = float(want.min() - (want.max() - want.min()))
    got = []
    for seed in gold["seeds"].tolist():
        Y = gpu_lib.umap_fit(X, int(gold["whole_k"]), dims, n_epochs=int(gold["whole_epochs"]), seed=seed, init=start)
        s, ie = ur.neighbour_share(Y, X)
        got.append(s)
        assert (grp[ie] == grp[:, None]).all(), "a cell's 10 nearest embedded neighbours left its group (seed %d)" % seed
    print("%s start, %d dims: device %.4f .. %.4f, restatement %.4f .. %.4f, floor %.4f" % (start, dims, min(got), max(got), want.min(), want.max(), floor))
    assert min(got) >= floor


# ---------------------------------------------------------------------------------------------------------------------
# end to end

def test_resident_lists_equal_the_public_knn(gpu_lib, cells_1000):
    """umap_fit (the lists stay on the device) and Umap fed with knn(X, X, k) through the host are one computation"""
    X = cells_1000[:700]
    a, b = gpu_lib.find_ab_params(1.0, 0.1)
    idx, dist = gpu_lib.knn(X, X, 12)
    for dims in (2, 3):
        want = gpu_lib.umap_fit(X, 12, dims, n_epochs=60, seed=7)
        with gpu_lib.Umap(700, dims, n_epochs=60, a=a, b=b, seed=7) as U:
            U.set_knn(idx, dist)
            host_graph = U.graph()
            U.set_embedding(_umap.start_positions("pca", X, 700, dims, 7))
            assert U.run() == 60
            got = U.get_embedding()
        assert got.tobytes() == want.tobytes()
    with gpu_lib.Umap(700, 2, n_epochs=60, a=a, b=b, seed=7) as U:
        resident_graph = U.fit_knn(X, 12).graph()
    for p, q in zip(host_graph, resident_graph):
        assert p.tobytes() == q.tobytes()
    ref = ur.fuzzy_graph(idx, dist, 60)                        # and the graph is the restatement's
    assert np.array_equal(host_graph[2], ref["ptr"]) and np.array_equal(host_graph[3], ref["nbr"])
    assert np.max(np.abs(host_graph[4] - ref["w"])) <= ur.W_TOL


@pytest.mark.parametrize("layout", ["cells", "dense"])
def test_make_umap_on_a_pca_file(gpu_lib, tmp_path, cells_1000, layout):
    h5py = pytest.importorskip("h5py")
    pytest.importorskip("pandas")
    import os
    from nabo_amd._mapping import _write_rows
    Z = cells_1000[:200]
    cells = ["c%03d-1" % i for i in np.random.default_rng(3).permutation(200)]
    fn = os.path.join(str(tmp_path), "pca_%s.h5" % layout)
    if layout == "dense":
        gpu_lib.write_dense_pca(fn, "data", cells, Z)
    else:
        with h5py.File(fn, "w") as h5:
            _write_rows(h5.create_group("data"), cells, Z)
    df = gpu_lib.make_umap(fn, 10, 2, 10, 1.0, 1.0, 0.1, 50, index_suffix="_WT", verbose=False, seed=2)
    order = np.argsort(cells)                                  # the file's name order
    assert list(df.index) == [cells[i] + "_WT" for i in order] and list(df.columns) == ["Dim1", "Dim2"]
    want = gpu_lib.umap_fit(Z[order][:, :10], 10, 2, n_epochs=50, seed=2)
    assert df.values.tobytes() == want.tobytes()

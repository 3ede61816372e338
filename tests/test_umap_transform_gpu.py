"""The UMAP transform on the MI355X (nabo_umap_transform_*, nabo_amd._umap) against the tests' float64 restatement of
include/nabo_umap_transform.h (tests/_umap_transform_ref.py).  umap-learn's own results and random stream are not pinned;
the header is the specification.

  graph       from given lists: sigma bit-equal, |a_gpu - a_ref| <= MEMB_TOL = 3 * 2^-53 (the two exp), the start within
              tests/_umap_transform_ref.start_bound (derived there from its k products and sums).  No row of the cases
              sits on a threshold of the sigma search (tests/test_umap_transform_cpu.py asserts it), so nothing is
              excused: equality is demanded everywhere.
  one epoch   ONE EPOCH AT A TIME from set_graph and the restatement's positions.  The counts of attractive terms and
              negative samples and the 64-bit sum of the sampled indices must be EQUAL -- they are the integer decisions
              -- and the positions within tests/_umap_ref.position_bound, as for the fit.
  bits        run(n) equals n times run(1); run(40) then run(60) equals run(100); two calls are equal; any split into
              batches, down to one row at a time, gives the bits of the whole; umap_transform equals the handle fed with
              knn(Z, X_ref, k) of the public API.
  whole run   by a property: the share of a target's 10 nearest embedded reference cells among its 30 nearest reference
              cells in the input, against what the restatement reached for the same seeds
              (tests/golden/umap_transform.npz), and every target's 10 nearest in its own group.
  end to end  make_target_umap on two PCA files.
"""
import os

import numpy as np
import pytest

from nabo_amd import _umap

import _umap_ref as ur
import _umap_transform_ref as tr

pytestmark = pytest.mark.gpu

GROUP = _umap.transform_geometry()
CASES = tr.list_cases()
AB = (1.5769436135065888, 0.8950607193577038)      # spread 1, min_dist 0.1; any positive pair would do here


@pytest.fixture(scope="module")
def graphs():
    """the restatement's graph of every list case, computed once and left unchanged"""
    return {name: tr.graph(c["idx"], c["dist"], c["Y"]) for name, c in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_graph_from_given_lists(gpu_lib, graphs, name):
    c, ref = CASES[name], graphs[name]
    assert not ref["flagged"].any(), "the case sits on a threshold: choose another"
    n_ref, dims = c["Y"].shape
    with gpu_lib.UmapTransform(n_ref, dims, n_epochs=100, a=AB[0], b=AB[1]) as T:
        T.set_embedding(c["Y"])
        sigma, memb, y0 = T.set_knn(c["idx"], c["dist"], first_row=5).graph()
        y = T.get_positions()
        ms = T.last_ms()
    assert sigma.tobytes() == ref["sigma"].tobytes(), np.nonzero(sigma != ref["sigma"])[0][:10]
    err = float(np.max(np.abs(memb - ref["memb"])))
    bound = tr.start_bound(c["idx"], ref["memb"], c["Y"])
    serr = np.abs(y0 - ref["y0"])
    print("%s: max |a - a_ref| = %.3g (bound %.3g), start error / bound %.3g" % (name, err, tr.MEMB_TOL, float((serr / bound).max())))
    assert err <= tr.MEMB_TOL
    assert np.isfinite(y0).all() and (serr <= bound).all()
    assert y.tobytes() == y0.tobytes() and ms["graph"] > 0 and ms["knn"] == 0
    if name == "zeros_k5_m17":
        assert (memb[2] == 1).all() and memb[5, 0] == 1 and memb[5, 1] == 1
    if name == "k15_m333":
        assert memb[3, 0] == 1
    if name == "k48_m17":
        assert memb[4, 0] == 1


# ---------------------------------------------------------------------------------------------------------------------
# one epoch at a time

N_EP = {"k56_m17": 20}                                         # 1 / 20 lies above that case's smallest membership (0.041): dead arcs
FIRST_ROW = 1000


def _check_epoch(T, ep, y, tag):
    """loads y, runs one epoch on the device and one in the restatement, compares; returns the restatement's result"""
    T.set_positions(y)
    o = ep.step(y)
    assert T.run(1) == 1
    c, got = T.last_run_counts(), T.get_positions()
    assert np.array_equal(c["n_attr"], o["n_attr"]) and np.array_equal(c["n_neg"], o["n_neg"]), tag
    assert np.array_equal(c["idx_sum"], o["idx_sum"]), tag
    bound = ur.position_bound(o, y)
    err = np.abs(got - o["y"])
    assert np.isfinite(got).all() and (err <= bound).all(), (tag, float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))
    o["err_over_bound"] = float((err / np.maximum(bound, 1e-300)).max())
    return o


# The clip acts where cells are CLOSE, on the repulsion; a start spread FAR apart clips nothing but feeds pow large
# arguments.  k56_m17 puts four arcs on a lane, k17_m17 two, k2_m17 leaves most lanes without one; k33_m17 and
# k48_m17 put three (the third round one lane wide, and full); k16_m17 and k32_m17 fill one round and two.
EPOCH_CASES = [("k15_m333", 2, 5, "plain"), ("k15_m333", 3, 1, "plain"), ("k56_m17", 3, 5, "neighbour"), ("k17_m17", 2, 1, "neighbour"),
               ("k15_m333", 3, 5, "far"), ("k2_m17", 2, 5, "far"), ("k15_m333", 2, 5, "crowded"), ("k56_m17", 2, 1, "crowded"),
               ("k33_m17", 2, 5, "plain"), ("k33_m17", 3, 1, "crowded"), ("k48_m17", 3, 5, "neighbour"), ("k16_m17", 2, 5, "far"),
               ("k32_m17", 3, 5, "plain")]


@pytest.mark.parametrize("name,dims,nsr,start", EPOCH_CASES)
def test_one_epoch_at_a_time(gpu_lib, graphs, name, dims, nsr, start):
    c = CASES[name]
    idx, memb = c["idx"], graphs[name]["memb"]
    n_ref = len(c["Y"])
    scale = {"far": 1e3, "crowded": 5e-3}.get(start, 1.0)
    Y = np.random.default_rng(31).uniform(0.0, 10.0, size=(n_ref, dims)) * scale
    y0 = tr.start(idx, memb, Y)
    if start == "neighbour":
        y0[::3] = Y[idx[::3, 0]]                               # on top of the nearest neighbour: the attraction's d2 == 0
    seed, n_ep = 3, N_EP.get(name, 50)
    ep = tr.Epochs(idx, memb, Y, FIRST_ROW, n_ep, nsr, 1.0, AB[0], AB[1], seed, GROUP)
    worst, clipped, terms, zero_d2 = 0.0, 0, 0, 0
    with gpu_lib.UmapTransform(n_ref, dims, n_epochs=n_ep, negative_sample_rate=nsr, a=AB[0], b=AB[1], seed=seed) as T:
        T.set_embedding(Y)
        T.set_graph(idx, memb, first_row=FIRST_ROW)
        assert np.max(np.abs(T.graph()[2] - tr.start(idx, memb, Y))) <= tr.start_bound(idx, memb, Y).max()
        for t in (0, n_ep // 2, n_ep - 1):                     # the first, a middle and the last epoch
            T.rewind()
            assert T.run(t) == t                               # the schedule does not depend on the positions
            ep.rewind()
            ep.advance(t)
            o = _check_epoch(T, ep, y0, (name, t))
            if t == 0:
                assert o["n_attr"].sum() == 0 and np.array_equal(T.get_positions(), y0)   # next = eps >= 1: nothing fires
            else:
                assert o["n_attr"].sum() > 0 and o["n_neg"].sum() > 0
            worst, clipped, terms, zero_d2 = max(worst, o["err_over_bound"]), clipped + o["clipped"], terms + o["terms"], zero_d2 + o["zero_d2"]
        clipped_at_start, terms_at_start = clipped, terms      # these three epochs ran from y0 itself
        assert T.run(5) == 0                                   # never past n_epochs
        # 10 epochs with the restatement stepping alongside; its positions are reloaded before each step
        T.rewind()
        ep.rewind()
        T.run(10)
        ep.advance(10)
        y = y0
        for t in range(10, 20):
            o = _check_epoch(T, ep, y, (name, t))
            y = o["y"]
            worst, clipped, terms, zero_d2 = max(worst, o["err_over_bound"]), clipped + o["clipped"], terms + o["terms"], zero_d2 + o["zero_d2"]
    print("%s, %d dims, %d samples per firing, %s start: %d terms, %d clipped, %d at d2 == 0; largest error / bound %.3g"
          % (name, dims, nsr, start, terms, clipped, zero_d2, worst))
    if start == "crowded" and nsr == 5:
        assert clipped_at_start > terms_at_start // 2, "the crowded start was meant to clip most terms"
    if start == "neighbour":
        assert zero_d2 > 0
    if name == "k56_m17":
        assert not ep.live.all(), "some arc was meant to lie below 1 / n_epochs"
    if name in ("k33_m17", "k48_m17"):                         # umap_transform_run_launch: three arcs to a lane
        assert -(-idx.shape[1] // GROUP) == 3


# ---------------------------------------------------------------------------------------------------------------------
# bits

def _handle(gpu_lib, c, n_epochs, seed=1, nsr=5):
    T = gpu_lib.UmapTransform(len(c["Y"]), c["Y"].shape[1], n_epochs=n_epochs, negative_sample_rate=nsr, a=AB[0], b=AB[1], seed=seed)
    return T.set_embedding(c["Y"])


@pytest.mark.parametrize("name", ["k15_m333", "k56_m17"])
def test_runs_split_and_repeat_to_the_same_bits(gpu_lib, name):
    c = CASES[name]
    with _handle(gpu_lib, c, 100) as T:
        T.set_knn(c["idx"], c["dist"])
        y0 = T.get_positions()
        assert T.run() == 100 and T.run(1) == 0
        whole, counts = T.get_positions(), T.last_run_counts()
        assert np.isfinite(whole).all() and (np.abs(whole - y0).max(axis=1) > 0).all()
        assert counts["n_attr"].min() > 0 and (counts["n_neg"] >= counts["n_attr"]).all()
        T.rewind().set_positions(y0)                           # run(40) then run(60)
        assert T.run(40) == 40
        first = T.last_run_counts()
        assert T.run(60) == 60
        second = T.last_run_counts()
        assert T.get_positions().tobytes() == whole.tobytes()
        for key in ("n_attr", "n_neg", "idx_sum"):             # the counts are those of one run
            assert np.array_equal(first[key] + second[key], counts[key])
        T.rewind().set_positions(y0)                           # run(12) against 12 times run(1)
        T.run(12)
        twelve = T.get_positions()
        T.rewind().set_positions(y0)
        for _ in range(12):
            assert T.run(1) == 1
        assert T.get_positions().tobytes() == twelve.tobytes() and twelve.tobytes() != whole.tobytes()
        T.set_knn(c["idx"], c["dist"])                         # the same call again, from the lists
        T.run()
        assert T.get_positions().tobytes() == whole.tobytes()
        T.set_params(seed=2)                                   # the seed reaches the samples
        T.set_positions(y0).run()
        assert T.get_positions().tobytes() != whole.tobytes()


@pytest.mark.parametrize("name,rows", [("k15_m333", 60), ("k56_m17", 17), ("k48_m17", 17)])
def test_batches_give_the_bits_of_the_whole(gpu_lib, name, rows):
    c = CASES[name]
    idx, dist = c["idx"], c["dist"]
    m = len(idx)
    with _handle(gpu_lib, c, 40) as T:
        T.set_knn(idx, dist, first_row=7)
        T.run()
        whole = T.get_positions()
        cut = m // 3
        parts = []
        for r0, r1 in ((0, cut), (cut, m)):                    # two batches with their first_row
            T.set_knn(idx[r0:r1], dist[r0:r1], first_row=7 + r0)
            T.run()
            parts.append(T.get_positions())
        assert np.concatenate(parts).tobytes() == whole.tobytes()
        for r in range(rows):                                  # every row alone
            T.set_knn(idx[r:r + 1], dist[r:r + 1], first_row=7 + r)
            assert T.run() == 40
            assert T.get_positions().tobytes() == whole[r:r + 1].tobytes(), r
        if m > 1:
            T.set_knn(idx[1:2], dist[1:2], first_row=7)        # another global row number: other samples
            T.run()
            assert T.get_positions().tobytes() != whole[1:2].tobytes()


def test_one_call_form_batches_and_public_knn(gpu_lib):
    """umap_transform in batches of 64 equals the unbatched call, and both equal the handle fed with knn(Z, X_ref, k) of
    the public API through the host"""
    c = CASES["k15_m333"]
    Z, X, Y = c["Z"], c["X"], c["Y"]
    a, b = gpu_lib.find_ab_params(1.0, 0.1)
    want = gpu_lib.umap_transform(Z, X, Y, 12, n_epochs=30, seed=7)
    assert want.shape == (333, 2) and np.isfinite(want).all()
    assert gpu_lib.umap_transform(Z, X, Y, 12, n_epochs=30, seed=7, batch=64).tobytes() == want.tobytes()
    idx, dist = gpu_lib.knn(Z, X, 12)
    with gpu_lib.UmapTransform(600, 2, n_epochs=30, a=a, b=b, seed=7) as T:
        T.set_embedding(Y).set_knn(idx, dist)
        host_graph = T.graph()
        assert T.run() == 30
        assert T.get_positions().tobytes() == want.tobytes()
        T.set_cells(X).query(Z, 12)
        ms = T.last_ms()
        for p, q in zip(host_graph, T.graph()):
            assert p.tobytes() == q.tobytes()
        assert ms["knn"] > 0 and ms["graph"] > 0
    ref_idx, _ = tr.knn_lists(Z, X, 12)
    assert np.array_equal(idx, ref_idx)
    # n_epochs=None: umap's 100 for up to 10000 targets
    assert gpu_lib.umap_transform(Z[:5], X, Y, 12, seed=7).tobytes() == gpu_lib.umap_transform(Z[:5], X, Y, 12, n_epochs=100, seed=7).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the whole run, by a property

@pytest.mark.parametrize("dims", (2, 3))
def test_whole_run_keeps_neighbourhoods(gpu_lib, golden, dims):
    gold = golden("umap_transform")
    X, grp = ur.blobs()
    ref, tgt = gold["ref_rows"], gold["target_rows"]
    Xr, Z, Y = np.ascontiguousarray(X[ref]), np.ascontiguousarray(X[tgt]), gold["ref_Y%d" % dims]
    di = gold["dims"].tolist().index(dims)
    want = gold["share"][di]
    assert gold["same_group"][di].all() and int(gold["group"]) == GROUP, "tests/golden/umap_transform.npz: run tools/gen_golden_umap_transform.py"
    floor = float(want.min() - (want.max() - want.min()))
    a, b = gold["ab"]
    got = []
    with gpu_lib.UmapTransform(len(ref), dims, n_epochs=int(gold["whole_epochs"]), a=a, b=b) as T:
        T.set_embedding(Y).set_cells(Xr)
        for seed in gold["seeds"].tolist():
            T.set_params(seed=seed)
            y0 = T.query(Z, int(gold["whole_k"])).graph()[2]
            assert T.run() == int(gold["whole_epochs"])
            P = T.get_positions()
            assert np.isfinite(P).all()
            assert (np.abs(P - y0).max(axis=1) > 0).all(), "a target did not move off its start (seed %d)" % seed
            s, ie = tr.target_share(P, Y, Z, Xr)
            got.append(s)
            assert (grp[ref][ie] == grp[tgt][:, None]).all(), "a target's 10 nearest embedded reference cells left its group (seed %d)" % seed
    print("%d dims: device %.4f .. %.4f, restatement %.4f .. %.4f, floor %.4f" % (dims, min(got), max(got), want.min(), want.max(), floor))
    assert min(got) >= floor


# ---------------------------------------------------------------------------------------------------------------------
# end to end

@pytest.mark.parametrize("layout", ["cells", "dense"])
def test_make_target_umap_on_two_pca_files(gpu_lib, tmp_path, layout):
    h5py = pytest.importorskip("h5py")
    pytest.importorskip("pandas")
    from nabo_amd._mapping import _write_rows
    from nabo_amd._synth import pca_like
    cells = pca_like(260, 12, seed=5)
    Xr, Z = cells[:200], cells[200:]
    rng = np.random.default_rng(3)
    ref_cells = ["r%03d-1" % i for i in rng.permutation(200)]
    tgt_cells = ["t%03d-1" % i for i in rng.permutation(60)]
    ref_fn, tgt_fn = os.path.join(str(tmp_path), "ref_%s.h5" % layout), os.path.join(str(tmp_path), "tgt_%s.h5" % layout)
    for fn, names, M in ((ref_fn, ref_cells, Xr), (tgt_fn, tgt_cells, Z)):
        if layout == "dense":
            gpu_lib.write_dense_pca(fn, "data", names, M)
        else:
            with h5py.File(fn, "w") as h5:
                _write_rows(h5.create_group("data"), names, M)
    ref_umap = gpu_lib.make_umap(ref_fn, 10, 2, 10, 1.0, 1.0, 0.1, 50, index_suffix="_WT", verbose=False, seed=2)
    df = gpu_lib.make_target_umap(ref_fn, tgt_fn, ref_umap, 10, 10, n_epochs=30, index_suffix="_KO", verbose=False, seed=2, batch=25)
    ro, to = np.argsort(ref_cells), np.argsort(tgt_cells)      # the files' name order
    assert list(df.index) == [tgt_cells[i] + "_KO" for i in to] and list(df.columns) == ["Dim1", "Dim2"]
    want = gpu_lib.umap_transform(Z[to][:, :10], Xr[ro][:, :10], ref_umap.values, 10, n_epochs=30, seed=2)
    assert df.values.tobytes() == want.tobytes() and np.isfinite(want).all()
    with pytest.raises(ValueError):
        gpu_lib.make_target_umap(ref_fn, tgt_fn, ref_umap.iloc[:-1], 10, 10, verbose=False)


def test_make_target_umap_frame_without_files(gpu_lib, monkeypatch):
    """the same with the files' reader stubbed (it is make_umap's, and needs h5py): the device step runs for real"""
    pd = pytest.importorskip("pandas")
    from nabo_amd._synth import pca_like
    cells = pca_like(260, 12, seed=5)
    Xr, Z = cells[:200], cells[200:]
    ref_cells, tgt_cells = ["r%03d-1" % i for i in range(200)], ["t%03d-1" % i for i in range(60)]
    monkeypatch.setattr(_umap, "_read_cells", lambda fn, grp, use_comps: (ref_cells, Xr[:, :use_comps]) if fn == "ref" else (tgt_cells, Z[:, :use_comps]))
    Y = gpu_lib.umap_fit(Xr[:, :10], 10, 3, n_epochs=50, seed=2)
    ref_umap = pd.DataFrame(Y, index=[c + "_WT" for c in ref_cells], columns=["Dim1", "Dim2", "Dim3"])
    df = gpu_lib.make_target_umap("ref", "tgt", ref_umap, 10, 10, n_epochs=30, index_suffix="_KO", verbose=False, seed=2, batch=25)
    assert list(df.index) == [c + "_KO" for c in tgt_cells] and list(df.columns) == ["Dim1", "Dim2", "Dim3"]
    want = gpu_lib.umap_transform(Z[:, :10], Xr[:, :10], Y, 10, n_epochs=30, seed=2)
    assert df.values.tobytes() == want.tobytes() and np.isfinite(want).all() and df.shape == (60, 3)

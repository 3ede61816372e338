"""Edge bundling (include/nabo_bundle.h, nabo_amd/_bundle.py) without a GPU: the header and its symbols, the yardstick
(tests/_bundle_ref.py) checked by hand, the host-side entry points through ctypes, the wrapper's validation, the edge rule
of `bundle_edges`, and the condition on the GPU tests' inputs that no integer decision sits within 1e-9 of its threshold."""
import os
import re

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _bundle, _lib

import _bundle_case as bc
import _bundle_ref as br

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-9


def test_public_names_and_symbols():
    for n in ("Bundle", "hammer_bundle", "bundle_edges"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))
    assert callable(nabo_amd.RefGraph.bundle_edges)
    src = open(os.path.join(REPO, "include", "nabo_bundle.h")).read()
    assert '#include "nabo_knn.h"' in src
    assert "nabo_bundle" not in open(os.path.join(REPO, "include", "nabo_knn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src))) == sorted(_lib.BUNDLE_SYMBOLS)
    assert not set(_lib.BUNDLE_SYMBOLS) & set(_lib.SYMBOLS + _lib.LAYOUT_SYMBOLS + _lib.UMAP_SYMBOLS + _lib.POTENTIAL_SYMBOLS)
    L = _lib.lib()
    for n in _lib.BUNDLE_SYMBOLS:
        assert hasattr(L, n), n


def test_header_is_plain_c(tmp_path):
    import subprocess
    src = tmp_path / "bundle_check.c"
    src.write_text('#include "nabo_bundle.h"\nint main(void) { nabo_bundle *b = 0; int32_t r = 0; (void)b; '
                   'return nabo_bundle_blur_weights(3.0, &r, 0, 0) != 0 || r != 6; }\n')
    exe = str(tmp_path / "bundle_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-L" + os.path.join(REPO, "nabo_amd"),
           "-lnabo_knn", "-Wl,-rpath," + os.path.join(REPO, "nabo_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    _lib.lib()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    assert subprocess.run([exe]).returncode == 0


def test_geometry_matches_the_source():
    g = _bundle.geometry()
    assert g["p_max"] == br.P_MAX == 256 and g["long_group"] == 64 and g["short_group"] in (4, 8, 16, 32)
    assert 2 < g["short_cap"] < g["p_max"]
    hip = open(os.path.join(REPO, "nabo_amd", "csrc", "bundle.hip")).read()
    assert "BND_SHORT_G = %d, BND_SHORT_CAP = %d" % (g["short_group"], g["short_cap"]) in hip


@pytest.mark.parametrize("b", [0.5, 2.0, 3.0, 24.0, 35.0])
def test_blur_weights(b):
    w = _bundle.blur_weights(b)
    sigma = b / 2
    R = int(np.ceil(4 * sigma))
    assert w.shape == (2 * R + 1,) and np.array_equal(w, w[::-1]) and abs(w.sum() - 1) < 1e-14
    t = np.arange(-R, R + 1)
    want = np.exp(-0.5 * (t / sigma) ** 2)
    assert np.allclose(w, want / want.sum(), rtol=1e-13, atol=0)
    with pytest.raises(ValueError):
        _bundle.blur_weights(0.1)
    with pytest.raises(ValueError):
        _bundle.blur_weights(float("nan"))


def test_a_known_polyline_resampled():
    # an L of length 0.03 + 0.03: tl = 0.012 gives m = ceil(5) + 1 = 6 points every 0.012, the corner not among them
    P = np.array([[0.1, 0.1], [0.13, 0.1], [0.13, 0.13]])
    Q = br.resample_one(P, 0.012)
    assert Q.shape == (6, 2) and np.array_equal(Q[0], P[0]) and np.array_equal(Q[-1], P[-1])
    want = np.array([[0.1, 0.1], [0.112, 0.1], [0.124, 0.1], [0.13, 0.106], [0.13, 0.118], [0.13, 0.13]])
    assert np.abs(Q - want).max() < 1e-15
    # zero length, shorter than tl, and the clamp at P_MAX
    assert np.array_equal(br.resample_one(np.array([[0.3, 0.3], [0.3, 0.3], [0.3, 0.3]]), 0.012), [[0.3, 0.3], [0.3, 0.3]])
    assert br.resample_one(np.array([[0.3, 0.3], [0.305, 0.3]]), 0.012).shape == (2, 2)
    off, pts = bc.special_polylines()
    noff, npts = br.resample(off, pts, bc.TL)
    assert list(np.diff(noff)) == [2, 2, 3, 256, 15, 2]
    zig = npts[noff[3]:noff[4]]
    assert np.array_equal(zig[0], pts[off[3]]) and np.array_equal(zig[-1], pts[off[4] - 1])
    assert (zig[:, 0] >= 0.3).all() and (zig[:, 0] <= 0.3 + 5.0 / 299 + 1e-15).all() and (zig[:, 1] == 0.5).all()
    # interior zero-length segments: evenly spaced along the two legs 0.05 + 0.11
    rep = npts[noff[4]:noff[5]]
    seg = np.sqrt(((rep[1:] - rep[:-1]) ** 2).sum(axis=1))
    assert np.allclose(seg.sum(), 0.16, atol=0.006) and (seg > 0).all()


def test_a_delta_blurs_to_the_outer_product_of_the_weights():
    A, b = 40, 6.0
    img = np.zeros((A + 1, A + 1), dtype=np.uint32)
    img[20, 17] = 1
    w = br.blur_weights(b)
    R = (len(w) - 1) // 2
    B, _, _ = br.field(img, b)
    want = np.zeros_like(B)
    want[20 - R:20 + R + 1, 17 - R:17 + R + 1] = np.outer(w, w)
    assert np.array_equal(B, want)
    # a radius beyond the image: what falls outside is dropped
    B2, _, _ = br.field(img, 24.0)
    w2 = br.blur_weights(24.0)
    R2 = (len(w2) - 1) // 2
    assert R2 > A and np.array_equal(B2, np.outer(w2[R2 - 20:R2 - 20 + A + 1], w2[R2 - 17:R2 - 17 + A + 1]))


def test_a_mirror_symmetric_image_gives_a_mirror_symmetric_field():
    A = 32
    rng = np.random.default_rng(5)
    half = rng.integers(0, 9, size=(A + 1, A + 1)).astype(np.uint32)
    img = half + half[::-1, :]
    B, GX, GY = br.field(img, 5.0)
    # the mirror image's blur sums run in the opposite order, so the symmetry holds to rounding: a sum of at most 21
    # non-negative terms is within 21 * 2^-53 of exact, relative; the field divides differences of D (<= 1, errors of a
    # few 1e-16) by mag >= 1e-5
    assert np.allclose(B, B[::-1, :], rtol=1e-14, atol=0)
    assert np.abs(GX + GX[::-1, :]).max() < 1e-9 and np.abs(GY - GY[::-1, :]).max() < 1e-9
    assert (np.sqrt(GX ** 2 + GY ** 2) < 1).all()
    # transposing the image swaps the roles of the two axes (and the order of the two blurs: again to rounding)
    Bt, GXt, GYt = br.field(np.ascontiguousarray(img.T), 5.0)
    assert np.abs(Bt - B.T).max() <= 1e-14 * B.max() and np.abs(GXt - GY.T).max() < 1e-9 and np.abs(GYt - GX.T).max() < 1e-9
    # the field points up the density
    img = np.zeros((A + 1, A + 1), dtype=np.uint32)
    img[16, 16] = 7
    _, GX, GY = br.field(img, 5.0)
    assert GX[12, 16] > 0.99 and GX[20, 16] < -0.99 and GY[16, 12] > 0.99 and GY[16, 20] < -0.99 and GX[16, 16] == 0


def test_density_and_steps_by_hand():
    A = 7
    pts = np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.99], [0.5, 0.99]])
    img = br.density(pts, A)
    assert img.dtype == np.uint32 and img.sum() == 4 and img[0, 0] == 1 and img[7, 7] == 1 and img[3, 6] == 2
    off = np.array([0, 3, 5])
    pts = np.array([[0.1, 0.1], [0.2, 0.3], [0.3, 0.1], [0.5, 0.5], [0.6, 0.6]])
    out = br.smooth(off, pts, 0.3, 1)
    assert np.array_equal(out[[0, 2, 3, 4]], pts[[0, 2, 3, 4]])
    assert np.allclose(out[1], 0.7 * pts[1] + 0.3 * 0.5 * (pts[0] + pts[2]), rtol=1e-15)
    GX, GY = np.full((A + 1, A + 1), -1.0), np.full((A + 1, A + 1), 1.0)
    moved = br.advect_step(off, np.array([[0.1, 0.1], [0.05, 0.95], [0.3, 0.1], [0.5, 0.5], [0.6, 0.6]]), GX, GY, A)
    assert np.array_equal(moved[1], [0.0, 1.0]) and np.array_equal(moved[[0, 2, 3, 4]], [[0.1, 0.1], [0.3, 0.1], [0.5, 0.5], [0.6, 0.6]])
    p, o = br.with_nan_rows(off, pts), off
    assert p.shape == (7, 2) and np.isnan(p[[3, 6]]).all() and np.array_equal(p[[0, 1, 2, 4, 5]], pts) and o[-1] == 5


def test_no_decision_of_the_step_cases_sits_on_a_threshold():
    """a condition on the GPU tests' inputs, checked on the yardstick alone: a miss means another seed, never an excuse"""
    m = {}
    for E in bc.RESAMPLE_E:
        br.resample(*bc.polylines(E), bc.TL, m)
    br.resample(*bc.special_polylines(), bc.TL, m)
    for A in (7, 64, 500):
        for kind in ("one_pixel", "ones", "random"):
            br.density(bc.density_points(kind, A)[1], A, m)
    for A, b in ((7, 24.0), (64, 4.0), (500, 35.0)):
        br.density(bc.polylines(64)[1], A, m)
    off, pts = bc.advect_state(64)
    _, GX, GY = br.field(br.density(pts, 64, m), 4.0)
    one = br.advect_step(off, pts, GX, GY, 64, m)
    inner = br.interior(off, len(pts))
    assert (one[inner] == 0.0).any() and (one[inner] == 1.0).any(), "the advection case must clamp at 0 and at 1"
    for n_steps, every in ((1, 2), (2, 1), (2, 2)):
        br.advect(off, pts, GX, GY, 64, n_steps, every, bc.TL, m)
    assert m["m"] > EPS and m["pixel"] > EPS and m["j"] > EPS, m


def test_no_decision_of_the_whole_run_sits_on_a_threshold(golden):
    g = golden("bundle")
    assert int(g["seed"]) == bc.SEED and tuple(g["accuracies"]) == bc.RUN_A and int(g["n_perturbed"]) == 8
    for A in bc.RUN_A:
        assert (g["margins_%d" % A] > EPS).all()
        assert (g["figure_margin_%d" % A] > 0).all() and (g["figure_margin_%d" % A] < g["figures_%d" % A]).all()
    # it bundles: the long edges' midpoints come together and the edges get longer
    assert g["figures_500"][0] < 0.7 * g["straight_figures"][0] and 1.05 < g["figures_500"][1] < 2


def test_the_golden_run_is_the_yardsticks(golden):
    import hashlib
    g = golden("bundle")
    pos, src, dst = bc.graph()
    assert len(src) == 2300 and pos.shape == (400, 2)
    m = {}
    pts, off = br.run(pos, src, dst, m, accuracy=500)
    assert np.array_equal(off, g["offsets_500"]) and hashlib.sha256(pts.tobytes()).hexdigest() == str(g["sha256_500"])
    assert np.array_equal([m["m"], m["pixel"], m["j"]], g["margins_500"])
    assert np.diff(off).max() < br.P_MAX and np.isnan(pts[off[1:] + np.arange(2300)]).all()


def test_validation():
    pos = np.array([[0.0, 0.0], [1.0, 2.0], [3.0, 1.0]])
    for bad in (dict(accuracy=1), dict(accuracy=4097), dict(decay=0.0), dict(decay=1.5), dict(tension=-0.1), dict(tension=1.1),
                dict(min_segment_length=0.0), dict(min_segment_length=0.02, max_segment_length=0.01), dict(no_such=1),
                dict(initial_bandwidth=float("nan")), dict(resample_every=0), dict(iterations=-1), dict(accuracy="x")):
        with pytest.raises(ValueError):
            nabo_amd.hammer_bundle(pos, [0], [1], **bad)
    for args in ((np.array([[0.0, np.inf], [1.0, 1.0]]), [0], [1]), (pos, [0], [3]), (pos, [-1], [1]), (pos, [], []),
                 (pos, [0, 1], [1]), (pos[:, :1], [0], [1])):
        with pytest.raises(ValueError):
            nabo_amd.hammer_bundle(*args)
    assert _bundle._check_params({})["accuracy"] == 500 and _bundle._check_params({"batch_size": 7})["batch_size"] == 7
    # valid arguments reach the library, which has no device here or runs
    try:
        pts, off = nabo_amd.hammer_bundle(pos, [0, 1], [1, 2])
        assert off[0] == 0 and pts.shape == (off[-1] + 2, 2)
    except nabo_amd.NaboError as e:
        assert nabo_amd.device_count() == 0 and "no HIP device" in str(e)


def test_the_edge_rule_of_bundle_edges():
    # rows in file order b, a, c (node ids 1, 0, 2); pair (a, b) listed twice, its LAST weight counts; c has no position
    pos = {"a": 0, "b": 1, "c": 2, "d": 3}
    rows, ptr = ["b", "a", "d"], np.array([0, 2, 4, 5])
    nbr, w = np.array([0, 3, 1, 2, 0]), np.array([0.9, 0.5, 0.1, 0.7, 0.3])
    layout = {"a": (0.0, 0.0), "b": (1.0, 0.0), "d": [2.0, 2.0], "c": None}
    ids, xy, src, dst = _bundle._ref_edges(rows, pos, ptr, nbr, w, layout, 0.2)
    assert list(ids) == [0, 1, 3] and np.array_equal(xy, [[0, 0], [1, 0], [2, 2]])
    # (b, a) first at arc 0 with last weight 0.1: dropped; (b, d) 0.5 kept; (a, c) no position; (d, a) 0.3 kept
    assert list(zip(ids[src], ids[dst])) == [(1, 3), (3, 0)]
    ids, xy, src, dst = _bundle._ref_edges(rows, pos, ptr, nbr, w, layout, 0)
    assert list(zip(ids[src], ids[dst])) == [(1, 0), (1, 3), (3, 0)]


def test_layout_files_read_back(tmp_path):
    layout = {"n1_WT": (0.25, 1.5), "n,2": (3.0, 0.1)}
    nabo_amd.save_layout_as_json(layout, str(tmp_path / "l.json"))
    nabo_amd.save_layout_as_csv(layout, str(tmp_path / "l.csv"))
    assert {k: tuple(v) for k, v in _bundle._read_layout(str(tmp_path / "l.json")).items()} == layout
    assert _bundle._read_layout(str(tmp_path / "l.csv")) == layout and _bundle._read_layout(layout) is layout

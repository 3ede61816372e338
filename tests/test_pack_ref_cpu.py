"""tests/_pack_ref.py (the numpy restatement tests/test_pack_gpu.py compares the packer with) against a case worked out by
hand: g = 3, two cells, centre (1, 0, -1), scale 4.

  cell 0: V = (1.5, 0.25, -1)            -> scaled (2, 1, 0); every value an f16, lo = 0; ||rep||^2 = 5
  cell 1: V = (1.25 + 2^-14, 0.75, 15)   -> scaled (1 + 2^-12, 3, 64); hi = (1, 3, 64), lo = (2^-12, 0, 0);
          ||rep||^2 = 4106 + 2^-11 + 2^-24, as fp32 4106 + 2^-11
  reference norm slots (x 2^-15):  cell 0: 5 2^-15 is an f16, nl = 0;  cell 1: 4106 = 2^12 (1 + 2.5 / 1024) lies just above
          the tie, nh = 4108 2^-15, nl = f16((-2 + 2^-11) 2^-15) = -2^-14 (tie to even)
  error slots: ey = f16(sqrt(ss) 1.002 (1 + 2^-9)), tx = f16(sqrt(ss) 2^-9 1.01 (1 + 2^-9)):
          cell 0: sqrt 5 = 2.2360680: ey = 2.2449162 -> 1149.40 2^-9 -> 1149 2^-9;  tx = 0.00441961 -> 1158.57 2^-18 -> 1159 2^-18
          cell 1: sqrt = 64.0781: ey = 64.33164 -> 1029.31 2^-4 -> 1029 2^-4;  tx = 0.1266509 -> 1037.52 2^-13 -> 1038 2^-13
"""
import numpy as np

import _pack_ref as pr

V = np.array([[1.5, 0.25, -1.0], [1.25 + 2.0 ** -14, 0.75, 15.0]])
CENTRE = np.array([1.0, 0.0, -1.0])
SCALE = 4.0
NH = (5 * 2.0 ** -15, 4108 * 2.0 ** -15)
NL = (0.0, -2.0 ** -14)
EY = (1149 * 2.0 ** -9, 1029 * 2.0 ** -4)
TX = (1159 * 2.0 ** -18, 1038 * 2.0 ** -13)
INF = float("inf")


def _f16(tile):
    return tile.view(np.float16).astype(np.float64)


def test_reference_one_product_layout16():
    out, norm64, nmax = pr.pack_reference(V, CENTRE, SCALE, 2, 1, True, True, 1)
    t = _f16(out)[0]                                    # [register][lane][8]
    assert norm64 is None
    assert nmax == int(np.float32(4106 + 2.0 ** -11).view(np.uint32))
    assert t.shape == (2, 64, 8)
    assert t[0, 0].tolist() == [2.0, 1.0, 0.0, NH[0], NL[0], EY[0], 0.0, 0.0]
    assert t[0, 1].tolist() == [1.0, 3.0, 64.0, NH[1], NL[1], EY[1], 0.0, 0.0]
    # padding cells: +inf norm in slot 3 (lanes 2..15 of register 0, lanes 0..15 of register 1), nothing else
    exp = np.zeros((2, 64, 8))
    exp[0, 2:16, 3] = INF
    exp[1, 0:16, 3] = INF
    exp[0, 0], exp[0, 1] = t[0, 0], t[0, 1]
    assert np.array_equal(t, exp)


def test_reference_masked_cell_leaves_the_filter():
    out, _, nmax = pr.pack_reference(V, CENTRE, SCALE, 2, 1, True, True, 1, mask=np.array([0, 1], dtype=np.uint8))
    t = _f16(out)[0]
    assert nmax == int(np.float32(5.0).view(np.uint32))
    assert t[0, 1].tolist() == [1.0, 3.0, 64.0, INF, 0.0, 0.0, 0.0, 0.0]


def test_target_one_product_layout16():
    out, norm64, nmax = pr.pack_reference(V, CENTRE, SCALE, 2, 1, False, True, 1)
    t = _f16(out)[0]
    assert nmax is None
    assert norm64.tolist() == [5.0 / 16.0, (4106 + 2.0 ** -11 + 2.0 ** -24) / 16.0]
    assert t[0, 0].tolist() == [-4.0, -2.0, -0.0, 32768.0, 32768.0, -TX[0], 0.0, 0.0]
    assert np.signbit(t[0, 0, 2])                        # (-2 x +0)
    assert t[0, 1].tolist() == [-2.0, -6.0, -128.0, 32768.0, 32768.0, -TX[1], 0.0, 0.0]
    assert t[0, 2].tolist() == [0.0, 0.0, 0.0, 32768.0, 32768.0, 0.0, 0.0, 0.0]      # padding rows carry the norm slots


def test_f16x3_split_both_layouts():
    # 3 (g + 1) = 12 slots: [hi | nh | lo | nl | hi | 0] for references, [-2hi | 2^15 | -2hi | 2^15 | -2lo | 0] for targets
    out, _, _ = pr.pack_reference(V, CENTRE, SCALE, 2, 1, True, True, 3)
    t = _f16(out)[0]
    assert t[0, 1].tolist() == [1.0, 3.0, 64.0, NH[1], 2.0 ** -12, 0.0, 0.0, NL[1]]     # slots 0..7: lane 1
    assert t[0, 17].tolist() == [1.0, 3.0, 64.0, 0.0, 0.0, 0.0, 0.0, 0.0]               # slots 8..15: lane 16 + 1
    out, _, _ = pr.pack_reference(V, CENTRE, SCALE, 1, 1, False, False, 3)
    t = _f16(out)[0]                                    # 32x32x16 layout: lane l: cell l & 31, slots 8 (l >> 5) + j
    assert t[0, 1].tolist() == [-2.0, -6.0, -128.0, 32768.0, -2.0, -6.0, -128.0, 32768.0]
    assert t[0, 33].tolist() == [-(2.0 ** -11), -0.0, -0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert t[0, 2].tolist() == [0.0] * 8                # padding rows of the f16x3 operands carry nothing


def test_out_of_range_and_non_finite_cells():
    W = np.array([[1.0, np.nan, -1.0], [1.0 + 30001.0 / 4, 0.0, -1.0], [np.inf, 0.0, -1.0], [1.0 + 30000.0 / 4, 0.0, -1.0]])
    out, norm64, _ = pr.pack_reference(W, CENTRE, SCALE, 2, 1, False, True, 1)
    t = _f16(out)[0]
    for c in range(3):
        assert np.isnan(norm64[c])
        assert t[0, c].tolist() == [0.0, 0.0, 0.0, 32768.0, 32768.0, 0.0, 0.0, 0.0]
    assert norm64[3] == 30000.0 ** 2 / 16.0 and t[0, 3, 0] == -60000.0       # 30000 itself is inside the range
    out, _, nmax = pr.pack_reference(W, CENTRE, SCALE, 2, 1, True, True, 1)
    t = _f16(out)[0]
    for c in range(3):
        assert t[0, c].tolist() == [0.0, 0.0, 0.0, INF, 0.0, 0.0, 0.0, 0.0]
    assert nmax == int(np.float32(9.0e8).view(np.uint32))

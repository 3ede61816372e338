"""The planner's partition where the two-level main launch comes with a tail launch (nabo_amd/csrc/plan.hip), without a GPU.
The main launch runs its rows as POSITIONS of the bucket-ordered copy -- lseed_columns(rows, C) columns of 128, every one of
the C buckets padding its rows to whole columns -- so it takes as many rows as fit its workgroups as positions, a whole
number of rounds of resident workgroups, and the tail launch takes the rest.  Plans without the stream or without a tail
are the ones whole workgroups give."""
import pytest

from nabo_amd import _knn

COL_ROWS = 128                        # local_seeds.h: LSEED_COL_ROWS
RPW = 384                             # geometry B


def lseed_columns(rows, C):
    return -(-rows // COL_ROWS) + C + 1


@pytest.mark.parametrize("n, m, options, wg_main", [
    (1000000, 1000000, None, 2560),                        # the flagship shape: five rounds
    (1000000, 200000, None, 512),                          # a small remainder: 521 workgroups of rows
    (1000000, 1000000, {"local_anchors": 32}, 2560),       # another C
])
def test_the_main_launch_fits_whole_rounds_as_positions(n, m, options, wg_main):
    p = _knn.query_plan(n, 50, m, 15, options=options)
    C = p["local_seed_buckets"]
    assert p["two_level"] == 2 and C == (options or {}).get("local_anchors", 64) and p["rows_per_wg"] == RPW, p
    assert p["workgroups_main"] == wg_main and p["workgroups_main"] % p["resident_workgroups"] == 0, p
    rows_main, rows_tail = p["rows_main"], m - p["rows_main"]
    assert rows_main == (wg_main * RPW // COL_ROWS - (C + 1)) * COL_ROWS, p
    assert lseed_columns(rows_main, C) * COL_ROWS <= p["workgroups_main"] * RPW, p
    assert lseed_columns(rows_main + COL_ROWS, C) * COL_ROWS > p["workgroups_main"] * RPW, "no column to spare"
    assert 0 < rows_tail and p["workgroups_tail"] == -(-rows_tail // RPW), p
    assert rows_main + rows_tail == m and rows_main % 32 == 0
    assert p["splits"] == 1 and p["splits_tail"] > 1 and p["workgroups_tail"] * p["splits_tail"] <= p["resident_workgroups"], p
    assert (p["workgroups_main"] + p["workgroups_tail"]) * RPW == p["rows_padded"] >= rows_main + p["workgroups_tail"] * RPW >= m
    assert p["workgroups"] == p["workgroups_main"] + p["workgroups_tail"] * p["splits_tail"]


def test_the_flagship_numbers():
    p = _knn.query_plan(1000000, 50, 1000000, 15)
    assert (p["rows_main"], p["workgroups_main"], p["workgroups_tail"], p["splits_tail"]) == (974720, 2560, 66, 7), p
    p = _knn.query_plan(1000000, 50, 200000, 15)
    assert (p["rows_main"], p["workgroups_main"], p["workgroups_tail"]) == (188288, 512, 31), p


def test_without_the_stream_or_without_a_tail_whole_workgroups():
    # two_level = 0 at the flagship shape: 2605 workgroups of rows, 2560 + 45
    p = _knn.query_plan(1000000, 50, 1000000, 15, options={"two_level": 0})
    assert p["two_level"] == 0 and (p["workgroups_main"], p["workgroups_tail"], p["splits_tail"]) == (2560, 45, 8), p
    assert p["rows_main"] == 2560 * RPW and p["rows_padded"] == 2605 * RPW
    p = _knn.query_plan(200000, 50, 200000, 15, options={"two_level": 0})
    assert (p["workgroups_main"], p["workgroups_tail"], p["rows_main"]) == (512, 9, 512 * RPW), p
    # no tail: a whole number of rounds of rows (the ordered launch then runs its extra positions as it did), one round, few rows
    for n, m in ((1000000, 512 * RPW), (1000000, 100000), (100000, 100000), (5000, 700)):
        p = _knn.query_plan(n, 50, m, 15)
        if p["workgroups_tail"] == 0:
            assert p["rows_main"] == m and p["rows_padded"] == p["workgroups_main"] * p["rows_per_wg"], p
    p = _knn.query_plan(1000000, 50, 512 * RPW, 15)
    assert p["workgroups_tail"] == 0 and p["workgroups_main"] == 512 and p["two_level"] == 2, p
    # the tail option off: one launch
    p = _knn.query_plan(1000000, 50, 1000000, 15, options={"tail_split": 0})
    assert p["workgroups_tail"] == 0 and p["workgroups_main"] == 2605 and p["rows_main"] == 1000000, p

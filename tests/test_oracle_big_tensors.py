"""The host image of every case of tests/test_gpu_big_tensors.py (no GPU, no library): what makes a wrapped index visible.

For every window row, halo and fresh alike, the row at element e differs from the rows at e - 2^30, e - 2^31 and e - 2^32 where
those exist and from the row at e mod 2^32: a kernel that reads or writes through a 32-bit element or byte offset meets other data
than the check expects.  An odd prime row count of the tile gives that; a power of two fails here.  `marks` covers the first row, the
last row and each power-of-two line of each case's shape."""
import numpy as np
import pytest

import big_tensors as BT


HEAD = 4096          # floats of a row that are compared: rows whose heads differ differ


def _row(c, e):
    return BT.expect_host(c, e, min(c.width, c.total - e, HEAD))


@pytest.mark.parametrize("name", sorted(BT.CASES))
def test_a_wrapped_index_lands_on_other_data(name):
    c = BT.CASES[name]
    assert c.tile_rows % 2 == 1 and all(c.tile_rows % d for d in range(3, int(c.tile_rows ** 0.5) + 1, 2)), "the tile's row count is an odd prime"
    checked = 0
    for first, count in BT.marks(c.total, c.width):
        for r in range(first, first + count):
            e = r * c.width
            here = _row(c, e)
            others = [e - line for line in BT.LINES if e - line >= 0] + ([e % BT.TWO32] if e >= BT.TWO32 else [])
            for o in others:
                there = _row(c, o)
                n = min(here.size, there.size)
                assert not np.array_equal(here[:n], there[:n]), (name, r, e, o)
                checked += 1
    assert checked > 0 or c.total <= BT.TWO30                               # (a tensor below 2^30 elements has no line to wrap at)


@pytest.mark.parametrize("name", sorted(BT.CASES))
def test_marks_cover_the_ends_and_every_line(name):
    c = BT.CASES[name]
    win = BT.marks(c.total, c.width)
    nrows = BT.rows_of(c.total, c.width)
    assert win[0][0] == 0 and win[-1][0] + win[-1][1] == nrows
    assert all(a[0] + a[1] <= b[0] for a, b in zip(win, win[1:])), "disjoint and ascending"
    for line in BT.LINES:
        if line < c.total:
            r = line // c.width                                             # the row that holds element `line`
            assert any(f < r < f + n for f, n in win), (name, line)          # ... and the row before it, in one window
            k = [i for i, (f, n) in enumerate(win) if f <= r < f + n][0]
            lo, cnt = BT.fresh_rows(c.total, c.width, k)
            assert lo <= r - 1 and r < lo + cnt, "fresh rows on both sides of the line"
    # the windows' fresh data differs from the tile it replaces and between windows
    tile = BT.tile_host(c)
    seen = []
    for k in range(len(win)):
        lo, data = BT.window_host(c, k)
        under = tile[(lo + np.arange(data.size, dtype=np.int64)) % tile.size]
        assert not np.array_equal(data, under)
        assert all(not np.array_equal(data[:min(data.size, s.size)], s[:min(data.size, s.size)]) for s in seen)
        seen.append(data)
    mult, fresh = BT.multiplicity(c)
    assert int(mult.sum()) + sum(d.size for _, d in fresh) == c.total


def test_a_power_of_two_tile_is_caught():
    """the condition the seeds and the prime must satisfy is a real one: 4096 rows of 1024 repeat at every line"""
    c = BT.case("bad", BT.N31, 1024, 4096, 1)
    first, _ = BT.marks(c.total, c.width)[2]                                # the window on element 2^31; its first rows are halo
    e = first * c.width
    assert np.array_equal(_row(c, e), _row(c, e - BT.TWO30))

"""Device tensors past 2^31 elements for tests/test_gpu_big_tensors.py, without gigabytes on the host.

A tensor of `total` floats is read as rows of `width` (the last row may be ragged).  It holds one random TILE of `tile_rows` rows
repeated from element 0 on - `tile_rows` an odd prime, so the period tile_rows * width divides no power of two and the row at
element e never equals the row at e - 2^30, e - 2^31 or e - 2^32 - and, inside every WINDOW of `marks`, fresh random rows that differ
from the tile and from every other window.  The windows are what a test downloads and checks: the first rows, the rows that straddle
elements 2^30 (byte offset 2^32), 2^31 and, where the tensor reaches it, 2^32, and the last rows with the ragged tail.  The outer
HALO rows of a window keep the tile's data, the inner rows are fresh: an index that wraps reads or writes something the check sees in
either kind of row.  tests/test_oracle_big_tensors.py holds these conditions on the host image, case by case.

Nothing here downloads or uploads more than a window or a tile."""
import functools
from collections import namedtuple

import numpy as np

TWO30, TWO31, TWO32 = 1 << 30, 1 << 31, 1 << 32
LINES = (TWO30, TWO31, TWO32)
WINDOW_ROWS, HALO = 24, 4
GUARD_FLOATS, GUARD = 64, -12345.5

# total floats, row width, rows of the tile (an odd prime), seed, value range
Case = namedtuple("Case", "name total width tile_rows seed lo hi")


def case(name, total, width, tile_rows, seed, lo=-1.0, hi=1.0):
    return Case(name, int(total), int(width), int(tile_rows), int(seed), float(lo), float(hi))


def rows_of(total, width):
    return (total + width - 1) // width


def marks(total, width):
    """[(first_row, rows)]: disjoint, ascending windows of WINDOW_ROWS rows (fewer where the tensor ends)"""
    nrows = rows_of(total, width)
    want = [0] + [line // width - WINDOW_ROWS // 2 for line in LINES if line < total] + [nrows - WINDOW_ROWS]
    out = []
    for first in want:
        first = max(first, out[-1][0] + out[-1][1] if out else 0)
        last = min(first + WINDOW_ROWS, nrows)
        if last > first:
            out.append((first, last - first))
    return out


def fresh_rows(total, width, k):
    """the rows of window k that hold fresh data: the window without its HALO rows, except at the tensor's two ends"""
    win = marks(total, width)
    first, count = win[k]
    lo = first if first == 0 else first + HALO
    hi = first + count if k == len(win) - 1 else first + count - HALO
    return lo, hi - lo


def _draw(seed, n, lo, hi):
    a = np.random.default_rng(seed).random(n, dtype=np.float32)
    a *= np.float32(hi - lo)
    a += np.float32(lo)
    return a


def _dominant(c, seed, n):
    """rows of sampling_cases.make("dominant", ...): one to three tokens far above the rest (n is a whole number of rows)"""
    import sampling_cases
    return sampling_cases.make("dominant", n // c.width, c.width, seed).reshape(-1)


def _make(c, seed, n):
    """uniform draws in [lo, hi), except the sampling case's rows"""
    return _dominant(c, seed, n) if c.name.startswith("sampling/") else _draw(seed, n, c.lo, c.hi)


@functools.lru_cache(maxsize=8)
def tile_host(c):
    """the tile's floats (read only: the result is shared between callers)"""
    a = _make(c, c.seed, c.tile_rows * c.width)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=8)
def window_host(c, k):
    """the fresh floats of window k, clipped at the tensor's end: (first element, data); read only, shared between callers"""
    first, count = fresh_rows(c.total, c.width, k)
    lo, hi = first * c.width, min((first + count) * c.width, c.total)
    a = _make(c, c.seed * 1000 + 7 * k + 1, hi - lo)
    a.flags.writeable = False
    return lo, a


def expect_at(c, idx):
    """the host image at the elements `idx` (any shape, int64): tile data with the windows' fresh data laid over it"""
    idx = np.asarray(idx, dtype=np.int64)
    assert idx.size == 0 or (0 <= idx.min() and idx.max() < c.total), (idx.min(), idx.max(), c.total)
    tile = tile_host(c)
    out = tile[idx % tile.size]
    for k in range(len(marks(c.total, c.width))):
        lo, data = window_host(c, k)
        inside = (idx >= lo) & (idx < lo + data.size)
        out[inside] = data[idx[inside] - lo]
    return out


def expect_host(c, first, count):
    """the host image of elements [first, first + count)"""
    assert 0 <= first and first + count <= c.total, (first, count, c.total)
    return expect_at(c, first + np.arange(count, dtype=np.int64))


def window_elems(c, k):
    """(first element, count) of the whole window k, halo included, clipped at the tensor's end"""
    first, count = marks(c.total, c.width)[k]
    lo = first * c.width
    return lo, min((first + count) * c.width, c.total) - lo


def multiplicity(c):
    """How often every element of the tile occurs in the tensor outside the windows' fresh data (int64, tile.size) and the fresh data
    itself: [(first element, data)].  Sums over the whole tensor in f64 come from these, never from a host copy of the tensor."""
    period = c.tile_rows * c.width
    mult = np.full(period, c.total // period, np.int64)
    mult[:c.total % period] += 1
    fresh = []
    for k in range(len(marks(c.total, c.width))):
        lo, data = window_host(c, k)
        np.subtract.at(mult, (lo + np.arange(data.size, dtype=np.int64)) % period, 1)
        fresh.append((lo, data))
    assert mult.min() >= 0 and int(mult.sum()) + sum(d.size for _, d in fresh) == c.total
    return mult, fresh


# ---- the cases of tests/test_gpu_big_tensors.py (tests/test_oracle_big_tensors.py holds the conditions above on each) ------------
N31 = TWO31 + 4099                     # flat families: 2 097 156 rows of 1024 and a ragged row of 3
N32 = TWO32 + 5                        # fill, copy, one unary forward: the only cases past the unsigned line
ROWS21 = (1 << 21) + 3                 # row families: (2^21 + 3) x 1024 and x 1027
CASES = {}


def _add(name, *a, **k):
    CASES[name] = case(name, *a, **k)


_add("flat32/x", N32, 1024, 4099, 101, -2.0, 2.0)
for _i, _n in enumerate(("x", "g", "d", "t")):
    _add("flat31/" + _n, N31, 1024, 4099, 110 + _i, -2.0, 2.0)
for _i, _n in enumerate(("x", "t")):
    _add("reduce/" + _n, N31, 1024, 4099, 120 + _i, 0.5, 1.5)
for _i, _n in enumerate(("l", "r", "g", "d")):
    _add("binary/" + _n, TWO31 + 4096, 1024, 4099, 130 + _i, 0.5, 2.0)
for _w in (1024, 1027):
    for _i, _n in enumerate(("x", "g", "d", "y")):
        _add("rows%d/%s" % (_w, _n), ROWS21 * _w, _w, 4099, 140 + 10 * (_w - 1024) + _i, -2.0, 2.0)
for _i, _n in enumerate(("w", "g", "m", "v")):
    _add("adamw/" + _n, N31, 1024, 4099, 190 + _i, *((0.0, 0.1) if _n == "v" else (-1.0, 1.0)))
_add("pool/x", ((1 << 10) + 1) * 64 * 184 * 184, 184 * 184, 127, 220, -2.0, 2.0)
_add("pool/g", ((1 << 10) + 1) * 64 * 92 * 92, 92 * 92, 127, 221, -2.0, 2.0)
for _i, _n in enumerate(("x", "g", "d")):
    _add("bnmap/" + _n, 129 * 64 * (1 << 18), 1 << 18, 17, 230 + _i, -2.0, 2.0)
for _i, _n in enumerate(("x", "g")):
    _add("bncol/" + _n, ROWS21 * 1024, 1024, 4099, 236 + _i, 0.5, 1.5)
for _i, _n in enumerate(("x", "d")):
    _add("ce/" + _n, ((1 << 15) + 1) * (1 << 16), 1 << 16, 61, 240 + _i, -4.0, 4.0)
_add("emb/g", ROWS21 * 1024, 1024, 4099, 250, -2.0, 2.0)
_add("sampling/x", 2049 * (1 << 20), 1 << 20, 3, 260, -8.0, 8.0)
_add("transpose/x", ((1 << 16) + 1) * (1 << 15), 1 << 15, 127, 210, -2.0, 2.0)
for _i, _n in enumerate(("x", "g", "d")):
    _add("rope/" + _n, ((1 << 15) + 1) * 512 * 128, 512 * 128, 61, 200 + _i, -3.0, 3.0)


# ---- device side ------------------------------------------------------------------------------------------------------------------
def alloc(dev, n):
    """`n` floats (zeroed); an out-of-memory status from the allocation skips the test - the one skip this suite allows"""
    import pytest
    from neuronika_amd import capi
    try:
        return dev.zeros((int(n),))
    except capi.NeuronikaHipError as e:
        if "out of memory" in str(e).lower():
            pytest.skip("device allocation of %.1f GiB: %s" % (n * 4 / 2.0 ** 30, e))
        raise


def window(arr, first, count):
    """non-owning view of exactly `count` floats of `arr` from element `first`: upload / numpy on that slice only"""
    assert 0 <= first and first + count <= arr.size, (first, count, arr.size)
    v = arr.view_offset(int(first))
    v.shape, v.size = (int(count),), int(count)
    return v


def guarded(dev, total, value=None):
    """`total` floats followed by GUARD_FLOATS guard floats; the body filled with `value` where given"""
    a = alloc(dev, total + GUARD_FLOATS)
    if value is not None:
        window(a, 0, total).fill(value)
    window(a, total, GUARD_FLOATS).upload(np.full(GUARD_FLOATS, GUARD, np.float32))     # (nk_fill wants a 16-byte aligned pointer)
    return a


def guard_intact(arr, total):
    return bool((window(arr, total, GUARD_FLOATS).numpy() == np.float32(GUARD)).all())


def tiled(dev, c):
    """the device tensor of case `c` (total floats + guard floats): the tile uploaded once and doubled with nk_copy, then the windows"""
    from neuronika_amd import capi
    arr = guarded(dev, c.total)
    tile = tile_host(c)
    period = tile.size
    window(arr, 0, min(period, c.total)).upload(tile[:c.total])
    filled = min(period, c.total)
    while filled < c.total:                                                 # [0, filled) -> [filled, ...): the period is kept
        n = min(filled, c.total - filled)
        capi.check(capi.lib.nk_copy(dev.h, window(arr, filled, n).p, arr.p, n))
        filled += n
    for k in range(len(marks(c.total, c.width))):
        lo, data = window_host(c, k)
        window(arr, lo, data.size).upload(data)
    return arr

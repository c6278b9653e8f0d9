"""The oracle of token sampling (semantics: include/neuronika_hip.h, nk_sample_fwd), restated in f64 NumPy.

    order      by value, -0 as +0, NaN below -inf, equal values by the lower index; m = the largest value
    greedy     temperature == 0, or m not finite: the lowest index that holds m
    top-k      S = {x >= the k-th largest value}, ties stay; off for k <= 0 or k >= V
    weights    p_i = exp((x_i - m) / T) in f64 for i in S, 0 for NaN and -inf
    top-p      the kept set shrinks to {i in S : x_i >= t}, t the largest value whose value-closed set has mass >= top_p of S's
    draw       u = r64 / 2^64 (clamped below 1) from Philox4x32-10, counter (lo32(offset), hi32(offset), r, 0x53414D50), key
               (lo32(seed), hi32(seed)), r64 = word1 << 32 | word0; the id is the first kept index whose CDF in index order exceeds u

The device takes the same decisions on integers (weights truncated to multiples of 2^-40); `ambiguity` names the rows on which a
decision lies so close to a boundary that the two could differ.  tests/test_oracle_sampling.py pins this file."""
from collections import namedtuple

import numpy as np

from oracle import neuronika_oracle as O

Params = namedtuple("Params", "temperature top_k top_p", defaults=(1.0, 0, 1.0))
STREAM = 0x53414D50


def _uniforms(seed, offsets, rows):
    """u at the counters (offsets[i], rows[i]), f64 in [0, 1)"""
    seed = int(seed)
    offsets, rows = np.asarray(offsets, np.uint64), np.asarray(rows, np.uint64)
    ctr = np.empty((offsets.size, 4), np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = offsets & np.uint64(0xFFFFFFFF), offsets >> np.uint64(32), rows, STREAM
    w = O.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    r64 = (w[:, 1].astype(np.uint64) << np.uint64(32)) | w[:, 0].astype(np.uint64)
    return np.minimum(r64.astype(np.float64) / 2.0 ** 64, np.nextafter(1.0, 0.0))


def uniforms(seed, offset, rows, row0=0):
    """u of rows row0 .. row0 + rows - 1 of one call"""
    return _uniforms(seed, np.full(rows, int(offset), np.uint64), np.arange(row0, row0 + rows))


def _row(x, prm):
    """One row: (greedy index or None, kept mask, p (V,) f64 with zeros outside the kept set, levels) - `levels` is the list of
    cumulative masses at the distinct-value levels of S, as fractions of S's mass (empty without top-p)."""
    v = x.astype(np.float64)
    nan = np.isnan(v)
    if nan.all():
        return 0, None, None, []
    lo = np.where(nan, -np.inf, v)
    m = lo.max()
    if prm.temperature == 0 or not np.isfinite(m):
        return int(np.flatnonzero((lo == m) & ~nan)[0]), None, None, []
    V = v.size
    S = np.ones(V, bool)
    if 0 < prm.top_k < V and prm.top_k <= V - int(nan.sum()):    # a k-th largest that is NaN keeps everything
        kth = np.sort(lo[~nan])[::-1][prm.top_k - 1]
        S = (lo >= kth) & ~nan
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.where(S & ~nan & np.isfinite(lo), np.exp((lo - m) / np.float64(prm.temperature)), 0.0)
    levels = []
    kept = S
    if prm.top_p < 1:
        P = p.sum()
        vals = np.unique(lo[S & (p > 0)])[::-1]                   # distinct values, descending
        order = np.argsort(-lo, kind="stable")
        csum = np.cumsum(p[order])
        # mass of {x >= vals[l]}: the cumulative sum at the last sorted position holding a value >= vals[l]
        last = np.searchsorted(-lo[order], -vals, side="right") - 1
        levels = list(csum[last] / P)
        hit = np.flatnonzero(np.asarray(levels) >= np.float64(np.float32(prm.top_p)))
        t = vals[hit[0]] if hit.size else vals[-1]
        kept = S & (lo >= t)
        p = np.where(kept, p, 0.0)
    return None, kept, p, levels


def kept_set(x, prm):
    """the kept mask of one row (None for a greedy row)"""
    return _row(np.asarray(x, np.float32), Params(*prm))[1]


def sample(x, prm, seed=0, offset=0, row0=0):
    """x: (rows, V) f32 -> ids (rows,) int64; row i of x is drawn as row row0 + i of the call"""
    x = np.asarray(x, np.float32)
    prm = Params(*prm)
    u = uniforms(seed, offset, x.shape[0], row0)
    ids = np.empty(x.shape[0], np.int64)
    for r in range(x.shape[0]):
        g, _, p, _ = _row(x[r], prm)
        if g is not None:
            ids[r] = g
            continue
        cdf = np.cumsum(p) / p.sum()
        i = int(np.searchsorted(cdf, u[r], side="right"))
        ids[r] = i if i < p.size else int(np.flatnonzero(p > 0)[-1])    # cdf[-1] may round below u: the last kept token
    return ids


def draws(row, prm, seed, offsets, r=0):
    """one row drawn as row r of the calls at `offsets`: what `sample` returns for it, call by call"""
    g, _, p, _ = _row(np.asarray(row, np.float32), Params(*prm))
    if g is not None:
        return np.full(len(offsets), g, np.int64)
    cdf = np.cumsum(p) / p.sum()
    i = np.searchsorted(cdf, _uniforms(seed, offsets, np.full(len(offsets), r)), side="right")
    return np.where(i < p.size, i, np.flatnonzero(p > 0)[-1]).astype(np.int64)


def ambiguity(x, prm, seed, offset, eps, row0=0):
    """The rows of x where a decision lies within eps of a boundary: a cumulative mass at a distinct-value level within eps of top_p,
    or u within eps of an inner CDF boundary of the kept set."""
    x = np.asarray(x, np.float32)
    prm = Params(*prm)
    u = uniforms(seed, offset, x.shape[0], row0)
    bad = []
    for r in range(x.shape[0]):
        g, _, p, levels = _row(x[r], prm)
        if g is not None:
            continue
        if levels and np.min(np.abs(np.asarray(levels) - np.float64(np.float32(prm.top_p)))) <= eps:
            bad.append(r)
            continue
        pos = p[p > 0]
        inner = (np.cumsum(pos) / pos.sum())[:-1]                  # the last boundary is 1: no u reaches it
        if inner.size and np.min(np.abs(inner - u[r])) <= eps:
            bad.append(r)
    return bad

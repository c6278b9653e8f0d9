"""tests/segment_oracle.py pinned without a GPU: band edges give tests/window_oracle.py exactly; a block-diagonal layout gives, document
by document, the causal oracle run on that document alone (f64, 1e-12 relative, forward and the three gradients); and the addresses
the document walk touches in the banded scratch - r * ld + k for lo[r] <= k <= r, with ld and the extent from the library's geometry
functions at window = max_len - are distinct and inside the extent for a grid of random layouts."""
import numpy as np
import pytest

import causal_oracle as CO
import segment_oracle as SO
import window_oracle as WO
from oracle import neuronika_oracle as O

EDGE_LENGTHS = (1, 31, 32, 33, 127, 128, 129)


def rnd(seed, shape, dt=np.float64):
    return (np.random.default_rng(seed).random(shape) * 2 - 1).astype(dt)


def test_layout_of_documents():
    lo, pos, longest = SO.layout(12, [[3, 4], [12]])
    assert lo.dtype == np.int32 and pos.dtype == np.int32
    assert lo.tolist() == [[0, 0, 0, 3, 3, 3, 3, 7, 7, 7, 7, 7], [0] * 12]               # the remainder is one more document
    assert pos[0].tolist() == [0, 1, 2, 0, 1, 2, 3, 0, 1, 2, 3, 4] and pos[1].tolist() == list(range(12))
    assert longest == 12
    assert SO.layout(12, [[3, 4], [5, 5]])[2] == 5
    for bad in ([[0, 3]], [[13]], [[-1]]):
        with pytest.raises(AssertionError):
            SO.layout(12, bad)


def test_the_clamp():
    S = 9
    r = np.arange(S)
    assert np.array_equal(SO.lo_eff(np.full((1, S), -7), 4)[0], np.maximum(0, r - 3))       # below the band: the band
    assert np.array_equal(SO.lo_eff(np.full((1, S), 2 ** 30), 4)[0], r)                      # right of the diagonal: the diagonal
    assert np.array_equal(SO.lo_eff(np.full((1, S), np.iinfo(np.int32).min), 1)[0], r)
    assert np.array_equal(SO.lo_eff(np.zeros((1, S)), S + 5)[0], np.zeros(S))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("B,S,H,dh,W", [(2, 40, 2, 8, 7), (1, 33, 1, 4, 1), (1, 50, 2, 8, 50), (2, 37, 1, 8, 64)])
def test_band_edges_give_the_window_oracle_exactly(B, S, H, dh, W, dt):
    q, k, v, g = (rnd(s, (B * S, H * dh), dt) for s in (1, 2, 3, 4))
    noise = (np.random.default_rng(5).random((B * H, S, S)) > 0.2).astype(dt)
    want_o, want_c = WO.attention_core_forward(q, k, v, H, B, 0.2, noise, W)
    want = O.attention_core_backward(want_c, g)
    for lo in (SO.band_lo(B, S, W), np.full((B, S), -7, np.int32)):
        got_o, got_c = SO.attention_core_forward(q, k, v, H, B, 0.2, noise, lo, W)
        got = SO.attention_core_backward(got_c, g)
        assert np.array_equal(got_o, want_o)
        for name in ("probs", "dropped", "scores"):
            assert np.array_equal(got_c[name], want_c[name]), name
        for name in want:
            assert np.array_equal(got[name], want[name]), name


@pytest.mark.parametrize("B,S,H,dh,docs", [(2, 48, 2, 8, [[5, 1, 20, 22], [30, 10]]), (1, 70, 1, 16, [[33, 1, 1, 35]]), (1, 40, 3, 4, [[40]])])
def test_every_document_is_the_causal_oracle_on_that_document_alone(B, S, H, dh, docs):
    """f64, 1e-12 relative: out, dq, dk and dv of a document's rows against tests/causal_oracle.py's core run with batch = 1, S = len."""
    q, k, v, g = (rnd(s, (B * S, H * dh)) for s in (11, 12, 13, 14))
    noise = np.ones((B * H, S, S))
    lo, _, longest = SO.layout(S, docs)
    o, cache = SO.attention_core_forward(q, k, v, H, B, 0.0, noise, lo, longest)
    got = dict(SO.attention_core_backward(cache, g), out=o)
    for b in range(B):
        for start in np.unique(lo[b]):
            rows = np.flatnonzero(lo[b] == start) + b * S
            n = rows.size
            o1, c1 = CO.attention_core_forward(q[rows], k[rows], v[rows], H, 1, 0.0, np.ones((H, n, n)), causal=True)
            want = dict(O.attention_core_backward(c1, g[rows]), out=o1)
            for name in ("out", "dq", "dk", "dv"):
                np.testing.assert_allclose(got[name][rows], want[name], rtol=1e-12, atol=1e-12 * np.abs(want[name]).max(), err_msg=name)


def _random_layouts(n, seed):
    """(S, doc lengths of one sample): S <= 400, lengths drawn from the edge lengths and from 1 .. 200, with and without a remainder"""
    rng = np.random.default_rng(seed)
    for i in range(n):
        S = int(rng.integers(1, 401))
        lens, left = [], S
        while left > 0 and rng.random() > 0.08:
            n_ = int(rng.choice(EDGE_LENGTHS)) if rng.random() < 0.5 else int(rng.integers(1, 201))
            n_ = min(n_, left)
            lens.append(n_); left -= n_
        yield S, lens


def test_touched_addresses_are_distinct_and_inside_the_band_extent():
    """2400 random layouts: every address r * ld + k with lo[r] <= k <= r is unique and below nk_attention_band_scratch(S, max_len)."""
    from neuronika_amd import capi as c
    seen = set()
    count = 0
    fixed = [(400, [1, 31, 32, 33, 127, 128]), (400, [129, 128, 127]), (385, [128, 129, 128]), (256, [128, 128]), (33, [1] * 33), (400, [1] * 400)]
    for S, lens in fixed + list(_random_layouts(2400, 2024)):
        lo, _, span = SO.layout(S, [lens])
        seen.update(np.unique(lo[0], return_counts=True)[1].tolist())       # the document lengths walked
        ld, ext = c.attention_band_ld(S, span), c.attention_band_scratch(S, span)
        r = np.arange(S, dtype=np.int64)
        assert (r - lo[0] + 1 <= span).all()
        first, last = r * ld + lo[0], r * ld + r                             # a row's touched addresses are one run
        assert (first[1:] > last[:-1]).all(), (S, lens)                      # the runs of consecutive rows do not meet
        assert first.min() >= 0 and last.max() < ext, (S, lens)
        count += 1
    assert count >= 2000 and set(EDGE_LENGTHS) <= seen

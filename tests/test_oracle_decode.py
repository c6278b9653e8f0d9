"""The decoding oracle (tests/decode_oracle.py) pinned without a GPU: stepping token by token, and in slices, reproduces the rows of
the causal core's forward (tests/causal_oracle.py, p = 0) to 1e-12 in f64; ragged starts equal per-sample runs; rows past the
capacity are dropped; positions past a sample's length are never read."""
import numpy as np
import pytest

import causal_oracle as CO
import decode_oracle as DO


def rnd(seed, shape, lo, hi):
    a = np.random.default_rng(seed).random(shape, dtype=np.float32)
    return np.asarray(a * np.float32(hi - lo) + np.float32(lo), dtype=np.float32)


def _rows(t, B, S, lo, hi):
    """rows lo .. hi - 1 of every sample of a (B*S, d) tensor, sample-major"""
    return np.concatenate([t[b * S + lo:b * S + hi] for b in range(B)])


@pytest.mark.parametrize("B,S,H,dh", [(1, 1, 1, 4), (2, 12, 2, 8), (3, 17, 1, 5)])
@pytest.mark.parametrize("slices", ["tokens", "4", "prefill+tokens"])
def test_stepping_equals_the_causal_forward(B, S, H, dh, slices):
    q, k, v = (rnd(s, (B * S, H * dh), -1, 1).astype(np.float64) for s in (1, 2, 3))
    want, _ = CO.attention_core_forward(q, k, v, H, B, 0.0, np.ones((B * H, S, S)))
    kc, vc = DO.new_cache(B, H, S, dh, np.float64, fill=np.nan)          # the tail is never read: NaN there must not matter
    sizes = {"tokens": [1] * S, "4": [4] * (S // 4) + [S % 4] * (S % 4 > 0), "prefill+tokens": [S // 2] * (S >= 2) + [1] * (S - S // 2)}[slices]
    start, got = np.zeros(B, dtype=np.int64), np.zeros_like(want)
    for T in sizes:
        lo = int(start[0])
        ctx, after = DO.step(_rows(q, B, S, lo, lo + T), _rows(k, B, S, lo, lo + T), _rows(v, B, S, lo, lo + T), kc, vc, start, T)
        for b in range(B):
            got[b * S + lo:b * S + lo + T] = ctx[b * T:(b + 1) * T]
        start = after
    assert np.all(start == S) and np.all(np.isfinite(got))
    assert np.abs(got - want).max() <= 1e-12


def test_ragged_starts_equal_per_sample_runs():
    B, H, dh, cap, T = 3, 2, 6, 20, 2
    start = np.array([7, 0, 15])
    kc, vc = (rnd(s, (B, H, cap, dh), -1, 1).astype(np.float64) for s in (4, 5))
    q, k, v = (rnd(s, (B * T, H * dh), -1, 1).astype(np.float64) for s in (6, 7, 8))
    kb, vb = kc.copy(), vc.copy()
    got, after = DO.step(q, k, v, kb, vb, start, T)
    assert list(after) == [9, 2, 17]
    for b in range(B):
        k1, v1 = kc[b:b + 1].copy(), vc[b:b + 1].copy()
        one, _ = DO.step(q[b * T:(b + 1) * T], k[b * T:(b + 1) * T], v[b * T:(b + 1) * T], k1, v1, start[b:b + 1], T)
        assert np.array_equal(one, got[b * T:(b + 1) * T])
        assert np.array_equal(k1[0], kb[b]) and np.array_equal(v1[0], vb[b])


def test_append_drops_rows_past_the_capacity_and_touches_nothing_else():
    B, H, dh, cap, T = 2, 2, 3, 5, 3
    kc, vc = DO.new_cache(B, H, cap, dh, np.float32, fill=7.0)
    k, v = rnd(1, (B * T, H * dh), -1, 1), rnd(2, (B * T, H * dh), -1, 1)
    DO.append(kc, vc, k, v, [1, 4], T)
    assert np.array_equal(kc[0, 1, 1:4], k[0:3, dh:2 * dh]) and np.array_equal(vc[0, 0, 1:4], v[0:3, 0:dh])
    assert np.array_equal(kc[1, 0, 4], k[3, 0:dh])                       # position 4 written, 5 and 6 dropped
    assert np.all(kc[0, :, [0, 4]] == 7.0) and np.all(kc[1, :, :4] == 7.0) and np.all(vc[1, :, :4] == 7.0)


def test_the_dtype_is_the_callers():
    B, H, dh, cap = 1, 1, 4, 3
    kc, vc = (rnd(s, (B, H, cap, dh), -1, 1) for s in (1, 2))
    q = rnd(3, (1, dh), -1, 1)
    assert DO.decode_forward(q, kc, vc, [2], 1).dtype == np.float32
    assert DO.decode_forward(q.astype(np.float64), kc.astype(np.float64), vc.astype(np.float64), [2], 1).dtype == np.float64

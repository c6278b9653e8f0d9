"""The causal oracle (tests/causal_oracle.py: the oracle's attention composition with the mask added in front of the Softmax) against a plain
NumPy restatement written here, independently of the oracle's node functions: per (sample, head) and per query row r a loop
over the keys k <= r - softmax over exactly those keys, dropout by the given 0/1 noise, and the four gradients by the chain
rule spelled out per row.  f64, no GPU.  (Drop probabilities are binary fractions: the reference divides by an f32 `1 - p`,
which the oracle reproduces and which is exact for them.)"""
import numpy as np
import pytest

from oracle import neuronika_oracle as O
import causal_oracle as CO


def _rowwise_causal(q, k, v, g, heads, batch, p, noise):
    """(o, dq, dk, dv, d_scores) on the (B*S, H*dh) projection layout; noise (B*H, S, S) of 0 / 1."""
    bs, d = q.shape
    s, dh = bs // batch, d // heads
    scale = 1.0 / np.sqrt(dh)
    keepf = 1.0 if p == 0.0 else 1.0 / (1.0 - p)
    o, dq, dk, dv = (np.zeros_like(q) for _ in range(4))
    dsc = np.zeros((batch * heads, s, s))
    for b in range(batch):
        for h in range(heads):
            rows, cols = slice(b * s, (b + 1) * s), slice(h * dh, (h + 1) * dh)
            Q, K, V, G = q[rows, cols], k[rows, cols], v[rows, cols], g[rows, cols]
            n = noise[b * heads + h]
            for r in range(s):
                z = np.array([Q[r] @ K[c] for c in range(r + 1)]) * scale
                e = np.exp(z - z.max())
                pr = e / e.sum()
                nz = n[r, :r + 1] if p != 0.0 else np.ones(r + 1)
                pd = pr * nz * keepf
                o[b * s + r, cols] = pd @ V[:r + 1]
                dpd = V[:r + 1] @ G[r]                     # d out / d pd
                dv[b * s:b * s + r + 1, cols] += np.outer(pd, G[r])
                dpr = dpd * nz                             # DropoutBackward: the 0/1 mask only (node/dropout/mod.rs:113-128)
                dz = pr * (dpr - (dpr * pr).sum())
                ds = dz * scale
                dsc[b * heads + h, r, :r + 1] = ds
                dq[b * s + r, cols] += ds @ K[:r + 1]
                dk[b * s:b * s + r + 1, cols] += np.outer(ds, Q[r])
    return o, dq, dk, dv, dsc


@pytest.mark.parametrize("batch,s,heads,dh,p", [(2, 7, 3, 4, 0.0), (1, 1, 2, 8, 0.125), (2, 2, 1, 4, 0.5), (3, 33, 2, 8, 0.25)])
def test_causal_core_equals_the_rowwise_restatement(batch, s, heads, dh, p):
    rng = np.random.default_rng(100 * s + heads)
    q, k, v, g = (rng.standard_normal((batch * s, heads * dh)) for _ in range(4))
    noise = (rng.random((batch * heads, s, s)) >= p).astype(np.float64)
    o, cache = CO.attention_core_forward(q, k, v, heads, batch, p, noise)
    grads = CO.attention_core_backward(cache, g)
    ro, rdq, rdk, rdv, rds = _rowwise_causal(q, k, v, g, heads, batch, p, noise)
    tri = np.triu_indices(s, 1)
    assert np.all(cache["probs"][:, tri[0], tri[1]] == 0.0) and np.all(cache["dropped"][:, tri[0], tri[1]] == 0.0)
    assert np.all(grads["d_scores"][:, tri[0], tri[1]] == 0.0)
    np.testing.assert_allclose(cache["probs"].sum(axis=2), 1.0, rtol=0, atol=1e-14)
    for name, got, want in (("o", o, ro), ("dq", grads["dq"], rdq), ("dk", grads["dk"], rdk), ("dv", grads["dv"], rdv),
                            ("d_scores", grads["d_scores"], rds)):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13, err_msg=name)


def test_causal_off_is_the_oracle_itself():
    rng = np.random.default_rng(3)
    batch, s, heads, dh = 2, 5, 2, 4
    q, k, v = (rng.standard_normal((batch * s, heads * dh)) for _ in range(3))
    noise = np.ones((batch * heads, s, s))
    a, _ = O.attention_core_forward(q, k, v, heads, batch, 0.0, noise)
    b, _ = CO.attention_core_forward(q, k, v, heads, batch, 0.0, noise, causal=False)
    c, _ = CO.attention_core_forward(q, k, v, heads, batch, 0.0, noise)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    # the first query of every sample sees one key: its context is that key's value row
    np.testing.assert_allclose(c[::s], v[::s], rtol=1e-14)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_causal_mha_uses_the_causal_core(dtype):
    rng = np.random.default_rng(11)
    batch, s, heads, dh, p = 2, 6, 2, 4, 0.25
    d = heads * dh
    x, g = (rng.standard_normal((batch * s, d)).astype(dtype) for _ in range(2))
    ws = [rng.standard_normal((d, d)).astype(dtype) * dtype(0.3) for _ in range(4)]
    bs_ = [rng.standard_normal(d).astype(dtype) for _ in range(4)]
    noise = (rng.random((batch * heads, s, s)) >= p).astype(dtype)
    out, grads = CO.mha_forward_backward(x, ws[0], bs_[0], ws[1], bs_[1], ws[2], bs_[2], ws[3], bs_[3], heads, batch, p, noise, g)
    assert out.dtype == dtype and all(np.isfinite(t).all() for t in grads.values())
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    w64, b64 = [w.astype(np.float64) for w in ws], [b.astype(np.float64) for b in bs_]
    q, k, v = (x64 @ w64[i].T + b64[i] for i in range(3))
    do = g64 @ w64[3]
    ro, rdq, rdk, rdv, _ = _rowwise_causal(q, k, v, do, heads, batch, p, noise.astype(np.float64))
    tol = 1e-11 if dtype == np.float64 else 2e-4
    np.testing.assert_allclose(out, ro @ w64[3].T + b64[3], rtol=tol, atol=tol)
    np.testing.assert_allclose(grads["x"], rdq @ w64[0] + rdk @ w64[1] + rdv @ w64[2], rtol=tol, atol=tol)
    np.testing.assert_allclose(grads["wk"], rdk.T @ x64, rtol=tol, atol=tol)
    np.testing.assert_allclose(grads["bv"], rdv.sum(axis=0), rtol=tol, atol=tol)


def test_causal_mha_restates_the_oracles_module_at_one_key():
    """S = 1: causal and full attention are the same function, so the module body restated in tests/causal_oracle.py around the
    causal core must give the oracle's own `mha_forward_backward` bit for bit - output and every gradient."""
    rng = np.random.default_rng(21)
    batch, heads, dh, p = 5, 2, 4, 0.5
    d = heads * dh
    x, g = rng.standard_normal((batch, d)), rng.standard_normal((batch, d))
    ws = [rng.standard_normal((d, d)) for _ in range(4)]
    bs_ = [rng.standard_normal(d) for _ in range(4)]
    noise = (rng.random((batch * heads, 1, 1)) >= p).astype(np.float64)
    args = (x, ws[0], bs_[0], ws[1], bs_[1], ws[2], bs_[2], ws[3], bs_[3], heads, batch, p, noise, g)
    a, ga = O.mha_forward_backward(*args)
    b, gb = CO.mha_forward_backward(*args)
    assert np.array_equal(a, b) and sorted(ga) == sorted(gb)
    for key in ga:
        assert np.array_equal(ga[key], gb[key]), key

"""tests/embedding_oracle.py against torch on the CPU: forward against `F.embedding`, backward against f64 autograd (`padding_idx`
included) within a rounding bound, the saturating id read, and the chunked summation order against the plain order."""
import os
import subprocess
import sys

import numpy as np

import embedding_oracle as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed, n, V, D, skew=False):
    rng = np.random.default_rng(seed)
    if skew:
        p = 1.0 / np.arange(1, V + 1)
        ids = rng.choice(V, size=n, p=p / p.sum())
    else:
        ids = rng.integers(0, V, n)
    return (rng.standard_normal((V, D)).astype(np.float32), ids.astype(np.float32), rng.standard_normal((n, D)).astype(np.float32),
            rng.standard_normal((V, D)).astype(np.float32))


# torch runs in a child process: a process that has loaded the HIP library must not import torch as well (a second HIP runtime
# in one address space aborts at exit; the suite's other torch users are child processes for the same reason)
_TORCH_CHECK = r"""
import sys
import numpy as np
import torch
import torch.nn.functional as F
sys.path.insert(0, sys.argv[1])
import embedding_oracle as E
from test_oracle_embedding import _case
cases = 0
for n, V, D, skew in [(1, 1, 1, False), (50, 7, 3, False), (3000, 40, 16, True), (2000, 5000, 8, False), (5000, 3, 4, False)]:
    for pad in (-1, 0, 2):
        if pad >= V:
            continue
        w, idx, g, dw0 = _case(n + V, n, V, D, skew)
        ti = torch.from_numpy(idx.astype(np.int64))
        assert np.array_equal(E.forward(w, idx), F.embedding(ti, torch.from_numpy(w)).numpy())
        w64 = torch.from_numpy(w.astype(np.float64)).requires_grad_()
        F.embedding(ti, w64, padding_idx=pad if pad >= 0 else None).backward(torch.from_numpy(g.astype(np.float64)))
        want = w64.grad.numpy()
        got = E.backward_assign(g, idx, V, pad)
        counts = np.bincount(idx.astype(np.int64), minlength=V)[:, None]
        bound = np.maximum(counts, 1) * np.finfo(np.float32).eps * np.abs(g).max() * np.maximum(counts, 1)
        assert (np.abs(got - want) <= bound).all()
        if pad >= 0:
            assert not got[pad].any()
        acc = E.backward(dw0, g, idx, pad)
        assert (np.abs(acc - (dw0.astype(np.float64) + want)) <= bound + np.finfo(np.float32).eps * np.abs(dw0 + want)).all()
        untouched = counts[:, 0] == 0
        assert np.array_equal(acc[untouched], dw0[untouched])
        cases += 1
print("cases", cases)
"""


def test_against_torch():
    """forward equal to F.embedding; both backward forms against f64 autograd, with and without padding_idx, uniform and skewed ids"""
    r = subprocess.run([sys.executable, "-c", _TORCH_CHECK, os.path.join(ROOT, "tests")], capture_output=True, text=True)
    assert r.returncode == 0 and "cases 14" in r.stdout, r.stdout + r.stderr


def test_forward_keeps_the_index_shape():
    w, idx, _, _ = _case(1, 24, 9, 5)
    out = E.forward(w, idx.reshape(2, 3, 4))
    assert out.shape == (2, 3, 4, 5) and np.array_equal(out.reshape(24, 5), E.forward(w, idx))


def test_saturating_id_read():
    f = np.array([0.0, -0.0, 0.99, 1.0, 1.5, -3.0, np.nan, np.inf, -np.inf, 1e19, 16777216.0, 3.4e38], np.float32)
    big = np.iinfo(np.int64).max
    assert E.read_ids(f).tolist() == [0, 0, 0, 1, 1, 0, 0, big, 0, big, 16777216, big]
    w = np.arange(6, dtype=np.float32).reshape(3, 2) + 1
    out = E.forward(w, np.array([2.9, 3.0, np.nan, -7.0, 1e30], np.float32))
    assert np.array_equal(out, [[5, 6], [0, 0], [1, 2], [1, 2], [0, 0]])
    g = np.ones((5, 2), np.float32)
    assert np.array_equal(E.backward_assign(g, np.array([2.9, 3.0, np.nan, -7.0, 1e30], np.float32), 3), [[2, 2], [0, 0], [1, 1]])


def test_one_contribution_is_a_plain_copy():
    g = np.array([[-0.0, 1.0]], np.float32)
    out = E.backward_assign(g, np.array([1.0], np.float32), 2)
    assert np.signbit(out[1, 0]) and out[1, 1] == 1.0 and not np.signbit(out[0]).any()


def test_chunked_order_against_the_plain_order():
    rng = np.random.default_rng(3)
    n, D = 5000, 6
    g = rng.standard_normal((n, D)).astype(np.float32)
    idx = np.zeros(n, np.float32)
    idx[::50] = 1.0
    plain, chunked = E.backward_assign(g, idx, 2, chunk=1 << 30), E.backward_assign(g, idx, 2)
    ref = np.stack([g[idx == v].astype(np.float64).sum(0) for v in (0, 1)])
    # the sequential f32 sum, restated the slow way
    slow = np.zeros((2, D), np.float32)
    for v in (0, 1):
        rows = g[idx == v]
        acc = rows[0].copy()
        for r in rows[1:]:
            acc = acc + r
        slow[v] = acc
    assert np.array_equal(plain, slow)
    assert np.array_equal(chunked[1], plain[1])                              # 100 tokens: one chunk, the plain order
    bound = n * np.finfo(np.float32).eps * np.abs(g).max() * 8
    assert (np.abs(chunked - ref) <= bound).all() and (np.abs(plain - ref) <= bound).all()
    assert not np.array_equal(chunked[0], plain[0])                          # 4900 tokens: many chunks, another rounding
    assert np.array_equal(E.backward_assign(g[:E.CHUNK], np.zeros(E.CHUNK, np.float32), 1), E.backward_assign(g[:E.CHUNK], np.zeros(E.CHUNK, np.float32), 1, chunk=1 << 30))

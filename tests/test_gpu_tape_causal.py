"""`nn::MultiheadAttention` with `causal = True` through the tape (`_tape`), on every graph path of `forward()`: the packed fused
core, the strided fused core, the node-by-node paths (`fused_core = False`, with and without `strided_heads`) and a head size the
core does not take.  The oracle is tests/causal_oracle.py (the oracle's composition with the mask added) fed the Philox mask the
device draws; the rule is tests/test_gpu_tape.py's (err_gpu <= max(2 * err_cpu32, 1e-6 * scale) against the f64 oracle, margins under `mha_causal:*`)."""
import numpy as np
import pytest

from oracle import neuronika_oracle as O
import causal_oracle as CO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nk():
    import neuronika_amd
    return neuronika_amd.tape


@pytest.fixture(scope="module")
def tdev(nk):
    return nk.Device(0)


def rnd(seed, shape, lo=0.0, hi=1.0):
    a = np.random.default_rng(seed).random(shape, dtype=np.float32)
    return np.asarray(a * np.float32(hi - lo) + np.float32(lo), dtype=np.float32).reshape(shape)


def _oracle(mha, x, g, H, B, p, noise, dt=np.float64):
    W = [getattr(mha, n).weight.data().astype(dt) for n in "qkvo"]
    Bs = [getattr(mha, n).bias.data().astype(dt) for n in "qkvo"]
    return CO.mha_forward_backward(x.astype(dt), W[0], Bs[0], W[1], Bs[1], W[2], Bs[2], W[3], Bs[3], H, B, p, noise.astype(dt), g.astype(dt),
                                  causal=True)


def _check(got, want, want32, what, floor=0.0):
    scale = max(np.abs(want).max(), floor)
    err_gpu, err_cpu = np.abs(got - want).max(), np.abs(want32 - want).max()
    from conftest import record_margin
    record_margin("mha_causal:" + what, err_gpu, err_cpu, 1e-6 * scale)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


# (name, switches, backward nodes of the graph with causal off / on, draws indexed in the padded tensor)
PATHS = {
    "packed core": (dict(), 2, 2, True),                                          # [projections + core] + out-projection
    "strided core": (dict(packed_qkv=False), 5, 5, True),                         # q, k, v, core, out
    # q, k, v, scores, probabilities, context, out = 7 | the probabilities spelled out: * scale, + M, softmax, dropout = 10
    "nodes, strided": (dict(fused_core=False), 7, 10, False),
    "nodes, unfused": (dict(fused_core=False, fused=False), 9, 10, False),
    # q, k, v + their three split copies, scores, probabilities, context, merge, out = 11 | 14
    "nodes, split heads": (dict(fused_core=False, strided_heads=False), 11, 14, False),
}


def _module(nk, tdev, d, H, p, switches, causal):
    mha = nk.nn.MultiheadAttention(tdev, d, H, p, 3)
    for key, value in switches.items():
        setattr(mha, key, value)
    mha.causal = causal
    return mha


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("p,S,d,H", [(0.1, 96, 128, 2), (0.0, 160, 128, 2), (0.25, 100, 128, 4), (0.2, 64, 256, 2)])   # dh = 64, 64, 32 (ragged), 128
def test_causal_mha_equals_oracle_on_every_path(nk, tdev, path, p, S, d, H):
    switches, n_full, n_causal, padded = PATHS[path]
    B = 2
    x, g = rnd(0, (B * S, d), -1, 1), rnd(5, (B * S, d), -1, 1)
    seed = 7654321
    nk.manual_seed(seed)
    mha = _module(nk, tdev, d, H, p, switches, True)
    assert mha.causal is True
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = mha.forward(X, B)
    assert y.history_len() == n_causal
    # `causal = False` still builds the graph it built before
    assert _module(nk, tdev, d, H, p, switches, False).forward(nk.from_ndarray(tdev, x).requires_grad(), B).history_len() == n_full
    G = nk.from_ndarray(tdev, g)
    leaves = [X] + [getattr(getattr(mha, n), w) for n in "qkvo" for w in ("weight", "bias")]
    SP = (S + 31) // 32 * 32 if padded else S     # the fused core indexes its draws in the padded tensor, the node path in (B*H, S, S)
    n = B * H * SP * SP
    for call in range(2):
        noise = (np.ascontiguousarray(O.dropout_noise(n, p, seed, call * O.dropout_draws_calls(n)).reshape(B * H, SP, SP)[:, :S, :S]) if p
                 else np.ones((B * H, S, S), np.float32))
        for v in leaves:
            v.zero_grad()
        y.forward(); y.no_grad(); y.with_grad()
        y.backward_from(G)
        ref, grads = _oracle(mha, x, g, H, B, p, noise)
        ref32, grads32 = _oracle(mha, x, g, H, B, p, noise, np.float32)
        assert np.isfinite(y.data()).all() and np.isfinite(X.grad()).all()
        _check(y.data(), ref, ref32, "out")
        _check(X.grad(), grads["x"], grads32["x"], "dx")
        for nme in "qkvo":
            _check(getattr(mha, nme).weight.grad(), grads["w" + nme], grads32["w" + nme], "dw" + nme)
            _check(getattr(mha, nme).bias.grad(), grads["b" + nme], grads32["b" + nme], "db" + nme, np.abs(grads["w" + nme]).max())
    # the first query of every sample attends to one key: it does not depend on the rest of the sample
    mha.drop.eval()
    y.forward(); base = y.data().copy()
    x2 = x.copy(); x2[1:S] += 1.0                  # sample 0, every row but the first
    y2 = mha.forward(nk.from_ndarray(tdev, x2).requires_grad(), B); y2.forward()
    assert np.array_equal(y2.data()[0], base[0]) and not np.array_equal(y2.data()[1], base[1])


@pytest.mark.parametrize("d,H", [(96, 2), (80, 5)])     # dh = 48: strided node path; dh = 16: below every core size
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_causal_mha_head_size_outside_the_core(nk, tdev, d, H, p):
    B, S = 2, 40
    assert not nk.Var.attention_core_supported(S, d // H, p)
    x, g = rnd(1, (B * S, d), -1, 1), rnd(6, (B * S, d), -1, 1)
    seed = 99
    nk.manual_seed(seed)
    mha = nk.nn.MultiheadAttention(tdev, d, H, p, 3)
    mha.causal = True
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = mha.forward(X, B)
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    n = B * H * S * S
    noise = O.dropout_noise(n, p, seed, 0).reshape(B * H, S, S) if p else np.ones((B * H, S, S), np.float32)
    ref, grads = _oracle(mha, x, g, H, B, p, noise)
    ref32, grads32 = _oracle(mha, x, g, H, B, p, noise, np.float32)
    _check(y.data(), ref, ref32, "out")
    _check(X.grad(), grads["x"], grads32["x"], "dx")
    for nme in "qkvo":
        _check(getattr(mha, nme).weight.grad(), grads["w" + nme], grads32["w" + nme], "dw" + nme)


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_causal_core_and_composition_agree_under_one_seed(nk, tdev, p):
    """Whole tiles (S % 32 == 0: the padded and the plain draw layouts coincide): the fused causal core and the composed
    fallback draw the same mask from the same seed and agree to f32 rounding in output and input gradient."""
    B, S, d, H = 2, 160, 128, 2
    x, g = rnd(2, (B * S, d), -1, 1), rnd(7, (B * S, d), -1, 1)
    res = []
    for switches in (dict(), dict(fused_core=False)):
        nk.manual_seed(4321)
        mha = _module(nk, tdev, d, H, p, switches, True)
        X = nk.from_ndarray(tdev, x).requires_grad()
        y = mha.forward(X, B)
        y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
        res.append((y.data().copy(), X.grad().copy(), mha.v.weight.grad().copy()))
    for a, b in zip(*res):
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-5 * max(1.0, float(np.abs(b).max())))
    # and causal is not full attention
    nk.manual_seed(4321)
    full = _module(nk, tdev, d, H, p, dict(), False)
    yf = full.forward(nk.from_ndarray(tdev, x).requires_grad(), B); yf.forward()
    assert not np.allclose(yf.data(), res[0][0], atol=1e-3)


def test_causal_forward_without_gradients_keeps_no_score_tensor(nk, tdev):
    """`Var::heads_attention(causal)` in a graph without gradients: the inference kernels, no (B*H, SP, SP) tensor - device memory
    grows by the output only - and the values of the differentiable node."""
    B, S, H, dh = 4, 512, 4, 64
    d = H * dh
    q, k, v = (rnd(s, (B * S, d), -1, 1) for s in (1, 2, 3))
    status = nk.Status(False)
    Q, K, V = (nk.from_ndarray(tdev, t) for t in (q, k, v))
    tdev.sync()
    before = tdev.bytes_in_use() if hasattr(tdev, "bytes_in_use") else None
    out = Q.heads_attention(K, V, B, S, H, dh, float(np.float32(1 / np.sqrt(dh))), 0.0, status, causal=True)
    out.forward()
    if before is not None:
        assert tdev.bytes_in_use() - before < B * H * S * S * 4 // 2       # (one score tensor would be 16 MB; the output is 1 MB)
    Qd, Kd, Vd = (nk.from_ndarray(tdev, t).requires_grad() for t in (q, k, v))
    kept = Qd.heads_attention(Kd, Vd, B, S, H, dh, float(np.float32(1 / np.sqrt(dh))), 0.0, status, causal=True)
    kept.forward()
    assert np.array_equal(out.data(), kept.data())
    o, _ = CO.attention_core_forward(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), H, B, 0.0, np.ones((B * H, S, S)), causal=True)
    np.testing.assert_allclose(out.data(), o, rtol=0, atol=2e-6)

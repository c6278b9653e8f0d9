"""Grouped-query attention through the tape (`_tape`): the `repeat_kv` node of `Var / VarDiff`, `nn::MultiheadAttention` with
`kv_heads < heads` on the unpacked paths of `forward()` (fused core, strided nodes, split heads; causal or not; rope on and off;
dropout) and `forward_step` against an `nn::KvCache` built with kv_heads.

The oracle is tests/gqa_oracle.py in f64 and f32; the rule is the one tests/test_gpu_tape_causal.py and tests/test_gpu_tape_rope.py
hold the same quantities to (err_gpu <= max(2 * err_cpu32, 1e-6 * scale) against the f64 oracle, the bias gradients with the weight
gradient's magnitude as floor; margins under `mha_gqa:*`).  The node itself is bit-exact: a copy forward, the f32 sum of the copies in
ascending order backward.  With kv_heads == heads a module gives the bits of the constructor without kv_heads."""
import numpy as np
import pytest

import gqa_oracle as GO
import rope_oracle as RO
from oracle import neuronika_oracle as O

pytestmark = pytest.mark.gpu

B = 2


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


def _check(got, want, want32, what, floor=0.0):
    scale = max(np.abs(want).max(), floor)
    err_gpu, err_cpu = np.abs(got - want).max(), np.abs(want32 - want).max()
    from conftest import record_margin
    record_margin("mha_gqa:" + what.split("[")[0].strip(), err_gpu, err_cpu, 1e-6 * scale)
    print(what, "err_gpu %.3g err_cpu32 %.3g bound %.3g" % (err_gpu, err_cpu, max(2 * err_cpu, 1e-6 * scale)))
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


def _params(mha, dt):
    return ([getattr(mha, n).weight.data().astype(dt) for n in "qkvo"], [getattr(mha, n).bias.data().astype(dt) for n in "qkvo"])


def _oracle(mha, x, g, batch, dt, rope=None, causal=True, p=0.0, noise=None):
    W, Bs = _params(mha, dt)
    s = x.shape[0] // batch
    noise = np.ones((batch * mha.heads, s, s), dt) if noise is None else noise.astype(dt)
    return GO.mha_forward_backward(x.astype(dt), W[0], Bs[0], W[1], Bs[1], W[2], Bs[2], W[3], Bs[3], mha.heads, mha.kv_heads, batch, p, noise,
                                   g.astype(dt), causal=causal, rope=rope)


def _check_all(mha, X, y, ref, grads, ref32, grads32, what):
    _check(y.data(), ref, ref32, "out" + what)
    _check(X.grad(), grads["x"], grads32["x"], "dx" + what)
    for nme in "qkvo":
        _check(getattr(mha, nme).weight.grad(), grads["w" + nme], grads32["w" + nme], "dw" + nme + what)
        _check(getattr(mha, nme).bias.grad(), grads["b" + nme], grads32["b" + nme], "db" + nme + what, np.abs(grads["w" + nme]).max())


def _leaves(mha, X):
    return [X] + [getattr(getattr(mha, n), w) for n in "qkvo" for w in ("weight", "bias")]


# ---------------------------------------------------------------------------------------------------------------- the node
@pytest.mark.parametrize("rows,Hkv,G,dh", [(6, 2, 3, 8), (5, 1, 4, 5), (3, 3, 1, 4)])
def test_node_forward_and_gradient(nk, tdev, rows, Hkv, G, dh):
    x, g = rnd(1, (rows, Hkv * dh), -3, 3), rnd(2, (rows, Hkv * G * dh), -3, 3)
    want, s = GO.repeat_kv(x, Hkv, G, dh), GO.repeat_kv_backward_f32(g, Hkv, G, dh)
    # a Var gives a Var: one forward node, no gradient
    v = nk.from_ndarray(tdev, x).repeat_kv(G, dh)
    assert type(v).__name__ == "Var" and v.history_len() == 1
    v.forward()
    assert np.array_equal(v.data(), want)
    # first writer of the input's gradient: the assign form onto memory that was never zeroed
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = X.repeat_kv(G, dh)
    assert y.history_len() == 1 and y.forward_history_len() == 1
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    assert np.array_equal(y.data(), want)
    first = X.grad().copy()
    assert np.array_equal(first, s)
    # the input used twice, through another kind of node, in both tape orders: the node is the later writer in one, the first in the other
    for order in (0, 1):
        X2 = nk.from_ndarray(tdev, x).requires_grad()
        z = X2.repeat_kv(G, dh) + X2.relu().repeat_kv(G, dh) if order == 0 else X2.relu().repeat_kv(G, dh) + X2.repeat_kv(G, dh)
        assert z.history_len() == 4
        z.forward(); z.backward_from(nk.from_ndarray(tdev, g))
        assert np.array_equal(X2.grad(), np.where(x > 0, s + s, s)), order               # f32 addition commutes: exact in both orders
    # and two nodes on one input
    X3 = nk.from_ndarray(tdev, x).requires_grad()
    z = X3.repeat_kv(G, dh) + X3.repeat_kv(G, dh)
    z.forward(); z.backward_from(nk.from_ndarray(tdev, g))
    assert np.array_equal(X3.grad(), s + s)
    # zero_grad and a second backward reproduce the first
    X.zero_grad(); y.zero_grad()
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    assert np.array_equal(X.grad().view(np.uint32), first.view(np.uint32))


def test_node_panics(nk, tdev):
    x = nk.from_ndarray(tdev, rnd(3, (4, 24), -1, 1))
    assert x.repeat_kv(2, 8).shape == [4, 48]
    for groups, dh in ((0, 8), (-1, 8), (2, 0), (2, 5), (2, 48)):
        with pytest.raises(RuntimeError):
            x.repeat_kv(groups, dh)
    with pytest.raises(RuntimeError):
        nk.from_ndarray(tdev, rnd(3, (4, 24), -1, 1)).requires_grad().repeat_kv(2, 7)


# ---------------------------------------------------------------------------------------------------------------- the module
PATHS = {"strided core": dict(), "nodes, strided": dict(fused_core=False), "nodes, split heads": dict(fused_core=False, strided_heads=False),
         "core, split heads off": dict(strided_heads=False)}


def _module(nk, tdev, d, H, Hkv, p=0.0, causal=True, seed=3):
    mha = nk.nn.MultiheadAttention(tdev, d, H, p, seed, kv_heads=Hkv)
    assert (mha.heads, mha.kv_heads, mha.d_model) == (H, Hkv, d)
    dkv = d // H * Hkv
    assert mha.k.weight.shape == [dkv, d] and mha.v.weight.shape == [dkv, d] and mha.q.weight.shape == [d, d]
    assert mha.k.bias.shape == [dkv] and mha.v.bias.shape == [dkv]
    mha.causal = causal
    return mha


def _rotary(nk, tdev, dh, max_pos=160):
    return nk.nn.RotaryEmbedding(tdev, dh, max_pos), RO.make(max_pos, dh)


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("d,H,Hkv,S", [(128, 4, 1, 40), (128, 4, 2, 40), (128, 4, 1, 128), (128, 4, 2, 128), (80, 4, 2, 40), (80, 4, 1, 40)])
def test_module_equals_oracle(nk, tdev, d, H, Hkv, S, causal, use_rope):
    """dh = 32 on the fused core (S = 40: a ragged tile; S = 128) and dh = 20 on the strided node path, every switch setting at S = 40."""
    mha = _module(nk, tdev, d, H, Hkv, causal=causal)
    r, ro = _rotary(nk, tdev, d // H) if use_rope else (None, None)
    mha.rope = r
    x, g = rnd(0, (B * S, d), -1, 1), rnd(5, (B * S, d), -1, 1)
    ref, grads = _oracle(mha, x, g, B, np.float64, ro, causal)
    ref32, grads32 = _oracle(mha, x, g, B, np.float32, ro, causal)
    paths = PATHS if S == 40 else {"strided core": dict()}
    for path, switches in paths.items():
        for key, value in switches.items():
            setattr(mha, key, value)
        X = nk.from_ndarray(tdev, x).requires_grad()
        y = mha.forward(X, B)
        for leaf in _leaves(mha, X):
            leaf.zero_grad()
        y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
        what = " [d %d H %d Hkv %d S %d, %s, %s, %s]" % (d, H, Hkv, S, path, "causal" if causal else "full", "rope" if use_rope else "plain")
        assert np.isfinite(y.data()).all() and np.isfinite(X.grad()).all(), what
        _check_all(mha, X, y, ref, grads, ref32, grads32, what)
        for key in switches:
            setattr(mha, key, True)


def test_the_grouped_graph_adds_two_nodes(nk, tdev):
    """kv_heads < heads: the unpacked graph of the module plus the two repeat nodes; with rope, K's rotation runs on kv_heads heads."""
    d, H, S = 128, 4, 40
    x = rnd(0, (B * S, d), -1, 1)
    plain = nk.nn.MultiheadAttention(tdev, d, H, 0.0, 3)
    plain.packed_qkv = False
    n_plain = plain.forward(nk.from_ndarray(tdev, x).requires_grad(), B).history_len()
    for Hkv in (1, 2):
        mha = _module(nk, tdev, d, H, Hkv)
        assert mha.forward(nk.from_ndarray(tdev, x).requires_grad(), B).history_len() == n_plain + 2
        mha.rope = _rotary(nk, tdev, d // H)[0]
        assert mha.forward(nk.from_ndarray(tdev, x).requires_grad(), B).history_len() == n_plain + 4


def test_module_train_mode_backward(nk, tdev):
    """Dropout active (p = 0.1) on the fused core: the oracle is fed the Philox mask the device draws (indexed in the padded tensor)."""
    p, seed, d, H, Hkv, S = 0.1, 24680, 128, 4, 2, 40
    nk.manual_seed(seed)
    mha = _module(nk, tdev, d, H, Hkv, p=p)
    x, g = rnd(0, (B * S, d), -1, 1), rnd(5, (B * S, d), -1, 1)
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = mha.forward(X, B)
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    SP = (S + 31) // 32 * 32
    n = B * H * SP * SP
    noise = np.ascontiguousarray(O.dropout_noise(n, p, seed, 0).reshape(B * H, SP, SP)[:, :S, :S])
    ref, grads = _oracle(mha, x, g, B, np.float64, None, True, p, noise)
    ref32, grads32 = _oracle(mha, x, g, B, np.float32, None, True, p, noise)
    _check_all(mha, X, y, ref, grads, ref32, grads32, " [train]")


@pytest.mark.parametrize("d,H", [(128, 2), (10, 2)])
def test_kv_heads_equal_to_heads_is_the_module_without_it(nk, tdev, d, H):
    """Same seed: parameters, graph and outputs of the constructor without kv_heads, bit for bit; forward_step too."""
    S = 24
    x, g = rnd(0, (B * S, d), -1, 1), rnd(5, (B * S, d), -1, 1)
    runs = []
    for kw in (dict(), dict(kv_heads=H), dict(kv_heads=0)):
        mha = nk.nn.MultiheadAttention(tdev, d, H, 0.0, 3, **kw)
        assert mha.kv_heads == H and mha.packed_qkv is (d % 4 == 0)
        mha.causal = True
        X = nk.from_ndarray(tdev, x).requires_grad()
        y = mha.forward(X, B)
        y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
        cache = nk.nn.KvCache(tdev, B, H, d // H, S)
        s0 = mha.forward_step(nk.from_ndarray(tdev, x[:B * 12]), B, cache); s0.forward()
        s1 = mha.forward_step(nk.from_ndarray(tdev, x[B * 12:B * 13]), B, cache); s1.forward()
        runs.append([y.history_len()] + [a.data() for a in (y, s0, s1)] + [X.grad()] + [l.data() for l in _leaves(mha, X)[1:]] +
                    [l.grad() for l in _leaves(mha, X)[1:]])
    for other in runs[1:]:
        assert other[0] == runs[0][0]
        for a, b in zip(runs[0][1:], other[1:]):
            assert np.array_equal(a, b)


def test_constructor_panics(nk, tdev):
    for H, Hkv in ((4, 3), (4, 8), (4, -1)):
        with pytest.raises(RuntimeError, match="kv_heads"):
            nk.nn.MultiheadAttention(tdev, 128, H, 0.0, 3, kv_heads=Hkv)
    lin = lambda i, o, s: nk.nn.Linear(tdev, i, o, s)
    nk.nn.MultiheadAttention(lin(128, 128, 1), lin(128, 64, 2), lin(128, 64, 3), lin(128, 128, 4), 4, 0.0, kv_heads=2)
    with pytest.raises(RuntimeError, match="k and v"):
        nk.nn.MultiheadAttention(lin(128, 128, 1), lin(128, 128, 2), lin(128, 128, 3), lin(128, 128, 4), 4, 0.0, kv_heads=2)
    with pytest.raises(RuntimeError, match="k and v"):
        nk.nn.MultiheadAttention(lin(128, 128, 1), lin(128, 64, 2), lin(128, 32, 3), lin(128, 128, 4), 4, 0.0, kv_heads=2)


# ---------------------------------------------------------------------------------------------------------------- forward_step
# name -> (d_model, heads, kv_heads, built from four handed-in Linears)
STEP_MODULES = {"packed dh 32 G 4": (128, 4, 1, False), "packed dh 64 G 2": (256, 4, 2, False), "generic dh 20 G 2": (80, 4, 2, False),
                "four Linears dh 32 G 2": (128, 4, 2, True)}


def _step_module(nk, tdev, name, use_rope):
    d, H, Hkv, handed = STEP_MODULES[name]
    dkv = d // H * Hkv
    if handed:
        outs = (d, dkv, dkv, d)
        mha = nk.nn.MultiheadAttention(*(nk.nn.Linear(tdev, d, outs[i], 11 + 2 * i) for i in range(4)), H, 0.1, kv_heads=Hkv)
    else:
        mha = nk.nn.MultiheadAttention(tdev, d, H, 0.1, 3, kv_heads=Hkv)
    assert mha.packed_qkv is (not handed) and mha.kv_heads == Hkv
    mha.causal = True
    mha.drop.eval()
    r, ro = _rotary(nk, tdev, d // H, 96) if use_rope else (None, None)
    mha.rope = r
    return mha, ro, d, H, Hkv


def _rows(x, S, lo, hi, batch=B):
    return np.ascontiguousarray(np.concatenate([x[b * S + lo:b * S + hi] for b in range(batch)]))


def _step(nk, tdev, mha, cache, rows, batch=B):
    y = mha.forward_step(nk.from_ndarray(tdev, rows), batch, cache)
    assert y.history_len() == 1                                           # ONE forward node
    y.forward()
    return y


def _walk(nk, tdev, mha, cache, x, S, slices, batch=B):
    out, pos = np.zeros_like(x), 0
    for T in slices:
        assert cache.lens() == [pos] * batch
        got = _step(nk, tdev, mha, cache, _rows(x, S, pos, pos + T, batch), batch).data()
        for b in range(batch):
            out[b * S + pos:b * S + pos + T] = got[b * T:(b + 1) * T]
        pos += T
    assert pos == S and cache.lens() == [S] * batch
    return out


def _forward_oracle(mha, x, batch, dt, ro):
    W, Bs = _params(mha, dt)
    return GO.mha_forward(x.astype(dt), W, Bs, mha.heads, mha.kv_heads, batch, causal=True, rope=ro)


def _stepped_oracle(mha, x, S, slices, batch, dt, ro):
    """tests/gqa_oracle.py's mha_step over the same slices, on (batch, kv_heads, S, dh) caches"""
    W, Bs = _params(mha, dt)
    dh = mha.d_model // mha.heads
    kc, vc = np.full((batch, mha.kv_heads, S, dh), np.nan, dt), np.full((batch, mha.kv_heads, S, dh), np.nan, dt)
    out, start = np.zeros((batch * S, mha.d_model), dt), np.zeros(batch, dtype=np.int64)
    for T in slices:
        pos = int(start[0])
        got, start = GO.mha_step(_rows(x, S, pos, pos + T, batch).astype(dt), W, Bs, mha.heads, mha.kv_heads, kc, vc, start, T, rope=ro)
        for b in range(batch):
            out[b * S + pos:b * S + pos + T] = got[b * T:(b + 1) * T]
    return out


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("name", list(STEP_MODULES))
def test_prefill_then_steps_and_chunked_prefill(nk, tdev, name, use_rope):
    """Prefill 40 + 6 single steps (the core on the repeated rows, then the grouped decode kernels), and a chunked prefill 16 + 3 + 3
    (T = 3 at start > 0) + steps: against the stepped oracle, the oracle's full causal forward, and forward() over the whole prefix."""
    S, T0 = 46, 40
    mha, ro, d, H, Hkv = _step_module(nk, tdev, name, use_rope)
    x = rnd(0, (B * S, d), -1, 1)
    ref, ref32 = _forward_oracle(mha, x, B, np.float64, ro), _forward_oracle(mha, x, B, np.float32, ro)
    full = mha.forward(nk.from_ndarray(tdev, x).requires_grad(), B)
    full.forward()
    _check(full.data(), ref, ref32, "forward [%s]" % name)
    bound = max(2 * np.abs(ref32 - ref).max(), 1e-6 * np.abs(ref).max())
    for slices in ([T0] + [1] * (S - T0), [16, 3, 3] + [1] * (S - 22)):
        cache = nk.nn.KvCache(tdev, B, Hkv, d // H, S)
        assert (cache.batch, cache.heads, cache.capacity, cache.head_dim) == (B, Hkv, S, d // H)     # (B, Hkv, cap, dh)
        got = _walk(nk, tdev, mha, cache, x, S, slices)
        _check(got, ref, ref32, "steps [%s %s]" % (name, slices[:3]))
        stepped = _stepped_oracle(mha, x, S, slices, B, np.float64, ro)
        assert np.abs(stepped - ref).max() <= 1e-9                        # the two oracles agree
        between = np.abs(got - full.data()).max()
        print("steps against forward [%s] distance %.3g bound %.3g" % (name, between, bound))
        assert between <= bound, (name, between, bound)


@pytest.mark.parametrize("name", ["packed dh 32 G 4", "generic dh 20 G 2", "four Linears dh 32 G 2"])
def test_ragged_prompts(nk, tdev, name):
    """Right-padded prompts of true lengths (40, 23): prefill, truncate, step 6 tokens; every sample equals the oracle over its own
    positions, and sample 1 equals, in bits, a run of sample 1 alone."""
    mha, ro, d, H, Hkv = _step_module(nk, tdev, name, True)
    lens, T0, steps = [40, 23], 40, 6
    prompt, new = rnd(1, (B * T0, d), -1, 1), rnd(2, (B * steps, d), -1, 1)
    cache = nk.nn.KvCache(tdev, B, Hkv, d // H, 64)
    pre = _step(nk, tdev, mha, cache, prompt).data()
    cache.truncate(lens)
    outs = np.stack([_step(nk, tdev, mha, cache, _rows(new, steps, s, s + 1)).data() for s in range(steps)], axis=1)   # (B, steps, d)
    assert cache.lens() == [l + steps for l in lens]
    for b in range(B):
        xb = np.concatenate([prompt[b * T0:b * T0 + lens[b]], new[b * steps:(b + 1) * steps]])
        got = np.concatenate([pre[b * T0:b * T0 + lens[b]], outs[b]])
        _check(got, _forward_oracle(mha, xb, 1, np.float64, ro), _forward_oracle(mha, xb, 1, np.float32, ro), "ragged [%s]" % name)
    alone = nk.nn.KvCache(tdev, 1, Hkv, d // H, 64)
    _step(nk, tdev, mha, alone, np.ascontiguousarray(prompt[T0:T0 + lens[1]]), 1)
    for s in range(steps):
        one = _step(nk, tdev, mha, alone, np.ascontiguousarray(new[steps + s:steps + s + 1]), 1).data()
        assert np.array_equal(one[0], outs[1, s]), (name, s)


@pytest.mark.parametrize("name", ["packed dh 32 G 4", "four Linears dh 32 G 2"])
def test_a_second_forward_of_a_node_changes_nothing(nk, tdev, name):
    mha, ro, d, H, Hkv = _step_module(nk, tdev, name, True)
    x = rnd(5, (B * 12, d), -1, 1)
    cache = nk.nn.KvCache(tdev, B, Hkv, d // H, 16)
    pre = _step(nk, tdev, mha, cache, _rows(x, 12, 0, 8))
    y1 = _step(nk, tdev, mha, cache, _rows(x, 12, 8, 9))
    y2 = _step(nk, tdev, mha, cache, _rows(x, 12, 9, 10))
    a_pre, a1, a2 = pre.data(), y1.data(), y2.data()
    y1.forward(); pre.forward(); y1.forward()                            # earlier nodes again: the same rows to the same places
    assert cache.lens() == [10, 10]
    assert np.array_equal(pre.data(), a_pre) and np.array_equal(y1.data(), a1)
    y2.forward()
    assert np.array_equal(y2.data(), a2)


def test_a_cache_built_with_heads_panics(nk, tdev):
    mha, ro, d, H, Hkv = _step_module(nk, tdev, "packed dh 32 G 4", False)
    x = nk.from_ndarray(tdev, rnd(7, (B * 4, d), -1, 1))
    with pytest.raises(RuntimeError, match=r"%d heads of .* %d kv heads \(of %d query heads\)" % (H, Hkv, H)):
        mha.forward_step(x, B, nk.nn.KvCache(tdev, B, H, d // H, 8))
    cache = nk.nn.KvCache(tdev, B, Hkv, d // H, 8)
    mha.forward_step(x, B, cache)
    assert cache.lens() == [4, 4]


def test_serde_round_trip(nk, tdev):
    """The module serialises as its four Linears; the four-Linear constructor with kv_heads reproduces the outputs."""
    mha, ro, d, H, Hkv = _step_module(nk, tdev, "packed dh 32 G 4", False)
    sd = nk.serde
    layers = [sd.linear_from_json(tdev, sd.to_json(getattr(mha, n))) for n in "qkvo"]
    back = nk.nn.MultiheadAttention(*layers, H, 0.1, kv_heads=Hkv)
    back.causal = True
    back.drop.eval()
    assert back.kv_heads == Hkv and back.packed_qkv is False
    S = 20
    x = rnd(3, (B * S, d), -1, 1)
    a, b = (m.forward(nk.from_ndarray(tdev, x).requires_grad(), B) for m in (mha, back))
    a.forward(); b.forward()
    assert np.array_equal(a.data(), b.data())                             # both take the unpacked branch: the same launches
    ref, ref32 = _forward_oracle(mha, x, B, np.float64, None), _forward_oracle(mha, x, B, np.float32, None)
    ca, cb = nk.nn.KvCache(tdev, B, Hkv, d // H, S), nk.nn.KvCache(tdev, B, Hkv, d // H, S)
    slices = [12] + [1] * 8
    _check(_walk(nk, tdev, mha, ca, x, S, slices), ref, ref32, "serde packed steps")
    _check(_walk(nk, tdev, back, cb, x, S, slices), ref, ref32, "serde restored steps")

"""Rotary position embedding through the tape (`_tape`): the `rope` node of `Var / VarDiff`, `nn::MultiheadAttention` with `rope` set
on every path of `forward()` (causal or not) and `forward_step` against an `nn::KvCache`, on the modules of
tests/test_gpu_tape_decode.py: packed dh 64 / 32 / 128, generic dh 20, unpacked dh 5 (rot = 4) and four handed-in Linears.

The oracle is tests/rope_oracle.py in f64 and f32; the rule is tests/test_gpu_tape_causal.py's (err_gpu <= max(2 * err_cpu32,
1e-6 * scale) against the f64 oracle, margins under `mha_rope:*`).  The node itself is held to the elementwise bound of
tests/test_gpu_rope.py.  With `rope = None` a module gives the bits of a module that never had one."""
import numpy as np
import pytest

import rope_oracle as RO
from oracle import neuronika_oracle as O
from test_gpu_tape_decode import MODULES, _rows, rnd

pytestmark = pytest.mark.gpu

B, S, MAX_POS = 2, 72, 96


@pytest.fixture(scope="module")
def nk():
    import neuronika_amd
    return neuronika_amd.tape


@pytest.fixture(scope="module")
def tdev(nk):
    return nk.Device(0)


def _check(got, want, want32, what, floor=0.0):
    scale = max(np.abs(want).max(), floor)
    err_gpu, err_cpu = np.abs(got - want).max(), np.abs(want32 - want).max()
    from conftest import record_margin
    record_margin("mha_rope:" + what.split("[")[0].strip(), err_gpu, err_cpu, 1e-6 * scale)
    print(what, "err_gpu %.3g err_cpu32 %.3g bound %.3g" % (err_gpu, err_cpu, max(2 * err_cpu, 1e-6 * scale)))
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


def _rot(dh):
    return dh if dh % 2 == 0 else 4                                      # dh = 5: four rotated columns, one passes through


def _rotary(nk, tdev, dh, il=False, max_pos=MAX_POS):
    r = nk.nn.RotaryEmbedding(tdev, dh, max_pos, 10000.0, _rot(dh), il)
    assert (r.head_dim, r.max_pos, r.rot, r.interleaved) == (dh, max_pos, _rot(dh), il)
    return r, RO.make(max_pos, dh, _rot(dh), il)


def _module(nk, tdev, name, p=0.1, causal=True, train=False):
    d, H, handed = MODULES[name]
    if handed:
        mha = nk.nn.MultiheadAttention(*(nk.nn.Linear(tdev, d, d, 11 + 2 * i) for i in range(4)), H, p)
    else:
        mha = nk.nn.MultiheadAttention(tdev, d, H, p, 3)
    mha.causal = causal
    if not train:
        mha.drop.eval()
    return mha, d, H


def _oracle(mha, x, g, H, batch, dt, rope, causal=True, p=0.0, noise=None):
    W = [getattr(mha, n).weight.data().astype(dt) for n in "qkvo"]
    Bs = [getattr(mha, n).bias.data().astype(dt) for n in "qkvo"]
    s = x.shape[0] // batch
    noise = np.ones((batch * H, s, s), dt) if noise is None else noise.astype(dt)
    return RO.mha_forward_backward(x.astype(dt), W[0], Bs[0], W[1], Bs[1], W[2], Bs[2], W[3], Bs[3], H, batch, p, noise, g.astype(dt),
                                   causal=causal, rope=rope)


# ---------------------------------------------------------------------------------------------------------------- the node
@pytest.mark.parametrize("dh,rot,il", [(64, 64, False), (64, 32, True), (20, 20, False), (5, 4, False), (8, 8, True)])
def test_node_forward_and_gradient(nk, tdev, dh, rot, il):
    H, T = 3, 37
    r = nk.nn.RotaryEmbedding(tdev, dh, 64, 10000.0, rot, il)
    assert np.array_equal(r.table().shape, (64, rot // 2, 2))
    ro = RO.make(64, dh, rot, il)
    x, g = rnd(1, (B * T, H * dh), -3, 3), rnd(2, (B * T, H * dh), -3, 3)
    y64 = RO.rope(x.astype(np.float64), None, T, H, dh, rot, il, ro.table)
    d64 = RO.rope(g.astype(np.float64), None, T, H, dh, rot, il, ro.table, inverse=True)

    def pair_sum(a):
        ah = np.abs(a.astype(np.float64)).reshape(-1, H, dh)
        out = np.zeros_like(ah)
        c1, c2 = RO.pair_columns(rot, il)
        out[:, :, c1] = out[:, :, c2] = ah[:, :, c1] + ah[:, :, c2]
        return out.reshape(a.shape)

    # a Var gives a Var: one forward node, no gradient
    v = nk.from_ndarray(tdev, x).rope(r, B, H)
    assert type(v).__name__ == "Var" and v.history_len() == 1
    v.forward()
    assert np.all(np.abs(v.data() - y64) <= 2.0 ** -22 * pair_sum(x))
    # first writer of the input's gradient: the assign form onto memory that was never zeroed
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = X.rope(r, B, H)
    assert y.history_len() == 1 and y.forward_history_len() == 1
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    assert np.array_equal(y.data(), v.data())
    first = X.grad().copy()
    assert np.all(np.abs(first - d64) <= 2.0 ** -22 * pair_sum(g))
    # with another node on the same input, in both tape orders: the rope node is the later writer in one and the first in the other
    relu64 = g.astype(np.float64) * (x > 0)
    for order in (0, 1):
        X2 = nk.from_ndarray(tdev, x).requires_grad()
        z = X2.rope(r, B, H) + X2.relu() if order == 0 else X2.relu() + X2.rope(r, B, H)
        assert z.history_len() == 3
        z.forward(); z.backward_from(nk.from_ndarray(tdev, g))
        want = d64 + relu64
        assert np.all(np.abs(X2.grad() - want) <= 2.0 ** -22 * pair_sum(g) * (1 + 2.0 ** -24) + 2.0 ** -24 * np.abs(want)), order
    # and two rope nodes on one input
    X3 = nk.from_ndarray(tdev, x).requires_grad()
    z = X3.rope(r, B, H) + X3.rope(r, B, H)
    z.forward(); z.backward_from(nk.from_ndarray(tdev, g))
    assert np.all(np.abs(X3.grad() - 2 * d64) <= 2 * 2.0 ** -22 * pair_sum(g))        # first + first again: the doubling is exact
    # zero_grad and a second backward reproduce the first
    X.zero_grad(); y.zero_grad()
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    assert np.array_equal(X.grad().view(np.uint32), first.view(np.uint32))


def test_node_panics(nk, tdev):
    r = nk.nn.RotaryEmbedding(tdev, 8, 16)
    assert r.rot == 8 and r.interleaved is False and r.base == 10000.0   # rot defaults to head_dim
    x = nk.from_ndarray(tdev, rnd(3, (B * 8, 24), -1, 1))
    x.rope(r, B, 3)
    for batch, heads in ((B, 2), (B, 4), (3, 3), (0, 3)):
        with pytest.raises(RuntimeError):
            x.rope(r, batch, heads)
    with pytest.raises(RuntimeError, match="positions"):
        nk.from_ndarray(tdev, rnd(3, (B * 17, 24), -1, 1)).rope(r, B, 3)                 # T = 17 > max_pos = 16
    with pytest.raises(RuntimeError):
        nk.from_ndarray(tdev, rnd(3, (B * 8, 24), -1, 1)).requires_grad().rope(r, B, 2)
    for bad in (dict(rot=3), dict(rot=10), dict(rot=-2), dict(max_pos=0), dict(head_dim=0), dict(base=0.0)):
        a = dict(dict(head_dim=8, max_pos=16, base=10000.0, rot=8), **bad)
        with pytest.raises(RuntimeError):
            nk.nn.RotaryEmbedding(tdev, a["head_dim"], a["max_pos"], a["base"], a["rot"])


# ---------------------------------------------------------------------------------------------------------------- the module
# graph paths of forward(): switches -> backward nodes without / with rope (two more rope nodes wherever q and k are nodes of their own)
PATHS = {"default": dict(), "strided core": dict(packed_qkv=False), "nodes, strided": dict(fused_core=False),
         "nodes, split heads": dict(fused_core=False, strided_heads=False)}


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("name", list(MODULES))
def test_module_equals_oracle(nk, tdev, name, causal):
    mha, d, H = _module(nk, tdev, name, causal=causal)
    r, ro = _rotary(nk, tdev, d // H, il=name == "packed dh 32")
    mha.rope = r
    assert mha.rope is not None and mha.rope.head_dim == d // H
    x, g = rnd(0, (B * S, d), -1, 1), rnd(5, (B * S, d), -1, 1)
    ref, grads = _oracle(mha, x, g, H, B, np.float64, ro, causal)
    ref32, grads32 = _oracle(mha, x, g, H, B, np.float32, ro, causal)
    paths = PATHS if name == "packed dh 64" else {"default": dict()}
    for path, switches in paths.items():
        for key, value in switches.items():
            setattr(mha, key, value)
        X = nk.from_ndarray(tdev, x).requires_grad()
        mha.rope = None
        n_plain = mha.forward(X, B).history_len()
        mha.rope = r
        y = mha.forward(X, B)
        packed_node = name.startswith("packed") and path == "default"
        assert y.history_len() == n_plain + (0 if packed_node else 2), (name, path)
        for leaf in [X] + [getattr(getattr(mha, n), w) for n in "qkvo" for w in ("weight", "bias")]:
            leaf.zero_grad()
        y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
        what = " [%s, %s, %s]" % (name, path, "causal" if causal else "full")
        _check(y.data(), ref, ref32, "out" + what)
        _check(X.grad(), grads["x"], grads32["x"], "dx" + what)
        for nme in "qkvo":
            _check(getattr(mha, nme).weight.grad(), grads["w" + nme], grads32["w" + nme], "dw" + nme + what)
            _check(getattr(mha, nme).bias.grad(), grads["b" + nme], grads32["b" + nme], "db" + nme + what, np.abs(grads["w" + nme]).max())
        for key in switches:
            setattr(mha, key, True)


def test_module_train_mode_backward(nk, tdev):
    """Packed dh 64 with dropout active (p = 0.1): the oracle is fed the Philox mask the device draws."""
    p, seed = 0.1, 24680
    nk.manual_seed(seed)
    mha, d, H = _module(nk, tdev, "packed dh 64", p=p, train=True)
    r, ro = _rotary(nk, tdev, d // H)
    mha.rope = r
    x, g = rnd(0, (B * S, d), -1, 1), rnd(5, (B * S, d), -1, 1)
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = mha.forward(X, B)
    assert y.history_len() == 2
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    SP = (S + 31) // 32 * 32
    n = B * H * SP * SP
    noise = np.ascontiguousarray(O.dropout_noise(n, p, seed, 0).reshape(B * H, SP, SP)[:, :S, :S])
    ref, grads = _oracle(mha, x, g, H, B, np.float64, ro, True, p, noise)
    ref32, grads32 = _oracle(mha, x, g, H, B, np.float32, ro, True, p, noise)
    _check(y.data(), ref, ref32, "train out")
    _check(X.grad(), grads["x"], grads32["x"], "train dx")
    for nme in "qkvo":
        _check(getattr(mha, nme).weight.grad(), grads["w" + nme], grads32["w" + nme], "train dw" + nme)
        _check(getattr(mha, nme).bias.grad(), grads["b" + nme], grads32["b" + nme], "train db" + nme, np.abs(grads["w" + nme]).max())


@pytest.mark.parametrize("name", list(MODULES))
def test_rope_none_is_the_module_without_one(nk, tdev, name):
    """The no-behaviour-change check: set and cleared again, forward, backward and forward_step give the bits of a module that never
    had a rotary object."""
    res = []
    for touched in (False, True):
        mha, d, H = _module(nk, tdev, name)
        if touched:
            mha.rope = _rotary(nk, tdev, d // H)[0]
            mha.rope = None
        assert mha.rope is None
        x, g = rnd(0, (B * 40, d), -1, 1), rnd(5, (B * 40, d), -1, 1)
        X = nk.from_ndarray(tdev, x).requires_grad()
        y = mha.forward(X, B)
        y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
        cache = nk.nn.KvCache(tdev, B, H, d // H, 48)
        s0 = mha.forward_step(nk.from_ndarray(tdev, x), B, cache); s0.forward()
        s1 = mha.forward_step(nk.from_ndarray(tdev, _rows(g, 40, 0, 1)), B, cache); s1.forward()
        res.append((y.history_len(), y.data().copy(), X.grad().copy(), mha.q.weight.grad().copy(), s0.data().copy(), s1.data().copy()))
    assert res[0][0] == res[1][0]
    for a, b in zip(res[0][1:], res[1][1:]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


def test_module_panics(nk, tdev):
    mha, d, H = _module(nk, tdev, "packed dh 64")
    x = nk.from_ndarray(tdev, rnd(7, (B * 20, d), -1, 1)).requires_grad()
    mha.rope = nk.nn.RotaryEmbedding(tdev, 32, 64)
    with pytest.raises(RuntimeError, match="heads of"):
        mha.forward(x, B)                                                 # built for another head size
    with pytest.raises(RuntimeError, match="heads of"):
        mha.forward_step(x, B, nk.nn.KvCache(tdev, B, H, d // H, 32))
    mha.rope = nk.nn.RotaryEmbedding(tdev, 64, 16)
    with pytest.raises(RuntimeError, match="positions"):
        mha.forward(x, B)                                                 # S = 20 > max_pos = 16
    cache = nk.nn.KvCache(tdev, B, H, d // H, 17)
    with pytest.raises(RuntimeError, match="capacity"):
        mha.forward_step(nk.from_ndarray(tdev, rnd(7, (B, d), -1, 1)), B, cache)          # capacity 17 > max_pos 16
    assert cache.lens() == [0, 0]                                         # a refused step leaves the cache as it was
    mha.forward_step(nk.from_ndarray(tdev, rnd(7, (B, d), -1, 1)), B, nk.nn.KvCache(tdev, B, H, d // H, 16))


# ---------------------------------------------------------------------------------------------------------------- decoding
def _step(nk, tdev, mha, cache, rows, batch=B):
    y = mha.forward_step(nk.from_ndarray(tdev, rows), batch, cache)
    assert y.history_len() == 1                                           # still ONE forward node
    y.forward()
    return y


def _walk(nk, tdev, mha, cache, x, s, slices, batch=B):
    out, pos = np.zeros_like(x), 0
    for T in slices:
        got = _step(nk, tdev, mha, cache, _rows(x, s, pos, pos + T, batch), batch).data()
        for b in range(batch):
            out[b * s + pos:b * s + pos + T] = got[b * T:(b + 1) * T]
        pos += T
    assert cache.lens() == [s] * batch
    return out


_REF = {}


def _reference(nk, tdev, name):
    """(module with rope set, x, f64 reference, f32 reference) of the causal forward over all S positions: once per module, shared"""
    if name not in _REF:
        mha, d, H = _module(nk, tdev, name)
        r, ro = _rotary(nk, tdev, d // H, il=name == "packed dh 32")
        mha.rope = r
        x = rnd(0, (B * S, d), -1, 1)
        zero = np.zeros_like(x)
        ref, ref32 = _oracle(mha, x, zero, H, B, np.float64, ro)[0], _oracle(mha, x, zero, H, B, np.float32, ro)[0]
        for a in (x, ref, ref32):
            a.setflags(write=False)
        _REF[name] = (mha, x, ref, ref32, ro)
    return _REF[name]


@pytest.mark.parametrize("name", list(MODULES))
def test_prefill_then_steps(nk, tdev, name):
    """Prefill 40 (the causal core with every start 0 where the head size allows), then 32 single steps (the split-KV kernels)."""
    mha, x, ref, ref32, _ = _reference(nk, tdev, name)
    d, H, _h = MODULES[name]
    cache = nk.nn.KvCache(tdev, B, H, d // H, 80)
    got = _walk(nk, tdev, mha, cache, x, S, [40] + [1] * 32)
    _check(got, ref, ref32, "prefill + steps [%s]" % name)
    full = mha.forward(nk.from_ndarray(tdev, x).requires_grad(), B)
    full.forward()
    _check(full.data(), ref, ref32, "forward [%s]" % name)
    bound = max(2 * np.abs(ref32 - ref).max(), 1e-6 * np.abs(ref).max())
    between = np.abs(got - full.data()).max()
    print("steps against forward [%s] distance %.3g bound %.3g" % (name, between, bound))
    assert between <= bound, (name, between, bound)


@pytest.mark.parametrize("name", list(MODULES))
def test_chunked_prefill(nk, tdev, name):
    """16 + 16 + 8 (T > 1 at start > 0: rows rotated at start[b] + t), then steps; capacity = max_pos exactly."""
    mha, x, ref, ref32, _ = _reference(nk, tdev, name)
    d, H, _h = MODULES[name]
    cache = nk.nn.KvCache(tdev, B, H, d // H, MAX_POS)
    got = _walk(nk, tdev, mha, cache, x, S, [16, 16, 8] + [1] * 32)
    _check(got, ref, ref32, "chunked prefill [%s]" % name)


@pytest.mark.parametrize("name", ["packed dh 64", "generic dh 20", "unpacked dh 5", "four Linears dh 64"])
def test_ragged_prompts(nk, tdev, name):
    """Right-padded prompts of true lengths (40, 23) through `truncate`: the next rows of sample 1 are rotated at 23, 24, ..."""
    mha, _x, _r, _r32, ro = _reference(nk, tdev, name)
    d, H, _h = MODULES[name]
    lens, T0, steps = [40, 23], 40, 6
    prompt, new = rnd(1, (B * T0, d), -1, 1), rnd(2, (B * steps, d), -1, 1)
    cache = nk.nn.KvCache(tdev, B, H, d // H, 64)
    pre = _step(nk, tdev, mha, cache, prompt).data()
    cache.truncate(lens)
    outs = np.stack([_step(nk, tdev, mha, cache, _rows(new, steps, s, s + 1)).data() for s in range(steps)], axis=1)
    assert cache.lens() == [l + steps for l in lens]
    zero = None
    for b in range(B):
        xb = np.concatenate([prompt[b * T0:b * T0 + lens[b]], new[b * steps:(b + 1) * steps]])
        zero = np.zeros_like(xb)
        ref, ref32 = _oracle(mha, xb, zero, H, 1, np.float64, ro)[0], _oracle(mha, xb, zero, H, 1, np.float32, ro)[0]
        _check(np.concatenate([pre[b * T0:b * T0 + lens[b]], outs[b]]), ref, ref32, "ragged [%s]" % name)


@pytest.mark.parametrize("name", ["packed dh 64", "generic dh 20", "unpacked dh 5"])
def test_roll_back_and_a_second_forward(nk, tdev, name):
    mha, x, _r, _r32, _ = _reference(nk, tdev, name)
    d, H, _h = MODULES[name]
    s = 30
    xs = np.ascontiguousarray(np.concatenate([x[b * S:b * S + s] for b in range(B)]))
    cache = nk.nn.KvCache(tdev, B, H, d // H, 32)
    first = _walk(nk, tdev, mha, cache, xs, s, [12, 5] + [1] * 13)
    cache.truncate([17, 17])                                              # roll back, decode again: the same bits
    again = np.zeros_like(first)
    nodes = []
    for t in range(13):
        y = _step(nk, tdev, mha, cache, _rows(xs, s, 17 + t, 18 + t))
        nodes.append((y, y.data().copy()))
        again[17 + t], again[s + 17 + t] = y.data()[0], y.data()[1]
    assert np.array_equal(again[17:s], first[17:s]) and np.array_equal(again[s + 17:], first[s + 17:])
    # a second forward() of earlier step nodes: the same rows, rotated at the same positions, to the same places
    for y, was in nodes[:3]:
        y.forward()
        assert np.array_equal(y.data(), was)
    assert cache.lens() == [s, s]
    cache.truncate([29, 29])
    last = _step(nk, tdev, mha, cache, _rows(xs, s, 29, 30)).data()
    assert np.array_equal(last[0], first[29]) and np.array_equal(last[1], first[s + 29])

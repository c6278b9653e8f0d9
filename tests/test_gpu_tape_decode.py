"""`nn::MultiheadAttention::forward_step` with an `nn::KvCache` through the tape (`_tape`): prefill then single-token steps, chunked
prefill, ragged prompts through `truncate`, `reset`, the idempotence of a node's forward() and the panics, on packed modules
(dh = 64, 32, 128), the generic head size 20, the unpacked module at dh = 5 and a module built from four handed-in Linears.

The oracle is tests/causal_oracle.py's causal module forward over ALL positions, in f64 and f32; the rule is
tests/test_gpu_tape_causal.py's (err_gpu <= max(2 * err_cpu32, 1e-6 * scale) against the f64 oracle, margins under `mha_decode:*`).
The stepped outputs must also agree with `mha.forward(x, B)` in eval mode within the same bound: the two paths differ in
summation order, so bit equality is not asked between them - it is asked between runs of the SAME path."""
import numpy as np
import pytest

import causal_oracle as CO

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
    record_margin("mha_decode:" + what.split("[")[0].strip(), err_gpu, err_cpu, 1e-6 * scale)
    print(what, "err_gpu %.3g err_cpu32 %.3g bound %.3g" % (err_gpu, err_cpu, max(2 * err_cpu, 1e-6 * scale)))
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


# name -> (d_model, heads, built from four handed-in Linears)
MODULES = {"packed dh 64": (128, 2, False), "packed dh 32": (128, 4, False), "packed dh 128": (256, 2, False),
           "generic dh 20": (40, 2, False), "unpacked dh 5": (10, 2, False), "four Linears dh 64": (128, 2, True)}


def _module(nk, tdev, name, p=0.1, batch_size=B):
    d, H, handed = MODULES[name]
    if handed:
        mha = nk.nn.MultiheadAttention(*(nk.nn.Linear(tdev, d, d, 11 + 2 * i) for i in range(4)), H, p)
    else:
        mha = nk.nn.MultiheadAttention(tdev, d, H, p, 3)
    assert mha.packed_qkv is (not handed and d % 4 == 0)
    mha.causal = True
    mha.drop.eval()
    return mha, d, H


def _rows(x, S, lo, hi, batch=B):
    return np.ascontiguousarray(np.concatenate([x[b * S + lo:b * S + hi] for b in range(batch)]))


def _step(nk, tdev, mha, cache, rows, batch=B):
    y = mha.forward_step(nk.from_ndarray(tdev, rows), batch, cache)
    assert y.history_len() == 1                                           # ONE forward node
    y.forward()
    return y


def _walk(nk, tdev, mha, cache, x, S, slices, batch=B):
    """x (batch*S, d) through forward_step in slices; -> the stacked (batch*S, d) outputs"""
    out, pos = np.zeros_like(x), 0
    for T in slices:
        assert cache.lens() == [pos] * batch
        got = _step(nk, tdev, mha, cache, _rows(x, S, pos, pos + T, batch), batch).data()
        for b in range(batch):
            out[b * S + pos:b * S + pos + T] = got[b * T:(b + 1) * T]
        pos += T
    assert pos == S and cache.lens() == [S] * batch
    return out


def _oracle(mha, x, H, batch, dt):
    W = [getattr(mha, n).weight.data().astype(dt) for n in "qkvo"]
    Bs = [getattr(mha, n).bias.data().astype(dt) for n in "qkvo"]
    S = x.shape[0] // batch
    out, _ = CO.mha_forward_backward(x.astype(dt), W[0], Bs[0], W[1], Bs[1], W[2], Bs[2], W[3], Bs[3], H, batch, 0.0,
                                     np.ones((batch * H, S, S), dt), np.zeros(x.shape, dt), causal=True)
    return out


_REF = {}


def _reference(nk, tdev, name, S):
    """(module, x, f64 reference, f32 reference): computed once per module and shared, never modified"""
    if (name, S) not in _REF:
        mha, d, H = _module(nk, tdev, name)
        x = rnd(0, (B * S, d), -1, 1)
        ref, ref32 = _oracle(mha, x, H, B, np.float64), _oracle(mha, x, H, B, np.float32)
        for a in (x, ref, ref32):
            a.setflags(write=False)
        _REF[(name, S)] = (mha, x, ref, ref32)
    return _REF[(name, S)]


@pytest.mark.parametrize("name", list(MODULES))
def test_prefill_then_steps_equal_the_causal_forward(nk, tdev, name):
    S, T0 = 72, 40
    mha, x, ref, ref32 = _reference(nk, tdev, name, S)
    d, H, _ = MODULES[name]
    cache = nk.nn.KvCache(tdev, B, H, d // H, 80)
    assert cache.capacity == 80 and cache.lens() == [0, 0]
    got = _walk(nk, tdev, mha, cache, x, S, [T0] + [1] * (S - T0))
    _check(got, ref, ref32, "prefill + steps [%s]" % name)
    full = mha.forward(nk.from_ndarray(tdev, x).requires_grad(), B)       # the whole prefix at once, eval mode
    full.forward()
    _check(full.data(), ref, ref32, "forward [%s]" % name)
    # the two device paths against each other, within the same bound
    scale = np.abs(ref).max()
    bound = max(2 * np.abs(ref32 - ref).max(), 1e-6 * scale)
    between = np.abs(got - full.data()).max()
    print("steps against forward [%s] distance %.3g bound %.3g" % (name, between, bound))
    assert between <= bound, (name, between, bound)


@pytest.mark.parametrize("name", list(MODULES))
def test_chunked_prefill(nk, tdev, name):
    """Slices of 16 + 16 + 8 (T > 1 at start > 0: the decode kernels over (b, h, t)), then steps."""
    S = 72
    mha, x, ref, ref32 = _reference(nk, tdev, name, S)
    d, H, _ = MODULES[name]
    cache = nk.nn.KvCache(tdev, B, H, d // H, S)                          # capacity = the final length exactly
    got = _walk(nk, tdev, mha, cache, x, S, [16, 16, 8] + [1] * (S - 40))
    _check(got, ref, ref32, "chunked prefill [%s]" % name)


@pytest.mark.parametrize("name", ["packed dh 64", "generic dh 20", "unpacked dh 5", "four Linears dh 64"])
def test_ragged_prompts(nk, tdev, name):
    """Right-padded prompts of true lengths (40, 23): prefill 40 rows of both, truncate to the true lengths, step 10 tokens.  Every
    sample equals the oracle over its own positions, and sample 1 equals, in bits, a run of sample 1 alone."""
    mha, d, H = _module(nk, tdev, name)
    lens, T0, steps = [40, 23], 40, 10
    prompt = rnd(1, (B * T0, d), -1, 1)                                   # rows 23 .. 39 of sample 1 are padding
    new = rnd(2, (B * steps, d), -1, 1)
    cache = nk.nn.KvCache(tdev, B, H, d // H, 64)
    pre = _step(nk, tdev, mha, cache, prompt).data()
    cache.truncate(lens)
    assert cache.lens() == lens
    outs = []
    for s in range(steps):
        outs.append(_step(nk, tdev, mha, cache, _rows(new, steps, s, s + 1)).data())
        assert cache.lens() == [l + s + 1 for l in lens]
    outs = np.stack(outs, axis=1)                                         # (B, steps, d)
    for b in range(B):
        xb = np.concatenate([prompt[b * T0:b * T0 + lens[b]], new[b * steps:(b + 1) * steps]])
        ref, ref32 = _oracle(mha, xb, H, 1, np.float64), _oracle(mha, xb, H, 1, np.float32)
        got = np.concatenate([pre[b * T0:b * T0 + lens[b]], outs[b]])
        _check(got, ref, ref32, "ragged [%s]" % name)
    alone = nk.nn.KvCache(tdev, 1, H, d // H, 64)
    _step(nk, tdev, mha, alone, np.ascontiguousarray(prompt[T0:T0 + lens[1]]), 1)
    for s in range(steps):
        one = _step(nk, tdev, mha, alone, np.ascontiguousarray(new[steps + s:steps + s + 1]), 1).data()
        assert np.array_equal(one[0], outs[1, s]), (name, s)
    with pytest.raises(RuntimeError):
        cache.truncate([lens[0] + steps + 1, 0])                          # a sample cannot grow
    with pytest.raises(RuntimeError):
        cache.truncate([1])


@pytest.mark.parametrize("name", ["packed dh 64", "generic dh 20"])
def test_reset_reproduces_the_first_run(nk, tdev, name):
    S = 30
    mha, d, H = _module(nk, tdev, name)
    x = rnd(4, (B * S, d), -1, 1)
    cache = nk.nn.KvCache(tdev, B, H, d // H, 32)
    slices = [12, 5] + [1] * 13
    first = _walk(nk, tdev, mha, cache, x, S, slices)
    cache.reset()
    assert cache.lens() == [0, 0]
    assert np.array_equal(_walk(nk, tdev, mha, cache, x, S, slices), first)
    cache.truncate([17, 17])                                              # roll back to the end of the second slice, decode again
    again = np.zeros_like(first)
    for s in range(13):
        got = _step(nk, tdev, mha, cache, _rows(x, S, 17 + s, 18 + s)).data()
        again[17 + s], again[S + 17 + s] = got[0], got[1]
    assert np.array_equal(again[17:S], first[17:S]) and np.array_equal(again[S + 17:], first[S + 17:])


@pytest.mark.parametrize("name", ["packed dh 64", "unpacked dh 5"])
def test_a_second_forward_of_a_node_changes_nothing(nk, tdev, name):
    mha, d, H = _module(nk, tdev, name)
    x = rnd(5, (B * 12, d), -1, 1)
    cache = nk.nn.KvCache(tdev, B, H, d // H, 16)
    pre = _step(nk, tdev, mha, cache, _rows(x, 12, 0, 8))
    y1 = _step(nk, tdev, mha, cache, _rows(x, 12, 8, 9))
    y2 = _step(nk, tdev, mha, cache, _rows(x, 12, 9, 10))
    a_pre, a1, a2 = pre.data(), y1.data(), y2.data()
    assert cache.lens() == [10, 10]
    y1.forward(); pre.forward(); y1.forward()                            # earlier nodes again: the same rows to the same places
    assert cache.lens() == [10, 10]
    assert np.array_equal(pre.data(), a_pre) and np.array_equal(y1.data(), a1)
    y2.forward()
    assert np.array_equal(y2.data(), a2)
    y3 = _step(nk, tdev, mha, cache, _rows(x, 12, 10, 11))                # and the cache is what an undisturbed run holds
    fresh = nk.nn.KvCache(tdev, B, H, d // H, 16)
    _step(nk, tdev, mha, fresh, _rows(x, 12, 0, 8))
    for s in (8, 9):
        _step(nk, tdev, mha, fresh, _rows(x, 12, s, s + 1))
    assert np.array_equal(_step(nk, tdev, mha, fresh, _rows(x, 12, 10, 11)).data(), y3.data())


def test_the_workspace_grows_with_the_slice(nk, tdev):
    """Sized for T = 1 at construction: a longer slice at start > 0 (decode kernels, more than one chunk of keys) arrives later."""
    from neuronika_amd import capi
    mha, d, H = _module(nk, tdev, "packed dh 64")
    ch = capi.attention_decode_chunk(d // H)
    S = ch + 24
    x = rnd(6, (B * S, d), -1, 1)
    cache = nk.nn.KvCache(tdev, B, H, d // H, 2 * ch)
    got = _walk(nk, tdev, mha, cache, x, S, [1, 1, ch - 2, 16, 8])       # T = 1 first, then longer slices crossing the chunk seam
    ref, ref32 = _oracle(mha, x, H, B, np.float64), _oracle(mha, x, H, B, np.float32)
    _check(got, ref, ref32, "growing slices")


def test_panics(nk, tdev):
    mha, d, H = _module(nk, tdev, "packed dh 64")
    x = nk.from_ndarray(tdev, rnd(7, (B * 4, d), -1, 1))
    cache = nk.nn.KvCache(tdev, B, H, d // H, 6)
    mha.forward_step(x, B, cache)
    assert cache.lens() == [4, 4]
    with pytest.raises(RuntimeError, match="capacity"):
        mha.forward_step(x, B, cache)                                     # 4 + 4 > 6
    assert cache.lens() == [4, 4]                                         # a refused step leaves the cache as it was
    cache.reset()
    mha.causal = False
    with pytest.raises(RuntimeError, match="causal"):
        mha.forward_step(x, B, cache)
    mha.causal = True
    mha.drop.train()
    with pytest.raises(RuntimeError, match="eval"):
        mha.forward_step(x, B, cache)                                     # p = 0.1 in train mode
    mha.drop.eval()
    with pytest.raises(RuntimeError, match="batch"):
        mha.forward_step(x, 4, cache)                                     # the cache was built for a batch of 2
    with pytest.raises(RuntimeError):
        mha.forward_step(x, B, nk.nn.KvCache(tdev, B, H + 2, d // H, 6))
    with pytest.raises(RuntimeError):
        mha.forward_step(x, B, nk.nn.KvCache(tdev, B, H, d // H // 2, 6))
    assert cache.lens() == [0, 0]
    quiet = nk.nn.MultiheadAttention(tdev, d, H, 0.0, 3)                  # p = 0 in train mode is not active dropout
    quiet.causal = True
    quiet.forward_step(x, B, cache)
    assert cache.lens() == [4, 4]
    with pytest.raises(RuntimeError):
        nk.nn.KvCache(tdev, B, H, d // H, 0)

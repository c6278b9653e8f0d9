"""Sliding-window attention through the tape (`_tape`): `nn::MultiheadAttention::window` on `forward()` (S <= window: the module
without a window, bit for bit; S > window: the node-by-node paths with the banded constant) and on `forward_step()` against linear
and rolling `nn::KvCache`s (prefill on the causal core or the window kernel, then single-token steps that wrap the ring many times).

The oracle is tests/window_oracle.py in f64 and f32; the rule is the one tests/test_gpu_tape_causal.py and tests/test_gpu_tape_gqa.py
hold the same quantities to (err_gpu <= max(2 * err_cpu32, 1e-6 * scale) against the f64 oracle, the bias gradients with the weight
gradient's magnitude as floor; margins under `attention_window:*`).  A rolling cache gives the bits of a linear one.
No existing decode tape test captures a step into a graph, so none is captured here either."""
import numpy as np
import pytest

import rope_oracle as RO
import window_oracle as WO

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
    record_margin("attention_window:tape " + what.split("[")[0].strip(), err_gpu, err_cpu, 1e-6 * scale)
    print(what, "err_gpu %.3g err_cpu32 %.3g bound %.3g" % (err_gpu, err_cpu, max(2 * err_cpu, 1e-6 * scale)))
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


def _params(mha, dt):
    return ([getattr(mha, n).weight.data().astype(dt) for n in "qkvo"], [getattr(mha, n).bias.data().astype(dt) for n in "qkvo"])


def _leaves(mha, X):
    return [X] + [getattr(getattr(mha, n), w) for n in "qkvo" for w in ("weight", "bias")]


def _module(nk, tdev, d, H, Hkv, window, use_rope, max_pos=160, seed=3):
    mha = nk.nn.MultiheadAttention(tdev, d, H, 0.0, seed, kv_heads=Hkv)
    mha.causal = True
    assert mha.window == 0                                                # off by default
    mha.window = window
    ro = None
    if use_rope:
        mha.rope = nk.nn.RotaryEmbedding(tdev, d // H, max_pos)
        ro = RO.make(max_pos, d // H)
    return mha, ro


def _rows(x, S, lo, hi, batch=B):
    return np.ascontiguousarray(np.concatenate([x[b * S + lo:b * S + hi] for b in range(batch)]))


# ---------------------------------------------------------------------------------------------------------------- forward()
@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("d,H,Hkv", [(128, 4, 4), (128, 4, 2), (80, 4, 2)])
def test_a_window_that_covers_the_sequence_is_the_module_without_it(nk, tdev, d, H, Hkv, use_rope):
    """S <= window: the same graph, the same launches - output and all gradients equal bit for bit (the packed fused core at
    Hkv == H, the strided core grouped, the node path at dh = 20)."""
    S = 24
    x, g = rnd(0, (B * S, d), -1, 1), rnd(5, (B * S, d), -1, 1)
    runs = []
    for window in (0, S, S + 9):
        mha, _ = _module(nk, tdev, d, H, Hkv, window, use_rope)
        X = nk.from_ndarray(tdev, x).requires_grad()
        y = mha.forward(X, B)
        y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
        runs.append([y.history_len()] + [y.data(), X.grad()] + [l.grad() for l in _leaves(mha, X)[1:]])
    for other in runs[1:]:
        assert other[0] == runs[0][0]
        for a, b in zip(runs[0][1:], other[1:]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("S,W", [(40, 7), (33, 32)])
@pytest.mark.parametrize("d,H,Hkv", [(128, 4, 4), (128, 4, 2), (64, 4, 2), (80, 4, 4)])
def test_banded_forward_equals_oracle(nk, tdev, d, H, Hkv, S, W, use_rope):
    """S > window: output and every parameter / input gradient against the banded oracle, on the strided node path and with split
    heads (dh = 32 and 16, which the fused core would take without a window, and dh = 20)."""
    mha, ro = _module(nk, tdev, d, H, Hkv, W, use_rope)
    x, g = rnd(0, (B * S, d), -1, 1), rnd(5, (B * S, d), -1, 1)
    refs = []
    for dt in (np.float64, np.float32):
        Wt, Bs = _params(mha, dt)
        refs.append(WO.mha_forward_backward(x.astype(dt), Wt[0], Bs[0], Wt[1], Bs[1], Wt[2], Bs[2], Wt[3], Bs[3], H, Hkv, B, 0.0,
                                            np.ones((B * H, S, S), dt), g.astype(dt), W, rope=ro))
    (ref, grads), (ref32, grads32) = refs
    for path, switches in {"nodes, strided": dict(), "nodes, split heads": dict(strided_heads=False)}.items():
        for key, value in switches.items():
            setattr(mha, key, value)
        X = nk.from_ndarray(tdev, x).requires_grad()
        y = mha.forward(X, B)
        for leaf in _leaves(mha, X):
            leaf.zero_grad()
        y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
        what = " [d %d H %d Hkv %d S %d W %d, %s, %s]" % (d, H, Hkv, S, W, path, "rope" if use_rope else "plain")
        assert np.isfinite(y.data()).all() and np.isfinite(X.grad()).all(), what
        _check(y.data(), ref, ref32, "out" + what)
        _check(X.grad(), grads["x"], grads32["x"], "dx" + what)
        for nme in "qkvo":
            _check(getattr(mha, nme).weight.grad(), grads["w" + nme], grads32["w" + nme], "dw" + nme + what)
            _check(getattr(mha, nme).bias.grad(), grads["b" + nme], grads32["b" + nme], "db" + nme + what, np.abs(grads["w" + nme]).max())
        for key in switches:
            setattr(mha, key, True)


# ---------------------------------------------------------------------------------------------------------------- forward_step()
def _step(nk, tdev, mha, cache, rows, batch=B):
    y = mha.forward_step(nk.from_ndarray(tdev, rows), batch, cache)
    assert y.history_len() == 1                                           # ONE forward node
    y.forward()
    return y.data()


def _walk(nk, tdev, mha, cache, x, S, slices, batch=B):
    out, pos = np.zeros_like(x), 0
    for T in slices:
        assert cache.lens() == [pos] * batch
        got = _step(nk, tdev, mha, cache, _rows(x, S, pos, pos + T, batch), batch)
        for b in range(batch):
            out[b * S + pos:b * S + pos + T] = got[b * T:(b + 1) * T]
        pos += T
    assert pos == S and cache.lens() == [S] * batch
    return out


def _stepped_oracle(mha, x, S, slices, cap, batch, dt, ro):
    """tests/window_oracle.py's mha_step over the same slices, on a RING of (batch, kv_heads, cap, dh)"""
    Wt, Bs = _params(mha, dt)
    dh = mha.d_model // mha.heads
    kc, vc = np.full((batch, mha.kv_heads, cap, dh), np.nan, dt), np.full((batch, mha.kv_heads, cap, dh), np.nan, dt)
    out, start = np.zeros((batch * S, mha.d_model), dt), np.zeros(batch, dtype=np.int64)
    for T in slices:
        pos = int(start[0])
        got, start = WO.mha_step(_rows(x, S, pos, pos + T, batch).astype(dt), Wt, Bs, mha.heads, mha.kv_heads, kc, vc, start, T, mha.window,
                                 ring=True, rope=ro)
        for b in range(batch):
            out[b * S + pos:b * S + pos + T] = got[b * T:(b + 1) * T]
    return out


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("T0", [5, 10], ids=["prefill in the window", "prefill beyond the window"])
@pytest.mark.parametrize("d,H,Hkv", [(128, 4, 4), (128, 4, 2), (80, 4, 2)])
def test_prefill_then_steps_on_a_rolling_cache(nk, tdev, d, H, Hkv, T0, use_rope):
    """W = 7.  A prefill of 5 rows (the causal core at dh = 32, then the ring append) or 10 rows (the window kernel over T = 10),
    then 2 * capacity + 1 single-token steps on a rolling cache of the smallest legal capacity W + T0 - 1: every slot is overwritten
    at least twice.  Rows against the stepped ring oracle, the banded full-sequence oracle, and forward() over the whole sequence;
    the same walk on a linear cache gives the same bits."""
    W = 7
    cap = W + T0 - 1
    steps = 2 * cap + 1
    S = T0 + steps
    slices = [T0] + [1] * steps
    mha, ro = _module(nk, tdev, d, H, Hkv, W, use_rope)
    x = rnd(0, (B * S, d), -1, 1)
    rolling = nk.nn.KvCache(tdev, B, Hkv, d // H, cap, rolling=True)
    assert rolling.rolling is True and rolling.capacity == cap and rolling.high_water() == [0] * B
    got = _walk(nk, tdev, mha, rolling, x, S, slices)
    assert rolling.lens() == [S] * B and rolling.high_water() == [S] * B and S > 2 * cap
    linear = nk.nn.KvCache(tdev, B, Hkv, d // H, S)
    assert linear.rolling is False
    assert np.array_equal(_walk(nk, tdev, mha, linear, x, S, slices), got)
    what = "[d %d Hkv %d T0 %d %s]" % (d, Hkv, T0, "rope" if use_rope else "plain")
    stepped, stepped32 = (_stepped_oracle(mha, x, S, slices, cap, B, dt, ro) for dt in (np.float64, np.float32))
    _check(got, stepped, stepped32, "steps " + what)
    refs = []
    for dt in (np.float64, np.float32):
        Wt, Bs = _params(mha, dt)
        refs.append(WO.mha_forward(x.astype(dt), Wt, Bs, H, Hkv, B, W, rope=ro))
    ref, ref32 = refs
    assert np.abs(stepped - ref).max() <= 1e-9                            # the two oracles agree
    _check(got, ref, ref32, "steps against the banded forward " + what)
    full = mha.forward(nk.from_ndarray(tdev, x).requires_grad(), B)
    full.forward()
    _check(full.data(), ref, ref32, "forward " + what)
    bound = max(2 * np.abs(ref32 - ref).max(), 1e-6 * np.abs(ref).max())
    between = np.abs(got - full.data()).max()
    print("steps against forward %s distance %.3g bound %.3g" % (what, between, bound))
    assert between <= bound, (what, between, bound)


def test_chunked_prefill_on_a_rolling_cache(nk, tdev):
    """A prompt longer than capacity - window + 1 goes in slices: 4 + 4 + 3 rows at W = 7 on a ring of 10 slots, then steps."""
    d, H, Hkv, W, cap = 128, 4, 2, 7, 10
    slices = [4, 4, 3] + [1] * 14
    S = sum(slices)
    mha, ro = _module(nk, tdev, d, H, Hkv, W, True)
    x = rnd(1, (B * S, d), -1, 1)
    got = _walk(nk, tdev, mha, nk.nn.KvCache(tdev, B, Hkv, d // H, cap, rolling=True), x, S, slices)
    stepped, stepped32 = (_stepped_oracle(mha, x, S, slices, cap, B, dt, ro) for dt in (np.float64, np.float32))
    _check(got, stepped, stepped32, "chunked prefill")


@pytest.mark.parametrize("d,H,Hkv", [(128, 4, 2), (80, 4, 4)])
def test_ragged_prompts_and_roll_back_on_a_rolling_cache(nk, tdev, d, H, Hkv):
    """Right-padded prompts of true lengths (10, 6) at W = 7 on a ring of 16 slots: prefill, truncate, 30 steps; every sample
    equals the banded oracle over its own positions.  Then roll-back: two tokens back is allowed (the window of the next query
    still lies in the ring), ten tokens back is refused; reset() clears the marks."""
    W, cap, T0, steps, lens = 7, 16, 10, 30, [10, 6]
    mha, ro = _module(nk, tdev, d, H, Hkv, W, True)
    prompt, new = rnd(1, (B * T0, d), -1, 1), rnd(2, (B * steps, d), -1, 1)
    cache = nk.nn.KvCache(tdev, B, Hkv, d // H, cap, rolling=True)
    pre = _step(nk, tdev, mha, cache, prompt)
    cache.truncate(lens)                                                  # T0 <= capacity: nothing was overwritten yet
    assert cache.lens() == lens and cache.high_water() == [T0] * B
    outs = np.stack([_step(nk, tdev, mha, cache, _rows(new, steps, s, s + 1)) for s in range(steps)], axis=1)   # (B, steps, d)
    after = [l + steps for l in lens]
    assert cache.lens() == after and cache.high_water() == after
    for b in range(B):
        xb = np.concatenate([prompt[b * T0:b * T0 + lens[b]], new[b * steps:(b + 1) * steps]])
        got = np.concatenate([pre[b * T0:b * T0 + lens[b]], outs[b]])
        refs = []
        for dt in (np.float64, np.float32):
            Wt, Bs = _params(mha, dt)
            refs.append(WO.mha_forward(xb.astype(dt), Wt, Bs, H, Hkv, 1, W, rope=ro))
        _check(got, refs[0], refs[1], "ragged [d %d sample %d]" % (d, b))
    with pytest.raises(RuntimeError, match="overwritten"):
        cache.truncate([l - 10 for l in after])                           # max(0, l - 10 - 7) < high - 16
    assert cache.lens() == after                                          # a refused truncate changes nothing
    with pytest.raises(RuntimeError, match="asked for"):
        cache.truncate([l + 1 for l in after])
    back = [l - 2 for l in after]
    cache.truncate(back)                                                  # l - 2 - 7 >= high - 16
    assert cache.lens() == back and cache.high_water() == after
    again = np.stack([_step(nk, tdev, mha, cache, _rows(new, steps, s, s + 1)) for s in (steps - 2, steps - 1)], axis=1)
    assert np.array_equal(again, outs[:, steps - 2:])                     # the same tokens at the same positions: the same bits
    cache.reset()
    assert cache.lens() == [0] * B and cache.high_water() == [0] * B
    assert np.array_equal(_step(nk, tdev, mha, cache, prompt), pre)


@pytest.mark.parametrize("rolling", [False, True], ids=["linear", "rolling"])
def test_a_prefill_the_core_takes_asks_for_no_scratch(nk, tdev, rolling):
    """A fresh prefill with T <= window runs the causal core, which reads no decode scratch: the cache's workspace stays what the
    constructor sized for one row, exactly as with window = 0 - while the window is still remembered for truncate().  Node builds
    only (nothing is run) at T = 65536, where a T-row window scratch would be 2 * 65536 * 4 * 129 * 34 = 2.3e9 floats: beyond 31
    bits, a panic if it were asked for.  A small prefill is then run and stepped to show the path is the core's."""
    d, H, Hkv, T = 128, 4, 4, 65536
    dh = d // H
    x = nk.from_ndarray(tdev, np.zeros((B * T, d), np.float32))
    plain, _ = _module(nk, tdev, d, H, Hkv, 0, False)
    base = nk.nn.KvCache(tdev, B, Hkv, dh, T)
    before = base.workspace_floats()
    assert before > 0
    plain.forward_step(x, B, base)
    assert base.workspace_floats() == before                              # the parent's behaviour: the core path allocates none
    mha, _ = _module(nk, tdev, d, H, Hkv, T, False)
    cache = nk.nn.KvCache(tdev, B, Hkv, dh, T, rolling=rolling)
    assert cache.workspace_floats() == before
    mha.forward_step(x, B, cache)                                         # T <= window, fresh: the core; no panic, no scratch
    assert cache.lens() == [T] * B and cache.workspace_floats() == before
    # the window was remembered all the same: on a rolling cache truncate() judges by it
    W = 7
    small, _ = _module(nk, tdev, d, H, Hkv, W, False)
    ring = nk.nn.KvCache(tdev, B, Hkv, dh, 16, rolling=True)
    size0 = ring.workspace_floats()
    rows = rnd(3, (B * 6, d), -1, 1)
    pre = _step(nk, tdev, small, ring, rows)                              # T = 6 <= W: the core
    assert ring.workspace_floats() == size0
    for s in range(20):
        _step(nk, tdev, small, ring, rnd(10 + s, (B, d), -1, 1))
    assert ring.workspace_floats() >= size0 and ring.high_water() == [26] * B
    with pytest.raises(RuntimeError, match="a window of 7"):
        ring.truncate([16] * B)                                           # max(0, 16 - 7) < 26 - 16
    ring.truncate([17] * B)
    ref = nk.nn.KvCache(tdev, B, Hkv, dh, 16)
    assert np.array_equal(_step(nk, tdev, small, ref, rows), pre)         # and the prefill's bits are the linear cache's


def test_panics(nk, tdev):
    d, H, Hkv, W = 128, 4, 2, 7
    dh = d // H
    mha, _ = _module(nk, tdev, d, H, Hkv, W, False)
    x = lambda T: nk.from_ndarray(tdev, rnd(7, (B * T, d), -1, 1))
    # a window needs the causal rule, on both entry points
    mha.causal = False
    with pytest.raises(RuntimeError, match="causal"):
        mha.forward(x(12).requires_grad(), B)
    with pytest.raises(RuntimeError, match="causal"):
        mha.forward_step(x(1), B, nk.nn.KvCache(tdev, B, Hkv, dh, 16, rolling=True))
    mha.causal = True
    mha.window = -1
    with pytest.raises(RuntimeError, match="window"):
        mha.forward(x(12).requires_grad(), B)
    with pytest.raises(RuntimeError, match="window"):
        mha.forward_step(x(1), B, nk.nn.KvCache(tdev, B, Hkv, dh, 16))
    # a rolling cache needs a window
    mha.window = 0
    cache = nk.nn.KvCache(tdev, B, Hkv, dh, 16, rolling=True)
    with pytest.raises(RuntimeError, match="rolling cache.*window > 0"):
        mha.forward_step(x(1), B, cache)
    assert cache.lens() == [0] * B                                        # a refused step advances nothing
    # window + T - 1 <= capacity for a step the window kernel takes; the message tells the caller to chunk the prompt
    mha.window = W
    with pytest.raises(RuntimeError, match=r"window \+ T - 1 <= capacity.*chunk the prompt"):
        mha.forward_step(x(11), B, cache)                                 # T = 11 > W: 7 + 11 - 1 > 16
    mha.forward_step(x(4), B, cache)                                      # a fresh prefill inside the window: fine
    with pytest.raises(RuntimeError, match=r"window \+ T - 1 <= capacity"):
        mha.forward_step(x(11), B, cache)                                 # not fresh any more
    with pytest.raises(RuntimeError, match="chunk the prompt"):
        mha.forward_step(x(17), B, cache)                                 # T > capacity
    assert cache.lens() == [4] * B
    mha.forward_step(x(10), B, cache)                                     # 7 + 10 - 1 == 16
    assert cache.lens() == [14] * B
    # a linear cache overflows as without a window
    linear = nk.nn.KvCache(tdev, B, Hkv, dh, 8)
    mha.forward_step(x(8), B, linear)
    with pytest.raises(RuntimeError, match="capacity"):
        mha.forward_step(x(1), B, linear)
    # rope on a rolling cache: the capacity may be far below max_pos or above it; the POSITIONS must stay inside the table
    mha.rope = nk.nn.RotaryEmbedding(tdev, dh, 12)
    rolling = nk.nn.KvCache(tdev, B, Hkv, dh, 16, rolling=True)           # capacity 16 > max_pos 12: no panic for that
    mha.forward_step(x(6), B, rolling)
    mha.forward_step(x(6), B, rolling)
    assert rolling.lens() == [12] * B
    with pytest.raises(RuntimeError, match="rope's table of 12"):
        mha.forward_step(x(1), B, rolling)
    with pytest.raises(RuntimeError, match="rope's table"):
        mha.forward_step(x(1), B, nk.nn.KvCache(tdev, B, Hkv, dh, 16))    # the linear cache keeps its guard: capacity > max_pos

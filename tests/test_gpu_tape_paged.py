"""`nn::MultiheadAttention::forward_step` over an `nn::PagedKvCache` through the tape (`_tape`), on a grouped-query module with rope
(d_model 128, 4 query heads over 2 kv heads of 32: the vector kernels, chunk C = 512), page 16.

Everything is asked in BITS against the same module stepped over an `nn::KvCache`: the paged kernels are the contiguous bodies behind a
table lookup, the prefill takes the same causal core, and a row's projections do not depend on the other rows of a step (what
tests/test_gpu_tape_decode.py's ragged test already relies on).  Generation over 2C + 5 steps with the two sequences' pages
interleaved; continuous batching (a sequence leaves, a new prompt takes its id, `seqs` changes order) against each sequence's solo
run; a fork that diverges inside a shared page; a windowed layer that releases the pages behind its window every step against the
rolling cache; and the panics, which leave the table as it was."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, H, HKV, DH, PAGE = 128, 4, 2, 32, 16
MAX_POS = 1100


@pytest.fixture(scope="module")
def nk():
    import neuronika_amd
    return neuronika_amd.tape


@pytest.fixture(scope="module")
def tdev(nk):
    return nk.Device(0)


def rnd(seed, shape, lo=-1.0, hi=1.0):
    a = np.random.default_rng(seed).random(shape, dtype=np.float32)
    return np.asarray(a * np.float32(hi - lo) + np.float32(lo), dtype=np.float32).reshape(shape)


def _module(nk, tdev, window=0):
    mha = nk.nn.MultiheadAttention(tdev, D, H, 0.0, 3, kv_heads=HKV)
    mha.causal = True
    mha.drop.eval()
    mha.window = window
    mha.rope = nk.nn.RotaryEmbedding(tdev, DH, MAX_POS)
    return mha


def _step(nk, tdev, mha, cache, rows, who):
    """who: the batch of a KvCache, or the sequence ids of a PagedKvCache"""
    y = mha.forward_step(nk.from_ndarray(tdev, np.ascontiguousarray(rows)), who, cache)
    assert y.history_len() == 1                                           # ONE forward node
    y.forward()
    return y.data()


def _solo(nk, tdev, mha, slices, capacity):
    """one sequence alone on a contiguous cache: the outputs of every slice"""
    cache = nk.nn.KvCache(tdev, 1, HKV, DH, capacity)
    return [_step(nk, tdev, mha, cache, rows, 1) for rows in slices]


def test_generation_equals_the_contiguous_cache_bit_for_bit(nk, tdev):
    from neuronika_amd import capi
    C = capi.attention_decode_chunk(DH)
    T0, steps, B = 7, 2 * C + 5, 2
    total = T0 + steps
    assert total <= MAX_POS
    mha = _module(nk, tdev)
    max_pages = (total + PAGE - 1) // PAGE + 1
    paged = nk.nn.PagedKvCache(tdev, B * max_pages + 4, PAGE, HKV, DH, B, max_pages)
    flat = nk.nn.KvCache(tdev, B, HKV, DH, total)
    x = rnd(1, (B * T0, D))
    assert np.array_equal(_step(nk, tdev, mha, paged, x, [0, 1]), _step(nk, tdev, mha, flat, x, B))
    for s in range(steps):
        x = rnd(10 + s, (B, D))
        got, want = _step(nk, tdev, mha, paged, x, [0, 1]), _step(nk, tdev, mha, flat, x, B)
        assert np.array_equal(got, want), (s, np.abs(got - want).max())
    assert paged.lens() == [total, total] == flat.lens()
    assert paged.pages(0)[:3] == [0, 2, 4] and paged.pages(1)[:3] == [1, 3, 5]             # interleaved between the sequences
    assert len(paged.free_pages()) == paged.num_pages - 2 * ((total + PAGE - 1) // PAGE)


def test_continuous_batching_equals_every_sequences_solo_run(nk, tdev):
    """Sequences a (id 0) and b (id 1) run together; b finishes and is released; a new prompt c takes id 1 and the batch goes on as
    seqs = [1, 0]."""
    mha = _module(nk, tdev)
    Ta, Tc, first, second = 6, 20, 5, 21
    xa = [rnd(1, (Ta, D))] + [rnd(100 + s, (1, D)) for s in range(first + second)]
    xb = [rnd(2, (Ta, D))] + [rnd(200 + s, (1, D)) for s in range(first)]
    xc = [rnd(3, (Tc, D))] + [rnd(300 + s, (1, D)) for s in range(second)]
    cache = nk.nn.PagedKvCache(tdev, 9, PAGE, HKV, DH, 3, 4)
    got = {"a": [], "b": [], "c": []}
    out = _step(nk, tdev, mha, cache, np.concatenate([xa[0], xb[0]]), [0, 1])
    got["a"].append(out[:Ta]); got["b"].append(out[Ta:])
    for s in range(first):
        out = _step(nk, tdev, mha, cache, np.concatenate([xa[1 + s], xb[1 + s]]), [0, 1])
        got["a"].append(out[:1]); got["b"].append(out[1:])
    held = cache.pages(1)
    cache.release(1)
    assert cache.lens()[1] == 0 and cache.pages(1) == [] and all(cache.refcount(p) == 0 for p in held)
    got["c"].append(_step(nk, tdev, mha, cache, xc[0], [1]))             # the new prompt: a fresh prefill of its own
    assert cache.pages(1)[0] == held[0]                                   # ... into the pages b gave back
    for s in range(second):
        out = _step(nk, tdev, mha, cache, np.concatenate([xc[1 + s], xa[1 + first + s]]), [1, 0])
        got["c"].append(out[:1]); got["a"].append(out[1:])
    assert cache.lens() == [Ta + first + second, Tc + second, 0]
    for name, xs in (("a", xa), ("b", xb), ("c", xc)):
        want = _solo(nk, tdev, mha, xs, 64)
        assert len(want) == len(got[name])
        for s, (g, w) in enumerate(zip(got[name], want)):
            assert np.array_equal(g, w), (name, s, np.abs(g - w).max())


def test_fork_copies_one_page_and_both_continue_as_their_independent_runs(nk, tdev):
    mha = _module(nk, tdev)
    T0, steps = 20, 15                                                    # the fork point is inside the second page; 35 positions: a third
    prompt = rnd(1, (T0, D))
    xp, xc = [rnd(100 + s, (1, D)) for s in range(steps)], [rnd(200 + s, (1, D)) for s in range(steps)]
    cache = nk.nn.PagedKvCache(tdev, 8, PAGE, HKV, DH, 2, 4)
    _step(nk, tdev, mha, cache, prompt, [0])
    parent_pages = cache.pages(0)
    assert parent_pages == [0, 1]
    k0, v0 = cache.k_data()[parent_pages], cache.v_data()[parent_pages]
    cache.fork(0, 1)
    assert cache.row(1) == cache.row(0) and cache.lens() == [T0, T0] and [cache.refcount(p) for p in parent_pages] == [2, 2]
    free = len(cache.free_pages())
    got_p, got_c = [], []
    for s in range(steps):
        out = _step(nk, tdev, mha, cache, np.concatenate([xc[s], xp[s]]), [1, 0])       # the child first: it takes the copy
        got_c.append(out[:1]); got_p.append(out[1:])
        if s == 0:                                                        # exactly one page was copied: the partial one, for the child
            assert cache.pages(0) == parent_pages and cache.pages(1) == [0, 2]
            assert len(cache.free_pages()) == free - 1 and [cache.refcount(p) for p in (0, 1, 2)] == [2, 1, 1]
    assert cache.pages(0) == [0, 1, 4] and cache.pages(1) == [0, 2, 3]    # the third pages, the child first again
    # the parent's pages up to the fork point did not change
    k1, v1 = cache.k_data()[parent_pages], cache.v_data()[parent_pages]
    assert np.array_equal(k0[0], k1[0]) and np.array_equal(v0[0], v1[0])
    assert np.array_equal(k0[1][:, :T0 - PAGE], k1[1][:, :T0 - PAGE]) and np.array_equal(v0[1][:, :T0 - PAGE], v1[1][:, :T0 - PAGE])
    for name, got, xs in (("parent", got_p, xp), ("child", got_c, xc)):
        want = _solo(nk, tdev, mha, [prompt] + xs, 64)[1:]
        for s, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (name, s, np.abs(g - w).max())


def test_a_windowed_layer_releases_behind_and_equals_the_rolling_cache(nk, tdev):
    from neuronika_amd import capi
    C = capi.attention_decode_chunk(DH)
    W, T0, B = 40, 8, 2
    steps = C + 30                                                        # the window crosses the first chunk seam on the way
    mha = _module(nk, tdev, window=W)
    total = T0 + steps
    max_pages = (total + PAGE - 1) // PAGE
    held = (W + PAGE - 2) // PAGE + 1                                     # pages a window of W positions can touch
    num_pages = B * (held + 1)                                            # far fewer than B * max_pages: the memory is bounded by the window
    assert num_pages < B * max_pages // 4
    paged = nk.nn.PagedKvCache(tdev, num_pages, PAGE, HKV, DH, B, max_pages)
    ring = nk.nn.KvCache(tdev, B, HKV, DH, W + T0, rolling=True)
    x = rnd(1, (B * T0, D))
    assert np.array_equal(_step(nk, tdev, mha, paged, x, [0, 1]), _step(nk, tdev, mha, ring, x, B))
    for s in range(steps):
        for b in range(B):                                                # the next row reads from position len + 1 - W on
            paged.release_behind(b, max(0, paged.lens()[b] + 1 - W))
        assert len(paged.free_pages()) >= num_pages - B * held, (s, paged.free_pages())
        x = rnd(10 + s, (B, D))
        got, want = _step(nk, tdev, mha, paged, x, [0, 1]), _step(nk, tdev, mha, ring, x, B)
        assert np.array_equal(got, want), (s, np.abs(got - want).max())
    assert paged.lens() == [total, total] and paged.behind(0) == (total - W) // PAGE * PAGE      # the last release, at length total - 1
    assert all(p == -1 for p in paged.row(0)[:paged.behind(0) // PAGE])


def test_the_panics_leave_the_table_as_it_was(nk, tdev):
    mha = _module(nk, tdev)
    cache = nk.nn.PagedKvCache(tdev, 3, PAGE, HKV, DH, 2, 4)
    cache.reserve([0], 2 * PAGE)
    cache.reserve([1], PAGE)

    def state():
        return cache.lens(), [cache.row(s) for s in range(2)], cache.free_pages(), [cache.refcount(p) for p in range(3)]

    before = state()
    assert before[2] == []
    x = nk.from_ndarray(tdev, rnd(1, (2, D)))
    with pytest.raises(RuntimeError, match="pages needed"):
        mha.forward_step(x, [0, 1], cache)                                # out of pages
    assert state() == before
    with pytest.raises(RuntimeError, match="listed twice"):
        mha.forward_step(x, [1, 1], cache)
    with pytest.raises(RuntimeError, match="outside"):
        mha.forward_step(x, [0, 2], cache)
    cache.truncate(1, 3)
    with pytest.raises(RuntimeError, match="max_pages"):
        mha.forward_step(nk.from_ndarray(tdev, rnd(1, (4 * PAGE, D))), [1], cache)     # 3 + 64 positions: a fifth page
    cache.truncate(0, PAGE + 1)
    cache.release_behind(0, PAGE)
    now = state()
    with pytest.raises(RuntimeError, match="window > 0"):
        mha.forward_step(nk.from_ndarray(tdev, rnd(1, (1, D))), [0], cache)            # pages released behind, a layer without a window
    mha.window = PAGE
    with pytest.raises(RuntimeError, match="would read below"):
        mha.forward_step(nk.from_ndarray(tdev, rnd(1, (1, D))), [0], cache)            # row 0 reads from position 2 on, 16 is the first held
    mha.window = 2
    rope = mha.rope
    mha.rope = nk.nn.RotaryEmbedding(tdev, DH, PAGE + 1)
    with pytest.raises(RuntimeError, match="rope's table"):
        mha.forward_step(nk.from_ndarray(tdev, rnd(1, (1, D))), [0], cache)
    mha.rope = rope
    assert state() == now
    out = mha.forward_step(nk.from_ndarray(tdev, rnd(1, (1, D))), [0], cache)          # and with a window inside what is held, it runs
    out.forward()
    assert out.data().shape == (1, D) and cache.lens()[0] == PAGE + 2    # (position 16 was reserved, never written: no value is asked)

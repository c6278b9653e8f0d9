"""GPU parity of incremental decoding through the C ABI: nk_kv_cache_append (a bit-exact transposing copy into the (B, H, cap, dh)
caches) and nk_attention_decode_fwd (single-query attention over the caches, split-KV partials merged in chunk order) against
tests/decode_oracle.py.

Tolerance: tests/test_gpu_attention_causal.py's rule - kernels and f32 oracle both measured against the f64 oracle; pass iff
err_gpu <= max(2 * err_cpu32, 1e-6 * scale), scale = max(|ref|max, |v|max) (SURVEY.md 8c ii), margins recorded under
`attention_decode:*`.

Bit contracts checked here (include/neuronika_hip.h): the bits of o for (b, h, t) depend on that problem's q, its n keys / values
and scale only - not on what the cache holds at positions >= n (NaN, 1e30), the other samples, B, cap, or the run."""
import numpy as np
import pytest

import decode_oracle as DO

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


def capi():
    from neuronika_amd import capi as c
    return c


def rnd(seed, shape, lo, hi):
    a = np.random.default_rng(seed).random(shape, dtype=np.float32)
    return np.asarray(a * np.float32(hi - lo) + np.float32(lo), dtype=np.float32)


def _check(got, want64, want32, vmax, what):
    scale = max(np.abs(want64).max(), vmax)
    err_gpu, err_cpu = np.abs(got - want64).max(), np.abs(want32 - want64).max()
    from conftest import record_margin
    record_margin("attention_decode:" + what.split("[")[0].strip(), err_gpu, err_cpu, 1e-6 * scale)
    print(what, "err_gpu %.3g err_cpu32 %.3g bound %.3g" % (err_gpu, err_cpu, max(2 * err_cpu, 1e-6 * scale)))
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


def _scale(dh):
    return float(np.float32(1.0 / np.sqrt(dh)))


def _decode(dev, q, kc, vc, start, T, ldq=None, q_offset=0):
    """nk_attention_decode_fwd on host arrays: q (rows, ldq) or (B*T, H*dh), kc / vc (B, H, cap, dh) -> (B*T, H*dh)"""
    c = capi()
    B, H, cap, dh = kc.shape
    Q, Kc, Vc, S = dev.array(q), dev.array(kc), dev.array(vc), dev.int_array(start)
    out = dev.full((B * T, H * dh), np.nan)
    ws = dev.full((c.attention_decode_workspace(B, T, H, dh, cap),), np.nan)
    c.attention_decode_fwd(dev, Q.view_offset(q_offset) if q_offset else Q, ldq or H * dh, Kc, Vc, S, out, ws, B, T, H, dh, cap, _scale(dh))
    return out.numpy()


def _oracles(q, kc, vc, start, T):
    dh = kc.shape[3]
    return tuple(DO.decode_forward(q.astype(dt), kc.astype(dt), vc.astype(dt), start, T, _scale(dh)) for dt in (np.float64, np.float32))


def _vmax(vc, start, T):
    return max(float(np.abs(vc[b, :, :min(int(s) + T, vc.shape[2])]).max()) for b, s in enumerate(start))


# ---- append ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,H,dh", [(2, 1, 3, 64), (3, 4, 2, 32), (2, 5, 2, 20), (2, 3, 2, 5), (1, 40, 4, 128)])
@pytest.mark.parametrize("packed", [True, False])
def test_append_is_a_bit_exact_transposing_copy(dev, B, T, H, dh, packed):
    c = capi()
    d, cap = H * dh, 50
    start = np.array([7, 0, 3][:B], dtype=np.int32)
    if T == 40:
        start[:] = 10
    kc0, vc0 = np.full((B, H, cap, dh), SENTINEL, np.float32), np.full((B, H, cap, dh), -SENTINEL, np.float32)
    Kc, Vc, S = dev.array(kc0), dev.array(vc0), dev.int_array(start)
    if packed:                                                           # K and V are column blocks of one (B*T, 3d) matrix
        qkv = rnd(1, (B * T, 3 * d), -1, 1)
        QKV = dev.array(qkv)
        k, v = qkv[:, d:2 * d], qkv[:, 2 * d:]
        c.kv_cache_append(dev, Kc, Vc, QKV.view_offset(d), QKV.view_offset(2 * d), 3 * d, S, B, T, H, dh, cap)
    else:
        k, v = rnd(2, (B * T, d), -1, 1), rnd(3, (B * T, d), -1, 1)
        c.kv_cache_append(dev, Kc, Vc, dev.array(k), dev.array(v), d, S, B, T, H, dh, cap)
    DO.append(kc0, vc0, k, v, start, T)                                  # every other element keeps its sentinel
    assert np.array_equal(Kc.numpy(), kc0) and np.array_equal(Vc.numpy(), vc0)
    assert np.count_nonzero(kc0 != SENTINEL) == B * T * H * dh


@pytest.mark.parametrize("dh", [64, 5])
def test_append_drops_rows_past_the_capacity(dev, dh):
    c = capi()
    B, T, H, cap = 2, 4, 2, 6
    start = np.array([4, 6], dtype=np.int32)                             # sample 0 keeps rows 0, 1; sample 1 keeps none
    k, v = rnd(1, (B * T, H * dh), -1, 1), rnd(2, (B * T, H * dh), -1, 1)
    kc0, vc0 = np.full((B, H, cap, dh), SENTINEL, np.float32), np.full((B, H, cap, dh), SENTINEL, np.float32)
    guard = 64                                                           # the caches sit inside a larger allocation: nothing around them moves
    big_k, big_v = dev.full((guard + kc0.size + guard,), SENTINEL), dev.full((guard + vc0.size + guard,), SENTINEL)
    c.kv_cache_append(dev, big_k.view_offset(guard), big_v.view_offset(guard), dev.array(k), dev.array(v), H * dh, dev.int_array(start), B, T, H, dh, cap)
    DO.append(kc0, vc0, k, v, start, T)
    for big, want in ((big_k, kc0), (big_v, vc0)):
        got = big.numpy()
        assert np.all(got[:guard] == SENTINEL) and np.all(got[-guard:] == SENTINEL)
        assert np.array_equal(got[guard:-guard].reshape(want.shape), want)
    assert np.all(kc0[1] == SENTINEL) and np.count_nonzero(kc0[0] != SENTINEL) == 2 * H * dh


# ---- decode against the oracle ------------------------------------------------------------------------------------------------------
def _lengths(dh):
    ch = capi().attention_decode_chunk(dh)
    return [1, 2, 3, ch - 1, ch, ch + 1, 2 * ch - 1, 2 * ch + 1, 3 * ch + 7, 1000]


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("B,H", [(1, 1), (2, 3), (3, 2)])
@pytest.mark.parametrize("dh", [32, 64, 128, 20, 5])
def test_decode_equals_oracle(dev, dh, B, H, T):
    """Every length in `_lengths` is what the FIRST new row of some sample reads (start = n - 1; the later rows of a T = 4 slice
    read n + 1 .. n + 3 keys, crossing the seams again); samples of one call take different lengths (ragged starts); each call runs
    with the capacity equal to the longest length and well above it.  The new rows reach the cache through nk_kv_cache_append
    from a packed (B*T, 3d) projection, which the queries are read from in place (ldq = 3d)."""
    c = capi()
    d, ch = H * dh, c.attention_decode_chunk(dh)
    ns = _lengths(dh)
    ns = ns + ns[:(-len(ns)) % B]                                        # whole groups of B
    for g0 in range(0, len(ns), B):
        group = ns[g0:g0 + B]
        start = np.array([n - 1 for n in group], dtype=np.int32)
        for cap in (max(group) - 1 + T, max(group) - 1 + T + 2 * ch + 13):
            kc, vc = rnd(10 + g0, (B, H, cap, dh), -1, 1), rnd(20 + g0, (B, H, cap, dh), -1, 1)
            qkv = rnd(30 + g0, (B * T, 3 * d), -1, 1)
            Kc, Vc, S, QKV = dev.array(kc), dev.array(vc), dev.int_array(start), dev.array(qkv)
            c.kv_cache_append(dev, Kc, Vc, QKV.view_offset(d), QKV.view_offset(2 * d), 3 * d, S, B, T, H, dh, cap)
            out = dev.full((B * T, d), np.nan)
            ws = dev.full((c.attention_decode_workspace(B, T, H, dh, cap),), np.nan)
            c.attention_decode_fwd(dev, QKV, 3 * d, Kc, Vc, S, out, ws, B, T, H, dh, cap, _scale(dh))
            q = np.ascontiguousarray(qkv[:, :d])
            DO.append(kc, vc, qkv[:, d:2 * d], qkv[:, 2 * d:], start, T)
            ref, ref32 = _oracles(q, kc, vc, start, T)
            got = out.numpy()
            assert np.all(np.isfinite(got)), (group, cap)
            _check(got, ref, ref32, _vmax(vc, start, T), "decode [dh %d B %d H %d T %d n %s cap %d]" % (dh, B, H, T, group, cap))


# ---- what the result may depend on --------------------------------------------------------------------------------------------------
def _ragged_case(dh, B, H, T, cap_extra, seed=0):
    ch = capi().attention_decode_chunk(dh)
    start = np.array([ch + 3, 2, 2 * ch + ch // 2 + 1][:B], dtype=np.int32)
    cap = int(start.max()) + T + cap_extra
    kc, vc = rnd(seed + 1, (B, H, cap, dh), -1, 1), rnd(seed + 2, (B, H, cap, dh), -1, 1)
    q = rnd(seed + 3, (B * T, H * dh), -1, 1)
    return q, kc, vc, start, cap


def _with_tail(a, start, T, value):
    out = a.copy()
    for b, s in enumerate(start):
        out[b, :, int(s) + T:] = value
    return out


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("dh", [32, 64, 128, 20, 5])
def test_the_cache_tail_never_reaches_the_result(dev, dh, T):
    """The same call with the caches beyond each sample's length holding 0, NaN and 1e30: identical bits, all finite."""
    B, H = 3, 2
    q, kc, vc, start, cap = _ragged_case(dh, B, H, T, cap_extra=capi().attention_decode_chunk(dh) + 9)
    runs = [_decode(dev, q, _with_tail(kc, start, T, fill), _with_tail(vc, start, T, fill), start, T) for fill in (0.0, np.nan, 1e30)]
    assert np.all(np.isfinite(runs[0]))
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    ref, ref32 = _oracles(q, kc, vc, start, T)
    _check(runs[1], ref, ref32, _vmax(vc, start, T), "tail [dh %d T %d]" % (dh, T))


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("dh", [32, 64, 128, 20, 5])
def test_a_sample_does_not_depend_on_its_batch_or_the_capacity(dev, dh, T):
    """Sample b computed inside B = 3 equals, in bits, the same sample computed alone; and the same across two capacities."""
    B, H = 3, 2
    q, kc, vc, start, cap = _ragged_case(dh, B, H, T, cap_extra=5)
    together = _decode(dev, q, kc, vc, start, T)
    for b in range(B):
        alone = _decode(dev, q[b * T:(b + 1) * T], kc[b:b + 1], vc[b:b + 1], start[b:b + 1], T)
        assert np.array_equal(alone, together[b * T:(b + 1) * T]), b
    extra = 3 * capi().attention_decode_chunk(dh) + 1                    # more chunks in the grid, the same keys per problem
    pad = lambda a: np.concatenate([a, np.full((B, H, extra, dh), np.nan, np.float32)], axis=2)
    assert np.array_equal(_decode(dev, q, pad(kc), pad(vc), start, T), together)
    # one head of one sample alone (H = 1): the other heads do not matter either
    b, h = 2, 1
    one = _decode(dev, np.ascontiguousarray(q[b * T:(b + 1) * T, h * dh:(h + 1) * dh]), kc[b:b + 1, h:h + 1], vc[b:b + 1, h:h + 1], start[b:b + 1], T)
    assert np.array_equal(one, together[b * T:(b + 1) * T, h * dh:(h + 1) * dh])


def test_runs_repeat_bit_for_bit(dev):
    dh, B, H, T = 64, 4, 16, 1                                           # B * H = 64 problems of five chunks each
    n = 4 * capi().attention_decode_chunk(dh) + 5
    kc, vc, q = rnd(1, (B, H, n, dh), -1, 1), rnd(2, (B, H, n, dh), -1, 1), rnd(3, (B * T, H * dh), -1, 1)
    start = np.full(B, n - 1, dtype=np.int32)
    first = _decode(dev, q, kc, vc, start, T)
    for _ in range(3):
        assert np.array_equal(_decode(dev, q, kc, vc, start, T), first)
    ref, ref32 = _oracles(q, kc, vc, start, T)
    _check(first, ref, ref32, float(np.abs(vc).max()), "repeat")


def test_queries_are_read_with_their_row_stride(dev):
    """ldq > H*dh with a column offset: the query block of a wider matrix, read in place."""
    dh, B, H, T = 64, 2, 2, 3
    q, kc, vc, start, cap = _ragged_case(dh, B, H, T, cap_extra=0)
    wide = rnd(9, (B * T, 3 * H * dh + 4), -1, 1)
    wide[:, 4:4 + H * dh] = q
    assert np.array_equal(_decode(dev, wide, kc, vc, start, T, ldq=wide.shape[1], q_offset=4), _decode(dev, q, kc, vc, start, T))


# ---- magnitudes ----------------------------------------------------------------------------------------------------------------------
def test_large_inputs(dev):
    dh, B, H, T, n = 128, 2, 2, 1, 1000
    kc, vc, q = rnd(1, (B, H, n, dh), -4, 4), rnd(2, (B, H, n, dh), -4, 4), rnd(3, (B * T, H * dh), -4, 4)
    start = np.array([n - 1, n - 1 - capi().attention_decode_chunk(dh) // 2], dtype=np.int32)
    ref, ref32 = _oracles(q, kc, vc, start, T)
    _check(_decode(dev, q, kc, vc, start, T), ref, ref32, _vmax(vc, start, T), "inputs in (-4, 4)")


@pytest.mark.parametrize("dh", [64, 20])
def test_one_dominant_key(dev, dh):
    """k_j = 8 q / |q| for one j per problem, in different chunks: its probability is all but 1, every other chunk's partial is
    rescaled by a tiny factor in the merge."""
    B, H, T = 2, 2, 1
    ch = capi().attention_decode_chunk(dh)
    n = 3 * ch + 7
    kc, vc, q = rnd(1, (B, H, n, dh), -1, 1), rnd(2, (B, H, n, dh), -1, 1), rnd(3, (B * T, H * dh), -1, 1)
    for b in range(B):
        for h in range(H):
            qr = q[b, h * dh:(h + 1) * dh]
            kc[b, h, [0, ch + 1, 2 * ch - 1, n - 1][2 * b + h]] = np.float32(8.0) * qr / np.float32(np.linalg.norm(qr))
    start = np.full(B, n - 1, dtype=np.int32)
    ref, ref32 = _oracles(q, kc, vc, start, T)
    _check(_decode(dev, q, kc, vc, start, T), ref, ref32, float(np.abs(vc).max()), "dominant key [dh %d]" % dh)


# ---- rejections ----------------------------------------------------------------------------------------------------------------------
def _raises_invalid(fn):
    c = capi()
    with pytest.raises(c.NeuronikaHipError) as e:
        fn()
    assert e.value.code == 1, e.value                                            # NK_ERR_INVALID


def test_invalid_arguments_are_refused(dev):
    c = capi()
    B, T, H, dh, cap = 2, 1, 2, 64, 16
    d = H * dh
    Q, K, V = (dev.zeros((B * T, d)) for _ in range(3))
    Kc, Vc, S, out = dev.zeros((B, H, cap, dh)), dev.zeros((B, H, cap, dh)), dev.int_zeros((B,)), dev.zeros((B * T, d))
    ws = dev.zeros((c.attention_decode_workspace(B, T, H, dh, cap),))
    good = dict(B=B, T=T, H=H, dh=dh, cap=cap)
    c.attention_decode_fwd(dev, Q, d, Kc, Vc, S, out, ws, scale=0.125, **good)    # the valid call passes
    c.kv_cache_append(dev, Kc, Vc, K, V, d, S, **good)
    for key in good:
        for bad in (0, -1):
            args = dict(good, **{key: bad})
            _raises_invalid(lambda: c.attention_decode_fwd(dev, Q, d, Kc, Vc, S, out, ws, scale=0.125, **args))
            _raises_invalid(lambda: c.kv_cache_append(dev, Kc, Vc, K, V, d, S, **args))
    for scale in (0.0, -0.125, float("nan"), float("inf")):
        _raises_invalid(lambda: c.attention_decode_fwd(dev, Q, d, Kc, Vc, S, out, ws, scale=scale, **good))
    ptrs = [Q, Kc, Vc, S, out, ws]
    for i in range(len(ptrs)):
        a = list(ptrs); a[i] = None
        _raises_invalid(lambda: c.attention_decode_fwd(dev, a[0], d, a[1], a[2], a[3], a[4], a[5], scale=0.125, **good))
    ptrs = [Kc, Vc, K, V, S]
    for i in range(len(ptrs)):
        a = list(ptrs); a[i] = None
        _raises_invalid(lambda: c.kv_cache_append(dev, a[0], a[1], a[2], a[3], d, a[4], **good))
    _raises_invalid(lambda: c.attention_decode_fwd(dev, Q, d - 1, Kc, Vc, S, out, ws, scale=0.125, **good))   # rows would overlap
    _raises_invalid(lambda: c.kv_cache_append(dev, Kc, Vc, K, V, d - 1, S, **good))
    _raises_invalid(lambda: c.attention_decode_fwd(dev, Q, d, Kc.view_offset(1), Vc, S, out, ws, scale=0.125, B=B, T=T, H=H, dh=dh, cap=cap - 1))
    assert c.attention_decode_workspace(B, T, H, 0, cap) == 0 and c.attention_decode_chunk(0) == 0

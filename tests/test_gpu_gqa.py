"""GPU parity of grouped-query attention through the C ABI: nk_repeat_kv_fwd / _bwd / _bwd_assign (bit contracts: a copy, and the f32
sum of the copies' gradients in ascending copy order) and nk_attention_decode_gqa_fwd (the query heads of a group share one read of
their kv head's chunk) against tests/gqa_oracle.py.

Tolerance of the decode: tests/test_gpu_attention_decode.py's rule as it stands - kernels and f32 oracle both measured against the
f64 oracle; pass iff err_gpu <= max(2 * err_cpu32, 1e-6 * scale), scale = max(|ref|max, |v|max), margins recorded under
`attention_decode_gqa:*`.

Bit contracts checked here (include/neuronika_hip.h): the bits of o for (b, h, t) are those nk_attention_decode_fwd gives for the
same query on a cache whose head h holds kv head h / G's rows; Hkv == H is that entry point; they do not depend on the cache's
tail, the other samples, the capacity or the run."""
import numpy as np
import pytest

import decode_oracle as DO
import gqa_oracle as GO

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
REPEAT_SHAPES = [(5, 1, 4, 64), (3, 2, 3, 32), (4, 3, 2, 20), (2, 2, 2, 5), (7, 1, 8, 128), (3, 2, 1, 64)]   # rows, Hkv, G, dh
DECODE_HEADS = [(1, 4, 1), (2, 6, 2), (3, 8, 4), (1, 16, 1), (2, 3, 3)]                                      # B, H, Hkv
DHS = [32, 64, 128, 20, 5]


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
    record_margin("attention_decode_gqa:" + what.split("[")[0].strip(), err_gpu, err_cpu, 1e-6 * scale)
    print(what, "err_gpu %.3g err_cpu32 %.3g bound %.3g" % (err_gpu, err_cpu, max(2 * err_cpu, 1e-6 * scale)))
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


def _scale(dh):
    return float(np.float32(1.0 / np.sqrt(dh)))


# ---- repeat_kv ----------------------------------------------------------------------------------------------------------------------
def _blocks(rows, Hkv, G, dh, packed):
    """(narrow host array, column offset, wide host array, column offset): contiguous, or column blocks of wider buffers whose
    other columns hold the sentinel.  The packed offsets keep 16-byte alignment where dh % 4 == 0 allows the vector kernel, and
    one more case below breaks it."""
    wn, ww = Hkv * dh, Hkv * G * dh
    if not packed:
        return np.full((rows, wn), SENTINEL, np.float32), 0, np.full((rows, ww), SENTINEL, np.float32), 0
    return np.full((rows, 8 + wn + 12), SENTINEL, np.float32), 8, np.full((rows, 4 + ww + 8), SENTINEL, np.float32), 4


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("rows,Hkv,G,dh", REPEAT_SHAPES)
def test_repeat_kv_fwd_is_a_bit_exact_copy(dev, rows, Hkv, G, dh, packed):
    c = capi()
    xb, xo, yb, yo = _blocks(rows, Hkv, G, dh, packed)
    x = rnd(1, (rows, Hkv * dh), -1, 1)
    xb[:, xo:xo + Hkv * dh] = x
    X, Y = dev.array(xb), dev.array(yb)
    c.repeat_kv_fwd(dev, X.view_offset(xo) if xo else X, xb.shape[1], Y.view_offset(yo) if yo else Y, yb.shape[1], rows, Hkv, G, dh)
    yb[:, yo:yo + Hkv * G * dh] = GO.repeat_kv(x, Hkv, G, dh)
    assert np.array_equal(Y.numpy(), yb)                                 # the copies, and every other column its sentinel
    assert np.array_equal(X.numpy(), xb)


@pytest.mark.parametrize("assign", [False, True])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("rows,Hkv,G,dh", REPEAT_SHAPES)
def test_repeat_kv_bwd_sums_the_copies_in_order(dev, rows, Hkv, G, dh, packed, assign):
    c = capi()
    db, do, gb, go = _blocks(rows, Hkv, G, dh, packed)
    g = rnd(2, (rows, Hkv * G * dh), -1, 1)
    dx0 = rnd(3, (rows, Hkv * dh), -1, 1)                                # += runs on a non-zero dx; = must overwrite it
    gb[:, go:go + Hkv * G * dh] = g
    db[:, do:do + Hkv * dh] = dx0
    DX, Gd = dev.array(db), dev.array(gb)
    c.repeat_kv_bwd(dev, DX.view_offset(do) if do else DX, db.shape[1], Gd.view_offset(go) if go else Gd, gb.shape[1], rows, Hkv, G, dh,
                    assign=assign)
    s = GO.repeat_kv_backward_f32(g, Hkv, G, dh)
    db[:, do:do + Hkv * dh] = s if assign else dx0 + s
    assert np.array_equal(DX.numpy(), db)
    assert np.array_equal(Gd.numpy(), gb)
    if G == 1:                                                           # an add or a copy
        assert np.array_equal(s, g)


def test_repeat_kv_scalar_path_on_unaligned_blocks(dev):
    """dh % 4 == 0 with an odd column offset and an odd stride: the 16-byte kernel is not allowed, the result is the same."""
    c = capi()
    rows, Hkv, G, dh = 3, 2, 3, 32
    x = rnd(4, (rows, Hkv * dh), -1, 1)
    xb, yb = np.full((rows, Hkv * dh + 3), SENTINEL, np.float32), np.full((rows, Hkv * G * dh + 5), SENTINEL, np.float32)
    xb[:, 1:1 + Hkv * dh] = x
    X, Y = dev.array(xb), dev.array(yb)
    c.repeat_kv_fwd(dev, X.view_offset(1), xb.shape[1], Y.view_offset(3), yb.shape[1], rows, Hkv, G, dh)
    yb[:, 3:3 + Hkv * G * dh] = GO.repeat_kv(x, Hkv, G, dh)
    assert np.array_equal(Y.numpy(), yb)
    c.repeat_kv_bwd(dev, X.view_offset(1), xb.shape[1], Y.view_offset(3), yb.shape[1], rows, Hkv, G, dh)
    xb[:, 1:1 + Hkv * dh] = x + GO.repeat_kv_backward_f32(yb[:, 3:3 + Hkv * G * dh], Hkv, G, dh)
    assert np.array_equal(X.numpy(), xb)


# ---- decode -------------------------------------------------------------------------------------------------------------------------
def _gqa(dev, q, kc, vc, start, T, H, ldq=None, q_offset=0):
    """nk_attention_decode_gqa_fwd on host arrays: q (rows, ldq) or (B*T, H*dh), kc / vc (B, Hkv, cap, dh) -> (B*T, H*dh)"""
    c = capi()
    B, Hkv, cap, dh = kc.shape
    Q, Kc, Vc, S = dev.array(q), dev.array(kc), dev.array(vc), dev.int_array(start)
    out = dev.full((B * T, H * dh), np.nan)
    ws = dev.full((c.attention_decode_workspace(B, T, H, dh, cap),), np.nan)
    c.attention_decode_gqa_fwd(dev, Q.view_offset(q_offset) if q_offset else Q, ldq or H * dh, Kc, Vc, S, out, ws, B, T, H, Hkv, dh, cap,
                               _scale(dh))
    return out.numpy()


def _mha(dev, q, kc, vc, start, T):
    """nk_attention_decode_fwd (the existing entry point) on host arrays with H = kc.shape[1]"""
    c = capi()
    B, H, cap, dh = kc.shape
    Q, Kc, Vc, S = dev.array(q), dev.array(kc), dev.array(vc), dev.int_array(start)
    out = dev.full((B * T, H * dh), np.nan)
    ws = dev.full((c.attention_decode_workspace(B, T, H, dh, cap),), np.nan)
    c.attention_decode_fwd(dev, Q, H * dh, Kc, Vc, S, out, ws, B, T, H, dh, cap, _scale(dh))
    return out.numpy()


def _expand(a, G):
    return np.ascontiguousarray(np.repeat(a, G, axis=1))


def _oracles(q, kc, vc, start, T, H):
    dh = kc.shape[3]
    return tuple(GO.decode_forward_gqa(q.astype(dt), kc.astype(dt), vc.astype(dt), start, T, H, _scale(dh)) for dt in (np.float64, np.float32))


def _vmax(vc, start, T):
    return max(float(np.abs(vc[b, :, :min(int(s) + T, vc.shape[2])]).max()) for b, s in enumerate(start))


def _lengths(dh):
    ch = capi().attention_decode_chunk(dh)
    return [1, 2, 3, ch - 1, ch, ch + 1, 2 * ch - 1, 2 * ch + 1, 3 * ch + 7, 1000]


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("B,H,Hkv", DECODE_HEADS)
@pytest.mark.parametrize("dh", DHS)
def test_decode_equals_oracle_and_the_ungrouped_entry_point(dev, dh, B, H, Hkv, T):
    """tests/test_gpu_attention_decode.py::test_decode_equals_oracle's grid of lengths (each what the FIRST new row of some sample
    reads, ragged across the samples of a call, the capacity equal to the longest length and well above it), on grouped heads.  The
    step's rows reach the (B, Hkv, cap, dh) caches through nk_kv_cache_append from a packed (B*T, d + 2*dkv) buffer the queries
    are read from in place.  Each result is held to the oracle under the suite's rule AND must equal, bit for bit,
    nk_attention_decode_fwd on the host-expanded cache; with Hkv == H that is the same cache."""
    c = capi()
    G, d, dkv, ch = H // Hkv, H * dh, Hkv * dh, c.attention_decode_chunk(dh)
    ld = d + 2 * dkv
    ns = _lengths(dh)
    ns = ns + ns[:(-len(ns)) % B]                                        # whole groups of B
    for g0 in range(0, len(ns), B):
        group = ns[g0:g0 + B]
        start = np.array([n - 1 for n in group], dtype=np.int32)
        for cap in (max(group) - 1 + T, max(group) - 1 + T + 2 * ch + 13):
            kc, vc = rnd(10 + g0, (B, Hkv, cap, dh), -1, 1), rnd(20 + g0, (B, Hkv, cap, dh), -1, 1)
            qkv = rnd(30 + g0, (B * T, ld), -1, 1)
            Kc, Vc, S, QKV = dev.array(kc), dev.array(vc), dev.int_array(start), dev.array(qkv)
            c.kv_cache_append(dev, Kc, Vc, QKV.view_offset(d), QKV.view_offset(d + dkv), ld, S, B, T, Hkv, dh, cap)
            out = dev.full((B * T, d), np.nan)
            ws = dev.full((c.attention_decode_workspace(B, T, H, dh, cap),), np.nan)
            c.attention_decode_gqa_fwd(dev, QKV, ld, Kc, Vc, S, out, ws, B, T, H, Hkv, dh, cap, _scale(dh))
            q = np.ascontiguousarray(qkv[:, :d])
            DO.append(kc, vc, qkv[:, d:d + dkv], qkv[:, d + dkv:], start, T)
            assert np.array_equal(Kc.numpy(), kc) and np.array_equal(Vc.numpy(), vc)
            ref, ref32 = _oracles(q, kc, vc, start, T, H)
            got = out.numpy()
            what = "decode [dh %d B %d H %d Hkv %d T %d n %s cap %d]" % (dh, B, H, Hkv, T, group, cap)
            assert np.all(np.isfinite(got)), what
            _check(got, ref, ref32, _vmax(vc, start, T), what)
            assert np.array_equal(got, _mha(dev, q, _expand(kc, G), _expand(vc, G), start, T)), what


def _ragged_case(dh, B, Hkv, H, T, cap_extra, seed=0):
    ch = capi().attention_decode_chunk(dh)
    start = np.array([ch + 3, 2, 2 * ch + ch // 2 + 1][:B], dtype=np.int32)
    cap = int(start.max()) + T + cap_extra
    kc, vc = rnd(seed + 1, (B, Hkv, cap, dh), -1, 1), rnd(seed + 2, (B, Hkv, cap, dh), -1, 1)
    q = rnd(seed + 3, (B * T, H * dh), -1, 1)
    return q, kc, vc, start, cap


def _with_tail(a, start, T, value):
    out = a.copy()
    for b, s in enumerate(start):
        out[b, :, int(s) + T:] = value
    return out


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("dh", DHS)
def test_the_cache_tail_never_reaches_the_result(dev, dh, T):
    """The same call with the caches beyond each sample's length holding 0, NaN and 1e30: identical bits, all finite."""
    B, Hkv, H = 3, 2, 6
    q, kc, vc, start, cap = _ragged_case(dh, B, Hkv, H, T, cap_extra=capi().attention_decode_chunk(dh) + 9)
    runs = [_gqa(dev, q, _with_tail(kc, start, T, fill), _with_tail(vc, start, T, fill), start, T, H) for fill in (0.0, np.nan, 1e30)]
    assert np.all(np.isfinite(runs[0]))
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    ref, ref32 = _oracles(q, kc, vc, start, T, H)
    _check(runs[1], ref, ref32, _vmax(vc, start, T), "tail [dh %d T %d]" % (dh, T))


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("dh", DHS)
def test_a_sample_does_not_depend_on_its_batch_the_capacity_or_its_group(dev, dh, T):
    """Sample b inside B = 3 equals, in bits, the sample alone; the same across two capacities; and one query head alone against
    its kv head (G = 1, the existing kernels) equals that head inside its group of 12 (two head batches)."""
    B, Hkv, H = 3, 2, 24
    G = H // Hkv
    q, kc, vc, start, cap = _ragged_case(dh, B, Hkv, H, T, cap_extra=5)
    together = _gqa(dev, q, kc, vc, start, T, H)
    for b in range(B):
        alone = _gqa(dev, q[b * T:(b + 1) * T], kc[b:b + 1], vc[b:b + 1], start[b:b + 1], T, H)
        assert np.array_equal(alone, together[b * T:(b + 1) * T]), b
    extra = 3 * capi().attention_decode_chunk(dh) + 1                    # more chunks in the grid, the same keys per problem
    pad = lambda a: np.concatenate([a, np.full((B, Hkv, extra, dh), np.nan, np.float32)], axis=2)
    assert np.array_equal(_gqa(dev, q, pad(kc), pad(vc), start, T, H), together)
    for b, h in ((2, 13), (0, 8), (1, 23)):
        kv = h // G
        one = _mha(dev, np.ascontiguousarray(q[b * T:(b + 1) * T, h * dh:(h + 1) * dh]), kc[b:b + 1, kv:kv + 1], vc[b:b + 1, kv:kv + 1],
                   start[b:b + 1], T)
        assert np.array_equal(one, together[b * T:(b + 1) * T, h * dh:(h + 1) * dh]), (b, h)


def test_runs_repeat_bit_for_bit(dev):
    dh, B, H, Hkv, T = 64, 4, 16, 4, 1
    n = 4 * capi().attention_decode_chunk(dh) + 5
    kc, vc, q = rnd(1, (B, Hkv, n, dh), -1, 1), rnd(2, (B, Hkv, n, dh), -1, 1), rnd(3, (B * T, H * dh), -1, 1)
    start = np.full(B, n - 1, dtype=np.int32)
    first = _gqa(dev, q, kc, vc, start, T, H)
    for _ in range(3):
        assert np.array_equal(_gqa(dev, q, kc, vc, start, T, H), first)
    ref, ref32 = _oracles(q, kc, vc, start, T, H)
    _check(first, ref, ref32, float(np.abs(vc).max()), "repeat")


def test_queries_are_read_with_their_row_stride(dev):
    """ldq > H*dh with a column offset: the query block of a wider matrix, read in place."""
    dh, B, Hkv, H, T = 64, 2, 2, 4, 3
    q, kc, vc, start, cap = _ragged_case(dh, B, Hkv, H, T, cap_extra=0)
    wide = rnd(9, (B * T, 3 * H * dh + 4), -1, 1)
    wide[:, 4:4 + H * dh] = q
    assert np.array_equal(_gqa(dev, wide, kc, vc, start, T, H, ldq=wide.shape[1], q_offset=4), _gqa(dev, q, kc, vc, start, T, H))


def test_a_negative_start_gives_a_zero_row(dev):
    """n <= 0: every head of the block's batch writes zeros (the grouped kernel's early exit covers all its heads)."""
    dh, B, Hkv, H, T = 64, 2, 1, 12, 1
    kc, vc, q = rnd(1, (B, Hkv, 8, dh), -1, 1), rnd(2, (B, Hkv, 8, dh), -1, 1), rnd(3, (B * T, H * dh), -1, 1)
    start = np.array([-1, 3], dtype=np.int32)
    got = _gqa(dev, q, kc, vc, start, T, H)
    assert np.all(got[0] == 0)
    assert np.array_equal(got, _mha(dev, q, _expand(kc, H), _expand(vc, H), start, T))


# ---- rejections ----------------------------------------------------------------------------------------------------------------------
def _raises_invalid(fn):
    c = capi()
    with pytest.raises(c.NeuronikaHipError) as e:
        fn()
    assert e.value.code == 1, e.value                                            # NK_ERR_INVALID


def test_invalid_arguments_are_refused(dev):
    c = capi()
    B, T, H, Hkv, dh, cap = 2, 1, 4, 2, 64, 16
    d = H * dh
    Q = dev.zeros((B * T, d))
    Kc, Vc, S = dev.zeros((B, Hkv, cap, dh)), dev.zeros((B, Hkv, cap, dh)), dev.int_zeros((B,))
    out = dev.full((B * T, d), SENTINEL)
    ws = dev.zeros((c.attention_decode_workspace(B, T, H, dh, cap),))
    good = dict(B=B, T=T, H=H, Hkv=Hkv, dh=dh, cap=cap)

    def call(ptrs=None, scale=0.125, ldq=d, **kw):
        q_, kc_, vc_, s_, o_, w_ = ptrs or (Q, Kc, Vc, S, out, ws)
        c.attention_decode_gqa_fwd(dev, q_, ldq, kc_, vc_, s_, o_, w_, scale=scale, **dict(good, **kw))

    for hkv in (0, -1, 3, 8, 5):                                         # non-positive, no divisor of H, larger than H
        _raises_invalid(lambda: call(Hkv=hkv))
    for key in ("B", "T", "H", "dh", "cap"):
        for bad in (0, -1):
            _raises_invalid(lambda: call(**{key: bad}))
    for scale in (0.0, -0.125, float("nan"), float("inf")):
        _raises_invalid(lambda: call(scale=scale))
    ptrs = [Q, Kc, Vc, S, out, ws]
    for i in range(len(ptrs)):
        a = list(ptrs); a[i] = None
        _raises_invalid(lambda: call(ptrs=a))
    _raises_invalid(lambda: call(ldq=d - 1))
    _raises_invalid(lambda: c.attention_decode_gqa_fwd(dev, Q, d, Kc.view_offset(1), Vc, S, out, ws, B, T, H, Hkv, dh, cap - 1, 0.125))
    assert np.all(out.numpy() == SENTINEL)                               # nothing was written
    call()                                                               # the valid call passes
    assert np.all(out.numpy() == 0)                                      # zero values: every row is 0

    rows, G = 3, 2
    x, y = dev.zeros((rows, Hkv * dh)), dev.full((rows, Hkv * G * dh), SENTINEL)
    rgood = dict(rows=rows, Hkv=Hkv, G=G, dh=dh)
    for key in rgood:
        for bad in (0, -1):
            args = dict(rgood, **{key: bad})
            _raises_invalid(lambda: c.repeat_kv_fwd(dev, x, Hkv * dh, y, Hkv * G * dh, **args))
            _raises_invalid(lambda: c.repeat_kv_bwd(dev, x, Hkv * dh, y, Hkv * G * dh, **args))
            _raises_invalid(lambda: c.repeat_kv_bwd(dev, x, Hkv * dh, y, Hkv * G * dh, assign=True, **args))
    _raises_invalid(lambda: c.repeat_kv_fwd(dev, x, Hkv * dh - 1, y, Hkv * G * dh, **rgood))
    _raises_invalid(lambda: c.repeat_kv_fwd(dev, x, Hkv * dh, y, Hkv * G * dh - 1, **rgood))
    _raises_invalid(lambda: c.repeat_kv_fwd(dev, None, Hkv * dh, y, Hkv * G * dh, **rgood))
    _raises_invalid(lambda: c.repeat_kv_bwd(dev, x, Hkv * dh, None, Hkv * G * dh, **rgood))
    assert np.all(y.numpy() == SENTINEL)

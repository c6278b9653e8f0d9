"""Weight-only quantised layers through the tape (`_tape`): `nn::QuantLinear` and `nn::MultiheadAttention::quantize`.

QuantLinear: forward against the f64 product over the oracle's dequantised weights under the contraction policy (tests/tolerance.py),
dequantize() equal to the oracle's w^ bit for bit, the source Linear untouched.  The attention module: a prefill of T = 5 and three
single-token steps on a `KvCache` and on a `PagedKvCache`, after quantize(8, 32) and after quantize(4, 0), against
tests/gqa_oracle.py's stepped forward fed the dequantised weights (err_gpu <= max(2 * err_cpu32, 1e-6 * scale) against the f64
oracle, the rule tests/test_gpu_tape_gqa.py holds the same quantities to; margins under `mha_quant:*`).  Without quantize() a module
gives the bits of an identically seeded twin: the off switch.

This file holds checks, not test ids: `checks()` lists them, every parametrisation spelled out, and the one test of
tests/test_gpu_quant_linear.py runs them behind the C-ABI checks of the same kernels.

The paged cache has pages of 16 positions, the smallest `nn::PageTable` accepts (a page of 4 is refused when the cache is built), so
the 5 + 1 + 1 + 1 walk stays inside one page; a second paged walk, 15 + 1 + 1 + 1, has its prefill fill a page to its last slot
but one and its steps cross into the next."""
import numpy as np
import pytest

import gqa_oracle as GO
import quant_oracle as Q
import rope_oracle as RO
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu

B, D, H, HKV, PAGE = 2, 128, 4, 2, 16
SLICES = (5, 1, 1, 1)
CROSSING = (15, 1, 1, 1)   # positions 15 | 16, 17: over the page boundary


def rnd(seed, shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def dequantised(w, bits, group):
    b, s = Q.pack(w, bits, group)
    return Q.unpack(b, s, bits, group, w.shape[1])


def check_quant_linear(nk, tdev, bits, group):
    lin = nk.nn.Linear(tdev, 96, 67, 5)
    w0, bias = lin.weight.data().copy(), lin.bias.data().copy()
    ql = nk.nn.QuantLinear(lin, bits, group)
    assert (ql.in_features, ql.out_features, ql.bits, ql.group) == (96, 67, bits, group)
    assert np.array_equal(lin.weight.data().view(np.uint32), w0.view(np.uint32)), "the source Linear changed"
    b, s = Q.pack(w0, bits, group)
    wq = Q.unpack(b, s, bits, group, 96)
    dq = ql.dequantize()
    assert dq.shape == [67, 96] and np.array_equal(dq.data().view(np.uint32), wq.view(np.uint32)), "dequantize() is not the oracle's w^"
    for rows in (1, 3, 8, 11):   # the rows kernels, and past the rule the GEMM over the unpacked weights
        x = rnd(rows, (rows, 96))
        for X in (nk.from_ndarray(tdev, x), nk.from_ndarray(tdev, x).requires_grad()):   # what forward_step accepts
            y = ql.forward(X)
            assert y.history_len() == 1 and y.shape == [rows, 67]
            y.forward()
            assert_contraction("quant_linear:tape:b%dg%d" % (bits, group), y.data(), Q.forward64(x, b, s, bias, bits, group), 96, amax=np.abs(x).max(),
                               bmax=np.abs(wq).max(), cpu32=Q.forward32(x, b, s, bias, bits, group), epilogue=True)
    with pytest.raises(Exception):
        ql.forward(nk.from_ndarray(tdev, rnd(0, (2, 64))))


def check_quant_linear_refuses_what_the_format_refuses(nk, tdev):
    for fin, bits, group in ((48, 8, 0), (96, 8, 64), (96, 3, 0), (96, 8, 16)):
        with pytest.raises(Exception):
            nk.nn.QuantLinear(nk.nn.Linear(tdev, fin, 8, 1), bits, group)


# ---- MultiheadAttention.quantize -------------------------------------------------------------------------------------------------
def _module(nk, tdev, handed, seed=3):
    dkv = D // H * HKV
    if handed:
        outs = (D, dkv, dkv, D)
        mha = nk.nn.MultiheadAttention(*(nk.nn.Linear(tdev, D, outs[i], seed + 2 * i) for i in range(4)), H, 0.0, kv_heads=HKV)
    else:
        mha = nk.nn.MultiheadAttention(tdev, D, H, 0.0, seed, kv_heads=HKV)
    assert mha.packed_qkv is (not handed)
    mha.causal = True
    mha.drop.eval()
    mha.rope = nk.nn.RotaryEmbedding(tdev, D // H, 32)
    return mha


def _rows(x, lo, hi):
    S = x.shape[0] // B
    return np.ascontiguousarray(np.concatenate([x[b * S + lo:b * S + hi] for b in range(B)]))


def _walk(nk, tdev, mha, cache, x, slices, seqs=None):
    out, pos, S = np.zeros_like(x), 0, x.shape[0] // B
    assert S == sum(slices)
    for T in slices:
        X = nk.from_ndarray(tdev, _rows(x, pos, pos + T))
        y = mha.forward_step(X, B, cache) if seqs is None else mha.forward_step(X, seqs, cache)
        assert y.history_len() == 1
        y.forward()
        got = y.data()
        for b in range(B):
            out[b * S + pos:b * S + pos + T] = got[b * T:(b + 1) * T]
        pos += T
    return out


def _caches(nk, tdev):
    """(name, slices, cache, seqs)"""
    yield "KvCache", SLICES, nk.nn.KvCache(tdev, B, HKV, D // H, sum(SLICES)), None
    yield "PagedKvCache", SLICES, nk.nn.PagedKvCache(tdev, B * 2 + 2, PAGE, HKV, D // H, B, 2), list(range(B))
    yield "PagedKvCache over a page boundary", CROSSING, nk.nn.PagedKvCache(tdev, B * 2 + 2, PAGE, HKV, D // H, B, 2), list(range(B))


def _stepped_oracle(W, Bs, x, slices, dt, ro):
    dh, S = D // H, sum(slices)
    kc, vc = np.full((B, HKV, S, dh), np.nan, dt), np.full((B, HKV, S, dh), np.nan, dt)
    out, start = np.zeros((B * S, D), dt), np.zeros(B, dtype=np.int64)
    for T in slices:
        pos = int(start[0])
        got, start = GO.mha_step(_rows(x, pos, pos + T).astype(dt), [w.astype(dt) for w in W], [b.astype(dt) for b in Bs], H, HKV, kc, vc, start, T, rope=ro)
        for b in range(B):
            out[b * S + pos:b * S + pos + T] = got[b * T:(b + 1) * T]
    return out


def check_quantized_steps_against_the_oracle_on_dequantised_weights(nk, tdev, handed):
    from conftest import record_margin
    mha = _module(nk, tdev, handed)
    ro = RO.make(32, D // H)
    xs = {sl: rnd(len(sl) + sl[0], (B * sum(sl), D)) for sl in (SLICES, CROSSING)}
    Wf = [getattr(mha, n).weight.data() for n in "qkvo"]
    Bs = [getattr(mha, n).bias.data() for n in "qkvo"]
    assert not mha.quantized
    for bits, group in ((8, 32), (4, 0)):
        mha.quantize(bits, group)
        assert mha.quantized
        W = [dequantised(w, bits, group) for w in Wf]
        for name, slices, cache, seqs in _caches(nk, tdev):
            x = xs[slices]
            ref, ref32 = _stepped_oracle(W, Bs, x, slices, np.float64, ro), _stepped_oracle(W, Bs, x, slices, np.float32, ro)
            scale = np.abs(ref).max()
            err_cpu = np.abs(ref32 - ref).max()
            got = _walk(nk, tdev, mha, cache, x, slices, seqs)
            err_gpu = np.abs(got - ref).max()
            record_margin("mha_quant:steps b%dg%d" % (bits, group), err_gpu, err_cpu, 1e-6 * scale)
            assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (name, bits, group, err_gpu, err_cpu, scale)
            # the images replaced the weights: the f32 module's steps are further away than the bound
            assert np.abs(_stepped_oracle(Wf, Bs, x, slices, np.float64, ro) - ref).max() > 10 * max(2 * err_cpu, 1e-6 * scale)
    for w, w0 in zip((getattr(mha, n).weight.data() for n in "qkvo"), Wf):
        assert np.array_equal(w.view(np.uint32), w0.view(np.uint32)), "quantize() changed an f32 weight"


def check_without_quantize_a_module_is_its_twin_bit_for_bit(nk, tdev):
    """the off switch: null images, the launches and bits of the module as it was"""
    a, b, c = _module(nk, tdev, False), _module(nk, tdev, False), _module(nk, tdev, False)
    c.quantize(8, 32)
    for (_, sl, ca, sa), (_, _, cb, sb), (_, _, cc, sc) in zip(_caches(nk, tdev), _caches(nk, tdev), _caches(nk, tdev)):
        x = rnd(1, (B * sum(sl), D))
        ya, yb, yc = _walk(nk, tdev, a, ca, x, sl, sa), _walk(nk, tdev, b, cb, x, sl, sb), _walk(nk, tdev, c, cc, x, sl, sc)
        assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32))
        assert not np.array_equal(ya.view(np.uint32), yc.view(np.uint32))   # and the switch does switch
    # training forward of the quantised module still reads the f32 weights
    fa, fc = a.forward(nk.from_ndarray(tdev, x).requires_grad(), B), c.forward(nk.from_ndarray(tdev, x).requires_grad(), B)
    fa.forward(); fc.forward()
    assert np.array_equal(fa.data().view(np.uint32), fc.data().view(np.uint32))


def check_a_stale_image_form_panics(nk, tdev):
    mha = _module(nk, tdev, False)
    mha.quantize(8, 32)
    mha.packed_qkv = False   # the step now takes three projections, the image is of the packed storage
    with pytest.raises(Exception):
        mha.forward_step(nk.from_ndarray(tdev, rnd(2, (B, D))), B, nk.nn.KvCache(tdev, B, HKV, D // H, 8))
    mha.quantize(8, 32)
    y = mha.forward_step(nk.from_ndarray(tdev, rnd(2, (B, D))), B, nk.nn.KvCache(tdev, B, HKV, D // H, 8))
    y.forward()
    assert np.isfinite(y.data()).all()
    with pytest.raises(Exception):
        mha.quantize(8, 48)


def checks():
    """[(name, callable)]: every check of this file on one tape device, the parametrisations spelled out"""
    import neuronika_amd
    nk = neuronika_amd.tape
    tdev = nk.Device(0)
    out = [("quant_linear[%d-%d]" % bg, lambda bg=bg: check_quant_linear(nk, tdev, *bg)) for bg in ((8, 32), (8, 0), (4, 32), (4, 0))]
    out.append(("quant_linear_refuses_what_the_format_refuses", lambda: check_quant_linear_refuses_what_the_format_refuses(nk, tdev)))
    out += [("quantized_steps_against_the_oracle_on_dequantised_weights[%s]" % ("four Linears" if h else "packed"),
             lambda h=h: check_quantized_steps_against_the_oracle_on_dequantised_weights(nk, tdev, h)) for h in (False, True)]
    out.append(("without_quantize_a_module_is_its_twin_bit_for_bit", lambda: check_without_quantize_a_module_is_its_twin_bit_for_bit(nk, tdev)))
    out.append(("a_stale_image_form_panics", lambda: check_a_stale_image_form_panics(nk, tdev)))
    return out

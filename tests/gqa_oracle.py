"""The oracle of grouped-query attention (semantics: include/neuronika_hip.h, nk_attention_decode_gqa_fwd / nk_repeat_kv_fwd), in
NumPy, in the dtype it is called with.  H query heads, Hkv kv heads, G = H / Hkv: query head h attends to kv head h // G.

Everything here is the REPEAT form - kv head k written G times (heads k*G .. k*G + G - 1) in front of the existing oracles
(`O.linear_forward`, tests/causal_oracle.py, tests/rope_oracle.py, tests/decode_oracle.py), the gradients of the copies summed
behind them.  tests/test_oracle_gqa.py pins it against a direct `h // G` loop and against torch's `repeat_interleave` autograd."""
import numpy as np

import causal_oracle as CO
import decode_oracle as DO
import rope_oracle as RO
from oracle import neuronika_oracle as O


def repeat_kv(x, Hkv, G, dh):
    """x (rows, Hkv*dh) -> (rows, Hkv*G*dh): y[r, (k*G + j)*dh + e] = x[r, k*dh + e]"""
    rows = x.shape[0]
    return np.ascontiguousarray(np.repeat(x.reshape(rows, Hkv, 1, dh), G, axis=2).reshape(rows, Hkv * G * dh))


def repeat_kv_backward(g, Hkv, G, dh):
    """g (rows, Hkv*G*dh) -> (rows, Hkv*dh): the sum of the copies' gradients in the dtype of g (NumPy's order)"""
    return g.reshape(g.shape[0], Hkv, G, dh).sum(axis=2).reshape(g.shape[0], Hkv * dh)


def repeat_kv_backward_f32(g, Hkv, G, dh):
    """The device's sum: ((g_0 + g_1) + g_2) + ... over the copies j ascending, every addition rounded to f32."""
    g4 = np.asarray(g, dtype=np.float32).reshape(g.shape[0], Hkv, G, dh)
    s = g4[:, :, 0].copy()
    for j in range(1, G):
        s = s + g4[:, :, j]
    return s.reshape(g.shape[0], Hkv * dh)


def decode_forward_gqa(q, kc, vc, start, T, H, scale=None):
    """q (B*T, H*dh); kc / vc (B, Hkv, cap, dh) -> (B*T, H*dh): tests/decode_oracle.py on the cache with every kv head repeated"""
    G = H // kc.shape[1]
    assert G * kc.shape[1] == H
    return DO.decode_forward(q, np.repeat(kc, G, axis=1), np.repeat(vc, G, axis=1), start, T, scale)


def mha_forward_backward(x, wq, bq, wk, bk, wv, bv, wo, bo, heads, kv_heads, batch, p, noise, g_out, causal=True, rope=None):
    """nn::MultiheadAttention with kv_heads: wk / wv are (kv_heads*dh, d_model).  Projections, rotate q (heads) and k (kv_heads),
    repeat k and v, the (causal) core on `heads` heads, out-projection; backward: the core, the sum of the copies, the inverse
    rotations, the linears.  kv_heads == heads is tests/rope_oracle.py's function, call for call."""
    if kv_heads == heads:
        return RO.mha_forward_backward(x, wq, bq, wk, bk, wv, bv, wo, bo, heads, batch, p, noise, g_out, causal=causal, rope=rope)
    S, dh, G = x.shape[0] // batch, wq.shape[0] // heads, heads // kv_heads
    assert G * kv_heads == heads and wk.shape[0] == kv_heads * dh and wv.shape[0] == kv_heads * dh
    if rope is None:
        rot = lambda t, nh, inv=False: t
    else:
        rot = lambda t, nh, inv=False: RO.rope(t, None, S, nh, dh, rope.rot, rope.interleaved, rope.table, inverse=inv)
    q, k, v = O.linear_forward(x, wq, bq), O.linear_forward(x, wk, bk), O.linear_forward(x, wv, bv)
    kf, vf = repeat_kv(rot(k, kv_heads), kv_heads, G, dh), repeat_kv(v, kv_heads, G, dh)
    o, cache = CO.attention_core_forward(rot(q, heads), kf, vf, heads, batch, p, noise, causal=causal)
    out = O.linear_forward(o, wo, bo)
    g = g_out
    dbo = np.zeros_like(bo); O.accumulate(dbo, g)
    dwo = np.zeros_like(wo); O.mm_t_backward_right(dwo, g, o)
    do = np.zeros_like(o); O.mm_t_backward_left(do, g, wo)
    core = CO.attention_core_backward(cache, do)
    dq = rot(core["dq"], heads, True)
    dk = rot(repeat_kv_backward(core["dk"], kv_heads, G, dh), kv_heads, True)
    dv = repeat_kv_backward(core["dv"], kv_heads, G, dh)
    grads = {}
    dx = np.zeros_like(x)
    for name, w, b, dz in (("q", wq, bq, dq), ("k", wk, bk, dk), ("v", wv, bv, dv)):
        dz = np.ascontiguousarray(dz)
        db = np.zeros_like(b); O.accumulate(db, dz)
        dw = np.zeros_like(w); O.mm_t_backward_right(dw, dz, x)
        O.mm_t_backward_left(dx, dz, w)
        grads["w" + name], grads["b" + name] = dw, db
    grads.update(wo=dwo, bo=dbo, x=dx)
    return out, grads


def mha_forward(x, W, Bs, heads, kv_heads, batch, causal=True, rope=None, with_context=False):
    """The module's inference forward (no dropout): W / Bs = the q, k, v, o weights and biases.  with_context: (output, the core's
    context in front of the output projection)."""
    S, dh, G = x.shape[0] // batch, W[0].shape[0] // heads, heads // kv_heads
    q, k, v = (O.linear_forward(x, W[i], Bs[i]) for i in range(3))
    if rope is not None:
        q = RO.rope(q, None, S, heads, dh, rope.rot, rope.interleaved, rope.table)
        k = RO.rope(k, None, S, kv_heads, dh, rope.rot, rope.interleaved, rope.table)
    ctx, _ = CO.attention_core_forward(q, repeat_kv(k, kv_heads, G, dh), repeat_kv(v, kv_heads, G, dh), heads, batch, 0.0,
                                       np.ones((batch * heads, S, S), dtype=x.dtype), causal=causal)
    out = O.linear_forward(ctx, W[3], Bs[3])
    return (out, ctx) if with_context else out


def mha_step(x, W, Bs, heads, kv_heads, kc, vc, start, T, rope=None):
    """The module's step on (B, kv_heads, cap, dh) caches: projections, q rotated on `heads` heads and k on `kv_heads` at
    start[b] + t, append, grouped attention, output projection.  Returns (output, lengths after the step)."""
    dh = W[0].shape[0] // heads
    q, k, v = (O.linear_forward(x, W[i], Bs[i]) for i in range(3))
    if rope is not None:
        q = RO.rope(q, start, T, heads, dh, rope.rot, rope.interleaved, rope.table)
        k = RO.rope(k, start, T, kv_heads, dh, rope.rot, rope.interleaved, rope.table)
    DO.append(kc, vc, k, v, start, T)
    ctx = decode_forward_gqa(q, kc, vc, start, T, heads)
    return O.linear_forward(ctx, W[3], Bs[3]), np.asarray(start) + T

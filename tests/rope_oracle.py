"""The oracle of the rotary position embedding (semantics: include/neuronika_hip.h, nk_rope_fwd), in NumPy, in the dtype it is called
with.

    table[p, j] = (cos, sin)(p * base^(-2j/rot))                  frequency, product and function in f64
    y1 = x1 c - x2 s;   y2 = x2 c + x1 s                          pairs (j, j + rot/2) or, interleaved, (2j, 2j+1); inverse: s -> -s

`mha_forward_backward(..., rope=...)` is tests/causal_oracle.py's module with the rotation of q and k in front of the core and the
inverse rotation of dq and dk behind it; `mha_step` is tests/decode_oracle.py's step with the rotation at start[b] + t before the
append.  Everything else is the oracle's own node functions.  tests/test_oracle_rope.py pins it."""
import math
from collections import namedtuple

import numpy as np

import causal_oracle as CO
import decode_oracle as DO
from oracle import neuronika_oracle as O

Rope = namedtuple("Rope", "table rot interleaved")


def table(max_pos, rot, base=10000.0, positions=None):
    """(max_pos, rot/2, 2) f64, or the rows of `positions`.  The frequency is libm's pow, as the library's host code forms it."""
    theta = np.array([math.pow(base, -2.0 * j / rot) for j in range(rot // 2)], dtype=np.float64)
    p = np.arange(max_pos, dtype=np.float64) if positions is None else np.asarray(positions, dtype=np.float64)
    a = p[:, None] * theta[None, :]
    return np.stack([np.cos(a), np.sin(a)], axis=-1)


def make(max_pos, dh, rot=None, interleaved=False, base=10000.0):
    rot = dh if rot is None else rot
    return Rope(table(max_pos, rot, base), rot, bool(interleaved))


def pair_columns(rot, interleaved):
    j = np.arange(rot // 2)
    return (2 * j, 2 * j + 1) if interleaved else (j, j + rot // 2)


def positions(start, B, T, max_pos):
    """Position of row b*T + t, clamped into the table as the kernel clamps it."""
    st = np.zeros(B, dtype=np.int64) if start is None else np.asarray(start, dtype=np.int64)
    return np.clip((st[:, None] + np.arange(T)[None, :]).reshape(-1), 0, max_pos - 1)


def rope(x, start, T, heads, dh, rot, interleaved, table, inverse=False):
    """x (B*T, >= heads*dh): the first `rot` columns of `heads` heads rotated; every other column as it is."""
    dt = x.dtype
    B = x.shape[0] // T
    tab = np.asarray(table)[positions(start, B, T, table.shape[0])].astype(dt)       # (rows, rot/2, 2)
    c, s = tab[:, None, :, 0], tab[:, None, :, 1]
    if inverse:
        s = -s
    y = x.copy()
    xh = x[:, :heads * dh].reshape(-1, heads, dh)
    yh = np.empty_like(xh)
    yh[...] = xh
    c1, c2 = pair_columns(rot, interleaved)
    x1, x2 = xh[:, :, c1], xh[:, :, c2]
    yh[:, :, c1] = x1 * c - x2 * s
    yh[:, :, c2] = x2 * c + x1 * s
    y[:, :heads * dh] = yh.reshape(-1, heads * dh)
    return y


_rotate = rope  # the functions below take the module's rotary description as `rope`


def mha_forward_backward(x, wq, bq, wk, bk, wv, bv, wo, bo, heads, batch, p, noise, g_out, causal=True, rope=None):
    """Projections, rotate q and k, the (causal) core, out-projection; backward: the core, inverse-rotate dq and dk, the linears."""
    if rope is None:
        return CO.mha_forward_backward(x, wq, bq, wk, bk, wv, bv, wo, bo, heads, batch, p, noise, g_out, causal=causal)
    S, dh = x.shape[0] // batch, wq.shape[0] // heads
    rot = lambda t, inv=False: _rotate(t, None, S, heads, dh, rope.rot, rope.interleaved, rope.table, inverse=inv)
    q, k, v = O.linear_forward(x, wq, bq), O.linear_forward(x, wk, bk), O.linear_forward(x, wv, bv)
    o, cache = CO.attention_core_forward(rot(q), rot(k), v, heads, batch, p, noise, causal=causal)
    out = O.linear_forward(o, wo, bo)
    g = g_out
    dbo = np.zeros_like(bo); O.accumulate(dbo, g)
    dwo = np.zeros_like(wo); O.mm_t_backward_right(dwo, g, o)
    do = np.zeros_like(o); O.mm_t_backward_left(do, g, wo)
    core = CO.attention_core_backward(cache, do)
    core = dict(dq=rot(core["dq"], True), dk=rot(core["dk"], True), dv=core["dv"])
    grads = {}
    dx = np.zeros_like(x)
    for name, w, b, dz in (("q", wq, bq, core["dq"]), ("k", wk, bk, core["dk"]), ("v", wv, bv, core["dv"])):
        db = np.zeros_like(b); O.accumulate(db, dz)
        dw = np.zeros_like(w); O.mm_t_backward_right(dw, dz, x)
        O.mm_t_backward_left(dx, dz, w)
        grads["w" + name], grads["b" + name] = dw, db
    grads.update(wo=dwo, bo=dbo, x=dx)
    return out, grads


def mha_step(x, W, Bs, heads, kc, vc, start, T, rope=None):
    """tests/decode_oracle.py's module step with the new q and k rows rotated at start[b] + t before the append."""
    if rope is None:
        return DO.mha_step(x, W, Bs, heads, kc, vc, start, T)
    dh = W[0].shape[0] // heads
    q, k, v = (O.linear_forward(x, W[i], Bs[i]) for i in range(3))
    q, k = (_rotate(t, start, T, heads, dh, rope.rot, rope.interleaved, rope.table) for t in (q, k))
    ctx, after = DO.step(q, k, v, kc, vc, start, T)
    return O.linear_forward(ctx, W[3], Bs[3]), after

"""The oracle of sliding-window attention (semantics: include/neuronika_hip.h, nk_attention_decode_window_fwd), in NumPy, in the
dtype it is called with.  Query position i attends to the keys max(0, i - W + 1) .. i.

Decoding: tests/decode_oracle.py with the window - for sample b, head h and the t-th new row, n = start[b] + t + 1 and
lo = max(0, n - W):   o = softmax(q . K[lo:n]^T * scale) . V[lo:n]   - on a linear cache (position p at slot p, n clipped to cap)
or a ring (position p at slot p % cap, n not clipped); grouped layers through tests/gqa_oracle.py's repeat of every kv head.

Full sequences: tests/causal_oracle.py with the BANDED constant on the Addition node - M[r][k] = 0 for r - W < k <= r, -inf
elsewhere.  Every row keeps its diagonal, so Softmax (node/softmax/mod.rs:37-53) and the backward nodes need nothing new.
Everything is built from the oracle's own node functions; only the mask and the slot arithmetic are added.
tests/test_oracle_window.py pins it against an independent per-row loop and against tests/causal_oracle.py for W >= S."""
import numpy as np

import gqa_oracle as GO
import rope_oracle as RO
from oracle import neuronika_oracle as O


# ---- decoding ---------------------------------------------------------------------------------------------------------------------
def slot(p, cap, ring):
    return p % cap if ring else p


def append(kc, vc, k, v, start, T, ring=False):
    """Row b*T + t of k / v ((B*T, H*dh)) -> slot of position start[b] + t of every head of sample b.  Linear: positions >= cap
    are dropped.  Ring: every position >= 0 is written (T <= cap)."""
    B, H, cap, dh = kc.shape
    assert not ring or T <= cap
    for b in range(B):
        for t in range(T):
            pos = int(start[b]) + t
            if pos < 0 or (not ring and pos >= cap):
                continue
            kc[b, :, slot(pos, cap, ring), :] = k[b * T + t].reshape(H, dh)
            vc[b, :, slot(pos, cap, ring), :] = v[b * T + t].reshape(H, dh)


def window_rows(start_b, t, W, cap, ring):
    """(lo, n) of query (b, t): the positions [lo, n) it reads"""
    n = int(start_b) + t + 1
    if not ring:
        n = min(n, cap)
    return max(0, n - W), n


def decode_forward(q, kc, vc, start, T, W, ring=False, H=None, scale=None):
    """q (B*T, H*dh); kc / vc (B, Hkv, cap, dh) already holding the step's rows -> (B*T, H*dh).  H: the query heads (default Hkv)."""
    B, Hkv, cap, dh = kc.shape
    H = Hkv if H is None else H
    G = H // Hkv
    assert G * Hkv == H and W >= 1 and (not ring or W + T - 1 <= cap)
    if G > 1:                                                            # tests/gqa_oracle.py's form: every kv head repeated
        kc, vc = np.repeat(kc, G, axis=1), np.repeat(vc, G, axis=1)
    dt = q.dtype
    scale = dt.type(1.0 / np.sqrt(dh)) if scale is None else dt.type(scale)
    out = np.zeros((B * T, H * dh), dtype=dt)
    for b in range(B):
        for t in range(T):
            lo, n = window_rows(start[b], t, W, cap, ring)
            if n <= 0:
                continue
            slots = [slot(p, cap, ring) for p in range(lo, n)]
            for h in range(H):
                qr = q[b * T + t, h * dh:(h + 1) * dh].reshape(1, dh)
                sc = np.matmul(qr, kc[b, h, slots].T) * scale
                pr = np.zeros_like(sc)
                O.softmax_forward(sc, pr, axis=1)
                out[b * T + t, h * dh:(h + 1) * dh] = np.matmul(pr, vc[b, h, slots])[0]
    return out


def ring_image(kc_lin, upto, cap):
    """The ring of `cap` slots that holds, for sample b, the last `cap` positions below upto[b] of a linear cache
    (B, H, >= max(upto), dh); slots no position has reached stay NaN."""
    B, H, _, dh = kc_lin.shape
    out = np.full((B, H, cap, dh), np.nan, dtype=kc_lin.dtype)
    for b in range(B):
        for p in range(max(0, int(upto[b]) - cap), int(upto[b])):
            out[b, :, p % cap] = kc_lin[b, :, p]
    return out


def mha_step(x, W_, Bs, heads, kv_heads, kc, vc, start, T, window, ring=False, rope=None):
    """The module's step on (B, kv_heads, cap, dh) caches: projections, q rotated on `heads` heads and k on `kv_heads` at
    start[b] + t, append, windowed (grouped) attention, output projection.  Returns (output, lengths after the step)."""
    dh = W_[0].shape[0] // heads
    q, k, v = (O.linear_forward(x, W_[i], Bs[i]) for i in range(3))
    if rope is not None:
        q = RO.rope(q, start, T, heads, dh, rope.rot, rope.interleaved, rope.table)
        k = RO.rope(k, start, T, kv_heads, dh, rope.rot, rope.interleaved, rope.table)
    append(kc, vc, k, v, start, T, ring)
    ctx = decode_forward(q, kc, vc, start, T, window, ring, H=heads)
    return O.linear_forward(ctx, W_[3], Bs[3]), np.asarray(start) + T


# ---- full sequences ----------------------------------------------------------------------------------------------------------------
def band_mask(s, W, dtype):
    """The constant operand of the Addition node: 0 where query - W < key <= query, -inf elsewhere."""
    r, k = np.arange(s)[:, None], np.arange(s)[None, :]
    m = np.zeros((s, s), dtype=dtype)
    m[(k > r) | (k <= r - W)] = -np.inf
    return m


def attention_core_forward(q, k, v, heads, batch, p, noise, window):
    """tests/causal_oracle.py's core with the banded mask.  Returns (context, cache for `O.attention_core_backward`)."""
    dt = q.dtype
    scale = dt.type(1.0 / np.sqrt(q.shape[1] // heads))
    qh, kh, vh = (O._heads_split(t, batch, heads) for t in (q, k, v))
    sc = np.matmul(qh, kh.transpose(0, 2, 1))
    scs = sc * scale + band_mask(sc.shape[1], window, dt)
    pr = np.zeros_like(scs)
    O.softmax_forward(scs, pr, axis=2)
    pd = np.zeros_like(pr)
    O.dropout_forward(pr, pd, noise, p, True)
    o = O._heads_merge(np.matmul(pd, vh), batch, heads)
    return o, dict(qh=qh, kh=kh, vh=vh, scores=sc, probs=pr, dropped=pd, noise=noise, p=p, scale=scale, heads=heads, batch=batch)


attention_core_backward = O.attention_core_backward


def mha_forward_backward(x, wq, bq, wk, bk, wv, bv, wo, bo, heads, kv_heads, batch, p, noise, g_out, window, rope=None):
    """tests/gqa_oracle.py's module around the banded core: projections, rotate q (heads) and k (kv_heads), repeat k and v, the
    core, out-projection; backward: the core, the sum of the copies, the inverse rotations, the linears.  (kv_heads == heads: the
    repeat is the identity and its backward a sum of one term.)"""
    S, dh, G = x.shape[0] // batch, wq.shape[0] // heads, heads // kv_heads
    assert G * kv_heads == heads and wk.shape[0] == kv_heads * dh and wv.shape[0] == kv_heads * dh
    if rope is None:
        rot = lambda t, nh, inv=False: t
    else:
        rot = lambda t, nh, inv=False: RO.rope(t, None, S, nh, dh, rope.rot, rope.interleaved, rope.table, inverse=inv)
    q, k, v = O.linear_forward(x, wq, bq), O.linear_forward(x, wk, bk), O.linear_forward(x, wv, bv)
    kf, vf = GO.repeat_kv(rot(k, kv_heads), kv_heads, G, dh), GO.repeat_kv(v, kv_heads, G, dh)
    o, cache = attention_core_forward(rot(q, heads), kf, vf, heads, batch, p, noise, window)
    out = O.linear_forward(o, wo, bo)
    g = g_out
    dbo = np.zeros_like(bo); O.accumulate(dbo, g)
    dwo = np.zeros_like(wo); O.mm_t_backward_right(dwo, g, o)
    do = np.zeros_like(o); O.mm_t_backward_left(do, g, wo)
    core = attention_core_backward(cache, do)
    dq = rot(core["dq"], heads, True)
    dk = rot(GO.repeat_kv_backward(core["dk"], kv_heads, G, dh), kv_heads, True)
    dv = GO.repeat_kv_backward(core["dv"], kv_heads, G, dh)
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


def mha_forward(x, W_, Bs, heads, kv_heads, batch, window, rope=None):
    """The module's inference forward (no dropout) with the banded core: W_ / Bs = the q, k, v, o weights and biases."""
    S, dh, G = x.shape[0] // batch, W_[0].shape[0] // heads, heads // kv_heads
    q, k, v = (O.linear_forward(x, W_[i], Bs[i]) for i in range(3))
    if rope is not None:
        q = RO.rope(q, None, S, heads, dh, rope.rot, rope.interleaved, rope.table)
        k = RO.rope(k, None, S, kv_heads, dh, rope.rot, rope.interleaved, rope.table)
    ctx, _ = attention_core_forward(q, GO.repeat_kv(k, kv_heads, G, dh), GO.repeat_kv(v, kv_heads, G, dh), heads, batch, 0.0,
                                    np.ones((batch * heads, S, S), dtype=x.dtype), window)
    return O.linear_forward(ctx, W_[3], Bs[3])


# ---- the chunks a window touches -----------------------------------------------------------------------------------------------------
def chunk_bound(W, C):
    """nk_attention_decode_window_workspace's per-problem chunk count"""
    return (W + C - 2) // C + 1

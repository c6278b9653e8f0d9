"""The oracle of packed sequences (document-masked causal attention; semantics: include/neuronika_hip.h, nk_attention_seg_fwd), in
NumPy, in the dtype it is called with.  Query position r of sample b attends to the keys lo_eff[b][r] .. r,
    lo_eff[r] = min(r, max(lo[b][r], r - span + 1, 0)).

It is tests/window_oracle.py's composition - tests/causal_oracle.py's core with a constant on the Addition node - with the
PER-SAMPLE constant M_b[r][k] = 0 for lo_eff[b][r] <= k <= r and -inf elsewhere, built from a (B, S) array.  Every row keeps its
diagonal, so Softmax and the backward nodes need nothing new.  Everything is built from the oracle's own node functions
(oracle.neuronika_oracle) and tests/window_oracle.py; only the mask and the per-row rotary positions are added.
tests/test_oracle_segments.py pins it against tests/window_oracle.py (band edges) and against the causal oracle run on every document
alone (block-diagonal layouts)."""
import numpy as np

import gqa_oracle as GO
import rope_oracle as RO
import window_oracle as WO
from oracle import neuronika_oracle as O


def layout(S, doc_lens):
    """(lo, pos, max_len) of nn::Segments: doc_lens holds per sample a list of positive lengths with sum <= S; a remainder forms one
    more document (the padding tail).  lo[b][t] = start of t's document, pos = t - lo, max_len = the longest document."""
    lo = np.zeros((len(doc_lens), S), np.int32)
    longest = 0
    for b, lens in enumerate(doc_lens):
        lens = [int(n) for n in lens]
        assert all(n > 0 for n in lens) and sum(lens) <= S, (b, lens)
        if sum(lens) < S:
            lens = lens + [S - sum(lens)]
        t = 0
        for n in lens:
            lo[b, t:t + n] = t
            t += n
        longest = max(longest, max(lens))
    pos = (np.arange(S, dtype=np.int32)[None, :] - lo).astype(np.int32)
    return lo, pos, longest


def band_lo(B, S, W):
    """The array that restates a sliding window: lo[b][r] = max(0, r - W + 1)."""
    return np.tile(np.maximum(0, np.arange(S) - W + 1).astype(np.int32), (B, 1))


def lo_eff(lo, span):
    """The kernels' clamp, in int64 (no content of `lo` overflows it)."""
    lo = np.asarray(lo, dtype=np.int64)
    r = np.arange(lo.shape[1], dtype=np.int64)[None, :]
    return np.minimum(r, np.maximum(np.maximum(lo, r - int(span) + 1), 0))


def allowed(lo, span):
    """(B, S, S) bool: lo_eff[b][r] <= k <= r"""
    le = lo_eff(lo, span)
    S = le.shape[1]
    r, k = np.arange(S)[None, :, None], np.arange(S)[None, None, :]
    return (k <= r) & (k >= le[:, :, None])


def seg_mask(lo, span, dtype):
    """The constant operand of the Addition node, per sample: (B, S, S), 0 where allowed, -inf elsewhere."""
    m = np.zeros(allowed(lo, span).shape, dtype=dtype)
    m[~allowed(lo, span)] = -np.inf
    return m


def attention_core_forward(q, k, v, heads, batch, p, noise, lo, span):
    """tests/window_oracle.py's core with the per-sample mask (shared by a sample's heads).  Returns (context, cache for
    `O.attention_core_backward`)."""
    dt = q.dtype
    scale = dt.type(1.0 / np.sqrt(q.shape[1] // heads))
    qh, kh, vh = (O._heads_split(t, batch, heads) for t in (q, k, v))
    sc = np.matmul(qh, kh.transpose(0, 2, 1))
    scs = sc * scale + np.repeat(seg_mask(lo, span, dt), heads, axis=0)
    pr = np.zeros_like(scs)
    O.softmax_forward(scs, pr, axis=2)
    pd = np.zeros_like(pr)
    O.dropout_forward(pr, pd, noise, p, True)
    o = O._heads_merge(np.matmul(pd, vh), batch, heads)
    return o, dict(qh=qh, kh=kh, vh=vh, scores=sc, probs=pr, dropped=pd, noise=noise, p=p, scale=scale, heads=heads, batch=batch)


attention_core_backward = O.attention_core_backward


def mha_forward_backward(x, wq, bq, wk, bk, wv, bv, wo, bo, heads, kv_heads, batch, p, noise, g_out, lo, span, pos=None, rope=None):
    """tests/window_oracle.py's module around the document-masked core.  With `rope`, row t of sample b is rotated at pos[b][t] (the
    position inside its document), q on `heads` heads and k on `kv_heads`."""
    dh, G = wq.shape[0] // heads, heads // kv_heads
    assert G * kv_heads == heads and wk.shape[0] == kv_heads * dh and wv.shape[0] == kv_heads * dh
    if rope is None:
        rot = lambda t, nh, inv=False: t
    else:
        start = np.asarray(pos).reshape(-1)
        rot = lambda t, nh, inv=False: RO.rope(t, start, 1, nh, dh, rope.rot, rope.interleaved, rope.table, inverse=inv)
    q, k, v = O.linear_forward(x, wq, bq), O.linear_forward(x, wk, bk), O.linear_forward(x, wv, bv)
    kf, vf = GO.repeat_kv(rot(k, kv_heads), kv_heads, G, dh), GO.repeat_kv(v, kv_heads, G, dh)
    o, cache = attention_core_forward(rot(q, heads), kf, vf, heads, batch, p, noise, lo, span)
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

"""The oracle of causal self-attention: `oracle/neuronika_oracle.py`'s node-by-node composition of the multi-head attention with ONE
more node - an a-4 Addition (node/addition/mod.rs:39-50) of the constant (S, S) mask M (0 where key <= query, -inf above the
diagonal), broadcast over batch * heads, in front of the Softmax:

    P = dropout(softmax(Q_bh.mm_t(K_bh) * scale + M, axis 1))

Softmax (node/softmax/mod.rs:37-53) gives exactly 0 at the -inf entries and every row keeps its diagonal, so the backward nodes
need nothing new: AdditionBackward passes the gradient through (M is a constant) and `attention_core_backward` reads the cache as
it is.  Everything here is built from the oracle's own node functions, in the dtype it is called with; only the mask is added.
tests/test_oracle_causal.py pins it against an independent per-row restatement."""
import numpy as np

from oracle import neuronika_oracle as O


def causal_mask(s, dtype):
    """The constant operand of the Addition node: 0 where key <= query, -inf above the diagonal."""
    m = np.zeros((s, s), dtype=dtype)
    m[np.triu_indices(s, 1)] = -np.inf
    return m


def attention_core_forward(q, k, v, heads, batch, p, noise, causal=True):
    """`O.attention_core_forward` with the mask added to the scaled scores.  Returns (context, cache for `O.attention_core_backward`)."""
    if not causal:
        return O.attention_core_forward(q, k, v, heads, batch, p, noise)
    dt = q.dtype
    scale = dt.type(1.0 / np.sqrt(q.shape[1] // heads))
    qh, kh, vh = (O._heads_split(t, batch, heads) for t in (q, k, v))
    sc = np.matmul(qh, kh.transpose(0, 2, 1))
    scs = sc * scale + causal_mask(sc.shape[1], dt)
    pr = np.zeros_like(scs)
    O.softmax_forward(scs, pr, axis=2)
    pd = np.zeros_like(pr)
    O.dropout_forward(pr, pd, noise, p, True)
    o = O._heads_merge(np.matmul(pd, vh), batch, heads)
    return o, dict(qh=qh, kh=kh, vh=vh, scores=sc, probs=pr, dropped=pd, noise=noise, p=p, scale=scale, heads=heads, batch=batch)


attention_core_backward = O.attention_core_backward


def mha_forward_backward(x, wq, bq, wk, bk, wv, bv, wo, bo, heads, batch, p, noise, g_out, causal=True):
    """`O.mha_forward_backward` around the causal core: projections, core, out-projection and their backward nodes."""
    if not causal:
        return O.mha_forward_backward(x, wq, bq, wk, bk, wv, bv, wo, bo, heads, batch, p, noise, g_out)
    q, k, v = O.linear_forward(x, wq, bq), O.linear_forward(x, wk, bk), O.linear_forward(x, wv, bv)
    o, cache = attention_core_forward(q, k, v, heads, batch, p, noise)
    out = O.linear_forward(o, wo, bo)
    g = g_out
    dbo = np.zeros_like(bo); O.accumulate(dbo, g)
    dwo = np.zeros_like(wo); O.mm_t_backward_right(dwo, g, o)
    do = np.zeros_like(o); O.mm_t_backward_left(do, g, wo)
    core = O.attention_core_backward(cache, do)
    grads = {}
    dx = np.zeros_like(x)
    for name, w, b, dz in (("q", wq, bq, core["dq"]), ("k", wk, bk, core["dk"]), ("v", wv, bv, core["dv"])):
        db = np.zeros_like(b); O.accumulate(db, dz)
        dw = np.zeros_like(w); O.mm_t_backward_right(dw, dz, x)
        O.mm_t_backward_left(dx, dz, w)
        grads["w" + name], grads["b" + name] = dw, db
    grads.update(wo=dwo, bo=dbo, x=dx)
    return out, grads

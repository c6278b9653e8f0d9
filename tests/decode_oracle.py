"""The oracle of incremental decoding: a key / value cache in NumPy and the single-query attention over it, per (sample, head, new
row), in the dtype it is called with.

    n = min(start[b] + t + 1, cap);   o = softmax(q . K_bh[0:n]^T * scale) . V_bh[0:n]

The per-row chain is the oracle's own node functions where they exist (`O.softmax_forward`, node/softmax/mod.rs:37-53; the two
products are NumPy matmuls as in `O.attention_core_forward`).  tests/test_oracle_decode.py pins it against
tests/causal_oracle.py: stepping token by token reproduces the rows of the causal core's forward."""
import numpy as np

from oracle import neuronika_oracle as O


def new_cache(batch, heads, cap, dh, dtype, fill=0.0):
    return (np.full((batch, heads, cap, dh), fill, dtype=dtype), np.full((batch, heads, cap, dh), fill, dtype=dtype))


def append(kc, vc, k, v, start, T):
    """Row b*T + t of k / v ((B*T, H*dh)) -> position start[b] + t of every head of sample b; positions >= cap are dropped."""
    B, H, cap, dh = kc.shape
    for b in range(B):
        for t in range(T):
            pos = int(start[b]) + t
            if pos < 0 or pos >= cap:
                continue
            kc[b, :, pos, :] = k[b * T + t].reshape(H, dh)
            vc[b, :, pos, :] = v[b * T + t].reshape(H, dh)


def decode_forward(q, kc, vc, start, T, scale=None):
    """q (B*T, H*dh); kc / vc (B, H, cap, dh) already holding the step's rows; start (B,) lengths before the step -> (B*T, H*dh)."""
    B, H, cap, dh = kc.shape
    dt = q.dtype
    scale = dt.type(1.0 / np.sqrt(dh)) if scale is None else dt.type(scale)
    out = np.zeros((B * T, H * dh), dtype=dt)
    for b in range(B):
        for t in range(T):
            n = min(int(start[b]) + t + 1, cap)
            if n <= 0:
                continue
            for h in range(H):
                qr = q[b * T + t, h * dh:(h + 1) * dh].reshape(1, dh)
                sc = np.matmul(qr, kc[b, h, :n].T) * scale
                pr = np.zeros_like(sc)
                O.softmax_forward(sc, pr, axis=1)
                out[b * T + t, h * dh:(h + 1) * dh] = np.matmul(pr, vc[b, h, :n])[0]
    return out


def step(q, k, v, kc, vc, start, T, scale=None):
    """One decoding step: append the new rows, attend, return (context, lengths after the step)."""
    append(kc, vc, k, v, start, T)
    return decode_forward(q, kc, vc, start, T, scale), np.asarray(start) + T


def mha_step(x, W, Bs, heads, kc, vc, start, T):
    """The module's step: projections (W / Bs = the q, k, v, o weights and biases), append, attention, output projection."""
    q, k, v = (O.linear_forward(x, W[i], Bs[i]) for i in range(3))
    ctx, after = step(q, k, v, kc, vc, start, T)
    return O.linear_forward(ctx, W[3], Bs[3]), after

"""Oracle of the group normalisation (the reference has no such layer, so neither does oracle/neuronika_oracle.py): the semantics
include/neuronika_hip.h fixes, in NumPy.  dtype-generic: arrays of float64 give the f64 oracle, arrays of float32 its two-pass
f32 twin (every intermediate stays in the input's dtype), as the suite's parity rule needs both.  x is (N, C, L), G groups of
Cg = C / G channels; group row (n, j) is the D = Cg * L values x[n, j * Cg : (j + 1) * Cg, :].

    mean = sum(x) / D ;  var = sum((x - mean)^2) / D  (biased, centred) ;  rstd = 1 / sqrt(var + eps)
    xhat = (x - mean) * rstd ;  y = xhat * gamma[c] + beta[c]
    gh = g * gamma[c] ;  dx = rstd * (gh - mean_D(gh) - xhat * mean_D(gh * xhat))
    dgamma[c] = sum over n, l of g * xhat ;  dbeta[c] = sum over n, l of g
G == C is instance normalisation, G == 1 layer normalisation over (C, L) with a per-channel affine.
"""
import numpy as np


def _rows(a, G):
    N, C, L = a.shape
    return a.reshape(N * G, (C // G) * L)


def group_stats(x, G, eps=1e-5):
    """x (N, C, L) -> stats (N * G, 2) = {mean, rstd}, in x's dtype"""
    dt = x.dtype
    r = _rows(x, G)
    D = dt.type(r.shape[1])
    mean = r.sum(axis=1, dtype=dt) / D
    c = r - mean[:, None]
    var = (c * c).sum(axis=1, dtype=dt) / D
    return np.stack([mean, dt.type(1) / np.sqrt(var + dt.type(eps))], axis=1)


def _xhat(x, G, stats):
    return ((_rows(x, G) - stats[:, :1]) * stats[:, 1:]).reshape(x.shape)


def normalise(x, G, stats, gamma=None, beta=None):
    dt = x.dtype
    y = _xhat(x, G, stats)
    if gamma is not None:
        y = y * gamma.astype(dt, copy=False).reshape(1, -1, 1)
    if beta is not None:
        y = y + beta.astype(dt, copy=False).reshape(1, -1, 1)
    return y


def backward(g, x, G, gamma, stats):
    """the contributions the device adds to (or assigns to) dx, dgamma, dbeta; gamma may be None"""
    dt = x.dtype
    xhat = _xhat(x, G, stats)
    gh = g * gamma.astype(dt, copy=False).reshape(1, -1, 1) if gamma is not None else g
    D = dt.type(_rows(x, G).shape[1])
    c1 = _rows(gh, G).sum(axis=1, dtype=dt) / D
    c2 = _rows(gh * xhat, G).sum(axis=1, dtype=dt) / D
    dx = (stats[:, 1:] * (_rows(gh, G) - c1[:, None] - _rows(xhat, G) * c2[:, None])).reshape(x.shape)
    return dx, (g * xhat).sum(axis=(0, 2), dtype=dt), g.sum(axis=(0, 2), dtype=dt)


def both(x, G, gamma, beta, g, eps=1e-5):
    """f64 oracle and f32 twin of one forward + backward on f32 inputs: two dicts with y, stats, dx, dgamma, dbeta"""
    out = []
    for dt in (np.float64, np.float32):
        c = lambda a: None if a is None else np.asarray(a, dtype=dt)
        xx = c(x)
        st = group_stats(xx, G, eps)
        dx, dg, db = backward(c(g), xx, G, c(gamma), st)
        out.append(dict(y=normalise(xx, G, st, c(gamma), c(beta)), stats=st, dx=dx, dgamma=dg, dbeta=db))
    return out

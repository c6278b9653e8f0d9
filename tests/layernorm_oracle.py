"""Oracle of the layer normalisation (the reference has no such layer, so neither does oracle/neuronika_oracle.py): the
semantics include/neuronika_hip.h fixes, in NumPy.  dtype-generic: arrays of float64 give the f64 oracle, arrays of float32
its f32 twin (every intermediate stays in the input's dtype), as the suite's parity rule needs both.

    mean = sum(x) / D ;  var = sum((x - mean)^2) / D   (biased, second pass over the centred values)
    rstd = 1 / sqrt(var + eps) ;  xhat = (x - mean) * rstd ;  y = xhat * gamma + beta
    gh = g * gamma ;  dx = rstd * (gh - mean_D(gh) - xhat * mean_D(gh * xhat)) ;  dgamma = sum_rows g * xhat ;  dbeta = sum_rows g
"""
import numpy as np


def forward(x, gamma=None, beta=None, eps=1e-5):
    """x (rows, D); gamma, beta (D,) or None.  Returns y (rows, D) and stats (rows, 2) = {mean, rstd}, in x's dtype."""
    dt = x.dtype
    D = dt.type(x.shape[1])
    mean = x.sum(axis=1, keepdims=True, dtype=dt) / D
    c = x - mean
    var = (c * c).sum(axis=1, keepdims=True, dtype=dt) / D
    rstd = dt.type(1) / np.sqrt(var + dt.type(eps))
    y = c * rstd
    if gamma is not None:
        y = y * gamma.astype(dt, copy=False)
    if beta is not None:
        y = y + beta.astype(dt, copy=False)
    return y, np.concatenate([mean, rstd], axis=1)


def backward(g, x, gamma, stats):
    """The contributions the device adds to (or assigns to) dx, dgamma, dbeta; gamma may be None."""
    dt = x.dtype
    D = dt.type(x.shape[1])
    mean, rstd = stats[:, :1].astype(dt, copy=False), stats[:, 1:].astype(dt, copy=False)
    xhat = (x - mean) * rstd
    gh = g * gamma.astype(dt, copy=False) if gamma is not None else g
    c1 = gh.sum(axis=1, keepdims=True, dtype=dt) / D
    c2 = (gh * xhat).sum(axis=1, keepdims=True, dtype=dt) / D
    dx = rstd * (gh - c1 - xhat * c2)
    return dx, (g * xhat).sum(axis=0, dtype=dt), g.sum(axis=0, dtype=dt)


def both(x, gamma, beta, g, eps=1e-5):
    """f64 oracle and f32 twin of one forward + backward on f32 inputs: two dicts with y, stats, dx, dgamma, dbeta."""
    out = []
    for dt in (np.float64, np.float32):
        c = lambda a: None if a is None else np.asarray(a, dtype=dt)
        y, st = forward(c(x), c(gamma), c(beta), eps)
        dx, dg, db = backward(c(g), c(x), c(gamma), st)
        out.append(dict(y=y, stats=st, dx=dx, dgamma=dg, dbeta=db))
    return out

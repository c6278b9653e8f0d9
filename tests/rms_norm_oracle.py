"""Oracle of the RMS normalisation (the reference has no such layer, so neither does oracle/neuronika_oracle.py): the semantics
include/neuronika_hip.h fixes, in NumPy.  dtype-generic: arrays of float64 give the f64 oracle, arrays of float32 its f32 twin
(every intermediate stays in the input's dtype), as the suite's parity rule needs both.

    ms = sum(x * x) / D  (no centring) ;  rstd = 1 / sqrt(ms + eps) ;  xhat = x * rstd ;  y = xhat * gamma
    gh = g * gamma ;  dx = rstd * (gh - xhat * sum_D(gh * xhat) / D) ;  dgamma = sum_rows g * xhat
"""
import numpy as np


def forward(x, gamma=None, eps=1e-6):
    """x (rows, D); gamma (D,) or None.  Returns y (rows, D) and stats (rows,) = rstd, in x's dtype."""
    dt = x.dtype
    D = dt.type(x.shape[1])
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        ms = (x * x).sum(axis=1, keepdims=True, dtype=dt) / D
        rstd = dt.type(1) / np.sqrt(ms + dt.type(eps))
        y = x * rstd
        if gamma is not None:
            y = y * gamma.astype(dt, copy=False)
    return y, rstd[:, 0]


def backward(g, x, gamma, stats):
    """The contributions the device adds to (or assigns to) dx and dgamma; gamma may be None."""
    dt = x.dtype
    D = dt.type(x.shape[1])
    rstd = stats.astype(dt, copy=False).reshape(-1, 1)
    with np.errstate(over="ignore", invalid="ignore"):
        xhat = x * rstd
        gh = g * gamma.astype(dt, copy=False) if gamma is not None else g
        c = (gh * xhat).sum(axis=1, keepdims=True, dtype=dt) / D
        dx = rstd * (gh - xhat * c)
        return dx, (g * xhat).sum(axis=0, dtype=dt)


def both(x, gamma, g, eps=1e-6):
    """f64 oracle and f32 twin of one forward + backward on f32 inputs: two dicts with y, stats, dx, dgamma."""
    out = []
    for dt in (np.float64, np.float32):
        c = lambda a: None if a is None else np.asarray(a, dtype=dt)
        y, st = forward(c(x), c(gamma), eps)
        dx, dg = backward(c(g), c(x), c(gamma), st)
        out.append(dict(y=y, stats=st, dx=dx, dgamma=dg))
    return out

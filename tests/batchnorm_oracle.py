"""Oracle of the batch normalisation (the reference has no such layer, so neither does oracle/neuronika_oracle.py): the
semantics include/neuronika_hip.h fixes, in NumPy.  dtype-generic: arrays of float64 give the f64 oracle, arrays of float32
its f32 twin (every intermediate stays in the input's dtype), as the suite's parity rule needs both.  x is (N, C, L).

    per channel over M = N * L values:  mean = sum(x) / M ;  var = sum((x - mean)^2) / M  (biased, centred)
    rstd = 1 / sqrt(var + eps) ;  xhat = (x - mean) * rstd ;  y = xhat * gamma + beta
    training: running_mean = (1 - m) running_mean + m mean ;  running_var = (1 - m) running_var + m var M / (M - 1)
    inference: mean = running_mean, rstd = 1 / sqrt(running_var + eps)
    s0 = sum g ;  s1 = sum g * xhat ;  dbeta = s0 ;  dgamma = s1
    dx = gamma rstd (g - s0 / M - xhat s1 / M)  in training,  gamma rstd g  in inference
"""
import numpy as np


def _c(v, dt):
    return v.astype(dt, copy=False).reshape(1, -1, 1)


def batch_stats(x, eps=1e-5):
    """x (N, C, L) -> stats (C, 2) = {mean, rstd} and the biased variance (C,), in x's dtype"""
    dt = x.dtype
    M = dt.type(x.shape[0] * x.shape[2])
    mean = x.sum(axis=(0, 2), dtype=dt) / M
    c = x - _c(mean, dt)
    var = (c * c).sum(axis=(0, 2), dtype=dt) / M
    rstd = dt.type(1) / np.sqrt(var + dt.type(eps))
    return np.stack([mean, rstd], axis=1), var


def running_stats(stats, eps=1e-5):
    """the inference statistics: stats = {running_mean, 1 / sqrt(running_var + eps)}"""
    rm, rv = stats
    dt = rm.dtype
    return np.stack([rm, dt.type(1) / np.sqrt(rv + dt.type(eps))], axis=1)


def running_update(rm, rv, stats, var, M, momentum=0.1):
    dt = rm.dtype
    m = dt.type(momentum)
    return (dt.type(1) - m) * rm + m * stats[:, 0], (dt.type(1) - m) * rv + m * (var * dt.type(M / (M - 1.0)))


def normalise(x, stats, gamma=None, beta=None):
    dt = x.dtype
    y = (x - _c(stats[:, 0], dt)) * _c(stats[:, 1], dt)
    if gamma is not None:
        y = y * _c(gamma, dt)
    if beta is not None:
        y = y + _c(beta, dt)
    return y


def backward(g, x, gamma, stats, training=True):
    """sums (C, 2) = {s0, s1} and the contributions the device adds to (or assigns to) dx, dgamma, dbeta; gamma may be None"""
    dt = x.dtype
    M = dt.type(x.shape[0] * x.shape[2])
    mean, rstd = _c(stats[:, 0], dt), _c(stats[:, 1], dt)
    xhat = (x - mean) * rstd
    s0, s1 = g.sum(axis=(0, 2), dtype=dt), (g * xhat).sum(axis=(0, 2), dtype=dt)
    gr = rstd * _c(gamma, dt) if gamma is not None else rstd
    dx = gr * (g - _c(s0 / M, dt) - xhat * _c(s1 / M, dt)) if training else gr * g
    return np.stack([s0, s1], axis=1), dx, s1, s0


def both(x, gamma, beta, g, eps=1e-5, momentum=0.1, running=None, training=True):
    """f64 oracle and f32 twin of one forward + backward on f32 inputs: two dicts with y, stats, running_mean, running_var,
    sums, dx, dgamma, dbeta.  `running` = (running_mean, running_var) before the call, or None."""
    out = []
    for dt in (np.float64, np.float32):
        c = lambda a: None if a is None else np.asarray(a, dtype=dt)
        xx, r = c(x), (None if running is None else (c(running[0]), c(running[1])))
        M = xx.shape[0] * xx.shape[2]
        if training:
            st, var = batch_stats(xx, eps)
            rm, rv = running_update(r[0], r[1], st, var, M, momentum) if r is not None else (None, None)
        else:
            st, (rm, rv) = running_stats(r, eps), r
        y = normalise(xx, st, c(gamma), c(beta))
        sums, dx, dg, db = backward(c(g), xx, c(gamma), st, training)
        out.append(dict(y=y, stats=st, running_mean=rm, running_var=rv, sums=sums, dx=dx, dgamma=dg, dbeta=db))
    return out

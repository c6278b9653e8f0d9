"""Oracle of max / average pooling and flatten (the reference has no pooling, so neither does oracle/neuronika_oracle.py): the
semantics include/neuronika_hip.h fixes, in NumPy.  dtype-generic: arrays of float64 give the f64 oracle, arrays of float32 its
f32 twin (every intermediate stays in the input's dtype).  x is (N, C, in_1 .. in_nd), nd = 1, 2, 3; kernel / stride / padding
are sequences of nd ints.

    out_i = (in_i + 2 p_i - k_i) // s_i + 1, floor mode, dilation 1, 0 <= p_i <= k_i // 2
    max:  the first maximum in row-major window order (`>`), padding never selected; the first NaN met wins; idx = the offset
          of the selected element inside its own (n, c) plane (int32)
    avg:  row-major sum of the in-range positions / (prod k_i  or  the number of in-range positions)
    backward: dx[idx[o]] += g[o]  /  dx[i] += sum over the windows holding i of g[o] / divisor(o)
"""
import itertools

import numpy as np


def out_shape(x_shape, kernel, stride, padding):
    """(N, C, out...) or ValueError for a geometry outside the contract"""
    nd = len(x_shape) - 2
    if not 1 <= nd <= 3 or not (len(kernel) == len(stride) == len(padding) == nd):
        raise ValueError("nd")
    if x_shape[0] < 0 or x_shape[1] < 0:
        raise ValueError("negative extent")
    out, pin, pout = [], 1, 1
    for n, k, s, p in zip(x_shape[2:], kernel, stride, padding):
        if n < 1 or k < 1 or s < 1 or p < 0 or p > k // 2 or n + 2 * p - k < 0:
            raise ValueError("axis")
        out.append((n + 2 * p - k) // s + 1)
        pin, pout = pin * n, pout * out[-1]
        if pin > 2 ** 31 - 1 or pout > 2 ** 31 - 1:
            raise ValueError("plane")
    return (x_shape[0], x_shape[1], *out)


def _geometry(x_shape, kernel, stride, padding):
    stride = tuple(stride) if len(stride) else tuple(kernel)
    return tuple(x_shape[2:]), out_shape(x_shape, kernel, stride, padding)[2:], tuple(kernel), stride, tuple(padding)


def _padded(x, padding, value):
    return np.pad(x, [(0, 0), (0, 0)] + [(p, p) for p in padding], constant_values=value)


def _window_slices(t, out, stride):
    """the strided view of a padded array that holds, for every output position, the window element at offset t"""
    return (slice(None), slice(None)) + tuple(slice(ti, ti + (o - 1) * s + 1, s) for ti, o, s in zip(t, out, stride))


def _positions(t, inn, out, stride, padding):
    """per output position: the input coordinates of window element t (broadcastable index arrays), and whether it is in range"""
    nd = len(inn)
    pos, ok = [], True
    for a in range(nd):
        shape = [1] * nd
        shape[a] = out[a]
        c = (np.arange(out[a]) * stride[a] - padding[a] + t[a]).reshape(shape)
        pos.append(c)
        ok = ok & (c >= 0) & (c < inn[a])
    return pos, np.broadcast_to(ok, out)


def _ravel(pos, inn):
    off = 0
    for c, n in zip(pos, inn):
        off = off * n + c
    return off


def max_pool_fwd(x, kernel, stride=(), padding=None):
    padding = tuple(padding) if padding is not None else (0,) * len(kernel)
    inn, out, k, s, p = _geometry(x.shape, kernel, stride, padding)
    xp = _padded(x, p, -np.inf)
    best = np.full(x.shape[:2] + out, -np.inf, dtype=x.dtype)
    first = [np.maximum(c, 0) for c in _positions((0,) * len(k), inn, out, s, p)[0]]
    idx = np.broadcast_to(_ravel(first, inn), best.shape).astype(np.int32).copy()
    for t in itertools.product(*[range(ki) for ki in k]):
        cand = xp[_window_slices(t, out, s)]
        pos, ok = _positions(t, inn, out, s, p)
        with np.errstate(invalid="ignore"):
            take = ok & ((cand > best) | (np.isnan(cand) & ~np.isnan(best)))
        best = np.where(take, cand, best)
        idx = np.where(take, np.broadcast_to(_ravel(pos, inn), best.shape).astype(np.int32), idx)
    return best, idx


def _divisor(inn, out, k, s, p, count_include_pad, dtype):
    if count_include_pad:
        return np.full(out, np.prod(k), dtype=dtype)
    div = np.ones(out, dtype=np.int64)
    for a in range(len(inn)):
        shape = [1] * len(inn)
        shape[a] = out[a]
        lo = np.arange(out[a]) * s[a] - p[a]
        div = div * (np.minimum(lo + k[a], inn[a]) - np.maximum(lo, 0)).reshape(shape)
    return div.astype(dtype)


def avg_pool_fwd(x, kernel, stride=(), padding=None, count_include_pad=True):
    padding = tuple(padding) if padding is not None else (0,) * len(kernel)
    inn, out, k, s, p = _geometry(x.shape, kernel, stride, padding)
    xp = _padded(x, p, 0)
    acc = np.zeros(x.shape[:2] + out, dtype=x.dtype)
    for t in itertools.product(*[range(ki) for ki in k]):
        acc = acc + xp[_window_slices(t, out, s)]
    return acc / _divisor(inn, out, k, s, p, count_include_pad, x.dtype)


def max_pool_bwd(g, idx, x_shape):
    """dx (x_shape) of an all-zero start, in g's dtype"""
    planes = x_shape[0] * x_shape[1]
    dx = np.zeros((planes, int(np.prod(x_shape[2:]))), dtype=g.dtype)
    if planes:
        rows = np.repeat(np.arange(planes), idx.size // planes)
        np.add.at(dx, (rows, idx.reshape(-1).astype(np.int64)), g.reshape(-1))
    return dx.reshape(x_shape)


def avg_pool_bwd(g, x_shape, kernel, stride=(), padding=None, count_include_pad=True):
    padding = tuple(padding) if padding is not None else (0,) * len(kernel)
    inn, out, k, s, p = _geometry(x_shape, kernel, stride, padding)
    dxp = np.zeros(tuple(x_shape[:2]) + tuple(n + 2 * pi for n, pi in zip(inn, p)), dtype=g.dtype)
    share = g / _divisor(inn, out, k, s, p, count_include_pad, g.dtype)
    for t in itertools.product(*[range(ki) for ki in k]):
        dxp[_window_slices(t, out, s)] += share
    crop = (slice(None), slice(None)) + tuple(slice(pi, pi + n) for pi, n in zip(p, inn))
    return np.ascontiguousarray(dxp[crop])


def global_avg_pool_fwd(x):
    return avg_pool_fwd(x, x.shape[2:], x.shape[2:], (0,) * (x.ndim - 2))


def flatten(x):
    return x.reshape(x.shape[0], -1)


def flatten_bwd(g, x_shape):
    return g.reshape(x_shape)

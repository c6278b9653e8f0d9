"""The smooth and gated activations of include/neuronika_hip.h restated in float64 NumPy, forward and backward: GELU (erfc form),
GELU (tanh form), SiLU, sigmoid, and the gated form y[r, j] = x[r, j] * act(x[r, H + j]).  Test infrastructure only: nothing under
neuronika_amd/ imports it.  `math.erfc` through `np.frompyfunc`: no SciPy.  Every formula is written so that it neither overflows nor
cancels in float64 over the whole finite float32 range (the sigmoid from exp(-|v|), the tanh form as x * sigmoid(2 u)); NaN passes
through to its own element."""
import math

import numpy as np

ACTIVATIONS = ("gelu", "gelu_tanh", "silu", "sigmoid")
C3 = 0.044715
K = math.sqrt(2.0 / math.pi)

_erfc = np.frompyfunc(lambda v: math.erfc(v) if v == v else float("nan"), 1, 1)

# +-{1e-30, 1e-6, 0.5, 5, 9, 20, 88, 100, 1e4, 1e13, 1e20, 3e38} and +-0
EXTREME = np.array([s * m for m in (0.0, 1e-30, 1e-6, 0.5, 5.0, 9.0, 20.0, 88.0, 100.0, 1e4, 1e13, 1e20, 3e38) for s in (1.0, -1.0)], np.float32)


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _sigma(v):
    """(sigma(v), sigma(v) (1 - sigma(v))) without overflow or cancellation"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e = np.exp(-np.abs(v))
        r = 1.0 / (1.0 + e)
        return np.where(v >= 0, r, e * r), e * r * r


def value_and_derivative(act, x):
    """(act(x), act'(x)) in float64, elementwise"""
    x = _f64(x)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if act == "gelu":
            phi_big = 0.5 * _erfc(-x / math.sqrt(2.0)).astype(np.float64)
            phi_small = np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
            return x * phi_big, phi_big + x * phi_small
        if act == "gelu_tanh":
            u2 = 2.0 * K * (x + C3 * x ** 3)                       # 0.5 (1 + tanh u) = sigma(2 u)
            s, ss = _sigma(u2)
            du2 = 2.0 * K * (1.0 + 3.0 * C3 * x * x)
            return x * s, s + x * (ss * du2)                        # float64 holds x^3 and x^2 of every finite float32
        if act == "silu":
            s, ss = _sigma(x)
            return x * s, s + x * ss
        if act == "sigmoid":
            return _sigma(x)
    raise KeyError(act)


def forward(act, x):
    return value_and_derivative(act, x)[0]


def backward(act, x, g, dx0=None):
    """dx0 + g * act'(x) (dx0 = None: the assign form)"""
    d = _f64(g) * value_and_derivative(act, x)[1]
    return d if dx0 is None else _f64(dx0) + d


def glu_forward(act, x, H):
    x = _f64(x).reshape(-1, 2 * H)
    return x[:, :H] * value_and_derivative(act, x[:, H:])[0]


def glu_backward(act, x, g, H, dx0=None):
    """dx[r, j] = g act(b), dx[r, H + j] = g a act'(b), added to dx0 when it is given"""
    x, g = _f64(x).reshape(-1, 2 * H), _f64(g).reshape(-1, H)
    v, d = value_and_derivative(act, x[:, H:])
    out = np.concatenate([g * v, g * x[:, :H] * d], axis=1)
    return out if dx0 is None else _f64(dx0).reshape(-1, 2 * H) + out

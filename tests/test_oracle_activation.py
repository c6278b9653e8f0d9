"""tests/activation_oracle.py against torch on the CPU in float64: F.gelu (both forms), F.silu, torch.sigmoid, F.glu and the
a * F.gelu(b) / a * F.silu(b) gates - values and autograd gradients, on random inputs in [-6, 6] and on the extreme set.

Bound: 1e-12 relative, taken against max(|reference|, 1).  The floor of 1 is torch's own: its GELU is 0.5 x (1 + erf(x / sqrt 2)) and
0.5 x (1 + tanh u), whose `1 +` cancels in the negative tail with an absolute error of about |x| 2^-53 wherever the result is not yet
exactly 0, while the oracle's erfc / sigmoid forms keep the tail's leading digits; both are far inside 1e-12 absolute there."""
import os
import subprocess
import sys

import numpy as np

import activation_oracle as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    assert err.max() <= RTOL, (what, float(err.max()), int(err.argmax()))


def inputs():
    rng = np.random.default_rng(0)
    return {"random": rng.uniform(-6.0, 6.0, 4001), "extreme": A.EXTREME.astype(np.float64)}


# torch runs in a child process: a process that has loaded the HIP library must not import torch as well
_TORCH_CHECK = r"""
import sys
import numpy as np
import torch
import torch.nn.functional as F
sys.path.insert(0, sys.argv[1])
import activation_oracle as A
from test_oracle_activation import close, inputs
TORCH = {"gelu": lambda t: F.gelu(t, approximate="none"), "gelu_tanh": lambda t: F.gelu(t, approximate="tanh"), "silu": F.silu,
         "sigmoid": torch.sigmoid}
cases = 0
for act in A.ACTIVATIONS:
    for which, x in inputs().items():
        rng = np.random.default_rng(1)
        g, dx0 = rng.uniform(-1.0, 1.0, x.shape), rng.uniform(-1.0, 1.0, x.shape)   # `+=` starts from a non-zero destination
        t = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        y = TORCH[act](t)
        y.backward(torch.tensor(g, dtype=torch.float64))
        close(A.forward(act, x), y.detach().numpy(), act + " forward " + which)
        close(A.backward(act, x, g), t.grad.numpy(), act + " backward, assign form " + which)
        close(A.backward(act, x, g, dx0), dx0 + t.grad.numpy(), act + " backward, += form " + which)
        cases += 1
        for H in (1, 5, 8):
            rng = np.random.default_rng(2 + H)
            rows = 7
            b = rng.choice(x, (rows, H))
            a = rng.uniform(-1.0, 1.0, (rows, H))                # the gate takes the extremes; a * act(b) stays in range
            xx = np.concatenate([a, b], axis=1)
            g, dx0 = rng.uniform(-1.0, 1.0, (rows, H)), rng.uniform(-1.0, 1.0, (rows, 2 * H))
            t = torch.tensor(xx, dtype=torch.float64, requires_grad=True)
            y = F.glu(t, dim=-1) if act == "sigmoid" else t[:, :H] * TORCH[act](t[:, H:])
            y.backward(torch.tensor(g, dtype=torch.float64))
            close(A.glu_forward(act, xx, H), y.detach().numpy(), act + " glu forward " + which)
            close(A.glu_backward(act, xx, g, H), t.grad.numpy(), act + " glu backward, assign form " + which)
            close(A.glu_backward(act, xx, g, H, dx0), dx0 + t.grad.numpy(), act + " glu backward, += form " + which)
            cases += 1
print("cases", cases)
"""


def test_against_torch():
    """4 activations x (random, extreme) x (pointwise + the gated form at H = 1, 5, 8) = 32 cases, values and both backward forms"""
    r = subprocess.run([sys.executable, "-c", _TORCH_CHECK, os.path.join(ROOT, "tests")], capture_output=True, text=True)
    assert r.returncode == 0 and "cases 32" in r.stdout, r.stdout + r.stderr


def test_nan_stays_in_its_own_element():
    x = np.array([1.0, np.nan, -2.0, 0.5])
    for act in A.ACTIVATIONS:
        v, d = A.value_and_derivative(act, x)
        assert np.isnan(v).tolist() == [False, True, False, False] and np.isnan(d).tolist() == [False, True, False, False], act


def test_every_finite_f32_input_gives_finite_results():
    for act in A.ACTIVATIONS:
        v, d = A.value_and_derivative(act, A.EXTREME)
        assert np.isfinite(v).all() and np.isfinite(d).all(), act


def test_the_gated_form_is_the_product_of_the_halves():
    rng = np.random.default_rng(4)
    x, g, dx0 = rng.uniform(-3, 3, (5, 6)), rng.uniform(-1, 1, (5, 3)), rng.uniform(-1, 1, (5, 6))
    for act in A.ACTIVATIONS:
        v, d = A.value_and_derivative(act, x[:, 3:])
        assert np.array_equal(A.glu_forward(act, x, 3), x[:, :3] * v)
        want = np.concatenate([g * v, g * x[:, :3] * d], axis=1)
        assert np.array_equal(A.glu_backward(act, x, g, 3), want) and np.array_equal(A.glu_backward(act, x, g, 3, dx0), dx0 + want)


def test_extreme_set_is_the_stated_one():
    mags = sorted(set(np.abs(A.EXTREME).tolist()))
    want = sorted(float(np.float32(v)) for v in (0.0, 1e-30, 1e-6, 0.5, 5, 9, 20, 88, 100, 1e4, 1e13, 1e20, 3e38))
    assert mags == want and A.EXTREME.size == 26
    assert np.signbit(A.EXTREME).sum() == 13                 # -0 included

"""CPU checks of the layer normalisation: its oracle (tests/layernorm_oracle.py) against torch's layer_norm and autograd in f64
and against central differences, and the static surface of the feature - the five entry points in the header, the library,
the ctypes table; the module in the tape; the node, the methods and the layer in the Rust binding."""
import os
import re

import numpy as np
import pytest

import layernorm_oracle as LN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nk_layer_norm_fwd", "nk_layer_norm_bwd", "nk_layer_norm_bwd_assign", "nk_layer_norm_bwd_params", "nk_layer_norm_bwd_params_assign"]


# torch runs in a child process: a process that has loaded the HIP library must not import torch as well (a second HIP runtime
# in one address space aborts at exit; the suite's other torch users are child processes for the same reason)
_TORCH_CHECK = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import layernorm_oracle as LN
n = 0
for rows, D in [(1, 1), (3, 5), (7, 64), (33, 100), (5, 1027), (64, 1024)]:
    for affine in (True, False):
        rng = np.random.default_rng(rows * 1000 + D)
        x, g = rng.standard_normal((rows, D)), rng.standard_normal((rows, D))
        gamma, beta = (rng.standard_normal(D) + 1.0, rng.standard_normal(D)) if affine else (None, None)
        y, stats = LN.forward(x, gamma, beta, 1e-5)
        dx, dgamma, dbeta = LN.backward(g, x, gamma, stats)
        assert y.dtype == np.float64 and dx.dtype == np.float64
        tx = torch.tensor(x, requires_grad=True)
        tw = torch.tensor(gamma, requires_grad=True) if affine else None
        tb = torch.tensor(beta, requires_grad=True) if affine else None
        ty = torch.nn.functional.layer_norm(tx, (D,), tw, tb, 1e-5)
        ty.backward(torch.tensor(g))
        np.testing.assert_allclose(y, ty.detach().numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(stats[:, 0], x.mean(axis=1), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(stats[:, 1], 1.0 / np.sqrt(x.var(axis=1) + 1e-5), rtol=1e-12)
        np.testing.assert_allclose(dx, tx.grad.numpy(), rtol=1e-9, atol=1e-10)
        if affine:
            np.testing.assert_allclose(dgamma, tw.grad.numpy(), rtol=1e-10, atol=1e-11)
            np.testing.assert_allclose(dbeta, tb.grad.numpy(), rtol=1e-10, atol=1e-11)
        n += 1
print("cases", n)
"""


def test_oracle_matches_torch_in_f64():
    """forward, statistics and the autograd gradients of x, gamma, beta at several (rows, D), with and without affine parameters"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", _TORCH_CHECK, os.path.join(ROOT, "tests")], capture_output=True, text=True)
    assert r.returncode == 0 and "cases 12" in r.stdout, r.stdout + r.stderr


def test_oracle_matches_central_differences():
    rng = np.random.default_rng(5)
    rows, D, h = 3, 6, 1e-6
    x, g = rng.standard_normal((rows, D)), rng.standard_normal((rows, D))
    gamma, beta = rng.standard_normal(D) + 1.0, rng.standard_normal(D)
    loss = lambda x_, w_, b_: float((LN.forward(x_, w_, b_, 1e-5)[0] * g).sum())
    dx, dgamma, dbeta = LN.backward(g, x, gamma, LN.forward(x, gamma, beta, 1e-5)[1])
    for got, arg in ((dx, 0), (dgamma, 1), (dbeta, 2)):
        args = [x, gamma, beta]
        num = np.zeros_like(args[arg])
        for i in np.ndindex(*num.shape):
            hi, lo = [a.copy() for a in args], [a.copy() for a in args]
            hi[arg][i] += h
            lo[arg][i] -= h
            num[i] = (loss(*hi) - loss(*lo)) / (2 * h)
        np.testing.assert_allclose(got, num, rtol=1e-6, atol=1e-8)


def test_f32_twin_stays_in_f32_and_degenerate_rows():
    x = np.full((2, 1), 3.5, np.float32)
    y, stats = LN.forward(x, np.array([2.0], np.float32), np.array([0.25], np.float32), 1e-5)
    assert y.dtype == np.float32 and stats.dtype == np.float32
    np.testing.assert_array_equal(y, np.full((2, 1), 0.25, np.float32))            # D = 1: y = beta
    dx, _, _ = LN.backward(np.ones((2, 1), np.float32), x, np.array([2.0], np.float32), stats)
    np.testing.assert_array_equal(dx, np.zeros((2, 1), np.float32))
    y, stats = LN.forward(np.full((1, 8), -7.0), None, None, 1e-5)                 # a constant row: var = 0, finite through eps
    assert np.isfinite(y).all() and np.isfinite(stats).all() and (y == 0).all()


def test_header_library_and_ctypes_carry_the_five_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neuronika_hip.h")).read(), flags=re.S)
    from neuronika_amd import capi
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(\s*nk_device\*" % name, src), name
        assert hasattr(capi.lib, name), name
        assert name in capi.EXPORTED, name
    # the header's arity: fwd (dev, x, gamma, beta, y, stats, rows, D, eps), the four gradients eight arguments each
    assert len(capi._SIGS["nk_layer_norm_fwd"]) == 9
    assert all(len(capi._SIGS[n]) == 8 for n in NAMES[1:])
    for wrapper in ("layer_norm_fwd", "layer_norm_bwd", "layer_norm_bwd_params"):
        assert callable(getattr(capi, wrapper)), wrapper


def test_tape_has_the_module_and_the_methods():
    import neuronika_amd
    t = neuronika_amd.tape
    assert hasattr(t.nn, "LayerNorm")
    assert hasattr(t.Var, "layer_norm") and hasattr(t.VarDiff, "layer_norm")
    assert hasattr(t.serde, "layer_norm_from_json")


def test_rust_binding_carries_the_node_the_methods_and_the_layer():
    hip = os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip")
    node = open(os.path.join(hip, "node", "normalization.rs")).read()
    assert re.search(r"^mod normalization;", open(os.path.join(hip, "node", "mod.rs")).read(), re.M)
    for item in ("pub(crate) struct LayerNorm<", "pub(crate) struct LayerNormBackward<", "impl<D: Dimension, E: Dimension> Forward for LayerNorm<D, E>",
                 "impl<D: Dimension, E: Dimension> Backward for LayerNormBackward<D, E>"):
        assert item in node, item
    for call in ("ffi::nk_layer_norm_fwd(", "ffi::nk_layer_norm_bwd(", "ffi::nk_layer_norm_bwd_params("):
        assert call in node, call
    var = open(os.path.join(hip, "hipvar.rs")).read()
    assert len(re.findall(r"pub fn layer_norm<", var)) == 2                          # HipVar and HipVarDiff
    assert "LayerNorm::new(" in var and "LayerNormBackward::new(" in var
    nn = open(os.path.join(ROOT, "integration", "neuronika-nn", "src", "hip.rs")).read()
    assert re.search(r"pub struct LayerNorm\b", nn)
    body = nn[nn.index("> LayerNorm<E>"):]
    assert "pub fn new(" in body and "pub fn forward" in body and ".layer_norm(" in body
    ffi = open(os.path.join(hip, "ffi.rs")).read()
    for name in NAMES:
        assert "pub fn %s(" % name in ffi, name

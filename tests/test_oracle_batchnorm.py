"""CPU checks of the batch normalisation's oracle (tests/batchnorm_oracle.py): against torch.nn.functional.batch_norm and autograd
in f64 for 1-d, 2-d and 3-d inputs, both modes, with and without affine parameters, and against central differences."""
import os

import numpy as np

import batchnorm_oracle as BN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# torch runs in a child process: a process that has loaded the HIP library must not import torch as well (a second HIP runtime
# in one address space aborts at exit; the suite's other torch users are child processes for the same reason)
_TORCH_CHECK = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import batchnorm_oracle as BN
n = 0
for shape in [(6, 3), (2, 1), (64, 8), (5, 4, 7), (3, 2, 1), (4, 3, 5, 6), (2, 5, 8, 8), (2, 3, 2, 3, 4)]:
    for affine in (True, False):
        for training in (True, False):
            rng = np.random.default_rng(sum(shape) * 10 + affine * 2 + training)
            C = shape[1]
            x, g = rng.standard_normal(shape) * 2.0 + 0.5, rng.standard_normal(shape)
            gamma, beta = (rng.standard_normal(C) + 1.0, rng.standard_normal(C)) if affine else (None, None)
            rm, rv = rng.standard_normal(C), rng.random(C) + 0.5
            x3, g3 = x.reshape(shape[0], C, -1), g.reshape(shape[0], C, -1)
            o = BN.both(x3, gamma, beta, g3, 1e-5, 0.3, (rm, rv), training)[0]
            assert o["y"].dtype == np.float64 and o["dx"].dtype == np.float64
            tx = torch.tensor(x, requires_grad=True)
            tw = torch.tensor(gamma, requires_grad=True) if affine else None
            tb = torch.tensor(beta, requires_grad=True) if affine else None
            trm, trv = torch.tensor(rm.copy()), torch.tensor(rv.copy())
            ty = torch.nn.functional.batch_norm(tx, trm, trv, tw, tb, training, 0.3, 1e-5)
            ty.backward(torch.tensor(g))
            np.testing.assert_allclose(o["y"].reshape(shape), ty.detach().numpy(), rtol=1e-11, atol=1e-11)
            np.testing.assert_allclose(o["running_mean"], trm.numpy(), rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(o["running_var"], trv.numpy(), rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(o["dx"].reshape(shape), tx.grad.numpy(), rtol=1e-8, atol=1e-9)
            if training:
                ax = tuple(i for i in range(len(shape)) if i != 1)
                np.testing.assert_allclose(o["stats"][:, 0], x.mean(axis=ax), rtol=1e-12, atol=1e-14)
                np.testing.assert_allclose(o["stats"][:, 1], 1.0 / np.sqrt(x.var(axis=ax) + 1e-5), rtol=1e-12)
            if affine:
                np.testing.assert_allclose(o["dgamma"], tw.grad.numpy(), rtol=1e-9, atol=1e-10)
                np.testing.assert_allclose(o["dbeta"], tb.grad.numpy(), rtol=1e-10, atol=1e-11)
            n += 1
print("cases", n)
"""


def test_oracle_matches_torch_in_f64():
    """forward, running statistics and the autograd gradients of x, gamma, beta for (N, C), (N, C, L), (N, C, H, W) and
    (N, C, D, H, W) inputs, training and inference, with and without affine parameters"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", _TORCH_CHECK, os.path.join(ROOT, "tests")], capture_output=True, text=True)
    assert r.returncode == 0 and "cases 32" in r.stdout, r.stdout + r.stderr


def test_oracle_matches_central_differences():
    rng = np.random.default_rng(5)
    N, C, L, h = 3, 2, 4, 1e-6
    x, g = rng.standard_normal((N, C, L)), rng.standard_normal((N, C, L))
    gamma, beta = rng.standard_normal(C) + 1.0, rng.standard_normal(C)
    running = (rng.standard_normal(C), rng.random(C) + 0.5)
    for training in (True, False):
        stats_of = lambda x_: BN.batch_stats(x_, 1e-5)[0] if training else BN.running_stats(running, 1e-5)
        loss = lambda x_, w_, b_: float((BN.normalise(x_, stats_of(x_), w_, b_) * g).sum())
        sums, dx, dgamma, dbeta = BN.backward(g, x, gamma, stats_of(x), training)
        assert np.array_equal(sums[:, 0], dbeta) and np.array_equal(sums[:, 1], dgamma)
        for got, arg in ((dx, 0), (dgamma, 1), (dbeta, 2)):
            args = [x, gamma, beta]
            num = np.zeros_like(args[arg])
            for i in np.ndindex(*num.shape):
                hi, lo = [a.copy() for a in args], [a.copy() for a in args]
                hi[arg][i] += h
                lo[arg][i] -= h
                num[i] = (loss(*hi) - loss(*lo)) / (2 * h)
            np.testing.assert_allclose(got, num, rtol=1e-6, atol=1e-8)


def test_f32_twin_stays_in_f32_and_degenerate_channels():
    x = np.full((4, 2, 3), 3.5, np.float32)                                        # constant channels: var = 0, finite through eps
    o64, o32 = BN.both(x, np.array([2.0, 1.0], np.float32), np.array([0.25, -1.0], np.float32), np.ones((4, 2, 3), np.float32), 1e-5, 0.1,
                       (np.zeros(2, np.float32), np.ones(2, np.float32)))
    for k, v in o32.items():
        assert v.dtype == np.float32, k
    for k, v in o64.items():
        assert v.dtype == np.float64 and np.isfinite(v).all(), k
    np.testing.assert_array_equal(o32["y"][:, 0], np.full((4, 3), 0.25, np.float32))   # xhat = 0: y = beta
    np.testing.assert_allclose(o64["running_mean"], 0.35)
    np.testing.assert_allclose(o64["running_var"], 0.9)
    # the running variance takes the unbiased estimate
    x = np.array([1.0, 3.0]).reshape(2, 1, 1)
    st, var = BN.batch_stats(x, 0.0)
    assert var[0] == 1.0 and st[0, 0] == 2.0
    rm, rv = BN.running_update(np.zeros(1), np.zeros(1), st, var, 2, 1.0)
    assert rm[0] == 2.0 and rv[0] == 2.0

"""The activation kernels at model sizes, once each, forward and backward (`+=` and assign), whole tensors against
tests/activation_oracle.py within the elementwise tolerance: GELU and SiLU on a (8192, 4096) hidden tensor (134 MB; the backward's
working set is 0.4 - 0.5 GB, so its `nt` loads are on), SwiGLU on rows = 8192, H = 11008 (721 MB in, 361 MB out).  The oracle walks
the tensors in row blocks so that its float64 copies stay small."""
import numpy as np
import pytest

import activation_oracle as A
from test_gpu_activation import within

pytestmark = pytest.mark.gpu

BLOCK = 1024  # rows per oracle block


def _uniform(rng, shape, lo, hi):
    a = rng.random(shape, dtype=np.float32)
    a *= np.float32(hi - lo)
    a += np.float32(lo)
    return a


@pytest.mark.parametrize("act", ["gelu", "silu"])
def test_hidden_tensor(dev, act):
    from neuronika_amd import capi as c
    rows, cols = 8192, 4096
    rng = np.random.default_rng(7)
    x, g, dx0 = _uniform(rng, (rows, cols), -6, 6), _uniform(rng, (rows, cols), -1, 1), _uniform(rng, (rows, cols), -1, 1)
    X, G, Y, DX, DA = dev.array(x), dev.array(g), dev.zeros(x.shape), dev.array(dx0), dev.zeros(x.shape)
    DA.fill(float("nan"))
    c.activation_fwd(dev, act, X, Y)
    c.activation_bwd(dev, act, DX, G, X)
    c.activation_bwd(dev, act, DA, G, X, assign=True)
    y, dx, da = Y.numpy(), DX.numpy(), DA.numpy()
    for lo in range(0, rows, BLOCK):
        s = slice(lo, lo + BLOCK)
        v, d = A.value_and_derivative(act, x[s])
        grad = g[s].astype(np.float64) * d
        within(y[s], v, "%s rows %d.. forward" % (act, lo))
        within(dx[s], dx0[s].astype(np.float64) + grad, "%s rows %d.. backward +=" % (act, lo))
        within(da[s], grad, "%s rows %d.. backward assign" % (act, lo))


def test_swiglu_feed_forward(dev):
    from neuronika_amd import capi as c
    rows, H = 8192, 11008
    rng = np.random.default_rng(8)
    x, g, dx0 = _uniform(rng, (rows, 2 * H), -6, 6), _uniform(rng, (rows, H), -1, 1), _uniform(rng, (rows, 2 * H), -1, 1)
    X, G, Y, DX = dev.array(x), dev.array(g), dev.zeros((rows, H)), dev.array(dx0)
    c.glu_fwd(dev, "silu", X, Y, rows, H)
    c.glu_bwd(dev, "silu", DX, G, X, rows, H)
    y, dx = Y.numpy(), DX.numpy()
    DX.fill(float("nan"))
    c.glu_bwd(dev, "silu", DX, G, X, rows, H, assign=True)
    da = DX.numpy()
    for lo in range(0, rows, BLOCK):
        s = slice(lo, lo + BLOCK)
        x64 = x[s].astype(np.float64)
        v, d = A.value_and_derivative("silu", x64[:, H:])
        g64 = g[s].astype(np.float64)
        grad = np.concatenate([g64 * v, g64 * x64[:, :H] * d], axis=1)
        within(y[s], x64[:, :H] * v, "swiglu rows %d.. forward" % lo)
        within(dx[s], dx0[s].astype(np.float64) + grad, "swiglu rows %d.. backward +=" % lo)
        within(da[s], grad, "swiglu rows %d.. backward assign" % lo)

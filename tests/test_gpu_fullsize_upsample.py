"""The oracle's rules at model size: (2, 64, 64, 64) -> (128, 128), nearest (the x2 class) and bilinear (the vector class).  The
forward is compared bit for bit through the vectorised NumPy forward; the backward on one (n, c) plane only, because the oracle's
backward loops over a plane's outputs in Python - planes are independent, and every plane runs the same code."""
import numpy as np
import pytest

import upsample_oracle as U

pytestmark = pytest.mark.gpu

SHAPE, SIZE = (2, 64, 64, 64), (128, 128)
PLANE = (1, 37)


def test_model_size_equals_the_oracle(dev):
    for mode in ("nearest", "linear"):
        _model_size_equals_the_oracle(dev, mode)


def _model_size_equals_the_oracle(dev, mode):
    from neuronika_amd import capi as c
    rng = np.random.default_rng(5)
    x, g = rng.standard_normal(SHAPE).astype(np.float32), rng.standard_normal(SHAPE[:2] + SIZE).astype(np.float32)
    Y, DX = dev.full(SHAPE[:2] + SIZE, np.nan), dev.full(SHAPE, np.nan)
    c.upsample_fwd(dev, dev.array(x), SHAPE, Y, SIZE, mode)
    c.upsample_bwd(dev, DX, SHAPE, dev.array(g), SIZE, mode, assign=True)
    assert Y.numpy().tobytes() == U.forward(x, SIZE, mode).tobytes()
    dx = DX.numpy()
    n, ch = PLANE
    want = U.backward(g[n:n + 1, ch:ch + 1], (1, 1) + SHAPE[2:], mode)
    assert dx[n:n + 1, ch:ch + 1].tobytes() == want.tobytes()
    assert np.isfinite(dx).all()
    if mode == "nearest":                                                    # every plane: each element is the ordered sum of its 2 x 2 outputs
        q = g.reshape(SHAPE[:2] + (64, 2, 64, 2))
        every = ((np.float32(0) + q[..., 0, :, 0]) + q[..., 0, :, 1] + q[..., 1, :, 0]) + q[..., 1, :, 1]
        assert dx.tobytes() == np.ascontiguousarray(every).tobytes()

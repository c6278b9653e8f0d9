"""nk_group_norm_* at model size, under the rules of tests/test_gpu_group_norm.py: the first stage of a diffusion U-Net at 64 x 64
(D = 8 * 4096 = 32768, the chunked class, 32 MiB per tensor) and a mid stage at 16 x 16 (D = 16 * 256 = 4096, a block per row)."""
import numpy as np
import pytest

import group_norm_oracle as GN
from test_gpu_group_norm import EPS, _compare, _device_run, _inputs, _shapes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,C,L,G", [(8, 256, 4096, 32), (16, 512, 256, 32)])
def test_model_sized_rows(dev, N, C, L, G):
    from neuronika_amd import capi as c
    x, g, gamma, beta = _inputs(N, C, L, C + L)
    o64, o32 = GN.both(x, G, gamma, beta, g, EPS)
    got = _device_run(dev, c, x, G, g, gamma, beta, True, [np.full(s, np.nan, np.float32) for s in _shapes(N, C, L)])
    _compare(got, o64, o32, x, G, g, gamma, "fullsize %d" % ((C // G) * L))

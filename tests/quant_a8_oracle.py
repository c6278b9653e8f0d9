"""NumPy statement of nk_quant_a8_linear_fwd (include/neuronika_hip.h, "quantised Linear, int8 activations"), bit exact: the rows of x
are quantised like a weight with bits = 8, group = 0; the integer products are summed exactly per span (the group, or F = 2048 k for
group 0); every span sum is converted to f32, multiplied by the weight scale and added in ascending span order; the row's activation
scale and the bias come last.  Every f32 operation is one IEEE operation of NumPy."""
import numpy as np

import quant_oracle as Q

F = 2048


def spans(K, group):
    """[(k0, k1, scale column)] in ascending order"""
    g = group or F
    return [(k0, min(k0 + g, K), k0 // g if group else 0) for k0 in range(0, K, g)]


def forward(x, b, s, bias, bits, group):
    """y f32 (M, N) from x f32 (M, K), the packed weight bytes b, their scales s and the bias (or None)"""
    x = np.asarray(x, np.float32)
    K = x.shape[1]
    xq, sx = Q.quantise(x, 8, 0)
    q = Q.from_bytes(b, bits, K).astype(np.int64)
    s = np.asarray(s, np.float32).reshape(q.shape[0], -1)
    acc = np.zeros((x.shape[0], q.shape[0]), np.float32)
    for k0, k1, col in spans(K, group):
        isum = xq[:, k0:k1].astype(np.int64) @ q[:, k0:k1].T          # exact
        acc = (acc + (isum.astype(np.float32) * s[None, :, col]).astype(np.float32)).astype(np.float32)
    y = (acc * sx).astype(np.float32)
    return y if bias is None else (y + np.asarray(bias, np.float32)[None, :]).astype(np.float32)

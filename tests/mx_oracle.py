"""NumPy statement of the microscaling format of nk_quant_mx_* (include/neuronika_hip.h), bit exact: E8M0 scales from the exponent field
of the absmax, elements scaled by a power of two and rounded ONCE at the spacing of their binade, ties to even; the sign is a code's top bit."""
import numpy as np


def table(mbits, bias, codes):
    c = np.arange(codes)
    ex, m = c >> mbits, c & ((1 << mbits) - 1)
    return np.where(ex == 0, m * 2.0 ** (1 - bias - mbits), (1 + m * 2.0 ** -mbits) * 2.0 ** (ex - bias))


FP4, FP8 = table(1, 1, 8), table(3, 7, 127)   # E2M1 up to 6, E4M3 up to 448
SIGN = {len(FP4): 8, len(FP8): 128}           # the sign bit of a code


def quantise(a, emax, mbits, tab):
    """(R, K) f32 -> codes (R, K) uint8, scale bytes (R, K / 32) uint8"""
    blk = np.ascontiguousarray(a, np.float32).reshape(a.shape[0], -1, 32)
    absbits = (blk.view(np.uint32) & 0x7fffffff).max(axis=2)
    e = np.where(absbits == 0, 127, np.clip((absbits >> 23).astype(np.int64) - emax, 0, 254))
    v = np.ldexp(np.abs(blk).astype(np.float64), (127 - e)[:, :, None])
    binade = np.maximum(np.frexp(v)[1] - 1, int(np.frexp(tab[1 << mbits])[1]) - 1)
    r = np.minimum(np.ldexp(np.rint(np.ldexp(v, mbits - binade)), binade - mbits), tab[-1])
    mag = np.searchsorted(tab, r)
    code = mag | (np.signbit(blk) & (mag != 0)) * SIGN[len(tab)]
    return code.reshape(a.shape).astype(np.uint8), e.astype(np.uint8)


def values(code, e, tab):
    """codes and scale bytes -> the f64 values element * 2^(e - 127)"""
    top = SIGN[len(tab)]
    el = np.where(code & top, -1.0, 1.0) * tab[code & (top - 1)]
    return np.ldexp(el, np.repeat(e.astype(np.int64), 32, axis=1) - 127)


def pack(W):
    """(N, K) f32 -> bytes (N, K / 2), even k in the low nibble, and scale bytes (N, K / 32)"""
    code, e = quantise(W, 2, 1, FP4)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).astype(np.uint8), e


def unpack(b, e):
    code = np.stack([b & 15, b >> 4], axis=2).reshape(b.shape[0], -1)
    return values(code, e, FP4).astype(np.float32)


def quantise_rows(x):
    return quantise(x, 8, 3, FP8)


def forward64(x, b, e, bias):
    """the f64 product of the dequantised operands plus bias, and sum_k |x^ w^| + |bias| for the error bound"""
    xh, wh = values(*quantise_rows(x), FP8), unpack(b, e).astype(np.float64)
    bias = np.zeros(b.shape[0]) if bias is None else bias.astype(np.float64)
    return xh @ wh.T + bias, np.abs(xh) @ np.abs(wh).T + np.abs(bias)

"""NumPy statement of the weight-only quantised Linear format (include/neuronika_hip.h, "weight-only quantised Linear"), bit exact:

    s  = fl32(absmax / qmax)                           per row and group, qmax = 127 (8 bits) / 7 (4 bits)
    q  = clamp(rint(fl32(w / s)), -qmax, qmax)         round-half-even; s == 0 gives q = 0
    w^ = fl32(float(q) * s)

int8 is stored as two's-complement bytes, int4 as the unsigned nibble q + 8 with element k in byte k / 2 and even k in the low
nibble; rows are contiguous.  Every operation is one IEEE f32 operation of NumPy, so the device must agree bit for bit."""
import numpy as np


def qmax(bits):
    return {8: 127, 4: 7}[bits]


def group_len(K, group):
    return K if group == 0 else group


def accepted(N, K, bits, group):
    return N > 0 and K > 0 and bits in (8, 4) and K % 32 == 0 and (group == 0 or (group in (32, 64, 128) and K % group == 0))


def quantise(W, bits, group):
    """-> (q int32 (N, K), scales f32 (N, K / group))"""
    W = np.asarray(W, np.float32)
    N, K = W.shape
    assert accepted(N, K, bits, group), (N, K, bits, group)
    g = group_len(K, group)
    Wg = W.reshape(N, K // g, g)
    absmax = np.abs(Wg).max(axis=2)
    s = (absmax / np.float32(qmax(bits))).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.rint((Wg / s[:, :, None]).astype(np.float32))
    r = np.where(s[:, :, None] == 0, np.float32(0), r)
    q = np.clip(r, -qmax(bits), qmax(bits)).astype(np.int32).reshape(N, K)
    return q, s


def to_bytes(q, bits):
    """the packed rows: uint8 (N, K * bits / 8)"""
    q = np.asarray(q, np.int32)
    if bits == 8:
        return q.astype(np.int8).view(np.uint8).copy()
    u = (q + 8).astype(np.uint8)
    return (u[:, 0::2] | (u[:, 1::2] << 4)).astype(np.uint8)


def from_bytes(b, bits, K):
    b = np.asarray(b, np.uint8).reshape(-1, K * bits // 8)
    if bits == 8:
        return b.view(np.int8).astype(np.int32)
    q = np.empty((b.shape[0], K), np.int32)
    q[:, 0::2] = (b & 15).astype(np.int32) - 8
    q[:, 1::2] = (b >> 4).astype(np.int32) - 8
    return q


def pack(W, bits, group):
    """-> (bytes uint8 (N, K * bits / 8), scales f32 (N, K / group))"""
    q, s = quantise(W, bits, group)
    return to_bytes(q, bits), s


def unpack(b, s, bits, group, K):
    """w^ = fl32(float(q) * s), f32 (N, K)"""
    q = from_bytes(b, bits, K)
    s = np.asarray(s, np.float32)
    g = group_len(K, group)
    return (q.astype(np.float32) * np.repeat(s.reshape(q.shape[0], K // g), g, axis=1)).astype(np.float32)


def forward64(x, b, s, bias, bits, group):
    """the f64 product over w^: y = x . w^T + bias"""
    x = np.asarray(x, np.float32)
    w = unpack(b, s, bits, group, x.shape[1]).astype(np.float64)
    y = x.astype(np.float64) @ w.T
    return y if bias is None else y + np.asarray(bias, np.float64)


def forward32(x, b, s, bias, bits, group):
    """the same product in NumPy f32: the CPU restatement of tests/tolerance.py"""
    x = np.asarray(x, np.float32)
    y = x @ unpack(b, s, bits, group, x.shape[1]).T
    return y if bias is None else (y + np.asarray(bias, np.float32)).astype(np.float32)


def tie_row(K, s0=2.0 ** -6):
    """a row whose absmax is 127 s0 (int8: s = s0 exactly) followed by the half-way values 0.5 s0 .. 7.5 s0 and their negatives: packs to
    [127, 0, 2, 2, 4, 4, 6, 6, 8, 0, -2, -2, -4, -4, -6, -6, -8, 0 ...] under round-half-even"""
    w = np.zeros(K, np.float32)
    h = (np.arange(8, dtype=np.float32) + np.float32(0.5)) * np.float32(s0)
    w[0] = np.float32(127 * s0)
    w[1:9] = h
    w[9:17] = -h
    return w


TIE_Q8 = [127, 0, 2, 2, 4, 4, 6, 6, 8, 0, -2, -2, -4, -4, -6, -6, -8]

"""The microscaling Linear without a GPU: header, symbols, ctypes, null-device refusal, tape.nn.MxLinear; the oracle against hand cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mx_oracle as O
from test_gpu_woq_linear_mx import KS, exact_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, I = C.c_void_p, C.c_int
ENTRIES = {
    "size_t nk_quant_mx_words(int N, int K);": [I, I],
    "size_t nk_quant_mx_scales(int N, int K);": [I, I],
    "int nk_quant_mx_pack(nk_device* dev, const float* W, int ldw, float* qw, float* sw, int N, int K);": [VP, VP, I, VP, VP, I, I],
    "int nk_quant_mx_unpack(nk_device* dev, const float* qw, const float* sw, float* W, int ldw, int N, int K);": [VP, VP, VP, VP, I, I, I],
    "int nk_quant_mx_rows(nk_device* dev, const float* x, int ldx, float* xq, float* sx, int M, int K);": [VP, VP, I, VP, VP, I, I],
    "int nk_quant_mx_linear_fwd(nk_device* dev, const float* x, int ldx, const float* qw, const float* sw, const float* bias, float* y, "
    "int ldy, int M, int N, int K);": [VP, VP, I, VP, VP, VP, VP, I, I, I, I],
}


def test_header_library_ctypes_and_host_layer():
    import neuronika_amd
    from neuronika_amd import capi
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neuronika_hip.h")).read(), flags=re.S))
    for proto, sig in ENTRIES.items():
        name = re.search(r"nk_\w+", proto).group(0)
        assert proto in flat and name in capi.EXPORTED and hasattr(capi.lib, name) and hasattr(capi, name[3:]), name
        assert capi._SIGS[name] == sig, name
        if sig[0] is VP:
            assert getattr(capi.lib, name)(*[None if t is VP else 0 for t in sig]) == 1, name   # a null device, before anything else
    assert capi.quant_mx_words(3, 64) == 24 and capi.quant_mx_scales(3, 64) == 2 and capi.quant_mx_words(3, 48) == 0
    assert all(hasattr(neuronika_amd.tape.nn.MxLinear, a) for a in ("forward", "dequantize", "in_features", "out_features"))


def row(*head):
    return np.array([list(head) + [0] * (32 - len(head))], np.float32)


@pytest.mark.parametrize("head,e,nibbles", (
    ((6, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5), 127, (7, 0, 2, 2, 4, 4, 6, 6)),        # every tie goes to the even mantissa
    ((7, -7, 6.5, -0.26, 0.74), 127, (7, 15, 7, 9, 1)),                               # 7 saturates at 6; just past / short of a tie
    ((4, 3, -0.5), 127, (6, 5, 9)),                                                   # absmax a power of two: e = log2 - 2
    ((8, 6, -1), 128, (6, 5, 9)),                                                     # ... and the next one doubles the scale
    ((3.99, 1), 126, (7, 4)),                                                         # just below it: the lower scale, 7.98 -> 6
    ((0, -0.0), 127, (0, 0)),                                                         # a zero block: e = 127, no signed zero
    ((2.0 ** -127,), 0, (2,)),                                                        # a subnormal absmax clamps e at 0: 2^-127 * 2^127 = 1
))
def test_oracle_pack_by_hand(head, e, nibbles):
    b, s = O.pack(row(*head))
    code = np.stack([b & 15, b >> 4], axis=2).ravel()
    assert s.tolist() == [[e]] and code[:len(nibbles)].tolist() == list(nibbles) and not code[len(nibbles):].any()


@pytest.mark.parametrize("head,e,codes", (
    ((256, 17, 19, -21, 1, 0.5), 127, (0x78, 0x58, 0x5a, 0xda, 0x38, 0x30)),          # 17 -> 16 and 19 -> 20: ties to even; 21 -> 20
    ((480, 464, 447), 127, (0x7e, 0x7e, 0x7e)),                                       # saturation at 448, never the NaN 0x7f
    (tuple(2.0 ** -8 * np.array([2.0 ** 17, 1.5, 2.5, -3.5, 0.5, 7.5])), 128, (0x78, 2, 2, 0x84, 0, 8)),   # subnormal ties, spacing 2^-9
))
def test_oracle_rows_by_hand(head, e, codes):
    c, s = O.quantise_rows(row(*head))
    assert s.tolist() == [[e]] and c[0, :len(codes)].tolist() == list(codes) and not c[0, len(codes):].any()


@pytest.mark.parametrize("K", KS)
def test_integer_data_is_lossless_in_both_formats(K):
    x, W, _ = exact_data(K)
    assert np.array_equal(O.unpack(*O.pack(W)), W) and np.array_equal(O.values(*O.quantise_rows(x), O.FP8), x)
    assert np.unique(O.pack(W)[1]).size == 5 and np.unique(O.quantise_rows(x)[1]).size == 3   # every block exponent occurs

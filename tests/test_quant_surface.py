"""The surface of the weight-only quantised Linear, layer by layer, without a GPU: the header declares the six entry points and the
tune knob, the ctypes table and the built library have them, the Rust mirror names them, the host module exposes `nn.QuantLinear` and
`MultiheadAttention.quantize`, the kernels live in one header that nk_norm.hip alone includes; the size functions; and the NumPy
oracle's own properties: the half-step error bound, the zero group, round-half-even on the tie row, and the int4 nibble order byte
for byte."""
import ctypes as C
import os
import re

import numpy as np

import quant_oracle as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nk_quant_linear_words", "nk_quant_linear_scales", "nk_quant_linear_rows_rule", "nk_quant_linear_pack", "nk_quant_linear_unpack",
           "nk_quant_linear_fwd")
HIP = os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip")
CSRC = os.path.join(ROOT, "neuronika_amd", "csrc")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", _read("include", "neuronika_hip.h"), flags=re.S))
    assert tuple(m.group(1) for m in re.finditer(r"(?:int|size_t) (nk_quant_linear\w*)\(", flat)) == ENTRIES
    for proto in ("size_t nk_quant_linear_words(int N, int K, int bits);", "size_t nk_quant_linear_scales(int N, int K, int group);",
                  "int nk_quant_linear_rows_rule(int bits);",
                  "int nk_quant_linear_pack(nk_device* dev, const float* W, int ldw, float* qw, float* scales, int N, int K, int bits, int group);",
                  "int nk_quant_linear_unpack(nk_device* dev, const float* qw, const float* scales, float* W, int ldw, int N, int K, int bits, int group);",
                  "int nk_quant_linear_fwd(nk_device* dev, const float* x, int ldx, const float* qw, const float* scales, const float* bias, float* y, "
                  "int ldy, int M, int N, int K, int bits, int group);"):
        assert proto in flat, proto
    assert "NK_TUNE_QUANT_ROWS = 9" in flat
    doc = _read("include", "neuronika_hip.h")
    for phrase in ("s = fl32(absmax / qmax)", "clamp(rint(fl32(w / s)), -qmax, qmax)", "w^ = fl32(float(q) * s)", "even k in the low nibble",
                   "acc += s * sum_unit(x * float(q))", "Bit contract", "NK_TUNE_QUANT_ROWS", "qw not 16-byte aligned"):
        assert phrase in doc, phrase


def test_ctypes_table_and_library_export_them():
    from neuronika_amd import capi
    VP, I = C.c_void_p, C.c_int
    for name in ENTRIES:
        assert name in capi.EXPORTED and hasattr(capi.lib, name), name
    assert capi._SIGS["nk_quant_linear_pack"] == [VP, VP, I, VP, VP, I, I, I, I]
    assert capi._SIGS["nk_quant_linear_unpack"] == [VP, VP, VP, VP, I, I, I, I, I]
    assert capi._SIGS["nk_quant_linear_fwd"] == [VP, VP, I, VP, VP, VP, VP, I, I, I, I, I, I]
    assert capi.TUNE_QUANT_ROWS == 9 and hasattr(capi.Device, "quant_rows")
    # the size functions and the rule need no device
    assert capi.quant_linear_words(5, 64, 4) == 40 and capi.quant_linear_words(5, 64, 8) == 80
    assert capi.quant_linear_scales(5, 64, 32) == 10 and capi.quant_linear_scales(5, 64, 0) == 5
    for N, K, bits in ((5, 48, 8), (5, 64, 3), (0, 64, 8), (5, 0, 8), (-1, 64, 4)):
        assert capi.quant_linear_words(N, K, bits) == 0, (N, K, bits)
    for N, K, group in ((5, 48, 0), (5, 96, 64), (5, 64, 16), (0, 64, 32), (5, 64, -32)):
        assert capi.quant_linear_scales(N, K, group) == 0, (N, K, group)
    for N, K, bits, group in ((5, 64, 8, 32), (3, 4224, 4, 128), (7, 96, 4, 0)):
        b, s = Q.pack(np.zeros((N, K), np.float32), bits, group)
        assert b.size == 4 * capi.quant_linear_words(N, K, bits) and s.size == capi.quant_linear_scales(N, K, group)
    assert capi.quant_linear_rows_rule(8) >= 1 and capi.quant_linear_rows_rule(4) >= 1 and capi.quant_linear_rows_rule(3) == 0
    # a null device is refused before anything else happens
    assert capi.lib.nk_quant_linear_fwd(None, None, 0, None, None, None, None, 0, 0, 0, 0, 0, 0) == 1
    assert capi.lib.nk_quant_linear_pack(None, None, 0, None, None, 0, 0, 0, 0) == 1


def test_rust_mirror_names_the_ffi_calls():
    ffi = open(os.path.join(HIP, "ffi.rs")).read()
    for name in ENTRIES:
        assert re.search(rf"pub fn {name}\(", ffi), name
    node = open(os.path.join(HIP, "node", "quant_linear.rs")).read()
    for name in ENTRIES:
        assert f"ffi::{name}(" in node, name
    assert re.search(r"^mod quant_linear;", open(os.path.join(HIP, "node", "mod.rs")).read(), re.M)
    hv = open(os.path.join(HIP, "hipvar.rs")).read()
    assert "pub fn quant_linear(" in hv and "QuantLinear::new(" in hv and "pub struct QuantLinearState" in hv


def test_host_module_exposes_the_layers():
    import neuronika_amd
    t = neuronika_amd.tape
    assert hasattr(t.nn, "QuantLinear") and hasattr(t.nn.MultiheadAttention, "quantize")
    for member in ("forward", "dequantize", "in_features", "out_features", "bits", "group"):
        assert hasattr(t.nn.QuantLinear, member), member
    hpp = _read("host", "neuronika.hpp")
    assert "struct QuantLinear" in hpp and "void quantize(int bits, int group = 0);" in hpp
    assert "serde of quantised layers is" in hpp   # the header says what is out of scope


def test_kernels_live_in_one_header_of_the_row_unit():
    units = [f for f in os.listdir(CSRC) if '#include "nk_quant_linear.h"' in open(os.path.join(CSRC, f)).read()]
    assert units == ["nk_norm.hip"] and _read("neuronika_amd", "csrc", "nk_norm.hip").count('#include "nk_quant_linear.h"') == 1
    src = _read("neuronika_amd", "csrc", "nk_quant_linear.h")
    kernels = set(re.findall(r"__global__ [^\n]*?void (\w+)\(", src))
    assert kernels == {"quant_pack_kernel", "quant_pack_row_kernel", "quant_unpack_kernel", "quant_linear_rows_kernel", "quant_bias_rows_kernel"}
    others = "".join(open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f != "nk_quant_linear.h")
    for k in kernels:
        assert not re.search(rf"\b{k}\b", others), k   # names new to the library
    code = re.sub(r"//[^\n]*", "", src)
    for banned in ("atomic", "hipMalloc", "hipDeviceSynchronize", "hipStreamSynchronize", "asm"):
        assert banned not in code, banned


# ---- the oracle's own properties ------------------------------------------------------------------------------------------------
def test_quantisation_error_is_half_a_step():
    W = np.random.default_rng(0).standard_normal((64, 1024)).astype(np.float32)
    for bits in (8, 4):
        for group in (32, 128, 0):
            b, s = Q.pack(W, bits, group)
            wq = Q.unpack(b, s, bits, group, 1024)
            step = np.repeat(s, Q.group_len(1024, group), axis=1).astype(np.float64)
            ratio = (np.abs(W.astype(np.float64) - wq.astype(np.float64)) / step).max()
            assert ratio <= 0.5 * (1 + 2.0 ** -20), (bits, group, ratio)
            assert ratio > 0.49, (bits, group, ratio)          # and the bound is not slack
            q = Q.from_bytes(b, bits, 1024)
            assert q.min() >= -Q.qmax(bits) and q.max() <= Q.qmax(bits) and np.abs(q).max() == Q.qmax(bits)


def test_zero_group_and_negative_absmax():
    W = np.random.default_rng(1).standard_normal((3, 128)).astype(np.float32)
    W[1, 32:64] = 0
    W[2, :32] = np.float32(0.25)
    W[2, 5] = -3.0
    for bits in (8, 4):
        q, s = Q.quantise(W, bits, 32)
        assert s[1, 1] == 0 and (q[1, 32:64] == 0).all()
        assert s[2, 0] == np.float32(3.0) / np.float32(Q.qmax(bits)) and q[2, 5] == -Q.qmax(bits)
        wq = Q.unpack(Q.to_bytes(q, bits), s, bits, 32, 128)
        assert (wq[1, 32:64] == 0).all() and np.isfinite(wq).all()


def test_tie_row_rounds_half_to_even():
    for K, group in ((32, 32), (128, 0), (128, 128)):
        q, s = Q.quantise(Q.tie_row(K)[None], 8, group)
        assert s[0, 0] == np.float32(2.0 ** -6)
        assert q[0, :17].tolist() == Q.TIE_Q8 == [127, 0, 2, 2, 4, 4, 6, 6, 8, 0, -2, -2, -4, -4, -6, -6, -8]
        assert (q[0, 17:] == 0).all()


def test_int4_nibble_order_byte_for_byte():
    q = np.zeros((2, 32), np.int32)
    q[0] = [-7, 7, 0, 1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6, 7] * 2
    q[1] = np.arange(32) % 15 - 7
    b = Q.to_bytes(q, 4)
    assert b.shape == (2, 16) and b.dtype == np.uint8
    # element k in byte k / 2, even k in the low nibble, stored as q + 8
    assert b[0].tolist() == [0xF1, 0x98, 0xA7, 0xB6, 0xC5, 0xD4, 0xE3, 0xF2] * 2
    assert b[1].tolist() == [0x21, 0x43, 0x65, 0x87, 0xA9, 0xCB, 0xED, 0x1F, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE, 0x21]
    assert np.array_equal(Q.from_bytes(b, 4, 32), q)
    # the same through pack: scales of 1 make the weights their own integers
    W = q.astype(np.float32)
    W[:, 0] = -7
    W[1, 1] = 7
    pb, ps = Q.pack(W, 4, 0)
    assert (ps == 1).all() and np.array_equal(Q.from_bytes(pb, 4, 32), W.astype(np.int32))
    # int8: two's-complement bytes
    assert Q.to_bytes(np.array([[-127, -1, 0, 127]]), 8).tolist() == [[0x81, 0xFF, 0x00, 0x7F]]

"""The surface of grouped-query attention, layer by layer, without a GPU: the header declares the four entry points and fixes the
semantics, the ctypes table and the built library have them, `_tape` has `kv_heads` and `repeat_kv`, the kernels live in their own
headers outside the inventoried units, the Rust mirror names the ffi calls, the example has the flag and reads nothing of the test
infrastructure."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nk_attention_decode_gqa_fwd", "nk_repeat_kv_fwd", "nk_repeat_kv_bwd", "nk_repeat_kv_bwd_assign")
HIP = os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points():
    doc = _read("include", "neuronika_hip.h")
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", doc, flags=re.S))
    assert ("int nk_attention_decode_gqa_fwd(nk_device* dev, const float* Q, int ldq, const float* Kc, const float* Vc, const int* start, "
            "float* O, float* workspace, int B, int T, int H, int Hkv, int dh, int cap, float scale);") in flat
    assert "int nk_repeat_kv_fwd(nk_device* dev, const float* x, int ldx, float* y, int ldy, int rows, int Hkv, int G, int dh);" in flat
    for name in ("nk_repeat_kv_bwd", "nk_repeat_kv_bwd_assign"):
        assert "int %s(nk_device* dev, float* dx, int lddx, const float* g, int ldg, int rows, int Hkv, int G, int dh);" % name in flat
    for phrase in ("(B, Hkv, cap, dh)", "h / G", "y[r, (k*G + j)*dh + e] = x[r, k*dh + e]", "((g_0 + g_1) + g_2)", "No atomics",
                   "Hkv == H forwards", "at most 8 query heads", "H % Hkv != 0", "K = QKV + d, V = QKV + d + dkv, ld = d + 2*dkv"):
        assert phrase in doc, phrase
    # the append serves the grouped cache as it is, and its comment says so
    append = doc[doc.index(" * nk_kv_cache_append:"):doc.index(" * nk_attention_decode_fwd:")]
    assert "H = Hkv" in append and "d + 2*dkv" in append


def test_ctypes_table_and_library_export_them():
    from neuronika_amd import capi
    for name in ENTRIES:
        assert name in capi.EXPORTED and hasattr(capi.lib, name), name
    assert len(capi._SIGS["nk_attention_decode_gqa_fwd"]) == 15
    assert len(capi._SIGS["nk_repeat_kv_fwd"]) == len(capi._SIGS["nk_repeat_kv_bwd"]) == len(capi._SIGS["nk_repeat_kv_bwd_assign"]) == 9
    for wrapper, keys in (("attention_decode_gqa_fwd", ("Q", "ldq", "Kc", "Vc", "start", "out", "workspace", "B", "T", "H", "Hkv", "dh", "cap", "scale")),
                          ("repeat_kv_fwd", ("x", "ldx", "y", "ldy", "rows", "Hkv", "G", "dh")),
                          ("repeat_kv_bwd", ("dx", "lddx", "g", "ldg", "rows", "Hkv", "G", "dh", "assign"))):
        params = inspect.signature(getattr(capi, wrapper)).parameters
        assert all(k in params for k in keys), (wrapper, list(params))


def test_bad_arguments_are_refused_before_a_device_is_touched():
    """A null device handle is the first check of every entry point: NK_ERR_INVALID without a GPU."""
    from neuronika_amd import capi
    assert capi.lib.nk_attention_decode_gqa_fwd(None, None, 0, None, None, None, None, None, 1, 1, 4, 2, 64, 16, 0.125) == 1
    for name in ENTRIES[1:]:
        assert getattr(capi.lib, name)(None, None, 0, None, 0, 1, 1, 1, 4) == 1, name


def test_host_classes_exist():
    import neuronika_amd
    t = neuronika_amd.tape
    nn = t.nn
    assert isinstance(nn.MultiheadAttention.kv_heads, property)
    init = nn.MultiheadAttention.__init__.__doc__
    assert re.search(r"dev: .*, d_model: .*, heads: .*, p: .* = 0.0, seed: .* = 0, kv_heads: .* = 0\) -> None", init)
    assert re.search(r"q: .*Linear, k: .*Linear, v: .*Linear, o: .*Linear, heads: .*, p: .* = 0.0, kv_heads: .* = 0\) -> None", init)
    assert re.search(r"repeat_kv\(self: [\w.]*Var, groups: .*, head_dim: .*\) -> [\w.]*Var\n", t.Var.repeat_kv.__doc__)
    assert re.search(r"repeat_kv\(self: [\w.]*VarDiff, groups: .*, head_dim: .*\) -> [\w.]*VarDiff\n", t.VarDiff.repeat_kv.__doc__)
    hpp = _read("host", "neuronika.hpp")
    assert "Var repeat_kv(int groups, int head_dim) const;" in hpp and "VarDiff repeat_kv(int groups, int head_dim) const;" in hpp
    assert "MultiheadAttention(DevicePtr dev, int d_model, int heads, int kv_heads, double p, uint64_t seed);" in hpp
    assert "MultiheadAttention(DevicePtr dev, int d_model, int heads, double p, uint64_t seed);" in hpp      # the old constructor stays
    assert "int kv_heads;" in hpp
    cpp = _read("host", "neuronika.cpp")
    for node in ("struct RepeatKvFwd : Forward", "struct RepeatKvBwd : Backward"):
        assert cpp.count(node) == 1, node
    bwd = cpp[cpp.index("struct RepeatKvBwd"):]
    bwd = bwd[:bwd.index("\n};")]
    assert "nk_repeat_kv_bwd_assign" in bwd and "nk_repeat_kv_bwd)" in bwd and bwd.count("borrow_first_write(") == 1
    step = cpp[cpp.index("struct DecodeStepFwd"):]
    step = step[:step.index("\n};")]
    for call in ("nk_attention_decode_gqa_fwd(", "nk_repeat_kv_fwd(", "nk_attention_decode_fwd(", "nk_attention_qkv_causal_fwd("):
        assert call in step, call
    assert "zeros_like" not in step and "make_shared" not in step                     # nothing is allocated inside forward()
    assert step.index("rope_inplace(") < step.index("nk_kv_cache_append(") < step.index("nk_attention_decode_gqa_fwd(")


def _kernel_text(src, name):
    """a kernel's own text in the decode header: from its `__global__` to the closing brace in column 0"""
    at = src.index(name + "(")
    start = src.rindex("__global__", 0, at)
    return src[start:src.index("\n}\n", at) + 1]


def test_kernels_live_in_their_own_headers_outside_the_inventoried_units():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dispatch_paths
    import dispatch_paths_mfma
    import list_unit_kernels as luk
    mine = {"adec_gqa_partial_kernel", "adec_gqa_generic_kernel", "repeat_kv_kernel"}
    assert mine - {"repeat_kv_kernel"} <= luk.file_kernels(os.path.join(luk.CSRC, "nk_attention_decode.h"))
    assert luk.file_kernels(os.path.join(luk.CSRC, "nk_repeat_kv.h")) == {"repeat_kv_kernel"}
    for header in ("nk_attention_decode.h", "nk_repeat_kv.h"):
        path = os.path.join(luk.CSRC, header)
        includers = [u for u in luk.all_units() if header in luk.unit_sources(u)]
        assert includers == ["nk_norm.hip"] and includers[0] in [u for u, _ in dispatch_paths_mfma.NOT_INVENTORIED], header
        assert _read("neuronika_amd", "csrc", "nk_norm.hip").count('#include "%s"' % header) == 1
        src = re.sub(r"//[^\n]*", "", open(path).read())
        assert "atomic" not in src.lower() and "num_cus" not in src and "tune_" not in src, header
        assert "hipMalloc" not in src and "Synchronize" not in src, header
    for u in dispatch_paths.UNITS + dispatch_paths_mfma.UNITS:
        assert not (mine & luk.source_kernels(u)), u
    assert not [f for f in os.listdir(luk.CSRC) if f.endswith(".hip") and ("gqa" in f or "repeat" in f)]   # no new translation unit
    rkv = re.sub(r"//[^\n]*", "", _read("neuronika_amd", "csrc", "nk_repeat_kv.h"))
    assert "__shared__" not in rkv and "__syncthreads" not in rkv and "float4" in rkv and "nk_stream_grid" in rkv
    dec = re.sub(r"//[^\n]*", "", _read("neuronika_amd", "csrc", "nk_attention_decode.h"))
    assert "constexpr int ADEC_GQA_HEADS = 8;" in dec and "adec_combine_kernel" in dec and "adec_chunk_of(" in dec
    # the grouped result is the plain result by construction: the arithmetic is stated once, in the bodies the kernels include, and in
    # no kernel's own text
    body = re.sub(r"//[^\n]*", "", _read("neuronika_amd", "csrc", "nk_attention_decode_body.h"))
    generic = re.sub(r"//[^\n]*", "", _read("neuronika_amd", "csrc", "nk_attention_decode_generic_body.h"))
    combine = re.sub(r"//[^\n]*", "", _read("neuronika_amd", "csrc", "nk_attention_decode_combine_body.h"))
    for txt in (body, generic):
        assert txt.count("? __builtin_amdgcn_exp2f(") == 1 and txt.count("__builtin_amdgcn_exp2f") == 1       # the select of a probability
        assert txt.count("for (int k = 1; k < G; ++k)") == 1                                                    # the groups in order
        assert "__global__" not in txt and "#pragma once" not in txt
    assert body.count("__shfl_xor(") == 1 and body.count("nk_wave_max(") == 1 and body.count("o / ls") == 1
    assert combine.count("__builtin_amdgcn_exp2f") == 1 and "__global__" not in combine
    for word in ("__builtin_amdgcn_exp2f", "__builtin_fmaf", "__shfl_xor", "fmaxf", "for (int k = 1;"):
        assert word not in dec, word
    for kernel, inc in (("adec_partial_kernel", "nk_attention_decode_body.h"), ("adec_gqa_partial_kernel", "nk_attention_decode_body.h"),
                        ("adec_generic_kernel", "nk_attention_decode_generic_body.h"),
                        ("adec_gqa_generic_kernel", "nk_attention_decode_generic_body.h")):
        own = _kernel_text(dec, kernel)
        assert own.count("#include") == 1 and '#include "%s"' % inc in own, kernel
        assert not re.search(r"\b(for|if|return)\b", own), kernel                   # switches and the include, no statement of its own
    assert "#define ADEC_GROUPED 0" in _kernel_text(dec, "adec_partial_kernel") and "#define ADEC_NH 1" in _kernel_text(dec, "adec_partial_kernel")
    assert "#define ADEC_GROUPED 1" in _kernel_text(dec, "adec_gqa_partial_kernel")
    assert "#define ADEC_NH ADEC_GQA_HEADS" in _kernel_text(dec, "adec_gqa_partial_kernel")


def test_rust_mirror_names_the_ffi_calls():
    ffi = open(os.path.join(HIP, "ffi.rs")).read()
    for name in ENTRIES:
        assert re.search(rf"pub fn {name}\(", ffi), name
    node = open(os.path.join(HIP, "node", "repeat_kv.rs")).read()
    for name in ("nk_repeat_kv_fwd", "nk_repeat_kv_bwd"):                            # this tape zeroes eagerly: no _assign twin
        assert f"ffi::{name}(" in node, name
    assert "ffi::nk_attention_decode_gqa_fwd(" in open(os.path.join(HIP, "node", "decode.rs")).read()
    assert re.search(r"^mod repeat_kv;", open(os.path.join(HIP, "node", "mod.rs")).read(), re.M)
    hv = open(os.path.join(HIP, "hipvar.rs")).read()
    assert hv.count("pub fn repeat_kv(") == 2 and "RepeatKvBackward::new(" in hv
    nn = open(os.path.join(ROOT, "integration", "neuronika-nn", "src", "hip.rs")).read()
    assert "pub kv_heads: usize" in nn and "pub fn new_grouped(" in nn
    step = nn[nn.index("pub fn forward_step("):]
    assert "self.kv_heads" in step and "self.heads + self.kv_heads" in step


def test_the_example_the_benchmark_and_the_docs():
    txt = _read("examples", "generate.py")
    assert '"tests"' not in txt and "tests/" not in txt and "oracle" not in txt      # nothing of the test infrastructure
    assert '"--kv-heads"' in txt and "kv_heads=kv_heads" in txt
    assert "KvCache(dev, batch, kv_heads," in txt and "logits_full" in txt           # caches built with N; the closing comparison stays
    heads = int(re.search(r"VOCAB, D_MODEL, HEADS, LAYERS, CONTEXT = \d+, \d+, (\d+),", txt).group(1))
    assert heads % 2 == 0 and heads > 2                                              # 2 and 1 kv heads are both proper groupings
    assert os.path.exists(os.path.join(ROOT, "benchmarks", "attention_decode_gqa.py"))
    assert "attention_decode_gqa.py" in _read("benchmarks", "README.md")
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "kv_heads" in _read(doc), doc
    design = _read("DESIGN.md")
    assert "nk_attention_decode_gqa_fwd" in design and "repeat_kv" in design
    out_of_scope = [l for l in design.splitlines() if "Out of scope" in l or "out of scope" in l]
    assert not any("grouped-query / multi-query heads" in l for l in out_of_scope)

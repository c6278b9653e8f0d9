"""The surface of sliding-window attention, layer by layer, without a GPU: the header declares the three entry points and fixes the
semantics, the ctypes table and the built library have them, the workspace function answers without a device and never looks at a
capacity, `_tape` has `window`, `rolling` and the high-water marks, the kernels live in their own header outside the inventoried
units, the Rust mirror names the new ffi calls, the example has the flags and reads nothing of the test infrastructure."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nk_attention_decode_window_fwd", "nk_attention_decode_window_workspace", "nk_kv_cache_append_ring")
HIP = os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points():
    doc = _read("include", "neuronika_hip.h")
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", doc, flags=re.S))
    assert ("int nk_attention_decode_window_fwd(nk_device* dev, const float* Q, int ldq, const float* Kc, const float* Vc, const int* start, "
            "float* O, float* workspace, int B, int T, int H, int Hkv, int dh, int cap, int window, int ring, float scale);") in flat
    assert "size_t nk_attention_decode_window_workspace(int B, int T, int H, int dh, int window);" in flat
    assert ("int nk_kv_cache_append_ring(nk_device* dev, float* Kc, float* Vc, const float* K, const float* V, int ld, const int* start, int B, "
            "int T, int H, int dh, int cap);") in flat
    section = doc[doc.index("sliding-window decoding --"):doc.index("int nk_attention_decode_window_fwd(")]
    for phrase in ("lo = max(0, n - W)", "softmax(q . K[lo:n]^T * scale) . V[lo:n]", "M[r][k] = 0 for r - W < k <= r", "p % cap",
                   "window + T - 1 <= cap", "(W + C - 2) / C + 1", "redirected to position n - 1", "SELECTED to 0", "No atomics",
                   "ascending chunk order", "never a function of cap", "(start[b] + t) % cap", "T > cap", "zero output row",
                   "no dependent load", "NaN or 1e30"):
        assert phrase in section, phrase
    # the derivation of the ring condition is there, not only the condition
    assert "appended before they are attended to" in section and "W + T - 1 consecutive positions" in section
    for n in "1234":
        assert "(%s)" % n in section[section.index("Bit contract"):], n


def test_ctypes_table_and_library_export_them():
    import ctypes
    from neuronika_amd import capi
    for name in ENTRIES:
        assert name in capi.EXPORTED and hasattr(capi.lib, name), name
    assert len(capi._SIGS["nk_attention_decode_window_fwd"]) == 17
    assert len(capi._SIGS["nk_attention_decode_window_workspace"]) == 5 and len(capi._SIGS["nk_kv_cache_append_ring"]) == 12
    assert capi.lib.nk_attention_decode_window_workspace.restype is ctypes.c_size_t
    for wrapper, keys in (("attention_decode_window_fwd", ("Q", "ldq", "Kc", "Vc", "start", "out", "workspace", "B", "T", "H", "Hkv", "dh", "cap",
                                                           "window", "ring", "scale")),
                          ("attention_decode_window_workspace", ("B", "T", "H", "dh", "window")),
                          ("kv_cache_append_ring", ("Kc", "Vc", "K", "V", "ld", "start", "B", "T", "H", "dh", "cap"))):
        params = inspect.signature(getattr(capi, wrapper)).parameters
        assert all(k in params for k in keys), (wrapper, list(params))


def test_the_workspace_is_a_function_of_the_window_and_needs_no_device():
    from neuronika_amd import capi
    for dh in (32, 64, 128, 20, 5):
        C = capi.attention_decode_chunk(dh)
        for W in (1, 2, C - 1, C, C + 1, 2 * C, 2 * C + 3, 4096, 1 << 30):
            for B, T, H in ((1, 1, 1), (3, 4, 8)):
                want = B * T * H * ((W + C - 2) // C + 1) * (dh + 2)
                assert capi.attention_decode_window_workspace(B, T, H, dh, W) == want, (dh, W, B, T, H)
        # one chunk for W = 1 whatever the position, two from W = 2 on (a window may straddle a seam)
        assert capi.attention_decode_window_workspace(1, 1, 1, dh, 1) == dh + 2
        assert capi.attention_decode_window_workspace(1, 1, 1, dh, 2) == 2 * (dh + 2)
        # a window of a whole number of chunks can need one more slot than a capacity-sized scratch of the same length has
        assert capi.attention_decode_window_workspace(1, 1, 1, dh, 2 * C) == capi.attention_decode_workspace(1, 1, 1, dh, 2 * C) // 2 * 3
    for bad in ((0, 1, 1, 64, 8), (1, 0, 1, 64, 8), (1, 1, 0, 64, 8), (1, 1, 1, 0, 8), (1, 1, 1, 64, 0), (1, 1, 1, 64, -3)):
        assert capi.attention_decode_window_workspace(*bad) == 0, bad


def test_bad_arguments_are_refused_before_a_device_is_touched():
    """A null device handle is the first check of every entry point: NK_ERR_INVALID without a GPU."""
    from neuronika_amd import capi
    assert capi.lib.nk_attention_decode_window_fwd(None, None, 0, None, None, None, None, None, 1, 1, 4, 2, 64, 16, 8, 1, 0.125) == 1
    assert capi.lib.nk_kv_cache_append_ring(None, None, None, None, None, 0, None, 1, 1, 1, 64, 16) == 1


def test_host_classes_exist():
    import neuronika_amd
    t = neuronika_amd.tape
    nn = t.nn
    assert isinstance(nn.MultiheadAttention.window, property) and isinstance(nn.KvCache.rolling, property)
    assert hasattr(nn.KvCache, "high_water") and hasattr(nn.KvCache, "workspace_floats")
    init = nn.KvCache.__init__.__doc__
    assert re.search(r"dev: .*, batch: .*, heads: .*, head_dim: .*, capacity: .*, rolling: bool = False\) -> None", init), init
    hpp = _read("host", "neuronika.hpp")
    assert "KvCache(DevicePtr dev, int batch, int heads, int head_dim, int capacity);" in hpp          # the old constructor stays
    assert "KvCache(DevicePtr dev, int batch, int heads, int head_dim, int capacity, bool rolling);" in hpp
    assert "int window = 0;" in hpp and "bool rolling;" in hpp and "high_water()" in hpp
    assert "Shared<HipArray> workspace(int T, int query_heads, int window = 0);" in hpp
    cpp = _read("host", "neuronika.cpp")
    step = cpp[cpp.index("struct DecodeStepFwd"):]
    step = step[:step.index("\n};")]
    for call in ("nk_attention_decode_window_fwd(", "nk_kv_cache_append_ring(", "nk_kv_cache_append(", "nk_attention_decode_gqa_fwd(",
                 "nk_attention_decode_fwd("):
        assert call in step, call
    assert "zeros_like" not in step and "make_shared" not in step                     # nothing is allocated inside forward()
    assert step.index("rope_inplace(") < step.index("nk_kv_cache_append_ring(") < step.index("nk_attention_decode_window_fwd(")
    assert "nk_attention_decode_window_workspace(" in cpp[cpp.index("KvCache::workspace"):cpp.index("void KvCache::advance")]
    # the panics of forward_step, each with its message
    fs = cpp[cpp.index("Var MultiheadAttention::forward_step("):]
    for msg in ("it needs a layer with window > 0", "(window + T - 1 <= capacity): chunk the prompt", "exceed rope's table of",
                "exceed the cache's capacity of"):
        assert msg in fs, msg


def _kernel_text(src, name):
    """a kernel's own text in the decode header: from its `__global__` to the closing brace in column 0"""
    at = src.index(name + "(")
    start = src.rindex("__global__", 0, at)
    return src[start:src.index("\n}\n", at) + 1]


def test_kernels_live_in_their_own_header_outside_the_inventoried_units():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dispatch_paths
    import dispatch_paths_mfma
    import list_unit_kernels as luk
    header = "nk_attention_decode.h"
    bodies = {"partial": "nk_attention_decode_body.h", "generic": "nk_attention_decode_generic_body.h",
              "combine": "nk_attention_decode_combine_body.h"}
    mine = {"adw_partial_kernel", "adw_generic_kernel", "adw_combine_kernel", "kv_append_ring_kernel"}
    path = os.path.join(luk.CSRC, header)
    assert mine <= luk.file_kernels(path) and len(luk.file_kernels(path)) == 10
    includers = [u for u in luk.all_units() if header in luk.unit_sources(u)]
    assert includers == ["nk_norm.hip"] and includers[0] in [u for u, _ in dispatch_paths_mfma.NOT_INVENTORIED]
    assert _read("neuronika_amd", "csrc", "nk_norm.hip").count('#include "%s"' % header) == 1
    for u in dispatch_paths.UNITS + dispatch_paths_mfma.UNITS:
        assert not (mine & luk.source_kernels(u)), u
    assert not [f for f in os.listdir(luk.CSRC) if f.endswith(".hip") and "window" in f]       # no new translation unit
    src = re.sub(r"//[^\n]*", "", open(path).read())
    for f in (header,) + tuple(bodies.values()):
        txt = re.sub(r"//[^\n]*", "", _read("neuronika_amd", "csrc", f))
        assert "atomic" not in txt.lower() and "num_cus" not in txt and "tune_" not in txt, f
        assert "hipMalloc" not in txt and "Synchronize" not in txt, f
    assert "float4" in src and "adec_chunk_of(" in src and "ADEC_GQA_HEADS" in src and "adw_chunks_of(" in src
    for inst in ("adw_partial_kernel<DH, 1>", "adw_partial_kernel<DH, ADEC_GQA_HEADS>", "kv_append_ring_kernel<float4>", "kv_append_ring_kernel<float>",
                 "kv_append_kernel<float4>", "kv_append_kernel<float>", "adec_partial_kernel<DH>", "adec_gqa_partial_kernel<DH>"):
        assert inst in src, inst
    for dh in (32, 64, 128):
        assert "ADEC_LAUNCH(%d);" % dh in src
    # the windowed result at n <= W is the plain and the grouped result by construction: each of the three partial kernels and each of
    # the three generic kernels is its switches around the ONE body, with no statement of its own
    switches = {"adec_partial_kernel": ("partial", "0", "1", "0"), "adec_gqa_partial_kernel": ("partial", "1", "ADEC_GQA_HEADS", "0"),
                "adw_partial_kernel": ("partial", "1", "NH", "1"), "adec_generic_kernel": ("generic", "0", None, "0"),
                "adec_gqa_generic_kernel": ("generic", "1", None, "0"), "adw_generic_kernel": ("generic", "1", None, "1"),
                "adec_combine_kernel": ("combine", None, None, "0"), "adw_combine_kernel": ("combine", None, None, "1")}
    for kernel, (body, grouped, nh, window) in switches.items():
        own = _kernel_text(src, kernel)
        assert own.count("#include") == 1 and '#include "%s"' % bodies[body] in own, kernel
        assert not re.search(r"\b(for|if|return)\b", own) and "__builtin" not in own, kernel
        for macro, value in (("ADEC_GROUPED", grouped), ("ADEC_NH", nh), ("ADEC_WINDOW", window)):
            assert (value is None and macro not in own) or "#define %s %s\n" % (macro, value) in own, (kernel, macro)
            assert value is None or "#undef %s\n" % macro in own, (kernel, macro)
    # the window and the slots live in the bodies, behind the switch
    partial = re.sub(r"//[^\n]*", "", _read("neuronika_amd", "csrc", bodies["partial"]))
    assert "#if ADEC_WINDOW" in partial and "lo % cap" in partial and "(unsigned)" in partial and "adec_wrap(" in partial
    ring = src[src.index("void kv_append_body("):]
    ring = ring[:ring.index("\n}\n")]
    assert "RING ? pos % cap : pos" in ring and "!RING && pos >= cap" in ring
    for kernel, flag in (("kv_append_kernel", "false"), ("kv_append_ring_kernel", "true")):
        assert "kv_append_body<T, %s>(" % flag in _kernel_text(src, kernel), kernel


def test_rust_mirror_names_the_ffi_calls():
    ffi = open(os.path.join(HIP, "ffi.rs")).read()
    for name in ENTRIES:
        assert re.search(rf"pub fn {name}\(", ffi), name
    assert re.search(r"pub fn nk_attention_decode_window_workspace\([^)]*\) -> usize;", ffi)
    node = open(os.path.join(HIP, "node", "decode.rs")).read()
    for name in ENTRIES:
        assert f"ffi::{name}(" in node, name
    assert "window: i32" in node and "ring: bool" in node
    hv = open(os.path.join(HIP, "hipvar.rs")).read()
    assert "pub fn new_rolling(" in hv and "decode_window_workspace(" in hv
    assert re.search(r"pub fn packed_decode_attention\(self, buffers: &KvBuffers, query_heads: usize, start: &\[usize\], scale: f32, window: usize\)", hv)
    nn = open(os.path.join(ROOT, "integration", "neuronika-nn", "src", "hip.rs")).read()
    assert "pub window: usize" in nn and "pub fn new_rolling(" in nn and "pub fn high_water(" in nn
    step = nn[nn.index("pub fn forward_step("):]
    assert "self.window" in step and "cache.rolling()" in step


def test_the_example_the_benchmark_and_the_docs():
    txt = _read("examples", "generate.py")
    assert '"tests"' not in txt and "tests/" not in txt and "oracle" not in txt      # nothing of the test infrastructure
    assert '"--window"' in txt and '"--rolling"' in txt and "rolling=True" in txt and "self.mha.window = window" in txt
    assert os.path.exists(os.path.join(ROOT, "benchmarks", "attention_decode_window.py"))
    assert "attention_decode_window.py" in _read("benchmarks", "README.md")
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "sliding-window" in _read(doc).lower(), doc
    design = _read("DESIGN.md")
    assert "nk_attention_decode_window_fwd" in design and "window + T - 1 <= cap" in design and "(W + C - 2) / C + 1" in design

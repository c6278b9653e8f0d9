"""The surface of incremental decoding, layer by layer, without a GPU: the header declares the four entry points, the ctypes table
and the built library have them, the host classes exist with the documented members, the kernels live in their own header outside
the inventoried units, and the Rust mirror names the ffi calls."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nk_kv_cache_append", "nk_attention_decode_fwd", "nk_attention_decode_workspace", "nk_attention_decode_chunk")
HIP = os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points():
    doc = _read("include", "neuronika_hip.h")
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", doc, flags=re.S))
    assert ("int nk_kv_cache_append(nk_device* dev, float* Kc, float* Vc, const float* K, const float* V, int ld, const int* start, "
            "int B, int T, int H, int dh, int cap);") in flat
    assert ("int nk_attention_decode_fwd(nk_device* dev, const float* Q, int ldq, const float* Kc, const float* Vc, const int* start, "
            "float* O, float* workspace, int B, int T, int H, int dh, int cap, float scale);") in flat
    assert "size_t nk_attention_decode_workspace(int B, int T, int H, int dh, int cap);" in flat
    assert "int nk_attention_decode_chunk(int dh);" in flat
    for phrase in ("(B, H, cap, dh)", "start[b] + t + 1", "No atomics", "compile-time constant", "node/softmax/mod.rs:37-53", "NaN"):
        assert phrase in doc, phrase


def test_ctypes_table_and_library_export_them():
    import ctypes
    from neuronika_amd import capi
    for name in ENTRIES:
        assert name in capi.EXPORTED and hasattr(capi.lib, name), name
    assert len(capi._SIGS["nk_kv_cache_append"]) == 12 and len(capi._SIGS["nk_attention_decode_fwd"]) == 14
    assert capi.lib.nk_attention_decode_workspace.restype is ctypes.c_size_t
    for wrapper, keys in (("kv_cache_append", ("Kc", "Vc", "K", "V", "ld", "start", "B", "T", "H", "dh", "cap")),
                          ("attention_decode_fwd", ("Q", "ldq", "Kc", "Vc", "start", "out", "workspace", "B", "T", "H", "dh", "cap", "scale")),
                          ("attention_decode_workspace", ("B", "T", "H", "dh", "cap")), ("attention_decode_chunk", ("dh",))):
        params = inspect.signature(getattr(capi, wrapper)).parameters
        assert all(k in params for k in keys), (wrapper, list(params))


def test_chunk_and_workspace_need_no_device():
    """Both are pure functions of the geometry: the chunk is a constant per head size, whatever else is going on."""
    from neuronika_amd import capi
    chunks = {dh: capi.attention_decode_chunk(dh) for dh in (32, 64, 128, 20, 5, 48, 256)}
    assert all(c >= 64 for c in chunks.values()), chunks
    assert chunks[20] == chunks[5] == chunks[48] == chunks[256]          # one generic instantiation
    assert capi.attention_decode_chunk(0) == 0 and capi.attention_decode_chunk(-3) == 0
    for dh, c in chunks.items():
        for B, T, H, cap in ((1, 1, 1, 1), (2, 4, 3, c), (2, 1, 3, c + 1), (8, 1, 16, 4096)):
            want = B * T * H * ((cap + c - 1) // c) * (dh + 2)           # (m, l, o[dh]) per (problem, chunk)
            assert capi.attention_decode_workspace(B, T, H, dh, cap) == want, (dh, B, T, H, cap)
    assert capi.attention_decode_workspace(0, 1, 1, 64, 16) == 0


def test_host_classes_exist():
    import neuronika_amd
    nn = neuronika_amd.tape.nn
    for member in ("lens", "reset", "truncate", "capacity", "batch", "heads", "head_dim"):
        assert hasattr(nn.KvCache, member), member
    assert hasattr(nn.MultiheadAttention, "forward_step") and hasattr(nn.MultiheadAttention, "forward")
    doc = nn.MultiheadAttention.forward_step.__doc__
    assert re.search(r"forward_step\(self: .*, x: [\w.]*Var, batch: .*, cache: [\w.]*KvCache\) -> [\w.]*Var\n", doc), doc
    assert not re.search(r"-> [\w.]*VarDiff", doc), doc                  # no overload returns a gradient
    assert re.search(r"__init__\(self: .*, dev: .*, batch: .*, heads: .*, head_dim: .*, capacity: .*\)", nn.KvCache.__init__.__doc__)
    hpp = _read("host", "neuronika.hpp")
    assert "Var forward_step(const Var& x, int batch, KvCache& cache) const;" in hpp
    assert "KvCache(DevicePtr dev, int batch, int heads, int head_dim, int capacity);" in hpp
    assert "void truncate(const std::vector<int>& lens);" in hpp


DECODE_HEADER = "nk_attention_decode.h"
DECODE_BODIES = ("nk_attention_decode_body.h", "nk_attention_decode_generic_body.h", "nk_attention_decode_combine_body.h")
DECODE_KERNELS = {"kv_append_kernel", "kv_append_ring_kernel", "adec_partial_kernel", "adec_gqa_partial_kernel", "adw_partial_kernel",
                  "adec_generic_kernel", "adec_gqa_generic_kernel", "adw_generic_kernel", "adec_combine_kernel", "adw_combine_kernel"}


def test_kernels_live_in_their_own_header_outside_the_inventoried_units():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dispatch_paths
    import dispatch_paths_mfma
    import list_unit_kernels as luk
    # one header holds every kernel signature of the three decode forms; the bodies they include hold no kernel of their own
    mine = luk.file_kernels(os.path.join(luk.CSRC, DECODE_HEADER))
    assert mine == DECODE_KERNELS
    for body in DECODE_BODIES:
        assert luk.file_kernels(os.path.join(luk.CSRC, body)) == set(), body
    assert not os.path.exists(os.path.join(luk.CSRC, "nk_attention_gqa.h")) and not os.path.exists(os.path.join(luk.CSRC, "nk_attention_window.h"))
    norm = _read("neuronika_amd", "csrc", "nk_norm.hip")
    for f in (DECODE_HEADER,) + DECODE_BODIES:
        includers = [u for u in luk.all_units() if f in luk.unit_sources(u)]     # a body included inside a kernel is found too
        assert includers == ["nk_norm.hip"] and includers[0] in [u for u, _ in dispatch_paths_mfma.NOT_INVENTORIED], f
        assert norm.count('#include "%s"' % f) == (1 if f == DECODE_HEADER else 0), f
    assert mine <= luk.source_kernels("nk_norm.hip")
    for u in dispatch_paths.UNITS + dispatch_paths_mfma.UNITS:
        assert not (mine & luk.source_kernels(u)), u
    assert not [f for f in os.listdir(luk.CSRC) if f.endswith(".hip") and "decode" in f]       # no translation unit of its own
    for f in (DECODE_HEADER,) + DECODE_BODIES:
        src = re.sub(r"//[^\n]*", "", _read("neuronika_amd", "csrc", f))
        assert "atomic" not in src.lower(), f                            # partials are merged in chunk order
        assert "num_cus" not in src and "tune_" not in src and "hipMalloc" not in src and "Synchronize" not in src, f
    # the chunk is a compile-time constant per head size: nothing of the device handle reaches it
    src = re.sub(r"//[^\n]*", "", _read("neuronika_amd", "csrc", DECODE_HEADER))
    fn = src[src.index("constexpr int adec_chunk_of"):]
    fn = fn[:fn.index("}") + 1]
    assert fn.startswith("constexpr int adec_chunk_of(int dh) {") and not (set(re.findall(r"[A-Za-z_]\w*", fn)) - {
        "constexpr", "int", "adec_chunk_of", "dh", "return", "ADEC_THREADS", "ADEC_KPG", "ADEC_CHUNK_GENERIC"}), fn


def test_rust_mirror_names_the_ffi_calls():
    ffi = open(os.path.join(HIP, "ffi.rs")).read()
    for name in ENTRIES:
        assert re.search(rf"pub fn {name}\(", ffi), name
    assert re.search(r"pub fn nk_attention_decode_workspace\([^)]*\) -> usize;", ffi)
    node = open(os.path.join(HIP, "node", "decode.rs")).read()
    for name in ENTRIES:
        assert f"ffi::{name}(" in node, name
    assert "pub(crate) mod decode;" in open(os.path.join(HIP, "node", "mod.rs")).read() or "mod decode;" in open(os.path.join(HIP, "node", "mod.rs")).read()
    nn = open(os.path.join(ROOT, "integration", "neuronika-nn", "src", "hip.rs")).read()
    assert "pub struct KvCache" in nn and "pub fn forward_step(" in nn[nn.index("impl MultiheadAttention"):]
    for member in ("pub fn lens(", "pub fn reset(", "pub fn truncate("):
        assert member in nn[nn.index("impl KvCache"):], member


def test_the_example_reads_nothing_of_the_test_infrastructure():
    txt = _read("examples", "generate.py")
    assert '"tests"' not in txt and "tests/" not in txt and "oracle" not in txt
    assert "forward_step" in txt and "KvCache" in txt and "Embedding" in txt and "LayerNorm" in txt

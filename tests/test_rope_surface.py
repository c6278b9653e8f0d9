"""The surface of the rotary position embedding, layer by layer, without a GPU: the header declares the four entry points and fixes
the semantics, the ctypes table and the built library have them, the host classes exist with the documented members, the kernels
live in their own header outside the inventoried units, and the Rust mirror names the ffi calls."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nk_rope_table", "nk_rope_fwd", "nk_rope_bwd", "nk_rope_bwd_assign")
HIP = os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points():
    doc = _read("include", "neuronika_hip.h")
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", doc, flags=re.S))
    assert "int nk_rope_table(nk_device* dev, float* table, int max_pos, int rot, double base);" in flat
    assert ("int nk_rope_fwd(nk_device* dev, const float* x, int ldx, float* y, int ldy, const float* table, const int* start, int B, int T, "
            "int NH, int dh, int rot, int max_pos, int interleaved);") in flat
    for name in ("nk_rope_bwd", "nk_rope_bwd_assign"):
        assert ("int %s(nk_device* dev, float* dx, int lddx, const float* g, int ldg, const float* table, const int* start, int B, int T, "
                "int NH, int dh, int rot, int max_pos, int interleaved);" % name) in flat
    for phrase in ("(start ? start[b] : 0) + t", "nk_kv_cache_append", "(j, j + rot/2)", "(2j, 2j+1)",
                   "y1 = fmaf(x1, c, -(x2 * s));   y2 = fmaf(x2, c, x1 * s)", "s -> -s", "(max_pos, rot/2, 2)", "base^(-2j/rot)", "in f64",
                   "clamped", "in-place form", "assign form only", "No atomics", "64-bit", "NK_ERR_INVALID"):
        assert phrase in doc, phrase


def test_ctypes_table_and_library_export_them():
    from neuronika_amd import capi
    for name in ENTRIES:
        assert name in capi.EXPORTED and hasattr(capi.lib, name), name
    assert len(capi._SIGS["nk_rope_table"]) == 5
    assert len(capi._SIGS["nk_rope_fwd"]) == len(capi._SIGS["nk_rope_bwd"]) == len(capi._SIGS["nk_rope_bwd_assign"]) == 14
    for wrapper, keys in (("rope_table", ("table", "max_pos", "rot", "base")),
                          ("rope_fwd", ("x", "ldx", "y", "ldy", "table", "start", "B", "T", "NH", "dh", "rot", "max_pos", "interleaved")),
                          ("rope_bwd", ("dx", "lddx", "g", "ldg", "table", "start", "B", "T", "NH", "dh", "rot", "max_pos", "interleaved", "assign"))):
        params = inspect.signature(getattr(capi, wrapper)).parameters
        assert all(k in params for k in keys), (wrapper, list(params))


def test_host_classes_exist():
    import neuronika_amd
    t = neuronika_amd.tape
    nn = t.nn
    for member in ("head_dim", "max_pos", "rot", "base", "interleaved", "table"):
        assert hasattr(nn.RotaryEmbedding, member), member
    assert re.search(r"__init__\(self: .*, dev: .*, head_dim: .*, max_pos: .*, base: .* = 10000.0, rot: .*, interleaved: bool = False\)",
                     nn.RotaryEmbedding.__init__.__doc__)
    assert isinstance(nn.MultiheadAttention.rope, property)
    assert re.search(r"rope\(self: [\w.]*Var, rotary: [\w.]*RotaryEmbedding, batch: .*, heads: .*\) -> [\w.]*Var\n", t.Var.rope.__doc__)
    assert re.search(r"rope\(self: [\w.]*VarDiff, rotary: [\w.]*RotaryEmbedding, batch: .*, heads: .*\) -> [\w.]*VarDiff\n", t.VarDiff.rope.__doc__)
    hpp = _read("host", "neuronika.hpp")
    assert "RotaryEmbedding(DevicePtr dev, int head_dim, int max_pos, double base = 10000.0, int rot = 0, bool interleaved = false);" in hpp
    assert "Var rope(const nn::RotaryEmbedding& rotary, int batch, int heads) const;" in hpp
    assert "VarDiff rope(const nn::RotaryEmbedding& rotary, int batch, int heads) const;" in hpp
    assert "Shared<RotaryEmbedding> rope;" in hpp
    cpp = _read("host", "neuronika.cpp")
    for node in ("struct RopeFwd : Forward", "struct RopeBwd : Backward"):
        assert node in cpp, node
    # the attention nodes rotate in place: the packed pair and the decode step name the helper, the backward applies the inverse
    for node in ("QkvAttentionFwd", "QkvAttentionBwd", "DecodeStepFwd"):
        body = cpp[cpp.index("struct %s" % node):]
        assert "rope_inplace(" in body[:body.index("\n};")], node
    step = cpp[cpp.index("struct DecodeStepFwd"):]
    step = step[:step.index("\n};")]
    assert step.index("rope_inplace(") < step.index("nk_kv_cache_append(")            # the cache holds rotated keys


def test_kernels_live_in_their_own_header_outside_the_inventoried_units():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dispatch_paths
    import dispatch_paths_mfma
    import list_unit_kernels as luk
    header = os.path.join(luk.CSRC, "nk_rope.h")
    mine = luk.file_kernels(header)
    assert {"rope_vec_kernel", "rope_scalar_kernel"} <= mine
    includers = [u for u in luk.all_units() if "nk_rope.h" in luk.unit_sources(u)]
    assert len(includers) == 1 and includers[0] in [u for u, _ in dispatch_paths_mfma.NOT_INVENTORIED]
    for u in dispatch_paths.UNITS + dispatch_paths_mfma.UNITS:
        assert not (mine & luk.source_kernels(u)), u
    src = re.sub(r"//[^\n]*", "", open(header).read())
    assert "atomic" not in src.lower() and "__shared__" not in src and "__syncthreads" not in src
    assert "fmaf(x1, c, -(x2 * s))" in src and "fmaf(x2, c, x1 * s)" in src and src.count("fmaf(") == 2     # ONE statement of the expression
    assert "float4" in src and "nk_stream_grid" in src
    assert "sinf" not in src and "cosf" not in src and "__sinf" not in src                                   # angles are never formed in f32
    assert open(os.path.join(luk.CSRC, "nk_norm.hip")).read().count('#include "nk_rope.h"') == 1


def test_rust_mirror_names_the_ffi_calls():
    ffi = open(os.path.join(HIP, "ffi.rs")).read()
    for name in ENTRIES:
        assert re.search(rf"pub fn {name}\(", ffi), name
    node = open(os.path.join(HIP, "node", "rope.rs")).read()
    for name in ENTRIES:
        assert f"ffi::{name}(" in node, name
    assert re.search(r"^mod rope;", open(os.path.join(HIP, "node", "mod.rs")).read(), re.M)
    hv = open(os.path.join(HIP, "hipvar.rs")).read()
    assert "pub struct RotaryTable" in hv and hv.count("pub fn rope(") == 2 and hv.count("pub fn rope_in_place(") == 2
    assert "RotaryTable" in open(os.path.join(HIP, "mod.rs")).read()
    nn = open(os.path.join(ROOT, "integration", "neuronika-nn", "src", "hip.rs")).read()
    assert "pub struct RotaryEmbedding" in nn and "pub rope: Option<Rc<RotaryEmbedding>>" in nn
    mha = nn[nn.index("impl MultiheadAttention"):]
    fwd, step = mha[mha.index("pub fn forward("):mha.index("pub fn forward_step(")], mha[mha.index("pub fn forward_step("):]
    assert ".rope_in_place(" in fwd and ".rope_in_place(" in step
    assert step.index(".rope_in_place(") < step.index(".packed_decode_attention(")    # rotated before the append


def test_the_example_and_the_benchmark_exist():
    txt = _read("examples", "generate.py")
    assert "--rope" in txt and "RotaryEmbedding" in txt and '"tests"' not in txt and "oracle" not in txt
    assert os.path.exists(os.path.join(ROOT, "benchmarks", "rope.py")) and "rope.py" in _read("benchmarks", "README.md")
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "nk_rope_fwd" in _read(doc) or "RotaryEmbedding" in _read(doc), doc

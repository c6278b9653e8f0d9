"""The surface of the group / instance normalisation, layer by layer, without a GPU: the header declares the five entry points,
the ctypes table has them with the header's argument counts, the Rust ffi names them, the host module exposes the layers and the
variable methods, and the kernels live in one header that nk_norm.hip alone includes, once, and that neither uses atomics nor
allocates, synchronises, asks for the CU count, reads a tuning override or takes the streaming switch."""
import ctypes as C
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nk_group_norm_fwd", "nk_group_norm_bwd", "nk_group_norm_bwd_assign", "nk_group_norm_bwd_params", "nk_group_norm_bwd_params_assign")
HIP = os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip")
CSRC = os.path.join(ROOT, "neuronika_amd", "csrc")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _header_arity():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", _read("include", "neuronika_hip.h"), flags=re.S))
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"int (nk_group_norm\w*)\(([^)]*)\);", flat)}, flat


def test_header_declares_the_entry_points():
    arity, flat = _header_arity()
    assert tuple(arity) == ENTRIES                                                       # named and ordered like LayerNorm's
    assert ("int nk_group_norm_fwd(nk_device* dev, const float* x, const float* gamma, const float* beta, float* y, float* stats, "
            "long long N, int C, long long L, int G, double eps);") in flat
    for name in ENTRIES[1:3]:
        assert ("int %s(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats, long long N, "
                "int C, long long L, int G);" % name) in flat
    for name in ENTRIES[3:]:
        assert ("int %s(nk_device* dev, float* dgamma, float* dbeta, const float* g, const float* x, const float* stats, long long N, "
                "int C, long long L, int G);" % name) in flat
    doc = _read("include", "neuronika_hip.h")
    for phrase in ("never E[x^2] - mean^2", "stats[N * G][2] = {mean, rstd}", "c = j * Cg + (offset in the row) / L", "G == C is instance normalisation",
                   "track_running_stats of instance norm is not built", "dx        += rstd * (gh - mean_D(gh) - xhat * mean_D(gh * xhat))",
                   "chunks of 8192 floats", "No atomics, and no block waits on another", "captured into a graph"):
        assert phrase in doc, phrase


def test_ctypes_table_has_the_headers_argument_counts():
    from neuronika_amd import capi
    arity, _ = _header_arity()
    VP = C.c_void_p
    for name in ENTRIES:
        assert name in capi.EXPORTED and hasattr(capi.lib, name), name
        assert len(capi._SIGS[name]) == arity[name], name
    geom = [C.c_longlong, C.c_int, C.c_longlong, C.c_int]
    assert capi._SIGS["nk_group_norm_fwd"] == [VP] * 6 + geom + [C.c_double]
    for name in ENTRIES[1:]:
        assert capi._SIGS[name] == [VP] * 6 + geom, name
    for wrapper, keys in (("group_norm_fwd", ("x", "gamma", "beta", "y", "stats", "N", "C", "L", "G", "eps")),
                          ("group_norm_bwd", ("dx", "g", "x", "gamma", "stats", "N", "C", "L", "G", "assign")),
                          ("group_norm_bwd_params", ("dgamma", "dbeta", "g", "x", "stats", "N", "C", "L", "G", "assign"))):
        params = inspect.signature(getattr(capi, wrapper)).parameters
        assert all(k in params for k in keys), (wrapper, list(params))


def test_rust_mirror_names_the_ffi_calls():
    ffi = open(os.path.join(HIP, "ffi.rs")).read()
    for name in ENTRIES:
        assert re.search(rf"pub fn {name}\(", ffi), name
    node = open(os.path.join(HIP, "node", "group_norm.rs")).read()
    for name in ("nk_group_norm_fwd", "nk_group_norm_bwd", "nk_group_norm_bwd_params"):   # that tape zeroes eagerly: no _assign twins
        assert f"ffi::{name}(" in node, name
    assert re.search(r"^mod group_norm;", open(os.path.join(HIP, "node", "mod.rs")).read(), re.M)
    hv = open(os.path.join(HIP, "hipvar.rs")).read()
    assert hv.count("pub fn group_norm(") == 2 and "GroupNormBackward::new(" in hv
    nn = open(os.path.join(ROOT, "integration", "neuronika-nn", "src", "hip.rs")).read()
    for layer in ("pub struct GroupNorm", "InstanceNorm1d", "InstanceNorm2d", "InstanceNorm3d"):
        assert layer in nn, layer


def test_host_module_exposes_the_layers_and_the_methods():
    import neuronika_amd
    t = neuronika_amd.tape
    for cls in (t.Var, t.VarDiff):
        doc = cls.group_norm.__doc__
        assert doc.count("group_norm(self") == 3 and "num_groups" in doc and doc.count(" = 1e-05) -> ") == 3, doc
    for member in ("weight", "bias", "num_groups", "num_channels", "eps", "affine", "forward"):
        assert hasattr(t.nn.GroupNorm, member), member
    init = t.nn.GroupNorm.__init__.__doc__
    assert re.search(r"dev: .*, num_groups: .*, num_channels: .*, eps: .* = 1e-05, affine: bool = True\) -> None", init)
    assert re.search(r"num_groups: .*, weight: [\w.:]*VarDiff, bias: [\w.:]*VarDiff, eps: .* = 1e-05\) -> None", init)   # from existing parameters
    for name in ("InstanceNorm1d", "InstanceNorm2d", "InstanceNorm3d"):
        layer = getattr(t.nn, name)
        assert issubclass(layer, t.nn.InstanceNormNd), name
        assert re.search(r"dev: .*, num_features: .*, eps: .* = 1e-05, affine: bool = False\) -> None", layer.__init__.__doc__), name
        assert not hasattr(layer, "running_mean") and not hasattr(layer, "track_running_stats")
    assert "GroupNorm" in t.serde.to_json.__doc__ and hasattr(t.serde, "group_norm_from_json")
    cpp = _read("host", "neuronika.cpp")
    for node in ("struct GroupNormFwd : Forward", "struct GroupNormBwd : Backward"):
        assert cpp.count(node) == 1, node
    bwd = cpp[cpp.index("struct GroupNormBwd"):]
    bwd = bwd[:bwd.index("\n};")]
    for call in ENTRIES[1:]:
        assert call in bwd, call
    assert bwd.count("borrow_first_write(") == 3                                         # dx, dgamma, dbeta: each its own first-writer state


def _stripped(path):
    txt = open(path).read()
    return re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", txt), flags=re.S)


def test_the_kernel_header_is_included_once_by_the_norm_unit_alone():
    includers = {}
    for f in sorted(os.listdir(CSRC)):
        n = len(re.findall(r'^\s*#\s*include\s+"nk_group_norm\.h"', open(os.path.join(CSRC, f)).read(), re.M))
        if n:
            includers[f] = n
    assert includers == {"nk_norm.hip": 1}
    assert not re.fullmatch(r"nk_norm_\w+_body\.h", "nk_group_norm.h")
    src = open(os.path.join(CSRC, "nk_norm.hip")).read()
    at = src.index('#include "nk_group_norm.h"')
    for helper in ("void quads_load(", "void row_stats(", "float owner_sum("):           # behind the helpers it builds on
        assert 0 <= src.index(helper) < at, helper
    code = _stripped(os.path.join(CSRC, "nk_group_norm.h"))
    for word in ("atomic", "hipMalloc", "Synchronize", "num_cus", "tune_", "nk_streams_past_cache("):
        assert word not in code, word
    assert "Atomic" not in code
    for helper in ("quads_load<", "row_stats<", "owner_sum<", "nk_workspace("):
        assert helper in code, helper


def test_the_kernels_are_in_the_built_library():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import list_unit_kernels as luk
    declared = luk.file_kernels(os.path.join(CSRC, "nk_group_norm.h"))
    assert declared == {"group_norm_fwd_kernel", "group_norm_bwd_kernel", "group_norm_chunk_stats_kernel", "group_norm_chunk_apply_kernel",
                        "group_norm_chunk_bwd_sums_kernel", "group_norm_chunk_bwd_kernel", "group_norm_fwd_generic_kernel",
                        "group_norm_bwd_generic_kernel", "group_norm_param_plane_kernel"}
    assert "nk_group_norm.h" in luk.unit_sources("nk_norm.hip")
    built = {re.sub(r"<.*$", "", k) for k in luk.unit_kernels(("nk_norm.hip",))["nk_norm.hip"]}
    assert declared <= built, sorted(declared - built)
    assert {"layer_norm_fwd_kernel", "rms_norm_fwd_kernel"} <= built                      # the same code object as the LayerNorm family


def test_the_benchmark_and_the_docs():
    assert os.path.exists(os.path.join(ROOT, "benchmarks", "group_norm.py")) and "group_norm.py" in _read("benchmarks", "README.md")
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        txt = _read(doc)
        assert "GroupNorm" in txt and "InstanceNorm" in txt, doc
    design = _read("DESIGN.md")
    assert "track_running_stats" in design and "8192" in design

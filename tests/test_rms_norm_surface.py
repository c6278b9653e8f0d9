"""The surface of the RMS normalisation, layer by layer, without a GPU: the header declares the five entry points and fixes the
semantics, the ctypes table and the built library have them with the right argument types, the host classes and the serde pair
exist, the kernels live in nk_norm.hip beside the LayerNorm family, the Rust mirror names the ffi calls, the example has the flag."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nk_rms_norm_fwd", "nk_rms_norm_bwd", "nk_rms_norm_bwd_assign", "nk_rms_norm_bwd_gamma", "nk_rms_norm_bwd_gamma_assign")
HIP = os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points():
    doc = _read("include", "neuronika_hip.h")
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", doc, flags=re.S))
    assert "int nk_rms_norm_fwd(nk_device* dev, const float* x, const float* gamma, float* y, float* stats, long long rows, int D, double eps);" in flat
    for name in ("nk_rms_norm_bwd", "nk_rms_norm_bwd_assign"):
        assert ("int %s(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats, long long rows, "
                "int D);" % name) in flat
    for name in ("nk_rms_norm_bwd_gamma", "nk_rms_norm_bwd_gamma_assign"):
        assert "int %s(nk_device* dev, float* dgamma, const float* g, const float* x, const float* stats, long long rows, int D);" % name in flat
    for phrase in ("ms   = sum(x * x) / D", "no centring, no mean", "rstd = 1 / sqrt(ms + eps)", "there is no beta", "stats[rows] = rstd",
                   "dx     += rstd * (gh - xhat * c)", "dgamma += sum over rows of g * xhat", "rstd = 1 / sqrt(eps)", "only that row",
                   "overflows f32 gives rstd = 0", "(1 + gamma)", "without atomics", "captured into a graph"):
        assert phrase in doc, phrase


def test_ctypes_table_and_library_export_them():
    from neuronika_amd import capi
    VP = C.c_void_p
    for name in ENTRIES:
        assert name in capi.EXPORTED and hasattr(capi.lib, name), name
    assert capi._SIGS["nk_rms_norm_fwd"] == [VP] * 5 + [C.c_longlong, C.c_int, C.c_double]
    for name in ("nk_rms_norm_bwd", "nk_rms_norm_bwd_assign"):
        assert capi._SIGS[name] == [VP] * 6 + [C.c_longlong, C.c_int], name
    for name in ("nk_rms_norm_bwd_gamma", "nk_rms_norm_bwd_gamma_assign"):
        assert capi._SIGS[name] == [VP] * 5 + [C.c_longlong, C.c_int], name
    for wrapper, keys in (("rms_norm_fwd", ("x", "gamma", "y", "stats", "rows", "D", "eps")),
                          ("rms_norm_bwd", ("dx", "g", "x", "gamma", "stats", "rows", "D", "assign")),
                          ("rms_norm_bwd_gamma", ("dgamma", "g", "x", "stats", "rows", "D", "assign"))):
        params = inspect.signature(getattr(capi, wrapper)).parameters
        assert all(k in params for k in keys), (wrapper, list(params))
    assert inspect.signature(capi.rms_norm_fwd).parameters["eps"].default == 1e-6


def test_host_classes_exist():
    import neuronika_amd
    t = neuronika_amd.tape
    for cls in (t.Var, t.VarDiff):
        doc = cls.rms_norm.__doc__
        assert doc.count("rms_norm(self") == 3 and doc.count(" = 1e-06) -> ") == 3 and "normalized_shape" in doc, doc
    for member in ("weight", "normalized_shape", "eps", "elementwise_affine", "forward"):
        assert hasattr(t.nn.RMSNorm, member), member
    assert not hasattr(t.nn.RMSNorm, "bias")
    init = t.nn.RMSNorm.__init__.__doc__
    assert re.search(r"dev: .*, normalized_shape: .*, eps: .* = 1e-06, elementwise_affine: bool = True\) -> None", init)
    assert re.search(r"weight: [\w.:]*VarDiff, eps: .* = 1e-06\) -> None", init)
    assert "RMSNorm" in t.serde.to_json.__doc__ and hasattr(t.serde, "rms_norm_from_json")
    hpp = _read("host", "neuronika.hpp")
    assert hpp.count("Var rms_norm(const Var& gamma, double eps = 1e-6) const;") == 1
    assert hpp.count("Var rms_norm(const Shape& normalized_shape, double eps = 1e-6) const;") == 1
    assert hpp.count("VarDiff rms_norm(const VarDiff& gamma, double eps = 1e-6) const;") == 2
    assert "VarDiff rms_norm(const Var& gamma, double eps = 1e-6) const;" in hpp
    assert "VarDiff rms_norm(const Shape& normalized_shape, double eps = 1e-6) const;" in hpp
    assert "std::string to_json(const nn::RMSNorm& l);" in hpp and "nn::RMSNorm rms_norm_from_json(" in hpp
    cpp = _read("host", "neuronika.cpp")
    for node in ("struct RmsNormFwd : Forward", "struct RmsNormBwd : Backward"):
        assert cpp.count(node) == 1, node
    bwd = cpp[cpp.index("struct RmsNormBwd"):]
    bwd = bwd[:bwd.index("\n};")]
    for call in ENTRIES[1:]:
        assert call in bwd, call
    assert bwd.count("borrow_first_write(") == 2                                       # each gradient through its own first-writer state


def test_kernels_sit_beside_the_layernorm_family():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import list_unit_kernels as luk
    mine = {k for k in luk.source_kernels("nk_norm.hip") if k.startswith("rms_norm_")}
    assert mine == {"rms_norm_fwd_kernel", "rms_norm_bwd_kernel", "rms_norm_fwd_general_kernel", "rms_norm_bwd_general_kernel",
                    "rms_norm_gamma_partial_kernel", "rms_norm_gamma_final_kernel"}
    def text(f):
        return re.sub(r"//[^\n]*", "", _read("neuronika_amd", "csrc", f))

    # each family's statements stand once, in a body header that defines no kernel and that both norms' kernels include
    bodies = sorted(f for f in os.listdir(luk.CSRC) if re.fullmatch(r"nk_norm_\w+_body\.h", f))
    assert len(bodies) == 6 and set(bodies) <= set(luk.unit_sources("nk_norm.hip"))
    assert not any(luk.file_kernels(os.path.join(luk.CSRC, f)) for f in bodies)
    src = text("nk_norm.hip")
    norm = src + "".join(text(f) for f in bodies)                  # the norm unit's own code: kernels, bodies and host paths
    assert "atomic" not in norm.lower() and "hipMemset" not in norm and "hipMalloc" not in norm and "Synchronize" not in norm
    assert "nk_workspace(" in norm and "nk_streams_past_cache(" in norm

    def expanded(name):
        """what the compiler sees of one kernel: the body header in place of its #include, `#if NORM_CENTRED` evaluated with the
        value the kernel defines"""
        k = src[src.index("void %s(" % name):]
        k = k[:k.index("\n}\n")]
        (centred,) = re.findall(r"^#define NORM_CENTRED ([01])$", k, re.M)
        (header,) = re.findall(r'^\s*#include "(nk_norm_\w+_body\.h)"$', k, re.M)
        k = k.replace('#include "%s"' % header, text(header))
        out, on = [], [True]
        for line in k.split("\n"):
            word = line.strip()
            if word.startswith("#if"):
                assert word == "#if NORM_CENTRED", word               # the one switch, so that nothing is evaluated wrongly here
                on.append(on[-1] and centred == "1")
            elif word == "#else":
                on[-1] = on[-2] and not on[-1]
            elif word == "#endif":
                on.pop()
            elif on[-1]:
                out.append(line)
        assert on == [True], name
        return "\n".join(out)

    # one reduction forward, one backward, no mean: the row-in-registers kernels and the general ones each call owner_sum once
    for name in ("rms_norm_fwd_kernel", "rms_norm_bwd_kernel", "rms_norm_fwd_general_kernel", "rms_norm_bwd_general_kernel"):
        body = expanded(name)
        assert body.count("owner_sum<") == 1, name
        assert "mean" not in body and "sub4" not in body, name
    # and the switch at 1 selects the centred branch: LayerNorm's dx has the second reduction
    for name in ("layer_norm_bwd_kernel", "layer_norm_bwd_general_kernel"):
        assert expanded(name).count("owner_sum<") == 2, name
    assert not [f for f in os.listdir(luk.CSRC) if f.endswith(".hip") and "rms" in f]   # no new translation unit


def test_rust_mirror_names_the_ffi_calls():
    ffi = open(os.path.join(HIP, "ffi.rs")).read()
    for name in ENTRIES:
        assert re.search(rf"pub fn {name}\(", ffi), name
    node = open(os.path.join(HIP, "node", "rms_norm.rs")).read()
    for name in ("nk_rms_norm_fwd", "nk_rms_norm_bwd", "nk_rms_norm_bwd_gamma"):     # this tape zeroes eagerly: no _assign twins
        assert f"ffi::{name}(" in node, name
    assert re.search(r"^mod rms_norm;", open(os.path.join(HIP, "node", "mod.rs")).read(), re.M)
    hv = open(os.path.join(HIP, "hipvar.rs")).read()
    assert hv.count("pub fn rms_norm<") == 2 and "RmsNormBackward::new(" in hv
    nn = open(os.path.join(ROOT, "integration", "neuronika-nn", "src", "hip.rs")).read()
    assert "pub struct RMSNorm" in nn


def test_the_example_the_benchmark_and_the_docs():
    txt = _read("examples", "generate.py")
    assert '"--rmsnorm"' in txt and "nn.RMSNorm" in txt and "nn.LayerNorm" in txt and '"tests"' not in txt and "oracle" not in txt
    assert os.path.exists(os.path.join(ROOT, "benchmarks", "rms_norm.py")) and "rms_norm.py" in _read("benchmarks", "README.md")
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "RMSNorm" in _read(doc), doc
    assert "Not built: RMSNorm" not in _read("DESIGN.md")

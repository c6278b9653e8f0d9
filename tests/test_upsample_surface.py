"""The surface of the upsampling, layer by layer, without a GPU: the header declares the entry points, the ctypes table has them with
the header's argument counts, the Rust ffi and node name them, the host module exposes the layer and the variable methods, and the
kernels live in one header that nk_pool.hip alone includes, once, and that neither uses atomics nor allocates, synchronises or takes
the streaming switch."""
import ctypes as C
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nk_upsample_out_size", "nk_upsample_fwd", "nk_upsample_bwd", "nk_upsample_bwd_assign")
HIP = os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip")
CSRC = os.path.join(ROOT, "neuronika_amd", "csrc")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _header_arity():
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", _read("include", "neuronika_hip.h"), flags=re.S))
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"int (nk_upsample\w*)\(([^)]*)\);", flat)}, flat


def test_header_declares_the_entry_points():
    arity, flat = _header_arity()
    assert tuple(arity) == ENTRIES
    assert "enum { NK_UPSAMPLE_NEAREST = 0, NK_UPSAMPLE_LINEAR = 1 };" in flat
    assert "int nk_upsample_out_size(int nd, const int* x_shape, const double* scale, int* out_size);" in flat
    assert ("int nk_upsample_fwd(nk_device* dev, int nd, int mode, int align_corners, const float* x, const int* x_shape, float* y, "
            "const int* out_size);") in flat
    for name in ENTRIES[2:]:
        assert ("int %s(nk_device* dev, int nd, int mode, int align_corners, float* dx, const int* x_shape, const float* g, "
                "const int* out_size);" % name) in flat
    doc = _read("include", "neuronika_hip.h")
    for phrase in ("src(o) = min((o * in) / out, in - 1)", "i0 = min((int)floorf(src), in - 1);  i1 = min(i0 + 1, in - 1);  l1 = src - (float)i0;  l0 = 1 - l1",
                   "out_i = floor(in_i * scale_i) in f64", "w = l_w; w = l_h * w;", "ascending row-major order", "No atomics", "captured into a graph",
                   "nearest x2", "every operation rounded on its own"):
        assert phrase in doc, phrase


def test_ctypes_table_has_the_headers_argument_counts():
    from neuronika_amd import capi
    arity, _ = _header_arity()
    VP, IP = C.c_void_p, C.POINTER(C.c_int)
    for name in ENTRIES:
        assert name in capi.EXPORTED and hasattr(capi.lib, name), name
        assert len(capi._SIGS[name]) == arity[name], name
    assert capi._SIGS["nk_upsample_out_size"] == [C.c_int, IP, C.POINTER(C.c_double), IP]
    for name in ENTRIES[1:]:
        assert capi._SIGS[name] == [VP, C.c_int, C.c_int, C.c_int, VP, IP, VP, IP], name
    for wrapper, keys in (("upsample_out_size", ("x_shape", "scale")), ("upsample_fwd", ("x", "x_shape", "y", "out_size", "mode", "align_corners")),
                          ("upsample_bwd", ("dx", "x_shape", "g", "out_size", "mode", "align_corners", "assign"))):
        params = inspect.signature(getattr(capi, wrapper)).parameters
        assert all(k in params for k in keys), (wrapper, list(params))
    assert (capi.UPSAMPLE_NEAREST, capi.UPSAMPLE_LINEAR) == (0, 1)
    # the host-only entry needs no device
    assert capi.upsample_out_size((1, 2, 6, 8), 1.5) == (9, 12) and capi.upsample_out_size((1, 2, 6, 8), (2, 2.5)) == (12, 20)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        try:
            capi.upsample_out_size((1, 2, 6, 8), bad)
        except capi.NeuronikaHipError as e:
            assert e.code == 1
        else:
            raise AssertionError("scale %r was accepted" % bad)
    # a null device is refused before anything else happens
    assert capi.lib.nk_upsample_fwd(None, 2, 0, 0, None, None, None, None) == 1


def test_rust_mirror_names_the_ffi_calls():
    ffi = open(os.path.join(HIP, "ffi.rs")).read()
    for name in ENTRIES:
        assert re.search(rf"pub fn {name}\(", ffi), name
    node = open(os.path.join(HIP, "node", "upsample.rs")).read()
    for name in ("nk_upsample_fwd", "nk_upsample_bwd"):                                   # that tape zeroes eagerly: no _assign twin
        assert f"ffi::{name}(" in node, name
    assert re.search(r"^mod upsample;", open(os.path.join(HIP, "node", "mod.rs")).read(), re.M)
    hv = open(os.path.join(HIP, "hipvar.rs")).read()
    assert hv.count("pub fn upsample(") == 2 and "Upsample::new(" in hv and "UpsampleBackward::new(" in hv
    nn = open(os.path.join(ROOT, "integration", "neuronika-nn", "src", "hip.rs")).read()
    assert "pub struct Upsample" in nn and "input.upsample(" in nn


def test_host_module_exposes_the_layer_and_the_methods():
    import neuronika_amd
    t = neuronika_amd.tape
    for cls in (t.Var, t.VarDiff):
        doc = cls.upsample.__doc__
        assert "out_size" in doc and "mode: str = 'nearest'" in doc and "align_corners: bool = False" in doc, doc
    for member in ("size", "scale_factor", "mode", "align_corners", "output_size", "forward"):
        assert hasattr(t.nn.Upsample, member), member
    init = t.nn.Upsample.__init__.__doc__
    assert re.search(r"size: .* = None, scale_factor: .* = None, mode: str = 'nearest', align_corners: bool = False\) -> None", init), init
    layer = t.nn.Upsample(scale_factor=1.5, mode="bilinear", align_corners=True)
    assert (list(layer.size), list(layer.scale_factor), layer.mode, layer.align_corners) == ([], [1.5], "bilinear", True)
    assert list(layer.output_size([1, 2, 6, 8])) == [9, 12]
    assert list(t.nn.Upsample(size=[5, 7]).output_size([1, 2, 6, 8])) == [5, 7]
    for kw in ({"size": [8, 8], "scale_factor": 2.0}, {}, {"scale_factor": 2.0, "mode": "bicubic"}, {"scale_factor": 2.0, "align_corners": True}):
        try:
            t.nn.Upsample(**kw)
        except RuntimeError:
            pass
        else:
            raise AssertionError("Upsample(%r) was accepted" % kw)
    assert not hasattr(t.serde, "upsample_from_json")                                    # no parameters, no serde state
    cpp = _read("host", "neuronika.cpp")
    for node in ("struct UpsampleFwd : Forward", "struct UpsampleBwd : Backward"):
        assert cpp.count(node) == 1, node
    bwd = cpp[cpp.index("struct UpsampleBwd"):]
    bwd = bwd[:bwd.index("\n};")]
    assert "nk_upsample_bwd_assign" in bwd and "nk_upsample_bwd)" in bwd and bwd.count("borrow_first_write(") == 1


def _stripped(path):
    txt = open(path).read()
    return re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", txt), flags=re.S)


def test_the_kernel_header_is_included_once_by_the_pooling_unit_alone():
    includers = {}
    for f in sorted(os.listdir(CSRC)):
        n = len(re.findall(r'^\s*#\s*include\s+"nk_upsample\.h"', open(os.path.join(CSRC, f)).read(), re.M))
        if n:
            includers[f] = n
    assert includers == {"nk_pool.hip": 1}
    src = open(os.path.join(CSRC, "nk_pool.hip")).read()
    at = src.index('#include "nk_upsample.h"')
    for helper in ("bool pool_al16(", "int pool_grid("):                                  # behind the helpers it uses
        assert 0 <= src.index(helper) < at, helper
    raw = open(os.path.join(CSRC, "nk_upsample.h")).read()
    assert "nk_streams_past_cache" not in raw                                             # not even in a comment: the ledger counts call sites
    assert "unmeasured" in raw and "`nt`" in raw                                          # and says why
    code = _stripped(os.path.join(CSRC, "nk_upsample.h"))
    for word in ("atomic", "Atomic", "hipMalloc", "Synchronize", "nk_workspace", "num_cus", "tune_", "nk_store_stream", "nk_load_stream", "__syncthreads"):
        assert word not in code, word
    assert code.count("UpAxis upsample_axis(") == 1                                       # ONE index function, called by forward and backward
    fwd = code[code.index("void upsample_fwd_kernel("):code.index("void upsample_readers(")]
    bwd = code[code.index("void upsample_readers("):code.index("void upsample_nearest2_fwd_kernel(")]
    assert "upsample_axis(" in fwd and "upsample_axis(" in bwd
    assert not re.search(r"\bfmaf?\s*\(|__fmaf_rn", code) and code.count("#pragma clang fp contract(off)") == 3


def test_the_kernels_are_in_the_built_library():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import list_unit_kernels as luk
    declared = luk.file_kernels(os.path.join(CSRC, "nk_upsample.h"))
    assert declared == {"upsample_fwd_kernel", "upsample_bwd_kernel", "upsample_nearest2_fwd_kernel", "upsample_nearest2_bwd_kernel"}
    others = set()
    for f in os.listdir(CSRC):
        if f != "nk_upsample.h" and f.endswith((".h", ".hip")):
            others |= luk.file_kernels(os.path.join(CSRC, f))
    assert not declared & others                                                          # unique across csrc
    assert "nk_upsample.h" in luk.unit_sources("nk_pool.hip")
    kernels = luk.unit_kernels(("nk_pool.hip",))["nk_pool.hip"]
    built = {re.sub(r"<.*$", "", k) for k in kernels}
    assert declared <= built, sorted(declared - built)
    assert {"pool_generic_fwd_kernel", "pool_win_fwd_kernel", "pool_plane_fwd_kernel"} <= built   # the same code object as the pooling family
    # nearest has no per-axis arithmetic (one instantiation per width); linear one per number of axes
    for k in ("upsample_fwd_kernel", "upsample_bwd_kernel"):
        assert {i for i in kernels if i.startswith(k + "<")} == {"%s<%d, %d, %d>" % (k, nd, mode, vec) for nd, mode in ((3, 0), (1, 1), (2, 1), (3, 1))
                                                                 for vec in (1, 4)}, k


def test_the_benchmark_and_the_docs():
    assert os.path.exists(os.path.join(ROOT, "benchmarks", "upsample.py")) and "upsample.py" in _read("benchmarks", "README.md")
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "Upsample" in _read(doc), doc
    assert "nn::Upsample" in _read("README.md")
    design = _read("DESIGN.md")
    assert "nk_upsample.h" in design and "nearest x2" in design and "row-major" in design

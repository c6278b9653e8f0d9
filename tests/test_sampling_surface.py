"""The surface of token sampling, layer by layer, without a GPU: the header declares the two entry points and fixes the semantics, the
ctypes table and the built library have them, the host classes exist with the documented members, the kernels live in their own header
outside the inventoried units, the Rust mirror names the ffi call, and the example and the benchmark are there."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nk_sample_fwd", "nk_sample_stage_limit")
HIP = os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points():
    doc = _read("include", "neuronika_hip.h")
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", doc, flags=re.S))
    assert ("int nk_sample_fwd(nk_device* dev, const float* logits, long long ld, int rows, int V, float* ids, float temperature, int top_k, "
            "float top_p, uint64_t seed, uint64_t offset);") in flat
    assert "int nk_sample_stage_limit(void);" in flat
    for phrase in ("0x53414D50", "2^40", "mulhi64", "lowest index", "Ties", "NK_ERR_INVALID", "-0 counts as +0", "NaN sorts below -inf",
                   "c = 1.44269504f / temperature", "(uint64)((double)top_p * (double)W)", "r64 = word1 << 32 | word0", "refuses", "never written"):
        assert phrase in doc, phrase


def test_ctypes_table_and_library_export_them():
    from neuronika_amd import capi
    for name in ENTRIES:
        assert name in capi.EXPORTED and hasattr(capi.lib, name), name
    assert len(capi._SIGS["nk_sample_fwd"]) == 11 and len(capi._SIGS["nk_sample_stage_limit"]) == 0
    params = inspect.signature(capi.sample_fwd).parameters
    assert list(params) == ["dev", "logits", "ld", "rows", "V", "ids", "temperature", "top_k", "top_p", "seed", "offset"]
    assert [params[k].default for k in ("temperature", "top_k", "top_p", "seed", "offset")] == [1.0, 0, 1.0, 0, 0]
    L = capi.sample_stage_limit()                                        # a pure function: no device needed
    assert isinstance(L, int) and 1024 <= L <= 160 * 1024 // 4


def test_host_classes_exist():
    import neuronika_amd
    t = neuronika_amd.tape
    for member in ("temperature", "top_k", "top_p", "seed", "offset", "forward"):
        assert hasattr(t.nn.Sampler, member), member
    for member in ("temperature", "top_k", "top_p", "seed", "offset"):
        assert isinstance(getattr(t.nn.Sampler, member), property) and getattr(t.nn.Sampler, member).fset is not None, member
    assert re.search(r"__init__\(self: .*, dev: .*, temperature: .* = 1.0, top_k: .* = 0, top_p: .* = 1.0, seed: .* = 0\)",
                     t.nn.Sampler.__init__.__doc__)
    fwd = t.nn.Sampler.forward.__doc__
    assert re.search(r"forward\(self: [\w.]*Sampler, logits: [\w.]*Var, batch: .*\) -> [\w.]*Var\n", fwd)
    assert re.search(r"forward\(self: [\w.]*Sampler, logits: [\w.]*VarDiff, batch: .*\) -> [\w.]*Var\n", fwd)
    assert re.search(r"sample\(self: [\w.]*Var, sampler: [\w.]*Sampler, batch: .*\) -> [\w.]*Var\n", t.Var.sample.__doc__)
    hpp = _read("host", "neuronika.hpp")
    assert "Sampler(DevicePtr dev, float temperature = 1.0f, int top_k = 0, float top_p = 1.0f, uint64_t seed = 0);" in hpp
    assert "Var forward(const Var& logits, int batch) const;" in hpp
    assert "Var sample(const nn::Sampler& sampler, int batch) const;" in hpp
    cpp = _read("host", "neuronika.cpp")
    assert "struct SampleFwd : Forward" in cpp
    node = cpp[cpp.index("struct SampleFwd : Forward"):]
    node = node[:node.index("\n};")]
    assert "nk_sample_fwd(" in node and node.index("nk_sample_fwd(") < node.index("++(*offset)")     # a refused call consumes nothing
    assert "struct SampleBwd" not in cpp                                 # ids are data: no gradient


def test_kernels_live_in_their_own_header_outside_the_inventoried_units():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dispatch_paths
    import dispatch_paths_mfma
    import list_unit_kernels as luk
    header = os.path.join(luk.CSRC, "nk_sampling.h")
    mine = luk.file_kernels(header)
    assert mine == {"sample_row_kernel"}
    includers = [u for u in luk.all_units() if "nk_sampling.h" in luk.unit_sources(u)]
    assert len(includers) == 1 and includers[0] in [u for u, _ in dispatch_paths_mfma.NOT_INVENTORIED]
    assert open(os.path.join(luk.CSRC, "nk_norm.hip")).read().count('#include "nk_sampling.h"') == 1
    for u in dispatch_paths.UNITS + dispatch_paths_mfma.UNITS:
        assert not (mine & luk.source_kernels(u)), u
    for f in os.listdir(luk.CSRC):                                      # the kernel's name occurs nowhere else in csrc/
        if f != "nk_sampling.h":
            assert "sample_row_kernel" not in open(os.path.join(luk.CSRC, f), errors="replace").read(), f
    whole = open(header).read()
    assert "atomicAdd(float" not in whole and "unsafeAtomicAdd" not in whole and "atomicAdd_system" not in whole
    assert whole.count("exp2f(") == 1                                    # ONE statement of the weight
    src = re.sub(r"//[^\n]*", "", whole)
    assert src.count("atomicAdd(") == 2 and all("&sm.hist[" in line for line in src.splitlines() if "atomicAdd(" in line)   # LDS, integer
    assert "philox4x32_10(" in src and "0x53414D50u" in src and "__umul64hi(" in src
    assert "float4" in src and "__shared__" in src and "hipMalloc" not in src and "nk_workspace" not in src
    assert "nk_refuse_capture" in src


def test_rust_mirror_names_the_ffi_call():
    ffi = open(os.path.join(HIP, "ffi.rs")).read()
    for name in ENTRIES:
        assert re.search(rf"pub fn {name}\(", ffi), name
    node = open(os.path.join(HIP, "node", "sample.rs")).read()
    for name in ENTRIES:
        assert f"ffi::{name}(" in node, name
    assert re.search(r"^mod sample;", open(os.path.join(HIP, "node", "mod.rs")).read(), re.M)
    hv = open(os.path.join(HIP, "hipvar.rs")).read()
    assert hv.count("pub fn sample(") == 1 and "Sample::new(" in hv
    nn = open(os.path.join(ROOT, "integration", "neuronika-nn", "src", "hip.rs")).read()
    assert "pub struct Sampler" in nn and ".sample(" in nn[nn.index("impl Sampler"):nn.index("impl Sampler") + 900]


def test_the_example_the_benchmark_and_the_documents():
    txt = _read("examples", "generate.py")
    for flag in ("--device-sample", "--temperature", "--top-k", "--top-p", "--rope"):
        assert flag in txt, flag
    assert "nn.Sampler" in txt and '"tests"' not in txt and "tests/" not in txt and "oracle" not in txt
    assert "argmax(axis=1)" in txt                                       # the host path is still there
    assert os.path.exists(os.path.join(ROOT, "benchmarks", "sampling.py")) and "`sampling.py`" in _read("benchmarks", "README.md")
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "nk_sample_fwd" in _read(doc) or "nn::Sampler" in _read(doc), doc

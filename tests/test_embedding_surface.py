"""The embedding feature's surface, without a GPU: the three entry points are declared in the header, exported by the built library,
bound in `capi` with the header's argument counts and present in the generated `ffi.rs`; `_tape` exposes the module and the
method; the Rust node file and layer exist; the kernels live in a header of the row-kernel unit and use no float atomics."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"nk_embedding_fwd": 7, "nk_embedding_bwd": 8, "nk_embedding_bwd_assign": 8}
HIP = os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip")


def test_symbols_are_declared_exported_and_bound():
    from neuronika_amd import capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neuronika_hip.h")).read(), flags=re.S)
    ffi = open(os.path.join(HIP, "ffi.rs")).read()
    for name, n in ARITY.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name + " is not declared in the header"
        assert len(m.group(1).split(",")) == n, name
        assert name in capi.EXPORTED and hasattr(capi.lib, name), name
        assert len(getattr(capi.lib, name).argtypes) == n, name
        assert re.search(r"pub fn %s\(" % name, ffi), name + " is not in ffi.rs"
    for fn in ("embedding_fwd", "embedding_bwd"):
        assert callable(getattr(capi, fn)), fn


def test_bad_sizes_are_refused_before_anything_is_launched():
    """argument checks come first: they need no device (a null handle is one more refused argument)"""
    from neuronika_amd import capi
    for args in ((None, None, None, None, 1, (1 << 24) + 1, 4), (None, None, None, None, 1, 0, 4), (None, None, None, None, 1, 8, 0)):
        assert capi.lib.nk_embedding_fwd(*args) == 1                       # NK_ERR_INVALID
        assert capi.lib.nk_embedding_bwd(*args, -1) == 1
        assert capi.lib.nk_embedding_bwd_assign(*args, -1) == 1


def test_tape_exposes_the_module_and_the_method():
    import neuronika_amd
    t = neuronika_amd.tape
    assert hasattr(t.VarDiff, "embedding")
    assert hasattr(t.nn, "Embedding")
    for attr in ("weight", "num_embeddings", "embedding_dim", "padding_idx", "forward"):
        assert hasattr(t.nn.Embedding, attr), attr
    assert hasattr(t.serde, "embedding_from_json")


def test_rust_node_and_layer_exist():
    node = open(os.path.join(HIP, "node", "embedding.rs")).read()
    assert "ffi::nk_embedding_fwd(" in node and "ffi::nk_embedding_bwd(" in node
    assert re.search(r"^mod embedding;", open(os.path.join(HIP, "node", "mod.rs")).read(), re.M)
    hipvar = open(os.path.join(HIP, "hipvar.rs")).read()
    assert "Embedding::new(" in hipvar and "EmbeddingBackward::new(" in hipvar and "pub fn embedding<" in hipvar
    nn = open(os.path.join(ROOT, "integration", "neuronika-nn", "src", "hip.rs")).read()
    assert re.search(r"pub struct Embedding\b", nn) and ".embedding(" in nn


def test_kernels_live_in_a_header_of_the_row_unit_without_float_atomics():
    csrc = os.path.join(ROOT, "neuronika_amd", "csrc")
    assert re.search(r'^#include "nk_embedding.h"', open(os.path.join(csrc, "nk_norm.hip")).read(), re.M)
    assert not os.path.exists(os.path.join(csrc, "nk_embedding.hip"))
    src = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "nk_embedding.h")).read())
    atomics = re.findall(r"\batomic\w*\s*\(([^;]*);", src)
    assert atomics and all(re.match(r"\s*&cnt\[", a) for a in atomics), atomics   # integer counts in LDS only
    assert "unsafeAtomicAdd" not in src and "__hip_atomic" not in src

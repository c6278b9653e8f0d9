"""The static surface of the batch normalisation, without a GPU: the seven entry points in the header, the built library and the
ctypes table; the modules and methods in the tape; the node pair, the methods and the layers in the Rust binding."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nk_batch_norm_fwd", "nk_batch_norm_infer_fwd", "nk_batch_norm_bwd_sums", "nk_batch_norm_bwd", "nk_batch_norm_bwd_assign",
         "nk_batch_norm_bwd_params", "nk_batch_norm_bwd_params_assign"]
ARITY = dict(zip(NAMES, (13, 12, 8, 10, 10, 5, 5)))


def test_header_library_and_ctypes_carry_the_seven_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neuronika_hip.h")).read(), flags=re.S)
    from neuronika_amd import capi
    for name in NAMES:
        m = re.search(r"\bint %s\s*\(\s*nk_device\*([^;]*)\)\s*;" % name, src)
        assert m, name
        assert m.group(1).count(",") + 1 == ARITY[name], name
        assert hasattr(capi.lib, name), name                                       # exported by the built library
        assert name in capi.EXPORTED and len(capi._SIGS[name]) == ARITY[name], name
    assert len(re.findall(r"\bint nk_batch_norm_\w+\s*\(", src)) == 7              # the split does not grow
    for wrapper in ("batch_norm_fwd", "batch_norm_infer_fwd", "batch_norm_bwd_sums", "batch_norm_bwd", "batch_norm_bwd_params"):
        assert callable(getattr(capi, wrapper)), wrapper


def test_kernels_live_in_their_own_translation_unit():
    csrc = os.path.join(ROOT, "neuronika_amd", "csrc")
    src = open(os.path.join(csrc, "nk_batchnorm.hip")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, src, re.M), name
    assert "atomic" not in src.replace("No atomics", "") and "cooperative" not in src
    for other in os.listdir(csrc):
        if other != "nk_batchnorm.hip":
            assert "nk_batch_norm" not in open(os.path.join(csrc, other)).read(), other


def test_tape_has_the_modules_and_the_methods():
    import neuronika_amd
    t = neuronika_amd.tape
    for cls in ("BatchNorm1d", "BatchNorm2d", "BatchNorm3d"):
        assert hasattr(t.nn, cls), cls
        for member in ("weight", "bias", "running_mean", "running_var", "train", "eval", "forward", "eps", "momentum"):
            assert hasattr(getattr(t.nn, cls), member), (cls, member)
    assert hasattr(t.Var, "batch_norm") and hasattr(t.VarDiff, "batch_norm")
    assert hasattr(t.serde, "batch_norm_load_json")


def test_rust_binding_carries_the_node_pair_the_methods_and_the_layers():
    hip = os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip")
    node = open(os.path.join(hip, "node", "normalization.rs")).read()
    for item in ("pub(crate) struct BatchNorm<", "pub(crate) struct BatchNormBackward<", "impl<D: Dimension> Forward for BatchNorm<D>",
                 "impl<D: Dimension> Backward for BatchNormBackward<D>"):
        assert item in node, item
    for call in ("ffi::nk_batch_norm_fwd(", "ffi::nk_batch_norm_infer_fwd(", "ffi::nk_batch_norm_bwd_sums(", "ffi::nk_batch_norm_bwd(",
                 "ffi::nk_batch_norm_bwd_params("):
        assert call in node, call
    var = open(os.path.join(hip, "hipvar.rs")).read()
    assert len(re.findall(r"pub fn batch_norm\(", var)) == 2                         # HipVar and HipVarDiff
    assert "BatchNorm::new(" in var and "BatchNormBackward::new(" in var
    nn = open(os.path.join(ROOT, "integration", "neuronika-nn", "src", "hip.rs")).read()
    macro = nn[nn.index("macro_rules! batch_norm_layer"):]
    assert "pub fn new(" in macro and "pub fn forward" in macro and ".batch_norm(" in macro
    for field in ("weight", "bias", "running_mean", "running_var"):
        assert re.search(r"pub %s:" % field, macro), field
    assert re.findall(r"batch_norm_layer!\((\w+),", nn) == ["BatchNorm1d", "BatchNorm2d", "BatchNorm3d"]
    ffi = open(os.path.join(hip, "ffi.rs")).read()
    for name in NAMES:
        assert "pub fn %s(" % name in ffi, name

"""The cross-entropy feature's surface, without a GPU: the three entry points are declared in the header, exported by the built
library, bound in `capi` with the header's argument counts and present in the generated `ffi.rs`; bad arguments are refused before
anything is launched; `_tape` exposes the methods and the module; the Rust node, methods and layer exist; the kernels live in a
header of the row-kernel unit and use no float atomics."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"nk_cross_entropy_fwd": 10, "nk_cross_entropy_bwd": 11, "nk_cross_entropy_bwd_assign": 11}
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
    for fn in ("cross_entropy_fwd", "cross_entropy_bwd"):
        assert callable(getattr(capi, fn)), fn


def test_the_header_states_the_contract():
    text = " ".join(open(os.path.join(ROOT, "include", "neuronika_hip.h")).read().split())
    for phrase in ("INACTIVE", "ignore_index", "label_smoothing", "NUMBER OF ACTIVE POSITIONS", "torch gives NaN", "No float atomics",
                   "f32::MIN", "bwd_assign"):
        assert phrase in text, phrase


def test_bad_arguments_are_refused_before_anything_is_launched():
    """argument checks come first and need no device: each refusal names its argument (the null handle is the last thing looked at)"""
    from neuronika_amd import capi
    lib = capi.lib
    one = (C.c_float * 8)()
    p = C.cast(one, C.c_void_p)

    def fwd(shape, red=1, ignore=-1, eps=0.0, nd=None, out=p):
        return lib.nk_cross_entropy_fwd(None, p, p, capi.ints(shape), len(shape) if nd is None else nd, red, ignore, eps, p, out)

    def bwd(name, shape, red=1, ignore=-1, eps=0.0, nd=None):
        return getattr(lib, name)(None, p, p, p, p, p, capi.ints(shape), len(shape) if nd is None else nd, red, ignore, eps)

    cases = [(dict(shape=(4,)), "dims"), (dict(shape=(4, 3), nd=99), "dims"), (dict(shape=(4, -3)), "negative extent"),
             (dict(shape=(4, 3), red=7), "unknown reduction"), (dict(shape=(4, 3), eps=1.0), "label_smoothing"),
             (dict(shape=(4, 3), eps=-0.1), "label_smoothing"), (dict(shape=(4, 3), eps=float("nan")), "label_smoothing"),
             (dict(shape=(1 << 20, 3, 1 << 20)), "positions"), (dict(shape=(4, 3)), "null device handle")]
    for kw, word in cases:
        assert fwd(**kw) == 1, kw                                            # NK_ERR_INVALID
        assert word in lib.nk_last_error().decode(), (kw, lib.nk_last_error().decode())
        for name in ("nk_cross_entropy_bwd", "nk_cross_entropy_bwd_assign"):
            assert bwd(name, **kw) == 1, (name, kw)
            assert word in lib.nk_last_error().decode(), (name, kw, lib.nk_last_error().decode())


def test_tape_exposes_the_methods_and_the_module():
    import neuronika_amd
    t = neuronika_amd.tape
    assert hasattr(t.Var, "cross_entropy") and hasattr(t.VarDiff, "cross_entropy")
    assert hasattr(t.nn, "CrossEntropyLoss")
    for attr in ("reduction", "ignore_index", "label_smoothing", "forward"):
        assert hasattr(t.nn.CrossEntropyLoss, attr), attr
    crit = t.nn.CrossEntropyLoss(t.Reduction.Sum, 3, 0.1)
    assert (crit.reduction, crit.ignore_index, crit.label_smoothing) == (t.Reduction.Sum, 3, 0.1)
    assert t.nn.CrossEntropyLoss().ignore_index == -1 and t.nn.CrossEntropyLoss().reduction == t.Reduction.Mean
    for bad in (1.0, -0.5, float("nan")):
        try:
            t.nn.CrossEntropyLoss(t.Reduction.Mean, -1, bad)
        except Exception as e:
            assert "label_smoothing" in str(e)
        else:
            raise AssertionError("label_smoothing %r was accepted" % bad)


def test_rust_node_methods_and_layer_exist():
    node = open(os.path.join(HIP, "node", "cross_entropy.rs")).read()
    assert "ffi::nk_cross_entropy_fwd(" in node and "ffi::nk_cross_entropy_bwd(" in node
    assert re.search(r"^mod cross_entropy;", open(os.path.join(HIP, "node", "mod.rs")).read(), re.M)
    hipvar = open(os.path.join(HIP, "hipvar.rs")).read()
    assert "CrossEntropy::new(" in hipvar and "CrossEntropyBackward::new(" in hipvar
    assert len(re.findall(r"pub fn cross_entropy\(", hipvar)) == 2                  # HipVar and HipVarDiff
    nn = open(os.path.join(ROOT, "integration", "neuronika-nn", "src", "hip.rs")).read()
    assert re.search(r"pub struct CrossEntropyLoss\b", nn) and ".cross_entropy(" in nn


def test_kernels_live_in_a_header_of_the_row_unit_without_float_atomics():
    csrc = os.path.join(ROOT, "neuronika_amd", "csrc")
    assert re.search(r'^#include "nk_cross_entropy.h"', open(os.path.join(csrc, "nk_norm.hip")).read(), re.M)
    assert not os.path.exists(os.path.join(csrc, "nk_cross_entropy.hip"))
    src = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "nk_cross_entropy.h")).read())
    assert len(re.findall(r"__global__", src)) >= 8
    assert not re.search(r"atomic", src, re.I)                                      # no atomic of any kind
    # the id read is the NLL one, restated identically
    body = lambda s: re.sub(r"\s+", " ", re.sub(r"//[^\n]*", "", s[s.index("rust_f32_as_usize(float t)"):].split("}", 1)[0]))
    assert body(open(os.path.join(csrc, "nk_cross_entropy.h")).read()) == body(open(os.path.join(csrc, "nk_loss.hip")).read())

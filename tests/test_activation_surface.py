"""The activation feature's surface, without a GPU: the six entry points are declared in the header, exported by the built library,
bound in `capi` with the header's argument counts and present in the generated `ffi.rs`; bad arguments are refused before anything is
launched; `_tape` exposes the methods, the enum and the modules; the Rust nodes, methods and layers exist; the kernels live in a header
of the row-kernel unit and use no atomics."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"nk_activation_fwd": 5, "nk_activation_bwd": 6, "nk_activation_bwd_assign": 6, "nk_glu_fwd": 6, "nk_glu_bwd": 7,
         "nk_glu_bwd_assign": 7}
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
    for fn in ("activation_fwd", "activation_bwd", "glu_fwd", "glu_bwd"):
        assert callable(getattr(capi, fn)), fn
    assert capi.ACTIVATION == {"gelu": 0, "gelu_tanh": 1, "silu": 2, "sigmoid": 3}
    m = re.search(r"enum nk_activation \{([^}]*)\}", header)
    assert m and re.sub(r"\s+", "", m.group(1)) == "NK_ACT_GELU=0,NK_ACT_GELU_TANH=1,NK_ACT_SILU=2,NK_ACT_SIGMOID=3"


def test_the_header_states_the_contract():
    text = " ".join(open(os.path.join(ROOT, "include", "neuronika_hip.h")).read().replace("\n *", " ").split())
    for phrase in ("0.5 erfc(-x / sqrt 2)", "0.044715", 'approximate="none"', 'approximate="tanh"', "keeps the INPUT", "A NaN stays in its own element",
                   "are finite", "F.glu", "GeGLU", "SwiGLU", "16-byte aligned", "launch nothing", "No atomics"):
        assert phrase in text, phrase


def test_bad_arguments_are_refused_before_anything_is_launched():
    """argument checks come first and need no device: each refusal names its argument (the null handle is the last thing looked at)"""
    from neuronika_amd import capi
    lib = capi.lib
    raw = (C.c_float * 16)()
    base = C.addressof(raw)
    p = C.c_void_p(base + (-base) % 16)                                          # a 16-byte aligned host address: nothing reads it
    off = C.c_void_p(p.value + 4)

    def refused(rc, word, what):
        assert rc == 1, (what, rc)                                               # NK_ERR_INVALID
        assert word in lib.nk_last_error().decode(), (what, word, lib.nk_last_error().decode())

    def every(act=0, x=p, y=p, g=p, n=8, rows=2, H=4):
        """the six entries with one argument set; y doubles as dx"""
        yield "nk_activation_fwd", lib.nk_activation_fwd(None, act, x, y, n)
        yield "nk_activation_bwd", lib.nk_activation_bwd(None, act, y, g, x, n)
        yield "nk_activation_bwd_assign", lib.nk_activation_bwd_assign(None, act, y, g, x, n)
        yield "nk_glu_fwd", lib.nk_glu_fwd(None, act, x, y, rows, H)
        yield "nk_glu_bwd", lib.nk_glu_bwd(None, act, y, g, x, rows, H)
        yield "nk_glu_bwd_assign", lib.nk_glu_bwd_assign(None, act, y, g, x, rows, H)

    cases = [(dict(act=-1), "unknown activation"), (dict(act=4), "unknown activation"),
             (dict(x=None), "x is a null pointer"), (dict(y=None), "is a null pointer"), (dict(x=off), "x is not 16-byte aligned"),
             (dict(y=off), "is not 16-byte aligned"), (dict(), "null device handle")]
    for kw, word in cases:
        for name, rc in every(**kw):
            refused(rc, word, (name, kw))
    for name, rc in every(g=None):
        if "bwd" in name:
            refused(rc, "g is a null pointer", name)
    for name, rc in every(g=off):
        if "bwd" in name:
            refused(rc, "g is not 16-byte aligned", name)
    for kw, word in [(dict(H=0), "H must be positive"), (dict(H=-8), "H must be positive"), (dict(rows=-1), "rows must not be negative"),
                     (dict(rows=1 << 40, H=1024), "index type"), (dict(rows=1 << 28, H=4), "index type"),
                     (dict(rows=(1 << 28) - 1, H=4), "null device handle")]:
        for name, rc in every(**kw):
            if "glu" in name:
                refused(rc, word, (name, kw))
    # empty calls are valid, so with a null handle they get as far as the handle
    for name, rc in every(n=0, rows=0, x=None, y=None, g=None):
        refused(rc, "null device handle", name)


def test_tape_exposes_the_methods_the_enum_and_the_modules():
    import neuronika_amd
    t = neuronika_amd.tape
    for cls in (t.Var, t.VarDiff):
        for method in ("gelu", "silu", "glu"):
            assert hasattr(cls, method), (cls, method)
    assert [int(getattr(t.Activation, n)) for n in ("Gelu", "GeluTanh", "Silu", "Sigmoid")] == [0, 1, 2, 3]
    for name in ("GELU", "SiLU", "GLU"):
        assert hasattr(t.nn, name) and hasattr(getattr(t.nn, name), "forward"), name
    assert t.nn.GELU().approximate_tanh is False and t.nn.GELU(True).approximate_tanh is True
    assert t.nn.GELU(approximate_tanh=True).approximate_tanh is True
    assert t.nn.GLU().gate == t.Activation.Sigmoid and t.nn.GLU(t.Activation.Silu).gate == t.Activation.Silu
    t.nn.SiLU()


def test_rust_nodes_methods_and_layers_exist():
    node = open(os.path.join(HIP, "node", "activation.rs")).read()
    for call in ("ffi::nk_activation_fwd(", "ffi::nk_activation_bwd(", "ffi::nk_glu_fwd(", "ffi::nk_glu_bwd("):
        assert call in node, call
    for struct in ("Activation", "ActivationBackward", "Glu", "GluBackward"):
        assert re.search(r"pub\(crate\) struct %s\b" % struct, node), struct
    assert re.search(r"^mod activation;", open(os.path.join(HIP, "node", "mod.rs")).read(), re.M)
    hipvar = open(os.path.join(HIP, "hipvar.rs")).read()
    for new in ("Activation::new(", "ActivationBackward::new(", "Glu::new(", "GluBackward::new("):
        assert new in hipvar, new
    for method in ("gelu", "gelu_tanh", "silu", "glu"):
        assert len(re.findall(r"pub fn %s\(" % method, hipvar)) == 2, method          # HipVar and HipVarDiff
    nn = open(os.path.join(ROOT, "integration", "neuronika-nn", "src", "hip.rs")).read()
    for layer, call in (("GELU", ".gelu()"), ("SiLU", ".silu()"), ("GLU", ".glu(")):
        assert re.search(r"pub struct %s\b" % layer, nn) and call in nn, layer


def test_kernels_live_in_a_header_of_the_row_unit_without_atomics():
    csrc = os.path.join(ROOT, "neuronika_amd", "csrc")
    assert re.search(r'^#include "nk_activation.h"', open(os.path.join(csrc, "nk_norm.hip")).read(), re.M)
    assert not os.path.exists(os.path.join(csrc, "nk_activation.hip"))
    whole = open(os.path.join(csrc, "nk_activation.h")).read()
    assert not re.search(r"atomic", whole, re.I)                                     # no atomic of any kind, comments included
    src = re.sub(r"//[^\n]*", "", whole)
    assert len(re.findall(r"__global__", src)) == 6
    for helper in ("nk_span_walk", "nk_load_stream", "nk_store_stream"):
        assert helper in src, helper
    assert "__shared__" not in src
    # the activation is a template parameter of every kernel
    assert len(re.findall(r"template <int ACT(?:, bool ASSIGN)?>\s*__global__", src)) == 6

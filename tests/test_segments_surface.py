"""The surface of packed sequences in the fused core (nk_attention_seg_*), without a GPU: the four entry points in the header, in the
ctypes table, in the Rust declarations and exported by the built library; the refusals a null device allows; where the kernels live;
and what `_tape` exposes (`nn.Segments`, the `forward` overload, the trailing `segments` of `heads_attention`)."""
import ctypes
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nk_attention_seg_fwd", "nk_attention_seg_bwd", "nk_attention_qkv_seg_fwd", "nk_attention_qkv_seg_bwd")
PAIRS = (("nk_attention_seg_fwd", "nk_attention_band_fwd"), ("nk_attention_seg_bwd", "nk_attention_band_bwd"),
         ("nk_attention_qkv_seg_fwd", "nk_attention_qkv_band_fwd"), ("nk_attention_qkv_seg_bwd", "nk_attention_qkv_band_bwd"))


def capi():
    from neuronika_amd import capi as c
    return c


def _from_band(args, lo_after, lo, span):
    """The band entry point's list turned into the seg one's: `lo` behind `lo_after`, `span` behind dh, no trailing window."""
    args = list(args[:-1])
    args.insert(args.index(lo_after) + 1, lo)
    args.insert(args.index("int dh") + 1, span)
    return args


def test_header_declares_the_entry_points():
    doc = open(os.path.join(ROOT, "include", "neuronika_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", doc, flags=re.S))
    args = lambda n: [a.strip() for a in re.search(r"int %s\(([^)]*)\);" % n, flat).group(1).split(",")]
    for seg, band in PAIRS:
        after = "const float* QKV" if "qkv" in seg else "const float* V"
        assert args(seg) == _from_band(args(band), after, "const int* lo", "int span"), seg
        assert args(band)[-1] == "int window"
    # no geometry functions of its own: the band's serve with window = span
    assert not re.search(r"nk_attention_seg_(ld|scratch|mask_words)", doc)
    comment = re.search(r"/\* Packed sequences.*?\*/", doc, flags=re.S).group(0)
    for word in ("nk_attention_band_scratch(S, span)", "nk_attention_band_ld(S, span)", "nk_attention_band_mask_words(S, span)", "PRECONDITION",
                 "memory-safe", "Bit contracts"):
        assert word in comment, word


def test_ctypes_table_and_library_export_them():
    c = capi()
    for name in ENTRIES:
        assert name in c.EXPORTED and hasattr(c.lib, name), name
    VP, I = ctypes.c_void_p, ctypes.c_int
    for seg, band in PAIRS:
        sig = [VP] + list(c._SIGS[band][:-1])                              # one more pointer (`lo`) among the leading pointers
        sig.insert(sig.index(I) + 4, I)                                    # span behind B, S, H, dh; no trailing window
        assert c._SIGS[seg] == sig, seg
    for wrapper in ("attention_seg_fwd", "attention_seg_bwd", "attention_qkv_seg_fwd", "attention_qkv_seg_bwd"):
        params = inspect.signature(getattr(c, wrapper)).parameters
        assert "span" in params and "lo" in params and "window" not in params, wrapper
    # exported by the built library itself, not only bound
    lib = ctypes.CDLL(c.LIB_PATH)
    for name in ENTRIES:
        assert getattr(lib, name) is not None, name


def test_bad_arguments_are_refused_before_a_device_is_touched():
    """A null device handle is the first check of the four entry points: NK_ERR_INVALID without a GPU, nothing written."""
    lib = capi().lib
    buf = np.full(64, 7.0, np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.nk_attention_seg_fwd(None, p, p, p, p, p, p, None, p, 1, 64, 1, 64, 8, 0.125, 0.0, 0, 0, 0) == 1
    assert lib.nk_attention_seg_bwd(None, p, p, p, p, p, p, p, p, p, None, p, p, p, p, 1, 64, 1, 64, 8, 0.125, 0.0, 0, 1, 1, 1) == 1
    assert lib.nk_attention_qkv_seg_fwd(None, p, p, p, p, None, p, 1, 64, 1, 64, 8, 0.125, 0.0, 0, 0, 0) == 1
    assert lib.nk_attention_qkv_seg_bwd(None, p, p, p, p, p, p, p, None, p, p, 1, 64, 1, 64, 8, 0.125, 0.0, 0, 1) == 1
    assert lib.nk_attention_qkv_seg_fwd(None, None, p, p, p, None, p, 1, 64, 1, 64, 8, 0.125, 0.0, 0, 0, 0) == 1
    assert (buf == 7.0).all()


def test_kernels_live_in_their_own_header_outside_the_inventoried_units():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dispatch_paths
    import dispatch_paths_mfma
    import list_unit_kernels as luk
    header = "nk_attention_band.h"   # the packed-sequence form is attention_band_kernel<..., SEG = true>: one kernel, one header
    assert luk.file_kernels(os.path.join(luk.CSRC, header)) == {"attention_band_kernel"}
    assert re.search(r"template <[^>]*\bbool SEG>\s*__global__[^\n]*\battention_band_kernel\(", open(os.path.join(luk.CSRC, header)).read())
    includers = [u for u in luk.all_units() if header in luk.unit_sources(u)]
    assert includers == ["nk_norm.hip"] and includers[0] in [u for u, _ in dispatch_paths_mfma.NOT_INVENTORIED]
    for u in dispatch_paths.UNITS + dispatch_paths_mfma.UNITS:
        assert "attention_band_kernel" not in luk.source_kernels(u), u
    shared = ("nk_attention_core.h", "nk_attention_tile.h")
    for name in shared:
        assert luk.file_kernels(os.path.join(luk.CSRC, name)) == set(), name
    for name in (header,) + shared:
        src = re.sub(r"//[^\n]*", "", open(os.path.join(luk.CSRC, name)).read())
        assert not re.search(r"atomic(Add|Max|Min|CAS|Exch)|__hip_atomic|__atomic_(fetch|load|store)", src)   # (fences only)
        # no host read of `lo`, no allocation, no synchronisation: the node can be captured
        assert not re.search(r"hipMalloc|hipMemset|hipMemcpy|Synchronize|nk_workspace", src), name


def test_tape_exposes_segments_and_the_forward_overload():
    import neuronika_amd
    t = neuronika_amd.tape
    assert inspect.isclass(t.nn.Segments)
    assert re.search(r"doc_lens", t.nn.Segments.__init__.__doc__)
    for field in ("batch", "S", "max_len", "lo", "pos"):
        assert hasattr(t.nn.Segments, field), field
    doc = t.nn.MultiheadAttention.forward.__doc__
    assert re.search(r"forward\(self: [^,]*, x: [^,]*, batch: [^,)]*\) ->", doc)               # the existing form, as it was
    assert re.search(r"forward\(self: [^,]*, x: [^,]*, batch: [^,)]*, segments: [\w.]*Segments\) ->", doc)
    for cls in (t.Var, t.VarDiff):
        doc = cls.heads_attention.__doc__
        assert re.search(r"causal: bool = False, window: [^,)]* = 0\)", doc), cls                # the existing form and its defaults
        assert re.search(r"window: [^,)]*, segments: [\w.]*Segments\)", doc), cls
        assert re.search(r"rope\(self: [^,]*, rotary: [^,]*, batch: [^,]*, heads: [^,)]*\)", cls.rope.__doc__), cls


def test_the_capture_check_of_the_host_layer_is_declared_and_bound():
    """nk_graph_refuse_capture: what nn::Segments calls before its synchronising uploads; a null device is refused without a GPU."""
    c = capi()
    doc = open(os.path.join(ROOT, "include", "neuronika_hip.h")).read()
    assert "int nk_graph_refuse_capture(nk_device* dev, const char* what);" in doc
    assert "nk_graph_refuse_capture" in c.EXPORTED and c.lib.nk_graph_refuse_capture(None, b"x") == 1
    host = open(os.path.join(ROOT, "host", "neuronika.cpp")).read()
    ctor = host[host.index("Segments::Segments("):]
    assert ctor.index("nk_graph_refuse_capture") < ctor.index("std::make_shared<HipArray>") < ctor.index("->upload(")


def test_rust_declarations_are_regenerated():
    ffi = open(os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip", "ffi.rs")).read()
    for name in ENTRIES:
        m = re.search(rf"pub fn {name}\(([^)]*)\)", ffi)
        assert m, name
        assert "lo: *const c_int" in m.group(1) and "span: c_int" in m.group(1) and "window" not in m.group(1), name
    assert re.search(r"pub fn nk_graph_refuse_capture\(", ffi)

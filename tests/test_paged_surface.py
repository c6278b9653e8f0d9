"""The surface of the paged key / value cache, layer by layer, without a GPU: the header declares the four entry points, the ctypes
table and the built library have them, the workspace function is pure and equals the contiguous forms', the kernels live in their
own header that only nk_norm.hip includes, the host classes exist - and `nn::PageTable`, which needs no device, is fuzzed against
the NumPy model of tests/paged_oracle.py."""
import inspect
import os
import re

import numpy as np
import pytest

import paged_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nk_kv_pages_append", "nk_kv_pages_copy", "nk_attention_decode_paged_workspace", "nk_attention_decode_paged_fwd")
HIP = os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip")
PAGED_HEADER = "nk_attention_decode_paged.h"
PAGED_KERNELS = {"kv_pages_append_kernel", "kv_pages_copy_kernel", "adp_partial_kernel", "adpw_partial_kernel", "adp_generic_kernel",
                 "adpw_generic_kernel"}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points():
    doc = _read("include", "neuronika_hip.h")
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", doc, flags=re.S))
    assert ("int nk_kv_pages_append(nk_device* dev, float* Kp, float* Vp, const float* K, const float* V, int ld, const int* start, "
            "const int* table, int max_pages, int B, int T, int H, int dh, int page, int num_pages);") in flat
    assert ("int nk_kv_pages_copy(nk_device* dev, float* Kp, float* Vp, const int* src, const int* dst, int n, int H, int dh, int page, "
            "int num_pages);") in flat
    assert "size_t nk_attention_decode_paged_workspace(int B, int T, int H, int dh, int max_pages, int page, int window);" in flat
    assert ("int nk_attention_decode_paged_fwd(nk_device* dev, const float* Q, int ldq, const float* Kp, const float* Vp, const int* start, "
            "const int* table, int max_pages, float* O, float* workspace, int B, int T, int H, int Hkv, int dh, int page, int num_pages, "
            "int window, float scale);") in flat
    section = doc[doc.index("paged decoding --"):doc.index("int nk_kv_pages_append(")]
    for phrase in ("(num_pages, Hkv, page, dh)", "table[b*max_pages + p / page]", "p % page", "power of two", "2^31 - 1024",
                   "min(start[b] + t + 1, cap_v)", "ring = 0", "one unsigned", "never an access outside the two allocations",
                   "redirected to position n - 1", "never read", "No atomics", "Bit contract", "NaN or 1e30"):
        assert phrase in section, phrase


def test_ctypes_table_and_library_export_them():
    import ctypes
    from neuronika_amd import capi
    for name in ENTRIES:
        assert name in capi.EXPORTED and hasattr(capi.lib, name), name
    assert [len(capi._SIGS[n]) for n in ENTRIES] == [15, 10, 7, 19]
    assert capi.lib.nk_attention_decode_paged_workspace.restype is ctypes.c_size_t
    for wrapper, keys in (("kv_pages_append", ("Kp", "Vp", "K", "V", "ld", "start", "table", "max_pages", "B", "T", "H", "dh", "page", "num_pages")),
                          ("kv_pages_copy", ("Kp", "Vp", "src", "dst", "n", "H", "dh", "page", "num_pages")),
                          ("attention_decode_paged_workspace", ("B", "T", "H", "dh", "max_pages", "page", "window")),
                          ("attention_decode_paged_fwd", ("Q", "ldq", "Kp", "Vp", "start", "table", "max_pages", "out", "workspace", "B", "T", "H",
                                                          "Hkv", "dh", "page", "num_pages", "window", "scale"))):
        params = inspect.signature(getattr(capi, wrapper)).parameters
        assert all(k in params for k in keys), (wrapper, list(params))


def test_the_workspace_is_pure_and_is_the_contiguous_forms():
    from neuronika_amd import capi
    for dh in (32, 64, 128, 20, 5):
        C = capi.attention_decode_chunk(dh)
        for page in (16, 64, C, 2 * C):
            for max_pages in (1, 3, 3 * C // 16 + 1):
                cap = max_pages * page
                for B, T, H in ((1, 1, 1), (3, 4, 8)):
                    assert capi.attention_decode_paged_workspace(B, T, H, dh, max_pages, page, 0) == capi.attention_decode_workspace(B, T, H, dh, cap)
                    for W in (1, page, C - 1, C + 1, 2 * C + 3, 1 << 30):
                        assert (capi.attention_decode_paged_workspace(B, T, H, dh, max_pages, page, W)
                                == capi.attention_decode_window_workspace(B, T, H, dh, W)), (dh, page, max_pages, W)
    for bad in ((0, 1, 1, 64, 4, 16, 0), (1, 1, 1, 64, 0, 16, 0), (1, 1, 1, 64, 4, 8, 0), (1, 1, 1, 64, 4, 48, 0), (1, 1, 1, 64, 4, 16, -1),
                (1, 1, 1, 64, 1 << 27, 16, 0)):
        assert capi.attention_decode_paged_workspace(*bad) == 0, bad


def test_bad_arguments_are_refused_before_a_device_is_touched():
    """A null device handle is the first check of every entry point: NK_ERR_INVALID without a GPU."""
    from neuronika_amd import capi
    assert capi.lib.nk_attention_decode_paged_fwd(None, None, 0, None, None, None, None, 4, None, None, 1, 1, 4, 2, 64, 16, 8, 0, 0.125) == 1
    assert capi.lib.nk_kv_pages_append(None, None, None, None, None, 0, None, None, 4, 1, 1, 1, 64, 16, 8) == 1
    assert capi.lib.nk_kv_pages_copy(None, None, None, None, None, 1, 1, 64, 16, 8) == 1


def test_kernels_live_in_the_new_header_which_only_the_row_unit_includes():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dispatch_paths
    import dispatch_paths_mfma
    import list_unit_kernels as luk
    assert luk.file_kernels(os.path.join(luk.CSRC, PAGED_HEADER)) == PAGED_KERNELS
    includers = [u for u in luk.all_units() if PAGED_HEADER in luk.unit_sources(u)]
    assert includers == ["nk_norm.hip"] and includers[0] in [u for u, _ in dispatch_paths_mfma.NOT_INVENTORIED]
    norm = _read("neuronika_amd", "csrc", "nk_norm.hip")
    assert norm.count('#include "%s"' % PAGED_HEADER) == 1
    assert norm.index('#include "nk_attention_decode.h"') < norm.index('#include "%s"' % PAGED_HEADER)
    assert PAGED_KERNELS <= luk.source_kernels("nk_norm.hip")
    for u in dispatch_paths.UNITS + dispatch_paths_mfma.UNITS:
        assert not (PAGED_KERNELS & luk.source_kernels(u)), u
    assert not [f for f in os.listdir(luk.CSRC) if f.endswith(".hip") and "paged" in f]        # no translation unit of its own
    src = re.sub(r"//[^\n]*", "", _read("neuronika_amd", "csrc", PAGED_HEADER))
    assert "atomic" not in src.lower() and "num_cus" not in src and "tune_" not in src
    assert "hipMalloc" not in src and "Synchronize" not in src
    # the partial and generic kernels are their switches around the existing bodies, with no arithmetic of their own; no new combine
    for kernel, body in (("adp_partial_kernel", "nk_attention_decode_body.h"), ("adpw_partial_kernel", "nk_attention_decode_body.h"),
                         ("adp_generic_kernel", "nk_attention_decode_generic_body.h"), ("adpw_generic_kernel", "nk_attention_decode_generic_body.h")):
        at = src.index(kernel + "(")
        own = src[src.rindex("__global__", 0, at):src.index("\n}\n", at) + 1]
        assert own.count("#include") == 1 and '#include "%s"' % body in own, kernel
        assert "#define ADEC_PAGED 1\n" in own and "#undef ADEC_PAGED\n" in own and "#define ADEC_GROUPED 1\n" in own, kernel
        assert ("#define ADEC_WINDOW %d\n" % kernel.startswith("adpw")) in own, kernel
        assert not re.search(r"\b(for|if|return)\b", own) and "__builtin" not in own, kernel
    assert "combine_body" not in src and "adec_combine_kernel," in src and "adw_combine_kernel," in src
    for inst in ("adp_partial_kernel<DH, 1>", "adp_partial_kernel<DH, ADEC_GQA_HEADS>", "adpw_partial_kernel<DH, 1>",
                 "adpw_partial_kernel<DH, ADEC_GQA_HEADS>", "kv_pages_append_kernel<float4>", "kv_pages_append_kernel<float>",
                 "kv_pages_copy_kernel<float4>", "kv_pages_copy_kernel<float>"):
        assert inst in src, inst
    # the switch is in both bodies, and the contiguous includers set it to 0
    for body in ("nk_attention_decode_body.h", "nk_attention_decode_generic_body.h"):
        assert "#if ADEC_PAGED" in _read("neuronika_amd", "csrc", body), body
    assert _read("neuronika_amd", "csrc", "nk_attention_decode.h").count("#define ADEC_PAGED 0\n") == 6


def test_host_classes_exist():
    import neuronika_amd
    nn = neuronika_amd.tape.nn
    for member in ("lens", "pages", "row", "refcount", "free_pages", "behind", "reserve", "truncate", "release", "fork", "release_behind", "reset"):
        assert hasattr(nn.PageTable, member) and hasattr(nn.PagedKvCache, member), member
    doc = nn.MultiheadAttention.forward_step.__doc__
    assert re.search(r"forward_step\(self: .*, x: [\w.]*Var, seqs: .*, cache: [\w.]*PagedKvCache\) -> [\w.]*Var\n", doc), doc
    assert re.search(r"forward_step\(self: .*, x: [\w.]*Var, batch: .*, cache: [\w.]*\.KvCache\) -> [\w.]*Var\n", doc), doc
    hpp = _read("host", "neuronika.hpp")
    assert "Var forward_step(const Var& x, const std::vector<int>& seqs, PagedKvCache& cache) const;" in hpp
    assert "PageTable(int num_pages, int page, int max_seqs, int max_pages);" in hpp
    assert "PagedKvCache(DevicePtr dev, int num_pages, int page, int kv_heads, int head_dim, int max_seqs, int max_pages);" in hpp
    cpp = _read("host", "neuronika.cpp")
    step = cpp[cpp.index("struct DecodeStepFwd"):]
    step = step[:step.index("\n};")]
    assert step.index("nk_kv_pages_copy(") < step.index("nk_kv_pages_append(") < step.index("nk_attention_decode_paged_fwd(")
    for bad in ((0, 16, 1, 1), (4, 8, 1, 1), (4, 24, 1, 1), (4, 16, 0, 1), (4, 16, 1, 0)):
        with pytest.raises(RuntimeError):
            nn.PageTable(*bad)


def test_rust_mirror_names_the_ffi_calls():
    ffi = open(os.path.join(HIP, "ffi.rs")).read()
    for name in ENTRIES:
        assert re.search(rf"pub fn {name}\(", ffi), name
    assert re.search(r"pub fn nk_attention_decode_paged_workspace\([^)]*\) -> usize;", ffi)
    node = open(os.path.join(HIP, "node", "decode.rs")).read()
    for name in ENTRIES:
        assert f"ffi::{name}(" in node, name
    nn = open(os.path.join(ROOT, "integration", "neuronika-nn", "src", "hip.rs")).read()
    assert "pub struct PageTable" in nn and "pub struct PagedKvCache" in nn and "pub fn forward_step_paged(" in nn


def _state(t):
    n = t.max_seqs
    return (list(t.lens()), [list(t.row(s)) for s in range(n)], [t.refcount(p) for p in range(t.num_pages)], list(t.free_pages()),
            [t.behind(s) for s in range(n)])


def _model_state(m):
    return (list(m.lens), [[int(p) for p in r] for r in m.rows], list(m.ref), sorted(m.free), list(m.behind))


def test_page_table_fuzz_against_the_model():
    """2000 random operations on `nn::PageTable` and on the NumPy model: after each, rows, lengths, reference counts, the free set
    and `behind` are equal; every page is free or referenced exactly refcount times; no page a reserve writes has another owner; a
    refused operation leaves every observable unchanged."""
    import neuronika_amd
    nn = neuronika_amd.tape.nn
    NP, PAGE, NS, MP = 24, 16, 6, 7
    t, m = nn.PageTable(NP, PAGE, NS, MP), PO.PageTableModel(NP, PAGE, NS, MP)
    assert _state(t) == _model_state(m)
    rng = np.random.default_rng(20)
    counts = {"ok": 0, "refused": 0, "copies": 0}
    for step in range(2000):
        op = rng.choice(["reserve", "reserve", "reserve", "truncate", "fork", "release", "release_behind"])
        seq = int(rng.integers(-1, NS + 1))                               # now and then an id out of range
        before = _state(t)
        if op == "reserve":
            k = int(rng.integers(1, 4))
            seqs = [int(s) for s in rng.integers(0, NS, k)] if rng.random() < 0.15 else [int(s) for s in rng.permutation(NS)[:k]]
            if rng.random() < 0.03:
                seqs[0] = seq
            args = (seqs, int(rng.choice([1, 1, 1, 2, 5, 15, 16, 17, 40])))
        elif op == "truncate":
            n = m.lens[seq] if 0 <= seq < NS else 0
            args = (seq, int(rng.integers(-1, n + 2)))
        elif op == "fork":
            args = (seq, int(rng.integers(0, NS)))
        elif op == "release":
            args = (seq,)
        else:
            n = m.lens[seq] if 0 <= seq < NS else 0
            args = (seq, int(rng.integers(-1, n + 2)))
        old_lens = list(m.lens)
        try:
            want = getattr(m, op)(*args)
            refused = False
        except PO.Refused:
            refused = True
        if refused:
            with pytest.raises(RuntimeError):
                getattr(t, op)(*args)
            assert _state(t) == before, (step, op, args)
            counts["refused"] += 1
        else:
            got = getattr(t, op)(*args)
            counts["ok"] += 1
            if op == "reserve":
                assert [tuple(c) for c in got] == want, (step, args)
                counts["copies"] += len(want)
                for s in args[0]:                                         # the pages the new positions land in have one owner
                    for pos in range(old_lens[s], old_lens[s] + args[1]):
                        pg = t.row(s)[pos // PAGE]
                        assert pg >= 0 and t.refcount(pg) == 1, (step, s, pos, pg)
        assert _state(t) == _model_state(m), (step, op, args)
        owners, free = m.owners(), set(t.free_pages())
        for p in range(NP):
            assert t.refcount(p) == owners[p] and (p in free) == (owners[p] == 0), (step, p)
    print("fuzz:", counts)
    assert counts["ok"] > 500 and counts["refused"] > 100 and counts["copies"] > 10, counts   # every kind of outcome was reached
    t.reset()
    m.reset()
    assert _state(t) == _model_state(m) and t.free_pages() == list(range(NP))

"""The surface of the sliding-window fused core (nk_attention_band_*), without a GPU: the three geometry functions against the walk
stated in include/neuronika_hip.h - by brute force over every touched (row, key), for every S and W of a sparse grid of 1 .. 700 that
holds every residue mod 32 and mod 128 - the refusals a null device allows, the ctypes
table, the header, and where the kernels live."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nk_attention_band_fwd", "nk_attention_band_bwd", "nk_attention_qkv_band_fwd", "nk_attention_qkv_band_bwd",
           "nk_attention_band_ld", "nk_attention_band_scratch", "nk_attention_band_mask_words")


def capi():
    from neuronika_amd import capi as c
    return c


def _grid():
    """1 .. 700 sparsely, every residue mod 32 and mod 128 included (129 .. 256 covers both), and the neighbours of the multiples."""
    v = set(range(1, 40)) | set(range(129, 257))
    for m in (256, 384, 512, 640):
        v |= {m - 1, m, m + 1}
    v |= {300, 333, 449, 577, 699, 700}
    v = sorted(x for x in v if 1 <= x <= 700)
    assert {x % 32 for x in v} == set(range(32)) and {x % 128 for x in v} == set(range(128))
    return v


def _walk(S, W):
    """The touched region of the banded tensors as the header states the walk: per block of 128 queries the staged key range (what
    the backward defines), per wave of 32 the computed tile range (what the forward writes).  Returns per row (first, one past
    last) staged column, and the list of computed (row tile, key tile) pairs."""
    SP = (S + 31) // 32 * 32
    ntile, nqb = SP // 32, (S + 127) // 128
    staged, tiles = np.zeros((SP, 2), np.int64), []
    for qb in range(nqb):
        js = max(0, 128 * qb - W + 1) // 128
        k0, k1 = 128 * js, 32 * min(ntile, 4 * qb + 4)
        for w in range(4):
            r0 = 128 * qb + 32 * w
            if r0 >= S:
                continue
            staged[r0:r0 + 32] = (k0, k1)
            for kt in range(max(0, r0 - W + 1) // 32, 4 * qb + w + 1):
                assert 4 * js <= kt < min(ntile, 4 * qb + 4)
                tiles.append((r0 // 32, kt))
    return SP, staged, tiles


GRID = _grid()


def test_row_stride_has_the_stated_value():
    c = capi()
    for S in GRID:
        SP = (S + 31) // 32 * 32
        for W in GRID:
            ld = c.attention_band_ld(S, W)
            assert ld == min(SP, 128 * (-(-(W - 1) // 128) + 1)), (S, W)
            assert ld % 32 == 0 and (ld % 128 == 0 or ld == SP)
            assert c.attention_band_scratch(S, W) == (SP - 1) * ld + SP
            assert c.attention_band_mask_words(S, W) == SP * (ld // 32)
            if W >= S:
                assert ld == SP and c.attention_band_scratch(S, W) == SP * SP, (S, W)      # the causal layout
    for bad in ((0, 5), (5, 0), (-1, 5), (5, -7)):
        assert c.attention_band_ld(*bad) == 0 and c.attention_band_scratch(*bad) == 0 and c.attention_band_mask_words(*bad) == 0
    assert c.lib.nk_attention_band_scratch.restype is ctypes.c_size_t and c.lib.nk_attention_band_mask_words.restype is ctypes.c_size_t
    # O(S W), not O(S^2): 8192 rows of a 256-key window
    assert c.attention_band_scratch(8192, 256) == 8191 * 384 + 8192 < 8192 * 8192 // 20


@pytest.mark.parametrize("S", GRID)
def test_touched_addresses_are_distinct_inside_the_extent_and_aligned(S):
    """Brute force: the address r * ld + k of every staged element is unique and below nk_attention_band_scratch; every 32-wide tile
    row starts on 16 bytes; the mask word of every computed tile is unique and below nk_attention_band_mask_words.  Every S of GRID
    against every W of GRID (both hold every residue mod 32 and mod 128), and W = S, S + 1."""
    c = capi()
    for W in sorted(set(GRID) | {S, S + 1}):
        SP, staged, tiles = _walk(S, W)
        ld, ext, words = c.attention_band_ld(S, W), c.attention_band_scratch(S, W), c.attention_band_mask_words(S, W)
        rows = np.flatnonzero(staged[:, 1] > 0)
        first, last = rows * ld + staged[rows, 0], rows * ld + staged[rows, 1] - 1        # a row's touched addresses are one run
        assert (staged[rows, 1] - staged[rows, 0] <= ld).all(), (S, W)
        assert (first[1:] > last[:-1]).all(), (S, W)                                        # runs of consecutive rows do not meet
        assert first.min() >= 0 and last.max() < ext, (S, W)
        assert (first % 4 == 0).all() and ld % 4 == 0 and ext % 4 == 0                      # 16-byte tile rows, 16-byte head bases
        assert (np.diff(staged[rows, 0]) >= 0).all()                                        # the start never decreases with r
        # the computed tiles lie inside the staged range; their mask words are distinct and inside the extent
        t = np.array(tiles, dtype=np.int64)
        qt, kt = t[:, 0], t[:, 1]
        assert (staged[32 * qt, 0] <= 32 * kt).all() and (32 * kt + 32 <= staged[32 * qt, 1]).all(), (S, W)
        rel = kt - 4 * (np.maximum(0, 128 * (qt // 4) - W + 1) // 128)
        assert (rel >= 0).all() and (rel < ld // 32).all(), (S, W)
        word = (qt * (ld // 32) + rel) * 32
        assert np.unique(word).size == word.size and (word + 32 <= words).all(), (S, W)
        # every (r, k) of the band lies in a computed tile
        tset = set(tiles)
        for r in (0, S // 2, S - 1):
            for k in (max(0, r - W + 1), r):
                assert (r // 32, k // 32) in tset, (S, W, r, k)


def test_bad_arguments_are_refused_before_a_device_is_touched():
    """A null device handle is the first check of the four entry points: NK_ERR_INVALID without a GPU, nothing written."""
    lib = capi().lib
    buf = np.full(64, 7.0, np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.nk_attention_band_fwd(None, p, p, p, p, p, None, p, 1, 64, 1, 64, 0.125, 0.0, 0, 0, 0, 8) == 1
    assert lib.nk_attention_band_bwd(None, p, p, p, p, p, p, p, p, p, None, p, p, p, 1, 64, 1, 64, 0.125, 0.0, 0, 1, 1, 1, 8) == 1
    assert lib.nk_attention_qkv_band_fwd(None, p, p, p, None, p, 1, 64, 1, 64, 0.125, 0.0, 0, 0, 0, 8) == 1
    assert lib.nk_attention_qkv_band_bwd(None, p, p, p, p, p, p, p, None, p, 1, 64, 1, 64, 0.125, 0.0, 0, 1, 8) == 1
    assert lib.nk_attention_qkv_band_fwd(None, None, p, p, None, p, 1, 64, 1, 64, 0.125, 0.0, 0, 0, 0, 8) == 1
    assert (buf == 7.0).all()


def test_ctypes_table_and_library_export_them():
    c = capi()
    for name in ENTRIES:
        assert name in c.EXPORTED and hasattr(c.lib, name), name
    # the causal entry points' lists plus `window`
    for band, causal in (("nk_attention_band_fwd", "nk_attention_causal_fwd"), ("nk_attention_band_bwd", "nk_attention_causal_bwd"),
                         ("nk_attention_qkv_band_fwd", "nk_attention_qkv_causal_fwd"), ("nk_attention_qkv_band_bwd", "nk_attention_qkv_causal_bwd")):
        assert c._SIGS[band] == c._SIGS[causal] + [ctypes.c_int], band
    for wrapper in ("attention_band_fwd", "attention_band_bwd", "attention_qkv_band_fwd", "attention_qkv_band_bwd"):
        assert "window" in inspect.signature(getattr(c, wrapper)).parameters, wrapper


def test_header_declares_the_entry_points():
    doc = open(os.path.join(ROOT, "include", "neuronika_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", doc, flags=re.S))
    for decl in ("int nk_attention_band_ld(int S, int window);", "size_t nk_attention_band_scratch(int S, int window);",
                 "size_t nk_attention_band_mask_words(int S, int window);"):
        assert decl in flat, decl
    for band, causal in (("nk_attention_band_fwd", "nk_attention_causal_fwd"), ("nk_attention_band_bwd", "nk_attention_causal_bwd"),
                         ("nk_attention_qkv_band_fwd", "nk_attention_qkv_causal_fwd"), ("nk_attention_qkv_band_bwd", "nk_attention_qkv_causal_bwd")):
        args = lambda n: re.search(r"int %s\(([^)]*)\);" % n, flat).group(1)
        assert args(band) == args(causal) + ", int window", band


def test_kernels_live_in_their_own_header_outside_the_inventoried_units():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dispatch_paths
    import dispatch_paths_mfma
    import list_unit_kernels as luk
    header = "nk_attention_band.h"
    assert luk.file_kernels(os.path.join(luk.CSRC, header)) == {"attention_band_kernel"}
    includers = [u for u in luk.all_units() if header in luk.unit_sources(u)]
    assert includers == ["nk_norm.hip"] and includers[0] in [u for u, _ in dispatch_paths_mfma.NOT_INVENTORIED]
    for u in dispatch_paths.UNITS + dispatch_paths_mfma.UNITS:
        assert "attention_band_kernel" not in luk.source_kernels(u), u
    # the helpers and the tile body it shares with nk_attention.hip define no kernel
    shared = ("nk_attention_core.h", "nk_attention_tile.h")
    for name in shared:
        assert luk.file_kernels(os.path.join(luk.CSRC, name)) == set(), name
    assert "nk_attention_core.h" in luk.unit_sources("nk_norm.hip") and "nk_attention_core.h" in luk.unit_sources("nk_attention.hip")
    for name in (header,) + shared:
        src = re.sub(r"//[^\n]*", "", open(os.path.join(luk.CSRC, name)).read())
        assert not re.search(r"atomic(Add|Max|Min|CAS|Exch)|__hip_atomic|__atomic_(fetch|load|store)", src), name   # (fences only)
        assert "hipMalloc" not in src and "hipMemset" not in src and "Synchronize" not in src, name


def test_tape_and_rust_take_the_window():
    import neuronika_amd
    t = neuronika_amd.tape
    for cls in (t.Var, t.VarDiff):
        assert re.search(r"causal: bool = False, window: [^,)]* = 0\)", cls.heads_attention.__doc__), cls
    ffi = open(os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip", "ffi.rs")).read()
    for name in ENTRIES:
        assert re.search(rf"pub fn {name}\(", ffi), name

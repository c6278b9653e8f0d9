"""The pooling feature's surface, without a GPU: the seven entry points are declared, exported and bound with the header's argument
counts; `nk_pool_out_shape` (host arithmetic, no device) gives the oracle's shapes and NK_ERR_INVALID for each rule of the
header; `_tape` exposes the methods and the six modules with torch's defaults."""
import ctypes
import os
import re

import pytest

import pooling_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"nk_pool_out_shape": 6, "nk_max_pool_fwd": 9, "nk_max_pool_bwd": 9, "nk_max_pool_bwd_assign": 9, "nk_avg_pool_fwd": 9,
         "nk_avg_pool_bwd": 9, "nk_avg_pool_bwd_assign": 9}


def test_symbols_are_declared_exported_and_bound():
    from neuronika_amd import capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neuronika_hip.h")).read(), flags=re.S)
    for name, n in ARITY.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name + " is not declared in the header"
        assert len(m.group(1).split(",")) == n, name
        assert name in capi.EXPORTED and hasattr(capi.lib, name), name
        assert len(getattr(capi.lib, name).argtypes) == n, name
    for fn in ("pool_out_shape", "max_pool_fwd", "max_pool_bwd", "avg_pool_fwd", "avg_pool_bwd"):
        assert callable(getattr(capi, fn)), fn
    assert issubclass(capi.HipIntArray, capi.HipArray)


GEOMETRIES = [((2, 3, 16), (2,), (2,), (0,)), ((2, 3, 17), (3,), (2,), (1,)), ((1, 2, 9), (4,), (3,), (2,)),
              ((128, 64, 112, 112), (3, 3), (2, 2), (1, 1)), ((128, 512, 7, 7), (7, 7), (7, 7), (0, 0)), ((2, 3, 12, 12), (3, 3), (2, 2), (0, 0)),
              ((1, 3, 13, 10), (5, 4), (3, 2), (2, 2)), ((1, 2, 5, 7, 9), (3, 2, 3), (2, 1, 2), (1, 1, 0)), ((0, 3, 8, 8), (2, 2), (2, 2), (1, 1)),
              ((1, 1, 46340, 46340), (1, 1), (1, 1), (0, 0))]


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_out_shape_matches_the_oracle(geom):
    from neuronika_amd import capi
    assert capi.pool_out_shape(*geom) == P.out_shape(*geom)


REJECTED = {
    "window-0": ((2, 3, 8, 8), (0, 2), (2, 2), (0, 0)),
    "stride-0": ((2, 3, 8, 8), (2, 2), (0, 2), (0, 0)),
    "padding-above-half-the-window": ((2, 3, 8, 8), (2, 2), (2, 2), (2, 0)),
    "padding-negative": ((2, 3, 8, 8), (3, 3), (2, 2), (-1, 0)),
    "window-beyond-the-padded-extent": ((2, 3, 2, 8), (5, 3), (1, 1), (1, 1)),
    "extent-0": ((2, 3, 0, 8), (2, 2), (2, 2), (1, 1)),
    "nd-0": ((2, 3), (), (), ()),
    "nd-4": ((2, 3, 4, 4, 4, 4), (1,) * 4, (1,) * 4, (0,) * 4),
    "negative-N": ((-1, 3, 8), (2,), (2,), (0,)),
    "input-plane-beyond-31-bits": ((1, 1, 65536, 65536), (1, 1), (1, 1), (0, 0)),
}


@pytest.mark.parametrize("name", list(REJECTED))
def test_out_shape_rejects(name):
    from neuronika_amd import capi
    with pytest.raises(ValueError):
        P.out_shape(*REJECTED[name])
    with pytest.raises(capi.NeuronikaHipError) as e:
        capi.pool_out_shape(*REJECTED[name])
    assert e.value.code == 1                                                # NK_ERR_INVALID


def test_out_shape_rejects_null_pointers():
    from neuronika_amd import capi
    three = (ctypes.c_int * 4)(1, 1, 8, 8)
    assert capi.lib.nk_pool_out_shape(2, three, None, three, three, three) == 1
    assert capi.lib.nk_pool_out_shape(2, three, three, three, three, None) == 1


def test_tape_exposes_methods_and_modules():
    import neuronika_amd
    t = neuronika_amd.tape
    for cls in (t.Var, t.VarDiff):
        for method in ("max_pool", "avg_pool", "global_avg_pool", "flatten"):
            assert hasattr(cls, method), (cls.__name__, method)
    for name in ("MaxPool1d", "MaxPool2d", "MaxPool3d", "AvgPool1d", "AvgPool2d", "AvgPool3d"):
        assert hasattr(t.nn, name), name
        assert issubclass(getattr(t.nn, name), t.nn.PoolNd)


def test_module_defaults_are_torchs():
    import neuronika_amd
    nn = neuronika_amd.tape.nn
    m = nn.MaxPool2d([3, 3])
    assert (m.kernel_size, m.stride, m.padding) == ([3, 3], [3, 3], [0, 0])
    m = nn.MaxPool2d([3, 3], [2, 2], [1, 1])
    assert (m.kernel_size, m.stride, m.padding) == ([3, 3], [2, 2], [1, 1])
    m = nn.MaxPool1d(2)
    assert (m.kernel_size, m.stride, m.padding) == ([2], [2], [0])
    m = nn.AvgPool1d(3, 2, 1, False)
    assert (m.kernel_size, m.stride, m.padding, m.count_include_pad) == ([3], [2], [1], False)
    m = nn.AvgPool3d([2, 2, 2])
    assert (m.kernel_size, m.stride, m.padding, m.count_include_pad) == ([2, 2, 2], [2, 2, 2], [0, 0, 0], True)
    assert nn.AvgPool2d([2, 2], count_include_pad=False).count_include_pad is False
    assert nn.MaxPool3d([3, 3, 3], padding=[1, 1, 1]).stride == [3, 3, 3]
    for bad in (lambda: nn.MaxPool2d([3]), lambda: nn.MaxPool2d([3, 3], [2, 2], [2, 2]), lambda: nn.AvgPool1d(0), lambda: nn.MaxPool3d([2, 2, 2], [0, 1, 1])):
        with pytest.raises(RuntimeError):
            bad()

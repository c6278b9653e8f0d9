"""Pins tests/upsample_oracle.py, without a GPU.  Nearest EQUALS torch's F.interpolate(size=...) on the suite's shapes (the integer
index is the definition; where torch's rounded f32 scale gives another index is recorded below and not chased).  Linear, forward and
backward, is held against torch in f64 within a bound derived here.  out == in returns x bit for bit.

The bound.  With u = 2^-24 (f32 unit roundoff) the one inexact step whose error grows with the geometry is the source coordinate:
s = in / out carries a relative error u, s * (o + 0.5) one more, and the subtraction of 0.5 one more, all of a value of at most
in <= m = max(in, out): |d src| <= 3 u m per axis.  l1 = src - i0 is exact, l0 = 1 - l1 adds u / 2.  One axis of the forward is a
piecewise-linear, continuous function of src with slope |b - a| <= 2 max|x| (so an i0 that moves by one when src crosses an integer
changes nothing beyond that slope), evaluated with two products and a sum (3 u max|x| more):
    |y32 - y64| <= u * max|x| * sum over the axes of (6 m_a + 3).
In the backward a corner's weight is a product of one l per axis, each off by at most 3 u m_a + u / 2, with nd - 1 roundings of the
product; a term w * g adds one rounding, and a sum of K terms of magnitude <= max|g| adds at most K u max|g| per term:
    |dx32 - dx64| <= u * max|g| * K * (sum over the axes of (3 m_a + 1) + nd + K),
K = the largest number of (output, corner) contributions to one input element, counted by the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import upsample_oracle as U

TESTS = os.path.dirname(os.path.abspath(__file__))
UNIT = 2.0 ** -24

# torch runs in ONE child process, once for the whole file: a process that has loaded the HIP library must not import torch as well
# (a second HIP runtime in one address space aborts at exit; the suite's other torch users are child processes for the same reason).
# It prints one JSON object: per shape the nearest comparison and the linear errors, and the (in, out) pairs on which torch's nearest
# index is not the integer form.
_TORCH_REPORT = r"""
import json
import sys
import numpy as np
import torch
import torch.nn.functional as TF
sys.path.insert(0, sys.argv[1])
import upsample_oracle as U
def data(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
out = {"nearest": [], "linear": [], "differ": [], "unread": None}
for shape, size in U.SHAPES:
    x, g = data(shape, 1), data(shape[:2] + tuple(size), 2)
    gi = np.round(4 * g).astype(np.float32)                      # integer-valued: the f32 sums of the backward are exact
    y64, dx64 = U.torch64(x, size, "nearest", g=gi)
    y, dx = U.forward(x, size, "nearest"), U.backward(gi, shape, "nearest")
    out["nearest"].append({"shape": list(shape), "size": list(size), "y_dtype": str(y.dtype), "y_shape": list(y.shape),
                           "y_equal": bool(np.array_equal(y, y64.astype(np.float32))), "dx_equal": bool(np.array_equal(dx, dx64.astype(np.float32)))})
    for align in (False, True):
        x, g = data(shape, 3), data(shape[:2] + tuple(size), 4)
        y64, dx64 = U.torch64(x, size, "linear", align, g=g)
        y, dx = U.forward(x, size, "linear", align), U.backward(g, shape, "linear", align)
        out["linear"].append({"shape": list(shape), "size": list(size), "align": align, "dtypes": [str(y.dtype), str(dx.dtype)],
                              "err_y": float(np.abs(y - y64).max()), "err_dx": float(np.abs(dx - dx64).max()),
                              "max_x": float(np.abs(x).max()), "max_g": float(np.abs(g).max()), "K": U.readers(shape, size, "linear", align)})
for n_in in range(1, 65):
    x = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in)
    for n_out in range(1, 130):
        theirs = TF.interpolate(x, size=(n_out,), mode="nearest").reshape(-1).numpy().astype(np.int64)
        if not np.array_equal(theirs, U.nearest_index(n_in, n_out)):
            out["differ"].append([n_in, n_out])
shape, size = (1, 1, 7, 8), (3, 4)                               # downsampling: the elements no output reads
g = np.ones((1, 1) + size, np.float32)
_, dx64 = U.torch64(np.zeros(shape), size, "linear", False, g=g)
dx = U.backward(g, shape, "linear", False)
out["unread"] = {"some": bool((dx == 0).any()), "same_zeros": bool(np.array_equal(dx == 0, dx64 == 0))}
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def torch_report():
    r = subprocess.run([sys.executable, "-c", _TORCH_REPORT, TESTS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _data(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


@pytest.mark.parametrize("at", range(len(U.SHAPES)), ids=lambda i: "x".join(map(str, U.SHAPES[i][0])))
def test_nearest_equals_torch_exactly(torch_report, at):
    shape, size = U.SHAPES[at]
    rec = torch_report["nearest"][at]
    assert (tuple(rec["shape"]), tuple(rec["size"])) == (shape, size)
    assert rec["y_dtype"] == "float32" and tuple(rec["y_shape"]) == shape[:2] + tuple(size)
    assert rec["y_equal"] and rec["dx_equal"]                               # the backward routes the same way (integer-valued g)


def test_where_torchs_f32_scale_leaves_the_integer_form(torch_report):
    differ = [tuple(p) for p in torch_report["differ"]]
    print("nearest: %d of %d (in, out) pairs differ from torch's f32 scale" % (len(differ), 64 * 129))
    assert (2, 82) in differ and (14, 46) in differ                         # the two the header names
    assert all(n_out % n_in or n_out // n_in >= 41 for n_in, n_out in differ)   # never an integer factor below 41 (2 -> 82 is one of 41)
    assert not any((s[2 + a], o[a]) in differ for s, o in U.SHAPES for a in range(len(o)))   # none of the suite's axes


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("at", range(len(U.SHAPES)), ids=lambda i: "x".join(map(str, U.SHAPES[i][0])))
def test_linear_is_within_the_derived_bound_of_torch_in_f64(torch_report, at, align):
    shape, size = U.SHAPES[at]
    nd = len(size)
    rec = torch_report["linear"][2 * at + int(align)]
    assert (tuple(rec["shape"]), tuple(rec["size"]), rec["align"]) == (shape, size, align)
    assert rec["dtypes"] == ["float32", "float32"]
    m = [max(shape[2 + a], size[a]) for a in range(nd)]
    K = rec["K"]
    bound_y = UNIT * rec["max_x"] * sum(6 * ma + 3 for ma in m)
    bound_dx = UNIT * rec["max_g"] * K * (sum(3 * ma + 1 for ma in m) + nd + K)
    print("linear %s -> %s align=%d: y %.1f u max|x| (bound %.0f), dx %.1f u max|g| (bound %.0f), K = %d" % (
        shape, size, align, rec["err_y"] / (UNIT * rec["max_x"]), bound_y / (UNIT * rec["max_x"]), rec["err_dx"] / (UNIT * rec["max_g"]),
        bound_dx / (UNIT * rec["max_g"]), K))
    assert rec["err_y"] <= bound_y, (rec["err_y"], bound_y)
    assert rec["err_dx"] <= bound_dx, (rec["err_dx"], bound_dx)


@pytest.mark.parametrize("shape", [(2, 3, 5), (2, 3, 4, 6), (1, 2, 3, 4, 5), (1, 1, 1, 1)])
def test_out_equal_to_in_returns_x_bit_for_bit(shape):
    x = _data(shape, 5)
    for mode, align in U.variants():
        assert U.forward(x, shape[2:], mode, align).tobytes() == x.tobytes(), (mode, align)
        g = _data(shape, 6)
        assert U.backward(g, shape, mode, align).tobytes() == g.tobytes(), (mode, align)


def test_out_size_is_floor_of_the_f64_product():
    assert U.out_size((1, 2, 6, 8), 1.5) == (9, 12)
    assert U.out_size((1, 2, 6, 8), (2, 2.5)) == (12, 20)
    assert U.out_size((1, 2, 7), 0.5) == (3,)


def test_downsampling_leaves_unread_elements_at_zero(torch_report):
    assert torch_report["unread"]["some"] and torch_report["unread"]["same_zeros"]

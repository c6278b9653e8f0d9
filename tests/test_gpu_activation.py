"""nk_activation_* and nk_glu_* through the C ABI (`capi`) against tests/activation_oracle.py (f64) within the project's elementwise
tolerance (tests/tolerance.py: |got - ref| <= ELEMENTWISE_ATOL + ELEMENTWISE_RTOL |ref|), with |g| <= 1 and destinations in [-1, 1].
Every device array sits between guard bands that must come back intact; every check prints its worst error / bound before it asserts."""
import ctypes as C

import numpy as np
import pytest

import activation_oracle as A
from test_gpu_embedding import Guarded, same_bits
from tolerance import ELEMENTWISE_ATOL, ELEMENTWISE_RTOL

pytestmark = pytest.mark.gpu

NS = (1, 3, 4, 5, 1023, 257 * 129, 2 ** 20 + 3)
ROWS = (1, 7, 513)
HS = (1, 3, 4, 5, 64, 100, 1024, 11008)


def within(got, ref, what):
    """finite where the oracle is finite, NaN exactly where the oracle is NaN, and inside the elementwise tolerance of |ref|"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert (np.isnan(got) == nan).all(), (what, "NaN pattern", np.flatnonzero(np.isnan(got) != nan)[:8])
    ok = ~nan
    assert np.isfinite(got[ok]).all(), (what, "not finite")
    ratio = np.abs(got[ok] - ref[ok]) / (ELEMENTWISE_ATOL + ELEMENTWISE_RTOL * np.abs(ref[ok]))
    worst = float(ratio.max()) if ratio.size else 0.0
    print("%-44s worst error / bound %.4f" % (what, worst))
    assert worst <= 1.0, (what, worst, int(ratio.argmax()), got[ok][ratio.argmax()], ref[ok][ratio.argmax()])


def run_activation(dev, act, x, g, dx0):
    """forward, `+=` onto dx0, `+=` onto zeros, assign onto NaN-filled memory; guard bands checked on every array"""
    from neuronika_amd import capi as c
    n = x.size
    XS, G = Guarded(dev, x), Guarded(dev, g)
    Y = Guarded(dev, np.full(n, np.nan, np.float32))
    DX, DZ, DA = Guarded(dev, dx0), Guarded(dev, np.zeros(n, np.float32)), Guarded(dev, np.full(n, np.nan, np.float32))
    c.activation_fwd(dev, act, XS.body, Y.body, n)
    c.activation_bwd(dev, act, DX.body, G.body, XS.body, n)
    c.activation_bwd(dev, act, DZ.body, G.body, XS.body, n)
    c.activation_bwd(dev, act, DA.body, G.body, XS.body, n, assign=True)
    for a in (XS, G):
        a.numpy()  # inputs: guards only
    return Y.numpy(), DX.numpy(), DZ.numpy(), DA.numpy()


def run_glu(dev, act, x, g, dx0, rows, H):
    from neuronika_amd import capi as c
    XS, G = Guarded(dev, x), Guarded(dev, g)
    Y = Guarded(dev, np.full(rows * H, np.nan, np.float32))
    DX, DZ = Guarded(dev, dx0), Guarded(dev, np.zeros(rows * 2 * H, np.float32))
    DA = Guarded(dev, np.full(rows * 2 * H, np.nan, np.float32))
    c.glu_fwd(dev, act, XS.body, Y.body, rows, H)
    c.glu_bwd(dev, act, DX.body, G.body, XS.body, rows, H)
    c.glu_bwd(dev, act, DZ.body, G.body, XS.body, rows, H)
    c.glu_bwd(dev, act, DA.body, G.body, XS.body, rows, H, assign=True)
    for a in (XS, G):
        a.numpy()
    return Y.numpy(), DX.numpy(), DZ.numpy(), DA.numpy()


def check_activation(dev, act, x, seed=0):
    rng = np.random.default_rng(seed)
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    g, dx0 = rng.uniform(-1, 1, x.size).astype(np.float32), rng.uniform(-1, 1, x.size).astype(np.float32)
    y, dx, dz, da = run_activation(dev, act, x, g, dx0)
    v, d = A.value_and_derivative(act, x)
    tag = "%s n=%d" % (act, x.size)
    within(y, v, tag + " forward")
    within(dx, dx0.astype(np.float64) + g.astype(np.float64) * d, tag + " backward +=")
    within(da, g.astype(np.float64) * d, tag + " backward assign")
    same_bits(da, dz, tag + ": assign on NaN-filled memory against += on zeros")
    return y, dx, da


def check_glu(dev, act, x, rows, H, seed=0):
    rng = np.random.default_rng(seed)
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    g, dx0 = rng.uniform(-1, 1, rows * H).astype(np.float32), rng.uniform(-1, 1, rows * 2 * H).astype(np.float32)
    y, dx, dz, da = run_glu(dev, act, x, g, dx0, rows, H)
    x2, g2 = x.astype(np.float64).reshape(rows, 2 * H), g.astype(np.float64).reshape(rows, H)
    v, d = A.value_and_derivative(act, x2[:, H:])
    grad = np.concatenate([g2 * v, g2 * x2[:, :H] * d], axis=1).reshape(-1)
    tag = "glu(%s) rows=%d H=%d" % (act, rows, H)
    within(y, (x2[:, :H] * v).reshape(-1), tag + " forward")
    within(dx, dx0.astype(np.float64) + grad, tag + " backward +=")
    within(da, grad, tag + " backward assign")
    same_bits(da, dz, tag + ": assign on NaN-filled memory against += on zeros")
    return y, dx, da


@pytest.mark.parametrize("act", A.ACTIVATIONS)
@pytest.mark.parametrize("n", NS)
def test_activation(dev, act, n):
    check_activation(dev, act, np.random.default_rng(n).uniform(-6, 6, n), seed=n + 1)


@pytest.mark.parametrize("act", A.ACTIVATIONS)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("H", HS)
def test_glu(dev, act, rows, H):
    check_glu(dev, act, np.random.default_rng(rows * 131 + H).uniform(-6, 6, rows * 2 * H), rows, H, seed=H + 1)


@pytest.mark.parametrize("act", A.ACTIVATIONS)
def test_extreme_inputs_stay_finite_and_within_tolerance(dev, act):
    """+-{1e-30 .. 3e38} and +-0: every output and every gradient finite (`within` asserts it) and inside the tolerance"""
    check_activation(dev, act, A.EXTREME)
    rng = np.random.default_rng(5)
    for H in (13, 52):                                       # the scalar and the 16-byte kernels; the gate takes the extremes
        rows = 2 * A.EXTREME.size // H if H == 52 else 4
        b = np.resize(A.EXTREME, rows * H).reshape(rows, H)
        a = rng.uniform(-1, 1, (rows, H)).astype(np.float32)
        check_glu(dev, act, np.concatenate([a, b], axis=1), rows, H)


@pytest.mark.parametrize("act", A.ACTIVATIONS)
def test_nan_poisons_its_own_element_only(dev, act):
    """`within` compares the NaN pattern with the oracle's: a NaN input is NaN in its own output and gradient element; in the gated
    form a NaN `a` reaches y[r, j] and dx[r, H + j], a NaN `b` reaches y[r, j] and both dx[r, j] and dx[r, H + j] - nothing else"""
    x = np.random.default_rng(0).uniform(-3, 3, 1031).astype(np.float32)
    x[[0, 5, 514, 1027, 1030]] = np.nan
    y, dx, da = check_activation(dev, act, x)
    assert np.flatnonzero(np.isnan(y)).tolist() == [0, 5, 514, 1027, 1030] == np.flatnonzero(np.isnan(da)).tolist()
    for rows, H in ((5, 8), (5, 7)):
        x = np.random.default_rng(1).uniform(-3, 3, (rows, 2 * H)).astype(np.float32)
        x[1, 2] = np.nan                                     # an `a`
        x[3, H + 4] = np.nan                                 # a `b`
        y, dx, da = check_glu(dev, act, x, rows, H)
        assert np.argwhere(np.isnan(y.reshape(rows, H))).tolist() == [[1, 2], [3, 4]]
        assert np.argwhere(np.isnan(da.reshape(rows, 2 * H))).tolist() == [[1, H + 2], [3, 4], [3, H + 4]]
        assert np.argwhere(np.isnan(dx.reshape(rows, 2 * H))).tolist() == [[1, H + 2], [3, 4], [3, H + 4]]


def test_two_runs_give_identical_bits(dev):
    rng = np.random.default_rng(9)
    for act in A.ACTIVATIONS:
        x = rng.uniform(-6, 6, 70001).astype(np.float32)
        g, dx0 = rng.uniform(-1, 1, x.size).astype(np.float32), rng.uniform(-1, 1, x.size).astype(np.float32)
        for got, again in zip(run_activation(dev, act, x, g, dx0), run_activation(dev, act, x, g, dx0)):
            same_bits(got, again, act)
        for rows, H in ((33, 260), (33, 261)):
            x = rng.uniform(-6, 6, rows * 2 * H).astype(np.float32)
            g, dx0 = rng.uniform(-1, 1, rows * H).astype(np.float32), rng.uniform(-1, 1, x.size).astype(np.float32)
            for got, again in zip(run_glu(dev, act, x, g, dx0, rows, H), run_glu(dev, act, x, g, dx0, rows, H)):
                same_bits(got, again, "glu " + act)


def test_bad_arguments_are_refused_with_a_live_device(dev):
    from neuronika_amd import capi as c
    lib = c.lib
    buf = dev.zeros(64)
    p, off, null = buf.p, buf.view_offset(1).p, None

    def refused(rc, word):
        assert rc == 1, (rc, word)                           # NK_ERR_INVALID
        assert word in lib.nk_last_error().decode(), (word, lib.nk_last_error().decode())

    for act in (-1, 4, 99):
        refused(lib.nk_activation_fwd(dev.h, act, p, p, 8), "unknown activation")
        refused(lib.nk_glu_fwd(dev.h, act, p, p, 2, 4), "unknown activation")
        for name in ("nk_activation_bwd", "nk_activation_bwd_assign"):
            refused(getattr(lib, name)(dev.h, act, p, p, p, 8), "unknown activation")
        for name in ("nk_glu_bwd", "nk_glu_bwd_assign"):
            refused(getattr(lib, name)(dev.h, act, p, p, p, 2, 4), "unknown activation")
    for bad, word in ((null, "null pointer"), (off, "not 16-byte aligned")):
        for args in ((bad, p), (p, bad)):
            refused(lib.nk_activation_fwd(dev.h, 0, *args, 8), word)
            refused(lib.nk_glu_fwd(dev.h, 0, *args, 2, 4), word)
        for args in ((bad, p, p), (p, bad, p), (p, p, bad)):
            for name in ("nk_activation_bwd", "nk_activation_bwd_assign"):
                refused(getattr(lib, name)(dev.h, 0, *args, 8), word)
            for name in ("nk_glu_bwd", "nk_glu_bwd_assign"):
                refused(getattr(lib, name)(dev.h, 0, *args, 2, 4), word)
    for rows, H, word in ((2, 0, "H must be positive"), (2, -4, "H must be positive"), (-1, 4, "rows must not be negative"),
                          (1 << 40, 1024, "index type"), (1 << 28, 4, "index type")):
        refused(lib.nk_glu_fwd(dev.h, 3, p, p, rows, H), word)
        for name in ("nk_glu_bwd", "nk_glu_bwd_assign"):
            refused(getattr(lib, name)(dev.h, 3, p, p, p, rows, H), word)
    same_bits(buf.numpy(), np.zeros(64, np.float32), "a refused call wrote")


def test_empty_inputs_succeed(dev):
    from neuronika_amd import capi as c
    lib = c.lib
    buf = dev.array(np.full(16, 7.0, np.float32))
    for act in range(4):
        for p in (buf.p, None):
            assert lib.nk_activation_fwd(dev.h, act, p, p, 0) == 0
            assert lib.nk_activation_bwd(dev.h, act, p, p, p, 0) == 0
            assert lib.nk_activation_bwd_assign(dev.h, act, p, p, p, 0) == 0
            assert lib.nk_glu_fwd(dev.h, act, p, p, 0, 4) == 0
            assert lib.nk_glu_bwd(dev.h, act, p, p, p, 0, 4) == 0
            assert lib.nk_glu_bwd_assign(dev.h, act, p, p, p, 0, 5) == 0
    same_bits(buf.numpy(), np.full(16, 7.0, np.float32), "an empty call wrote")

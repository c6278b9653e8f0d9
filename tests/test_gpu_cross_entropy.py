"""nk_cross_entropy_* through the C ABI (`capi`) against tests/cross_entropy_oracle.py (f64) within the oracle's derived bounds, over
the kernel families the header documents (row-in-registers by V, one block per row by width, generic), each entered at aligned and
misaligned row starts.  Every device array sits between guard bands that must come back intact."""
import itertools

import numpy as np
import pytest

import cross_entropy_oracle as X
from cross_entropy_rows import family, ownership
from test_gpu_embedding import Guarded, same_bits

pytestmark = pytest.mark.gpu


def run_all(dev, x, t, red, ignore=-1, eps=0.0, g=1.0, dx0=None, lead=4, lead_dx=None):
    """forward, `+=` backward onto dx0, assign backward onto NaN-filled memory; guard bands checked on every array"""
    from neuronika_amd import capi as c
    lead_dx = lead if lead_dx is None else lead_dx
    XS, T, G = Guarded(dev, x, lead), Guarded(dev, t, 4), Guarded(dev, np.array([g], np.float32), 4)
    LSE, OUT = Guarded(dev, np.full(t.shape, np.nan, np.float32), 4), Guarded(dev, np.full(1, np.nan, np.float32), 4)
    DX = Guarded(dev, dx0 if dx0 is not None else np.zeros(x.shape, np.float32), lead_dx)
    DA = Guarded(dev, np.full(x.shape, np.nan, np.float32), lead_dx)
    c.cross_entropy_fwd(dev, XS.body, T.body, LSE.body, OUT.body, x.shape, red, ignore, eps)
    c.cross_entropy_bwd(dev, DX.body, G.body, XS.body, T.body, LSE.body, x.shape, red, ignore, eps)
    c.cross_entropy_bwd(dev, DA.body, G.body, XS.body, T.body, LSE.body, x.shape, red, ignore, eps, assign=True)
    for a in (XS, T, G):
        a.numpy()  # inputs: guards only
    return float(OUT.numpy()[0]), LSE.numpy(), DX.numpy(), DA.numpy()


def check_case(dev, x, t, red, ignore=-1, eps=0.0, g=0.75, lead=4, lead_dx=None, seed=0):
    dx0 = np.random.default_rng(seed).standard_normal(x.shape).astype(np.float32)
    out, lse, dx, da = run_all(dev, x, t, red, ignore, eps, g, dx0, lead, lead_dx)
    C = x.shape[1]
    want_loss, want_lse = X.forward(x, t, red, ignore, eps)
    _, on = X.active_mask(t, C, ignore)
    count = int(on.sum())
    w = (1.0 / count if count else 0.0) if red == "mean" else 1.0
    finite = np.abs(x[np.isfinite(x)])
    b = X.bounds(C, float(finite.max()) if finite.size else 0.0, t.size, eps, g, w)
    assert np.abs(lse - want_lse).max() <= b["lse"], ("lse", np.abs(lse - want_lse).max(), b["lse"])
    assert abs(out - want_loss) <= b["loss"] * (max(count, 1) if red == "sum" else 1), ("loss", out, want_loss)
    want = X.backward(x, t, want_lse, g, red, ignore, eps)
    assert np.abs(da - want).max() <= b["dx"], ("assign", np.abs(da - want).max(), b["dx"])
    acc = dx0.astype(np.float64) + want
    assert (np.abs(dx - acc) <= b["dx"] + 2 * X.U * np.abs(acc)).all(), "+="
    rows_off = np.broadcast_to(~on.reshape((x.shape[0], 1) + x.shape[2:]), x.shape)
    assert not da[rows_off].any(), "an inactive position's gradient row must be written as zeros"
    same_bits(dx[rows_off], dx0[rows_off], "+= must not touch an inactive position's row")
    return out, lse, dx, da


def make(seed, shape, spread=3.0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * spread).astype(np.float32)
    t = rng.integers(0, shape[1], (shape[0],) + tuple(shape[2:])).astype(np.float32)
    return x, t


def _grid():
    for C in (1, 2, 3, 10, 255, 256, 257, 1000, 2048, 2049, 4099, 32000, 50257):
        for N in (1, 3, 64, 257):
            if N == 257 and C > 4099:
                continue
            yield C, N, 1
    for C, N, inner in itertools.product((1, 2, 3, 10, 255, 256, 257, 1000), (1, 3, 64), (7, 64)):
        yield C, N, inner
    yield 2049, 3, 7
    yield 4099, 3, 64


@pytest.mark.parametrize("C,N,inner", list(_grid()))
def test_grid(dev, C, N, inner):
    """both reductions, smoothing 0 / 0.1, ignore_index hit and not hit; the base pointers on and off a 16-byte boundary"""
    shape = (N, C) if inner == 1 else (N, C, inner)
    x, t = make(C * 131 + N * 7 + inner, shape)
    if C > 1:
        t.reshape(-1)[::3] = 1.0                        # ignore_index = 1 is hit
    for i, (red, eps, ignore) in enumerate(itertools.product(("sum", "mean"), (0.0, 0.1), (-1, 1))):
        check_case(dev, x, t, red, ignore, eps, lead=4 + i % 4, seed=i)


def test_ids_that_are_nan_negative_fractional_or_beyond_the_classes(dev):
    for shape in ((12, 10), (12, 2500), (2, 10, 6)):
        x, _ = make(3, shape)
        t = np.array([np.nan, -4.0, 2.75, 9.99, 10.0, 1e30, np.inf, -np.inf, 0.0, -0.0, 3.0, 16777216.0], np.float32)
        t = t.reshape((shape[0],) + shape[2:]) if len(shape) == 3 else t
        C = shape[1]
        ids, on = X.active_mask(t, C)
        assert ids.reshape(-1)[:4].tolist() == [0, 0, 2, 9]
        assert on.reshape(-1).tolist() == [True] * 4 + [C > 10] + [False] * 2 + [True] * 4 + [False]
        for red in ("sum", "mean"):
            check_case(dev, x, t, red)
            check_case(dev, x, t, red, ignore=0, eps=0.1)


def test_all_positions_inactive(dev):
    for shape in ((9, 10), (5, 3000), (2, 10, 5)):
        x, t = make(4, shape)
        t[...] = 4.0
        for red in ("sum", "mean"):
            out, lse, dx, da = check_case(dev, x, t, red, ignore=4)
            assert out == 0.0 and not da.any() and np.isfinite(lse).all()      # Mean over nothing: 0, not NaN
        t[...] = 1e9
        assert check_case(dev, x, t, "mean")[0] == 0.0


def test_empty_calls(dev):
    from neuronika_amd import capi as c
    OUT, G = Guarded(dev, np.full(1, np.nan, np.float32)), Guarded(dev, np.ones(1, np.float32))
    for shape in ((0, 10), (4, 0), (3, 5, 0)):
        OUT.whole.upload(np.concatenate([np.full(4, 37.25, np.float32), [np.nan], np.full(8, 37.25, np.float32)]))
        c.cross_entropy_fwd(dev, None, None, None, OUT.body, shape, "mean")
        assert OUT.numpy()[0] == 0.0
        c.cross_entropy_bwd(dev, None, G.body, None, None, None, shape, "mean")
        c.cross_entropy_bwd(dev, None, G.body, None, None, None, shape, "sum", assign=True)
    dev.sync()


def test_two_runs_are_bit_identical(dev):
    for shape, ignore in (((257, 1000), 1), ((33, 50257), -1), ((64, 4099), 7), ((3, 100, 64), 2)):
        x, t = make(8, shape)
        runs = [run_all(dev, x, t, "mean", ignore, 0.1, 0.5, dx0=np.ones(shape, np.float32), lead=5) for _ in range(2)]
        assert runs[0][0] == runs[1][0] or (np.isnan(runs[0][0]) and np.isnan(runs[1][0]))
        for a, b, what in zip(runs[0][1:], runs[1][1:], ("lse", "+=", "assign")):
            same_bits(a, b, what)


def test_assign_equals_accumulating_onto_zeros(dev):
    for shape in ((65, 1000), (9, 50257), (3, 17, 9)):
        x, t = make(9, shape)
        _, _, dx, da = run_all(dev, x, t, "mean", 1, 0.1, 0.5, dx0=np.zeros(shape, np.float32), lead=7)
        same_bits(dx, da, shape)


FAMILY_SHAPES = [(8, 1), (300, 1), (601, 1), (1100, 1), (2048, 1), (2049, 1), (9001, 1), (16384, 1), (16385, 1), (20000, 1), (65536, 1),
                 (65537, 1), (70001, 1), (12, 5)]


def test_every_kernel_family_at_aligned_and_misaligned_row_starts(dev):
    """C % 4 == 0 with an aligned base: every row aligned; the same with the base 1 .. 3 floats off, or C odd: rows start at every
    offset.  Shapes are chosen against the thresholds the header documents; the rule restated in `family` says which kernel ran."""
    seen = set()
    for C, inner in FAMILY_SHAPES:
        shape = (5, C) if inner == 1 else (5, C, inner)
        x, t = make(C, shape)
        for lead in (4, 5, 6, 7):
            check_case(dev, x, t, "mean", ignore=2, eps=0.1, lead=lead)
            seen.add(family(C, inner))
    assert seen == {"row1", "row2", "row4", "row8", "block256", "block512", "block1024", "generic"}
    # x and dx at different offsets from a 16-byte boundary: the backward takes the generic kernels, the forward does not care
    for C in (300, 9001):
        x, t = make(C + 1, (5, C))
        assert family(C, 1, together=False) == "generic"
        check_case(dev, x, t, "sum", lead=4, lead_dx=5)
        check_case(dev, x, t, "mean", ignore=2, eps=0.1, lead=6, lead_dx=4)


def composed(dev, x, t, red, g):
    """the device's own log_softmax + nll (+ the memset the fused loss spares)"""
    from neuronika_amd import capi as c
    XS, T, Y, OUT, G = dev.array(x), dev.array(t), dev.zeros(x.shape), dev.zeros(1), dev.array(np.array([g], np.float32))
    c.log_softmax_fwd(dev, XS, Y, 1)
    c.nll_fwd(dev, Y, T, OUT, red)
    GY, DX = dev.zeros(x.shape), dev.zeros(x.shape)
    c.nll_bwd(dev, GY, G, T, red)
    c.log_softmax_bwd(dev, DX, GY, Y, 1, assign=True)
    return OUT.item(), DX.numpy()


@pytest.mark.parametrize("shape", [(6, 10), (5, 3000), (5, 4099), (3, 16385)])
def test_non_finite_logits_follow_the_composed_device_path(dev, shape):
    """-inf is ordinary; a NaN or +inf logit gives the NaN pattern of log_softmax + nll on this library.  At C = 4099 and 16385 the
    block kernels run their four-quad trip (C = 3000: nb = 750 < 3 * 256, the partial trip alone): there each row's first non-finite
    value sits in slot u = 3 of a full trip (cross_entropy_rows.ownership)."""
    x, t = make(6, shape)
    N, C = shape

    def at(r, c):
        own = ownership(family(C, 1), C, (r * C) % 4)
        slot3 = np.flatnonzero(own.full & (own.u == 3))
        return int(slot3[slot3.size // 2 + c]) if slot3.size else c

    c0 = at(0, 2)
    x[0, c0] = -np.inf; x[1, at(1, 3)] = np.nan; x[2, at(2, 0)] = np.inf
    if N > 3:
        x[3, 1] = -np.inf; x[3, 7] = -np.inf
    t[:min(N, 4)] = [1.0, 0.0, 2.0, 5.0][:min(N, 4)]
    out, lse, _, da = run_all(dev, x, t, "sum", g=1.0)
    cout, cdx = composed(dev, x, t, "sum", 1.0)
    assert np.isnan(out) and np.isnan(cout)
    assert np.isnan(lse[1]) and np.isnan(lse[2]) and np.isfinite(np.delete(lse, [1, 2])).all()
    assert np.array_equal(np.isnan(da), np.isnan(cdx)) and np.array_equal(np.isinf(da), np.isinf(cdx))
    assert np.isnan(da[1]).all() and np.isnan(da[2]).all() and da[0, c0] == 0.0
    rest = np.delete(np.arange(shape[0]), [1, 2])
    b = X.bounds(shape[1], 20.0, shape[0])
    assert np.abs(da[rest] - cdx[rest]).max() <= 2 * b["dx"]
    x[1, at(1, 3)] = 0.0; x[2, at(2, 0)] = 0.0                     # with only -inf left everything is finite
    out, lse, _, da = run_all(dev, x, t, "sum", g=0.75)
    want_loss, want_lse = X.forward(x, t, "sum")
    b = X.bounds(shape[1], float(np.abs(x[np.isfinite(x)]).max()), shape[0], 0.0, 0.75)
    assert np.isfinite(out) and abs(out - want_loss) <= b["loss"] * shape[0]
    assert np.isfinite(lse).all() and np.abs(lse - want_lse).max() <= b["lse"]
    assert np.isfinite(da).all() and np.abs(da - X.backward(x, t, want_lse, 0.75, "sum")).max() <= b["dx"]


@pytest.mark.parametrize("shape,red", [((64, 10), "mean"), ((64, 1000), "sum"), ((33, 2049), "mean"), ((16, 50257), "mean"), ((16, 50257), "sum"),
                                       ((4, 100, 8, 8), "sum"), ((3, 7, 5), "sum")])
def test_fused_against_the_composed_device_path(dev, shape, red):
    """Sum for any shape, Mean for 2-d inputs with every position active: the two agree by definition.  The fused result is within
    the bound of the composed one and no further from the f64 oracle than the composed path is (up to an eighth of the bound)."""
    x, t = make(10, shape)
    g = 0.5
    out, _, _, da = run_all(dev, x, t, red, g=g)
    cout, cdx = composed(dev, x, t, red, g)
    want_loss, want_lse = X.forward(x, t, red)
    want = X.backward(x, t, want_lse, g, red)
    w = 1.0 / t.size if red == "mean" else 1.0
    b = X.bounds(shape[1], float(np.abs(x).max()), t.size, 0.0, g, w)
    scale = t.size if red == "sum" else 1
    assert abs(out - cout) <= 2 * b["loss"] * scale and np.abs(da - cdx).max() <= 2 * b["dx"]
    assert abs(out - want_loss) <= max(abs(cout - want_loss), b["loss"] * scale / 8)
    assert np.abs(da - want).max() <= max(np.abs(cdx - want).max(), b["dx"] / 8)

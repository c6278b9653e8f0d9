"""Tensors past 2^31 elements (2^32 for fill, copy and one unary forward) through the HBM-bound entry points.

Every tensor is built by tests/big_tensors.py: a tile repeated on the device and fresh rows in the windows of `marks` - the first
rows, the rows around elements 2^30, 2^31 (and 2^32), the last rows with the ragged tail.  Outputs start as NaN, only windows are
downloaded.  A row-local or elementwise pass holds when every output window equals BIT FOR BIT the same rows run as a small call of
their own (at the same 16-byte phase), holds no NaN, leaves its inputs' windows as they were and the guard floats behind every tensor
intact; the families' own files pin the small calls to their oracles.  Sums over a whole tensor are held against an f64 oracle built
from the tile's multiplicities (big_tensors.multiplicity) through tolerance.assert_contraction with K = the number of terms: at
n = 2^31 + 4099 that bound is loose by design - 1e-6 * n * max|a| * max|b| is about 1.5e-6 of the sum for data in (0.5, 1.5) - and
what it catches is the lost half, quarter or tail of a wrapped count, which moves the result by tens of per cent.

Entry points that refuse at a stated limit are called one past it with small real buffers: NK_ERR_INVALID, outputs untouched."""
import gc

import numpy as np
import pytest

import big_tensors as BT
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu
f32 = np.float32
NAN = float("nan")


def capi():
    from neuronika_amd import capi as c
    return c


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32).reshape(-1)


def build(dev, total, spec):
    """a Case: the tiled tensor; a float: `total` floats of it (NaN for outputs); both with guard floats behind"""
    return BT.tiled(dev, spec) if isinstance(spec, BT.Case) else BT.guarded(dev, total, spec)


def run_windows(dev, what, total, width, specs, big, outs, launch):
    """The big call, then every window as a small call of its own.  specs: name -> Case or float, what each tensor holds before the
    call; big: name -> the device tensors holding exactly that; outs: the names the call writes; launch(views, n) with flat views of
    n floats each."""
    launch({k: BT.window(a, 0, total) for k, a in big.items()}, total)
    for first, count in BT.marks(total, width):
        lo = first * width
        cnt = min((first + count) * width, total) - lo
        host, small, keep = {}, {}, []
        for k, s in specs.items():
            host[k] = BT.expect_host(s, lo, cnt) if isinstance(s, BT.Case) else np.full(cnt, s, f32)
            a = dev.zeros((cnt + 8,))
            keep.append(a)
            small[k] = BT.window(a, lo % 4, cnt)                            # the big call's 16-byte phase
            small[k].upload(host[k])
        launch(small, cnt)
        for k in specs:
            got = BT.window(big[k], lo, cnt).numpy()
            if k in outs:
                want = small[k].numpy().reshape(-1)
                assert not np.isnan(got).any(), (what, k, "NaN in rows %d.." % first, int(np.isnan(got).sum()))
                bad = np.flatnonzero(bits(got) != bits(want))
                assert bad.size == 0, (what, k, "rows %d..: the big call differs from the small one" % first, bad.size, lo + bad[:4], got[bad[:4]], want[bad[:4]])
            else:
                assert np.array_equal(bits(got), bits(host[k])), (what, k, "an input was written, rows %d.." % first)
        del small, keep
    for k, a in big.items():
        assert BT.guard_intact(a, total), (what, k, "guard floats")


def shaped(v, *shape):
    v.shape = tuple(int(s) for s in shape)
    return v


# ---- fill, copy, one unary forward: past 2^32 -------------------------------------------------------------------------------------
def test_fill_copy_unary_past_2_32(dev):
    """n = 2^32 + 5 (16 GiB a tensor, two live).  nk_copy takes its kernel for n % 4 == 0, so it copies the leading 2^32 + 4 floats
    and the last float must keep its NaN; the memcpy route takes all n."""
    c = capi()
    x = BT.CASES["flat32/x"]
    n, w = x.total, x.width
    Y = build(dev, n, NAN)
    BT.window(Y, 0, n).fill(1.5)
    for first, count in BT.marks(n, w):
        lo = first * w
        got = BT.window(Y, lo, min((first + count) * w, n) - lo).numpy()
        assert (got == f32(1.5)).all(), ("fill", first)
    assert BT.guard_intact(Y, n)
    BT.window(Y, 0, n).fill(NAN)
    X = build(dev, n, x)

    def copy(v, m):
        k = m - 1 if m == n else m                                          # the big call: 2^32 + 4 floats, the kernel's route
        c.check(c.lib.nk_copy(dev.h, v["y"].p, v["x"].p, k))
        if m == n:
            c.check(c.lib.nk_copy(dev.h, BT.window(v["y"], n - 1, 1).p, BT.window(v["x"], n - 1, 1).p, 1))
    run_windows(dev, "copy", n, w, dict(x=x, y=NAN), dict(x=X, y=Y), ("y",), copy)
    BT.window(Y, 0, n).fill(NAN)
    c.check(c.lib.nk_copy(dev.h, Y.p, X.p, n - 1))
    assert np.isnan(BT.window(Y, n - 1, 1).numpy()).all(), "the copy of 2^32 + 4 floats wrote the float behind them"
    BT.window(Y, 0, n).fill(NAN)
    run_windows(dev, "copy (memcpy route)", n, w, dict(x=x, y=NAN), dict(x=X, y=Y), ("y",), lambda v, m: c.check(c.lib.nk_copy(dev.h, v["y"].p, v["x"].p, m)))
    BT.window(Y, 0, n).fill(NAN)
    run_windows(dev, "tanh forward", n, w, dict(x=x, y=NAN), dict(x=X, y=Y), ("y",), lambda v, m: c.unary_fwd(dev, "tanh", v["x"], v["y"]))
    del X, Y
    gc.collect()


# ---- elementwise: n = 2^31 + 4099 -------------------------------------------------------------------------------------------------
def test_unary_and_relu(dev):
    """unary forward and backward (`+=`, with the reference operand), ReLU forward and backward (`+=` and assign)"""
    c = capi()
    x, g, d = (BT.CASES["flat31/" + k] for k in "xgd")
    n, w = x.total, x.width
    X, Y = build(dev, n, x), build(dev, n, NAN)
    run_windows(dev, "sigmoid forward", n, w, dict(x=x, y=NAN), dict(x=X, y=Y), ("y",), lambda v, m: c.unary_fwd(dev, "sigmoid", v["x"], v["y"]))
    BT.window(Y, 0, n).fill(NAN)
    run_windows(dev, "relu forward", n, w, dict(x=x, y=NAN), dict(x=X, y=Y), ("y",), lambda v, m: c.relu_fwd(dev, v["x"], v["y"]))
    G = build(dev, n, g)
    BT.window(Y, 0, n).fill(NAN)
    run_windows(dev, "relu backward assign", n, w, dict(x=x, g=g, d=NAN), dict(x=X, g=G, d=Y), ("d",),
                lambda v, m: c.relu_bwd(dev, v["d"], v["g"], v["x"], assign=True))
    del Y
    gc.collect()
    Dx = build(dev, n, d)
    run_windows(dev, "relu backward +=", n, w, dict(x=x, g=g, d=d), dict(x=X, g=G, d=Dx), ("d",), lambda v, m: c.relu_bwd(dev, v["d"], v["g"], v["x"]))
    del Dx
    gc.collect()
    Dx = build(dev, n, d)
    run_windows(dev, "tanh backward +=", n, w, dict(x=x, g=g, d=d), dict(x=X, g=G, d=Dx), ("d",),
                lambda v, m: c.unary_bwd(dev, "tanh", v["d"], v["g"], v["x"]))
    del X, G, Dx
    gc.collect()


def test_binary_same_shape(dev):
    """l * r over (2^21 + 4, 1024) = 2^31 + 4096 elements, forward and both gradients (`+=`): the collapsed extent is beyond an int"""
    c = capi()
    l, r, g, d = (BT.CASES["binary/" + k] for k in "lrgd")
    n, w = l.total, l.width

    def sh(v, m):
        return shaped(v, m // w, w)

    L, R, OUT = build(dev, n, l), build(dev, n, r), build(dev, n, NAN)
    run_windows(dev, "mul forward", n, w, dict(l=l, r=r, o=NAN), dict(l=L, r=R, o=OUT), ("o",),
                lambda v, m: c.binary_fwd(dev, "mul", sh(v["o"], m), sh(v["l"], m), sh(v["r"], m)))
    del OUT
    gc.collect()
    D = build(dev, n, d)                                                    # L stands in for the gradient
    run_windows(dev, "mul backward left +=", n, w, dict(g=l, r=r, d=d), dict(g=L, r=R, d=D), ("d",),
                lambda v, m: c.binary_bwd_left(dev, "mul", sh(v["d"], m), sh(v["g"], m), sh(v["r"], m)))
    del D
    gc.collect()
    D = build(dev, n, d)
    run_windows(dev, "div backward right +=", n, w, dict(g=g, l=l, r=r, d=d), dict(g=build(dev, n, g), l=L, r=R, d=D), ("d",),
                lambda v, m: c.binary_bwd_right(dev, "div", sh(v["d"], m), sh(v["g"], m), sh(v["l"], m), sh(v["r"], m)))
    del L, R, D
    gc.collect()


def test_binary_row_vector_against_matrix(dev):
    """(2^21 + 4, 1024) + (1024,): the broadcast forward, and the gradient of the matrix operand"""
    c = capi()
    l, d = BT.CASES["binary/l"], BT.CASES["binary/d"]
    n, w = l.total, l.width
    row = np.random.default_rng(77).random(w, dtype=f32) + f32(0.5)
    ROW = dev.array(row)

    def sh(v, m):
        return shaped(v, m // w, w)

    L, OUT = build(dev, n, l), build(dev, n, NAN)
    run_windows(dev, "add row forward", n, w, dict(l=l, o=NAN), dict(l=L, o=OUT), ("o",), lambda v, m: c.binary_fwd(dev, "add", sh(v["o"], m), sh(v["l"], m), ROW))
    BT.window(OUT, 0, n).fill(NAN)
    run_windows(dev, "mul row forward", n, w, dict(l=l, o=NAN), dict(l=L, o=OUT), ("o",), lambda v, m: c.binary_fwd(dev, "mul", sh(v["o"], m), sh(v["l"], m), ROW))
    del OUT
    gc.collect()
    D = build(dev, n, d)
    run_windows(dev, "mul row backward left +=", n, w, dict(g=l, d=d), dict(g=L, d=D), ("d",),
                lambda v, m: c.binary_bwd_left(dev, "mul", sh(v["d"], m), sh(v["g"], m), ROW))
    del L, D, ROW
    gc.collect()


def test_binary_scalar_operand_gradient(dev):
    """(2^21 + 4, 1024) (op) a scalar: the scalar's gradient sums all 2^31 + 4096 elements - sum g for add, sum g * l for mul - through
    the flat [R0][R1] split of nk_elementwise.hip (the two dims stay apart in the collapsed shape, their product being beyond an int,
    and must still be one flat range: the generic kernel would sum them in one thread).  The f64 oracle from the tile's
    multiplicities, tolerance.assert_contraction with K = n, data in (0.5, 2): a lost half is half the result."""
    c = capi()
    l, g = BT.CASES["binary/l"], BT.CASES["binary/g"]
    n, w = l.total, l.width
    mult, fresh_l = BT.multiplicity(l)
    _, fresh_g = BT.multiplicity(g)
    lt, gt = BT.tile_host(l).astype(np.float64), BT.tile_host(g).astype(np.float64)
    want_g = float((mult * gt).sum() + sum(b.astype(np.float64).sum() for _, b in fresh_g))
    want_gl = float((mult * gt * lt).sum() + sum((a.astype(np.float64) * b.astype(np.float64)).sum() for (_, a), (_, b) in zip(fresh_l, fresh_g)))
    L, G = build(dev, n, l), build(dev, n, g)
    LV, GV = shaped(BT.window(L, 0, n), n // w, w), shaped(BT.window(G, 0, n), n // w, w)
    R, D = dev.array(np.array([1.25], f32)), dev.full((1,), NAN)
    c.binary_bwd_right(dev, "add", D, GV, assign=True)
    assert_contraction("big/scalar add gradient", D.numpy(), [want_g], n, 2.0, 1.0)
    c.binary_bwd_right(dev, "mul", D, GV, LV, R, assign=True)
    assert_contraction("big/scalar mul gradient", D.numpy(), [want_gl], n, 2.0, 2.0)
    assert BT.guard_intact(L, n) and BT.guard_intact(G, n)
    del L, G, LV, GV, R, D
    gc.collect()


# ---- sum, mean, MSE ---------------------------------------------------------------------------------------------------------------
def test_sum_mean_mse(dev):
    """Forward: the f64 oracle from the tile's multiplicities, tolerance.assert_contraction with K = n (see the module's docstring for
    how loose that is and why it is enough: data in (0.5, 1.5), a lost half is 50 % of the result).  Backward: sum and MSE (sum
    reduction) window by window against small calls; the mean's backward divides by n, which no small call does, so its assign form
    must give one value everywhere, g / n to a rounding."""
    c = capi()
    x, t, d = BT.CASES["reduce/x"], BT.CASES["reduce/t"], BT.CASES["flat31/d"]
    n, w = x.total, x.width
    mult, fresh = BT.multiplicity(x)
    _, fresh_t = BT.multiplicity(t)
    xt, tt = BT.tile_host(x).astype(np.float64), BT.tile_host(t).astype(np.float64)
    want_sum = float((mult * xt).sum() + sum(a.astype(np.float64).sum() for _, a in fresh))
    want_sq = float((mult * (xt - tt) ** 2).sum() + sum(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum() for (_, a), (_, b) in zip(fresh, fresh_t)))
    X, T, OUT = build(dev, n, x), build(dev, n, t), dev.full((1,), NAN)
    XV, TV = BT.window(X, 0, n), BT.window(T, 0, n)
    c.sum_fwd(dev, XV, OUT)
    assert_contraction("big/sum", OUT.numpy(), [want_sum], n, 1.5, 1.0)
    c.mean_fwd(dev, XV, OUT)
    assert_contraction("big/mean", OUT.numpy(), [want_sum / n], n, 1.5, 1.0, scale=1.0 / n)
    c.mse_fwd(dev, XV, TV, OUT, "sum")
    assert_contraction("big/mse sum", OUT.numpy(), [want_sq], n, 1.0, 1.0)
    c.mse_fwd(dev, XV, TV, OUT, "mean")
    assert_contraction("big/mse mean", OUT.numpy(), [want_sq / n], n, 1.0, 1.0, scale=1.0 / n)
    G = dev.array(np.array([0.75], f32))
    D = build(dev, n, d)
    run_windows(dev, "sum backward +=", n, w, dict(d=d), dict(d=D), ("d",), lambda v, m: c.sum_bwd(dev, v["d"], G))
    del D
    gc.collect()
    D = build(dev, n, d)
    run_windows(dev, "mse backward += (sum)", n, w, dict(x=x, t=t, d=d), dict(x=X, t=T, d=D), ("d",),
                lambda v, m: c.mse_bwd(dev, v["d"], G, v["x"], v["t"], "sum"))
    BT.window(D, 0, n).fill(NAN)
    c.mean_bwd(dev, BT.window(D, 0, n), G, assign=True)
    first_value = BT.window(D, 0, 1).numpy()[0]
    assert abs(float(first_value) - 0.75 / n) <= 2.0 ** -23 * 0.75 / n
    for first, count in BT.marks(n, w):
        lo = first * w
        got = BT.window(D, lo, min((first + count) * w, n) - lo).numpy()
        assert (got == first_value).all(), ("mean backward assign", first)
    assert BT.guard_intact(D, n)
    del X, T, D, OUT, G
    gc.collect()


# ---- softmax and log-softmax ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1024, 1027], ids=["rows", "blocks"])
def test_softmax(dev, L):
    """(2^21 + 3) x 1024 through the row kernels (one wave a row), x 1027 through the block kernels: forward and `+=` backward of both"""
    c = capi()
    x, g, d, y = (BT.CASES["rows%d/%s" % (L, k)] for k in "xgdy")
    n = x.total

    def sh(v, m):
        return shaped(v, m // L, L)

    X, Y = build(dev, n, x), build(dev, n, NAN)
    run_windows(dev, "softmax forward", n, L, dict(x=x, y=NAN), dict(x=X, y=Y), ("y",), lambda v, m: c.softmax_fwd(dev, sh(v["x"], m), sh(v["y"], m), 1))
    BT.window(Y, 0, n).fill(NAN)
    run_windows(dev, "log-softmax forward", n, L, dict(x=x, y=NAN), dict(x=X, y=Y), ("y",), lambda v, m: c.log_softmax_fwd(dev, sh(v["x"], m), sh(v["y"], m), 1))
    del Y
    gc.collect()
    G = build(dev, n, g)                                                    # X stands in for y: any finite rows do for a bit-for-bit check
    for name, bwd in (("softmax backward +=", c.softmax_bwd), ("log-softmax backward +=", c.log_softmax_bwd)):
        D = build(dev, n, d)
        run_windows(dev, name, n, L, dict(y=x, g=g, d=d), dict(y=X, g=G, d=D), ("d",), lambda v, m: bwd(dev, sh(v["d"], m), sh(v["g"], m), sh(v["y"], m), 1))
        del D
        gc.collect()
    del X, G
    gc.collect()


# ---- LayerNorm and RMSNorm --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1024, 1027], ids=["registers", "general"])
@pytest.mark.parametrize("norm", ["layer", "rms"])
def test_norms(dev, norm, D):
    """(2^21 + 3) rows of 1024 (row-in-registers kernels) and of 1027 (general kernels).  Forward (y and stats) and dx `+=` window by
    window against small calls; the parameter gradients against the f64 oracle from the tile's row multiplicities and the windows'
    rows, tolerance.assert_contraction with K = rows, |g| <= 2 and max |xhat| from the oracle - a lost range of rows is a lost share of
    a sum of 2^21 terms that the bound, about 2^21 * 1e-6 * 2 * max|xhat|, does not hide when the range is a half or a quarter."""
    import layernorm_oracle as LN
    import rms_norm_oracle as RN
    c = capi()
    x, g, d = (BT.CASES["rows%d/%s" % (D, k)] for k in "xgd")
    n, rows = x.total, x.total // D
    W = 2 if norm == "layer" else 1
    rng = np.random.default_rng(D)
    gamma, beta = (1.0 + 0.5 * rng.standard_normal(D)).astype(f32), rng.standard_normal(D).astype(f32)
    GA, BE = dev.array(gamma), dev.array(beta)
    S = dev.full((rows * W,), NAN)
    order = {}

    def stats_of(m):
        """the big call: all of S; a window: a NaN-filled buffer of its own for the forward, the window's rows of S for the backward"""
        first = next(order["it"])
        if first is None:
            return S, None
        return dev.full((m // D * W,), NAN), first

    def fwd(v, m):
        st, first = stats_of(m)
        if norm == "layer":
            c.layer_norm_fwd(dev, v["x"], GA, BE, v["y"], st, m // D, D, 1e-5)
        else:
            c.rms_norm_fwd(dev, v["x"], GA, v["y"], st, m // D, D, 1e-6)
        if first is not None:
            got, want = BT.window(S, first * W, m // D * W).numpy(), st.numpy()
            assert not np.isnan(got).any() and np.array_equal(bits(got), bits(want)), (norm, "stats, rows %d.." % first)

    def dx(v, m):
        first = next(order["it"])
        st = S if first is None else BT.window(S, first * W, m // D * W)
        (c.layer_norm_bwd if norm == "layer" else c.rms_norm_bwd)(dev, v["d"], v["g"], v["x"], GA, st, m // D, D)

    def run(what, specs, big, outs, launch):
        order["it"] = iter([None] + [f for f, _ in BT.marks(n, D)])
        run_windows(dev, what, n, D, specs, big, outs, launch)

    X, Y = build(dev, n, x), build(dev, n, NAN)
    run(norm + " norm forward", dict(x=x, y=NAN), dict(x=X, y=Y), ("y",), fwd)
    del Y
    gc.collect()
    G, DX = build(dev, n, g), build(dev, n, d)
    run(norm + " norm dx +=", dict(x=x, g=g, d=d), dict(x=X, g=G, d=DX), ("d",), dx)
    del DX
    gc.collect()
    # parameter gradients: rows of the tile with their multiplicities, then the windows' fresh rows
    mult, fresh = BT.multiplicity(x)
    _, fresh_g = BT.multiplicity(g)
    blocks = [(BT.tile_host(x).reshape(-1, D), BT.tile_host(g).reshape(-1, D), mult[::D].astype(np.float64))]
    blocks += [(a.reshape(-1, D), b.reshape(-1, D), np.ones(a.size // D)) for (_, a), (_, b) in zip(fresh, fresh_g)]
    assert (mult.reshape(-1, D) == mult[::D, None]).all(), "the windows cover whole rows"
    dg64, db64, xhat_max = np.zeros(D), np.zeros(D), 0.0
    for xs, gs, m in blocks:
        xs, gs = xs.astype(np.float64), gs.astype(np.float64)
        if norm == "layer":
            _, st = LN.forward(xs, None, None, 1e-5)
            xhat = (xs - st[:, :1]) * st[:, 1:]
        else:
            _, st = RN.forward(xs, None, 1e-6)
            xhat = xs * st[:, None]
        dg64 += (m[:, None] * gs * xhat).sum(axis=0)
        db64 += (m[:, None] * gs).sum(axis=0)
        xhat_max = max(xhat_max, float(np.abs(xhat).max()))
    DG, DB = dev.full((D,), NAN), dev.full((D,), NAN)
    XV, GV = BT.window(X, 0, n), BT.window(G, 0, n)
    if norm == "layer":
        c.layer_norm_bwd_params(dev, DG, DB, GV, XV, S, rows, D, assign=True)
        assert_contraction("big/layernorm dbeta", DB.numpy(), db64, rows, 2.0, 1.0)
    else:
        c.rms_norm_bwd_gamma(dev, DG, GV, XV, S, rows, D, assign=True)
    assert_contraction("big/%snorm dgamma" % norm, DG.numpy(), dg64, rows, 2.0, xhat_max)
    assert BT.guard_intact(X, n) and BT.guard_intact(G, n)
    del X, G, S, DG, DB, GA, BE
    gc.collect()


# ---- activations ------------------------------------------------------------------------------------------------------------------
def test_gelu(dev):
    c = capi()
    x, g, d = (BT.CASES["flat31/" + k] for k in "xgd")
    n, w = x.total, x.width
    X, Y = build(dev, n, x), build(dev, n, NAN)
    run_windows(dev, "gelu forward", n, w, dict(x=x, y=NAN), dict(x=X, y=Y), ("y",), lambda v, m: c.activation_fwd(dev, "gelu", v["x"], v["y"], n=m))
    G = build(dev, n, g)
    BT.window(Y, 0, n).fill(NAN)
    run_windows(dev, "gelu backward assign", n, w, dict(x=x, g=g, d=NAN), dict(x=X, g=G, d=Y), ("d",),
                lambda v, m: c.activation_bwd(dev, "gelu", v["d"], v["g"], v["x"], n=m, assign=True))
    del Y
    gc.collect()
    D = build(dev, n, d)
    run_windows(dev, "gelu backward +=", n, w, dict(x=x, g=g, d=d), dict(x=X, g=G, d=D), ("d",),
                lambda v, m: c.activation_bwd(dev, "gelu", v["d"], v["g"], v["x"], n=m))
    del X, G, D
    gc.collect()


# ---- dropout ----------------------------------------------------------------------------------------------------------------------
def test_dropout(dev):
    """Forward with the mask stored: y and the mask window by window against small calls that continue the Philox stream at their first
    element (offset + first / 8), and the mask against the oracle's Philox at those element indices.  Backward `+=` with the stored
    mask."""
    c = capi()
    from oracle import neuronika_oracle as O
    x, g, d = (BT.CASES["flat31/" + k] for k in "xgd")
    n, w = x.total, x.width
    p, seed, offset = 0.3, 91, 12345
    X, Y, NZ = build(dev, n, x), build(dev, n, NAN), build(dev, n, NAN)
    c.dropout_fwd(dev, BT.window(X, 0, n), BT.window(Y, 0, n), BT.window(NZ, 0, n), p, True, seed, offset)
    for first, count in BT.marks(n, w):
        lo = first * w
        cnt = min((first + count) * w, n) - lo
        assert lo % 8 == 0
        noise = BT.window(NZ, lo, cnt).numpy()
        assert np.array_equal(noise, O.dropout_noise(cnt, p, seed, offset + lo // 8)), ("the mask at elements %d.." % lo)
        xs = BT.expect_host(x, lo, cnt)
        SX, SY, SZ = dev.array(xs), dev.full((cnt,), NAN), dev.full((cnt,), NAN)
        c.dropout_fwd(dev, SX, SY, SZ, p, True, seed, offset + lo // 8)
        got = BT.window(Y, lo, cnt).numpy()
        assert not np.isnan(got).any() and np.array_equal(bits(got), bits(SY.numpy())) and np.array_equal(SZ.numpy(), noise), ("dropout forward", first)
    assert BT.guard_intact(Y, n) and BT.guard_intact(NZ, n) and BT.guard_intact(X, n)
    del Y
    gc.collect()
    D = build(dev, n, d)                                                    # X stands in for the gradient; the mask is the device's own
    c.dropout_bwd(dev, BT.window(D, 0, n), BT.window(X, 0, n), BT.window(NZ, 0, n), p, True)
    for first, count in BT.marks(n, w):
        lo = first * w
        cnt = min((first + count) * w, n) - lo
        SD, SG, SZ = dev.array(BT.expect_host(d, lo, cnt)), dev.array(BT.expect_host(x, lo, cnt)), dev.array(O.dropout_noise(cnt, p, seed, offset + lo // 8))
        c.dropout_bwd(dev, SD, SG, SZ, p, True)
        got = BT.window(D, lo, cnt).numpy()
        assert not np.isnan(got).any() and np.array_equal(bits(got), bits(SD.numpy())), ("dropout backward", first)
    assert BT.guard_intact(D, n)
    del X, NZ, D
    gc.collect()


# ---- AdamW ------------------------------------------------------------------------------------------------------------------------
def test_adamw_one_parameter(dev):
    """one parameter of 2^31 + 4099 elements through nk_adamw_step_multi: w, m and v window by window against a small call with the same
    step and hyper-parameters; the gradient is read only"""
    c = capi()
    cs = {k: BT.CASES["adamw/" + k] for k in "wgmv"}
    n, w = cs["w"].total, cs["w"].width
    big = {k: build(dev, n, s) for k, s in cs.items()}
    hyper = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1)
    run_windows(dev, "adamw step", n, w, cs, big, ("w", "m", "v"),
                lambda v, m: c.adamw_step_multi(dev, [v["w"]], [v["g"]], [v["m"]], [v["v"]], None, steps=[3], **hyper))
    del big
    gc.collect()


# ---- rope -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("il", [False, True], ids=["half-split", "interleaved"])
def test_rope(dev, il):
    """B * T = 2^15 + 1 rows of 512 heads x 128: 2^31 + 65536 elements.  Items: half-split 32769 * 512 * 16 = 268 443 648, interleaved
    32769 * 512 * 32 = 536 887 296 - both below 2^32, the `small` branch of rope_split with 32-bit division, as in tests/test_gpu_rope.py
    (at most 201 * 24 * 32 items); the other branch needs more than 2^32 items, 64 GiB and more a tensor with these widths, and is not
    reached by any test.  What this shape crosses is the row offset rows * ld past 2^31 elements and 2^32 bytes.  B = 2^15 + 1 samples
    of one position each, so a window's rows are a call of their own with their slice of `start`."""
    c = capi()
    x, g, d = (BT.CASES["rope/" + k] for k in "xgd")
    n, w = x.total, x.width
    NH, dh, max_pos = 512, 128, 4096
    rows = n // w
    assert rows == (1 << 15) + 1 and rows * w == n
    start = ((np.arange(rows, dtype=np.int64) * 7919) % max_pos).astype(np.int32)
    table = dev.zeros((max_pos, dh // 2, 2))
    c.rope_table(dev, table, max_pos, dh)
    state = {}

    def geometry(m):
        first = 0 if m == n else state["first"]
        return dev.int_array(start[first:first + m // w]), m // w

    def fwd(v, m):
        st, b = geometry(m)
        c.rope_fwd(dev, v["x"], w, v["y"], w, table, st, b, 1, NH, dh, dh, max_pos, il)

    def bwd(v, m, assign):
        st, b = geometry(m)
        c.rope_bwd(dev, v["d"], w, v["g"], w, table, st, b, 1, NH, dh, dh, max_pos, il, assign=assign)

    def run(what, specs, big, outs, launch):
        # run_windows calls launch for the big tensor first, then once per window in the order of marks
        order = iter([None] + [f for f, _ in BT.marks(n, w)])

        def stepped(v, m):
            state["first"] = next(order)
            launch(v, m)
        run_windows(dev, what, n, w, specs, big, outs, stepped)

    X, Y = build(dev, n, x), build(dev, n, NAN)
    run("rope forward", dict(x=x, y=NAN), dict(x=X, y=Y), ("y",), fwd)
    BT.window(Y, 0, n).fill(NAN)
    run("rope backward assign", dict(g=x, d=NAN), dict(g=X, d=Y), ("d",), lambda v, m: bwd(v, m, True))
    del Y
    gc.collect()
    D = build(dev, n, d)
    run("rope backward +=", dict(g=x, d=d), dict(g=X, d=D), ("d",), lambda v, m: bwd(v, m, False))
    del X, D, table
    gc.collect()


# ---- pooling ----------------------------------------------------------------------------------------------------------------------
def test_pooling_2_2_0(dev):
    """Max and average pooling 2 / 2 / 0 over (2^10 + 1) x 64 planes of 184 x 184 (2^31 + 73 470 336 elements in, a quarter out), the
    windowed kernels: the window planes of y, idx and of the assign backward's dx against the same planes as a (1, planes) call."""
    c = capi()
    x, g = BT.CASES["pool/x"], BT.CASES["pool/g"]
    n, ip, op = x.total, x.width, g.width
    planes = n // ip
    shape, k, s, p = ((1 << 10) + 1, 64, 184, 184), (2, 2), (2, 2), (0, 0)
    assert planes == shape[0] * shape[1] and c.pool_out_shape(shape, k, s, p) == (shape[0], shape[1], 92, 92)
    X, G = build(dev, n, x), build(dev, g.total, g)
    Y, YA, DX = build(dev, g.total, NAN), build(dev, g.total, NAN), build(dev, n, NAN)
    I = dev.int_zeros((g.total + BT.GUARD_FLOATS,))
    XV, GV = BT.window(X, 0, n), BT.window(G, 0, g.total)
    c.max_pool_fwd(dev, XV, shape, Y, I, k, s, p)
    c.avg_pool_fwd(dev, XV, shape, YA, k, s, p)
    c.max_pool_bwd(dev, DX, shape, GV, I, k, s, p, assign=True)

    def plane_windows(which):
        for first, count in BT.marks(n, ip):
            small = (1, count, 184, 184)
            SX, SG = dev.array(BT.expect_host(x, first * ip, count * ip)), dev.array(BT.expect_host(g, first * op, count * op))
            SY, SYA, SD, SI = dev.full((count * op,), NAN), dev.full((count * op,), NAN), dev.full((count * ip,), NAN), dev.int_zeros((count * op,))
            if which == "max":
                c.max_pool_fwd(dev, SX, small, SY, SI, k, s, p)
                c.avg_pool_fwd(dev, SX, small, SYA, k, s, p)
                c.max_pool_bwd(dev, SD, small, SG, SI, k, s, p, assign=True)
                pairs = (("max y", Y, SY, op), ("avg y", YA, SYA, op), ("max dx", DX, SD, ip))
                iv = I.view_offset(first * op)
                iv.shape, iv.size = (count * op,), count * op
                assert np.array_equal(iv.numpy(), SI.numpy()), ("idx", "planes %d.." % first)
            else:
                c.avg_pool_bwd(dev, SD, small, SG, k, s, p, assign=True)
                pairs = (("avg dx", DX, SD, ip),)
            for what, big, sm, per in pairs:
                got = BT.window(big, first * per, count * per).numpy()
                assert not np.isnan(got).any() and np.array_equal(bits(got), bits(sm.numpy())), (what, "planes %d.." % first)

    plane_windows("max")
    BT.window(DX, 0, n).fill(NAN)
    c.avg_pool_bwd(dev, DX, shape, GV, k, s, p, assign=True)
    plane_windows("avg")
    for a, t in ((X, n), (G, g.total), (Y, g.total), (YA, g.total), (DX, n)):
        assert BT.guard_intact(a, t)
    del X, G, Y, YA, DX, I, XV, GV
    gc.collect()


# ---- batch norm as a map ----------------------------------------------------------------------------------------------------------
def test_batch_norm_inference_maps(dev):
    """(129, 64, 2^18) = 2^31 + 2^24 elements through the plane kernels: the inference forward and its dx (`+=`), window planes against
    (1, planes) calls whose per-channel vectors are the window's channels in order - the same scalars, so the same bits"""
    c = capi()
    x, g, d = (BT.CASES["bnmap/" + k] for k in "xgd")
    n, L = x.total, x.width
    N, C = 129, 64
    rng = np.random.default_rng(3)
    gamma, beta = (1.0 + 0.5 * rng.standard_normal(C)).astype(f32), rng.standard_normal(C).astype(f32)
    rm, rv = rng.standard_normal(C).astype(f32), (0.5 + rng.random(C)).astype(f32)
    GA, BE, RM, RV, S = dev.array(gamma), dev.array(beta), dev.array(rm), dev.array(rv), dev.full((C, 2), NAN)
    state = {}

    def vectors(m):
        """the big call: the layer's own vectors; a window of planes p0 ..: channel (p0 + i) % C in place i"""
        first = next(state["it"])
        if first is None:
            return N, C, GA, BE, RM, RV
        ch = (first + np.arange(m // L)) % C
        return 1, m // L, dev.array(gamma[ch]), dev.array(beta[ch]), dev.array(rm[ch]), dev.array(rv[ch])

    def fwd(v, m):
        nn, cc, ga, be, a, b = vectors(m)
        st = S if nn == N else dev.full((cc, 2), NAN)
        c.batch_norm_infer_fwd(dev, v["x"], ga, be, a, b, v["y"], st, nn, cc, L, 1e-5)

    def dx(v, m):
        nn, cc, ga, be, a, b = vectors(m)
        st = S if nn == N else dev.array(state["S"][(state["first"] + np.arange(cc)) % C])    # the forward's {mean, rstd} of those channels
        c.batch_norm_bwd(dev, v["d"], v["g"], None, ga, st, None, nn, cc, L)

    def run(what, specs, big, outs, launch):
        firsts = [None] + [f for f, _ in BT.marks(n, L)]                   # run_windows: the big call, then the windows in order
        state["it"] = iter(firsts)
        seen = iter(firsts)

        def stepped(v, m):
            state["first"] = next(seen)
            launch(v, m)
        run_windows(dev, what, n, L, specs, big, outs, stepped)

    X, Y = build(dev, n, x), build(dev, n, NAN)
    run("batch norm inference forward", dict(x=x, y=NAN), dict(x=X, y=Y), ("y",), fwd)
    state["S"] = S.numpy()
    assert np.isfinite(state["S"]).all()
    del Y
    gc.collect()
    D = build(dev, n, d)
    run("batch norm inference dx +=", dict(g=x, d=d), dict(g=X, d=D), ("d",), dx)
    del X, D
    gc.collect()


def test_batch_norm_training_columns(dev):
    """(2^21 + 3, 1024, 1) = 2^31 + 3072 elements through the column kernels, training form, x and g in (0.5, 1.5) so that a lost range
    of rows is a lost share of every sum.  The f64 oracle comes from the tile's row multiplicities and the windows' fresh rows.
    Through tolerance.assert_contraction with K = N = 2^21 + 3 terms: the mean (scale 1 / N), the variance recovered from rstd
    (operands up to 1.5, scale 1 / N, the elementwise tolerance on top for the reciprocal square root), the running statistics
    (the same with the momentum, and N / (N - 1) for the variance), the channel sums {sum g, sum g * xhat} and dgamma, dbeta.  The sums'
    oracle takes the DEVICE's stats, which are an input of nk_batch_norm_bwd_sums.  The two maps on the window rows, from the device's
    own stats and sums in f64: y inside the suite's elementwise tolerance; dx (assign) inside 32 * 2^-24 * |gamma * rstd| +
    2^-22 * |dx| - g - s0 / N - xhat * s1 / N takes at most eight roundings of values below 4 before the product with gamma * rstd,
    and the result two more.  A row read or written through a wrapped offset differs by tenths."""
    import batchnorm_oracle as BN
    from tolerance import ELEMENTWISE_ATOL, ELEMENTWISE_RTOL
    c = capi()
    x, g = BT.CASES["bncol/x"], BT.CASES["bncol/g"]
    n, C = x.total, x.width
    N = n // C
    assert N * C == n and N == (1 << 21) + 3
    eps, momentum = 1e-5, 0.1
    rng = np.random.default_rng(4)
    gamma, beta = (1.0 + 0.5 * rng.standard_normal(C)).astype(f32), rng.standard_normal(C).astype(f32)
    rm, rv = rng.standard_normal(C).astype(f32), (0.5 + rng.random(C)).astype(f32)
    # rows of the tile with their multiplicities, then the windows' fresh rows
    mult, fresh = BT.multiplicity(x)
    _, fresh_g = BT.multiplicity(g)
    assert (mult.reshape(-1, C) == mult[::C, None]).all(), "the windows cover whole rows"
    blocks = [(BT.tile_host(x).reshape(-1, C).astype(np.float64), BT.tile_host(g).reshape(-1, C).astype(np.float64), mult[::C].astype(np.float64))]
    blocks += [(a.reshape(-1, C).astype(np.float64), b.reshape(-1, C).astype(np.float64), np.ones(a.size // C)) for (_, a), (_, b) in zip(fresh, fresh_g)]
    assert int(sum(m.sum() for _, _, m in blocks)) == N
    mean64 = sum((m[:, None] * xs).sum(axis=0) for xs, _, m in blocks) / N
    var64 = sum((m[:, None] * (xs - mean64) ** 2).sum(axis=0) for xs, _, m in blocks) / N
    GA, BE, RM, RV = dev.array(gamma), dev.array(beta), dev.array(rm), dev.array(rv)
    S, SUMS, DG, DB = dev.full((C, 2), NAN), dev.full((C, 2), NAN), dev.full((C,), NAN), dev.full((C,), NAN)
    X, G, Y = build(dev, n, x), build(dev, n, g), build(dev, n, NAN)
    XV, GV, YV = BT.window(X, 0, n), BT.window(G, 0, n), BT.window(Y, 0, n)
    c.batch_norm_fwd(dev, XV, GA, BE, YV, S, RM, RV, N, C, 1, eps, momentum)
    st = S.numpy().astype(np.float64)
    assert np.isfinite(st).all()
    assert_contraction("big/batchnorm mean", st[:, 0], mean64, N, 1.5, 1.0, scale=1.0 / N)
    assert_contraction("big/batchnorm var", 1.0 / st[:, 1] ** 2 - eps, var64, N, 1.5, 1.5, scale=1.0 / N, epilogue=True)
    assert_contraction("big/batchnorm running_mean", RM.numpy(), (1 - momentum) * rm + momentum * mean64, N, 1.5, 1.0, scale=momentum / N, epilogue=True)
    assert_contraction("big/batchnorm running_var", RV.numpy(), (1 - momentum) * rv + momentum * var64 * (N / (N - 1.0)), N, 1.5, 1.5,
                       scale=momentum / (N - 1.0), epilogue=True)
    c.batch_norm_bwd_sums(dev, SUMS, GV, XV, S, N, C, 1)
    c.batch_norm_bwd_params(dev, DG, DB, SUMS, C, assign=True)
    sums = SUMS.numpy().astype(np.float64)
    s0 = sum((m[:, None] * gs).sum(axis=0) for _, gs, m in blocks)
    s1 = sum((m[:, None] * gs * (xs - st[:, 0]) * st[:, 1]).sum(axis=0) for xs, gs, m in blocks)
    xhat_max = max(float(np.abs((xs - st[:, 0]) * st[:, 1]).max()) for xs, _, _ in blocks)
    assert_contraction("big/batchnorm s0", sums[:, 0], s0, N, 1.5, 1.0)
    assert_contraction("big/batchnorm s1", sums[:, 1], s1, N, 1.5, xhat_max)
    assert_contraction("big/batchnorm dbeta", DB.numpy(), s0, N, 1.5, 1.0)
    assert_contraction("big/batchnorm dgamma", DG.numpy(), s1, N, 1.5, xhat_max)

    def windows(what, out, want_of, bound_of):
        for first, count in BT.marks(n, C):
            xs = BT.expect_host(x, first * C, count * C).reshape(1, count, C).transpose(1, 2, 0).astype(np.float64)    # (rows, C, 1)
            gs = BT.expect_host(g, first * C, count * C).reshape(1, count, C).transpose(1, 2, 0).astype(np.float64)
            got = BT.window(out, first * C, count * C).numpy().reshape(count, C, 1)
            want = want_of(xs, gs)
            assert not np.isnan(got).any(), (what, "NaN in rows %d.." % first)
            over = np.abs(got - want) - bound_of(want)
            assert (over <= 0).all(), (what, "rows %d.." % first, float(over.max()))

    windows("batch norm training forward", Y, lambda xs, gs: BN.normalise(xs, st, gamma.astype(np.float64), beta.astype(np.float64)),
            lambda want: ELEMENTWISE_ATOL + ELEMENTWISE_RTOL * np.abs(want))
    assert BT.guard_intact(Y, n)
    YV.fill(NAN)
    c.batch_norm_bwd(dev, YV, GV, XV, GA, S, SUMS, N, C, 1, assign=True)
    k = np.abs(gamma.astype(np.float64) * st[:, 1]).reshape(1, C, 1)

    def dx_of(xs, gs):
        """batchnorm_oracle.backward's dx with M = N and the device's sums (a window's own sums are not the tensor's)"""
        xhat = (xs - st[:, 0].reshape(1, C, 1)) * st[:, 1].reshape(1, C, 1)
        return gamma.astype(np.float64).reshape(1, C, 1) * st[:, 1].reshape(1, C, 1) * (gs - (sums[:, 0] / N).reshape(1, C, 1) - xhat * (sums[:, 1] / N).reshape(1, C, 1))

    windows("batch norm training dx", Y, dx_of, lambda want: 32 * 2.0 ** -24 * k + 2.0 ** -22 * np.abs(want))
    for a in (X, G, Y):
        assert BT.guard_intact(a, n)
    del X, G, Y, XV, GV, YV, S, SUMS
    gc.collect()


# ---- cross entropy ----------------------------------------------------------------------------------------------------------------
def test_cross_entropy(dev):
    """(2^15 + 1) positions x 65536 classes = 2^31 + 65536 logits through the block kernels.  lse on the window rows against small
    calls; the loss (mean and sum) against the f64 oracle - lse of the tile's rows and of the windows' fresh rows, the target's logit
    of every position from the host image - inside cross_entropy_oracle.bounds as the family's fullsize test uses it; backward assign
    and `+=` (sum reduction: no count that a small call would not share) on the window rows."""
    import cross_entropy_oracle as XO
    c = capi()
    x, d = BT.CASES["ce/x"], BT.CASES["ce/d"]
    n, C = x.total, x.width
    N = n // C
    t = ((np.arange(N, dtype=np.int64) * 7919 + 13) % C).astype(f32)
    t[::7] = 3.0                                                            # ignore_index = 3 is hit
    on = t != 3.0
    count = int(on.sum())
    T, LSE, OUT, G = dev.array(t), dev.full((N,), NAN), dev.full((1,), NAN), dev.array(np.array([0.5], f32))
    X = build(dev, n, x)
    XV = BT.window(X, 0, n)
    # the oracle: lse per row of the tile, per fresh row of the windows; x[r, t[r]] from the host image
    tile = BT.tile_host(x)

    def lse64(rows):
        r = rows.astype(np.float64)
        m = r.max(axis=1)
        return m + np.log(np.exp(r - m[:, None]).sum(axis=1))

    want_lse = lse64(tile.reshape(-1, C))[np.arange(N) % x.tile_rows]
    for k in range(len(BT.marks(n, C))):
        lo, data = BT.window_host(x, k)
        want_lse[lo // C:lo // C + data.size // C] = lse64(data.reshape(-1, C))
    picked = BT.expect_at(x, np.arange(N, dtype=np.int64) * C + t.astype(np.int64)).astype(np.float64)
    per = np.where(on, want_lse - picked, 0.0)
    b = XO.bounds(C, 4.0, N, 0.0, 0.5, 1.0 / count)
    for red, want in (("mean", per.sum() / count), ("sum", per.sum())):
        c.cross_entropy_fwd(dev, XV, T, LSE, OUT, (N, C), red, 3)
        assert abs(OUT.item() - want) <= b["loss"] * (count if red == "sum" else 1), (red, OUT.item(), want)
    lse = LSE.numpy()
    assert np.abs(lse - want_lse).max() <= b["lse"]
    state = {}

    def bwd(v, m, assign):
        first = state["first"]
        if first is None:
            c.cross_entropy_bwd(dev, v["d"], G, v["x"], T, LSE, (N, C), "sum", 3, assign=assign)
            return
        rows = m // C
        ST, SL, SO = dev.array(t[first:first + rows]), dev.full((rows,), NAN), dev.full((1,), NAN)
        c.cross_entropy_fwd(dev, v["x"], ST, SL, SO, (rows, C), "sum", 3)
        assert np.array_equal(bits(SL.numpy()), bits(lse[first:first + rows])), ("lse, rows %d.." % first)
        c.cross_entropy_bwd(dev, v["d"], G, v["x"], ST, SL, (rows, C), "sum", 3, assign=assign)

    def run(what, specs, big, assign):
        order = iter([None] + [f for f, _ in BT.marks(n, C)])

        def stepped(v, m):
            state["first"] = next(order)
            bwd(v, m, assign)
        run_windows(dev, what, n, C, specs, big, ("d",), stepped)

    D = build(dev, n, NAN)
    run("cross entropy backward assign", dict(x=x, d=NAN), dict(x=X, d=D), True)
    del D
    gc.collect()
    D = build(dev, n, d)
    run("cross entropy backward +=", dict(x=x, d=d), dict(x=X, d=D), False)
    del X, D, XV, T, LSE, OUT, G
    gc.collect()


# ---- KV cache, contiguous ---------------------------------------------------------------------------------------------------------
def test_kv_cache_contiguous(dev):
    """Caches of (9, 8, 2^18 + 16, 128) = 2^31 + 268 451 840 floats each: sample 8 lives wholly past element 2^31.  301 positions are
    appended to every sample (300 in one call, the step's own in a second) and nk_attention_decode_fwd runs T = 1 on them.  Sample 8's
    output must have the bits of the same rows through caches of B = 1; its cache rows must hold the appended rows bit for bit, the
    positions behind them and the guard floats must keep what they held."""
    c = capi()
    B, H, cap, dh, T0 = 9, 8, (1 << 18) + 16, 128, 300
    d, per = H * dh, H * cap * dh                                          # floats of a row of K; of a sample's cache
    total = B * per
    assert total > BT.TWO31 and 8 * per > BT.TWO31
    rng = np.random.default_rng(55)
    k0, v0 = (rng.random((B * T0, d), dtype=f32) * f32(2) - f32(1) for _ in range(2))
    k1, v1, q = (rng.random((B, d), dtype=f32) * f32(2) - f32(1) for _ in range(3))
    scale = float(f32(1.0 / np.sqrt(dh)))

    def run(b_lo, nb):
        """append and decode samples b_lo .. b_lo + nb - 1 through caches of their own; -> (Kc, Vc, out)"""
        n = nb * per
        Kc, Vc = BT.guarded(dev, n, NAN), BT.guarded(dev, n, NAN)
        rows = slice(b_lo * T0, (b_lo + nb) * T0)
        c.kv_cache_append(dev, Kc, Vc, dev.array(k0[rows]), dev.array(v0[rows]), d, dev.int_array(np.zeros(nb, np.int32)), nb, T0, H, dh, cap)
        S = dev.int_array(np.full(nb, T0, np.int32))
        c.kv_cache_append(dev, Kc, Vc, dev.array(k1[b_lo:b_lo + nb]), dev.array(v1[b_lo:b_lo + nb]), d, S, nb, 1, H, dh, cap)
        out = dev.full((nb, d), NAN)
        ws = dev.full((c.attention_decode_workspace(nb, 1, H, dh, cap),), NAN)
        c.attention_decode_fwd(dev, dev.array(q[b_lo:b_lo + nb]), d, Kc, Vc, S, out, ws, nb, 1, H, dh, cap, scale)
        o = out.numpy()
        assert BT.guard_intact(Kc, n) and BT.guard_intact(Vc, n)
        return Kc, Vc, o

    Kc, Vc, out = run(0, B)
    assert not np.isnan(out).any()
    for b in (0, 3, 8):                                                    # 3: the sample whose cache holds element 2^30; 8: past 2^31
        K1, V1, one = run(b, 1)
        assert np.array_equal(bits(out[b]), bits(one[0])), ("decode, sample %d against B = 1" % b)
        for h in (0, H - 1):
            at = (b * H + h) * cap * dh
            for big, small, first, last in ((Kc, K1, k0, k1), (Vc, V1, v0, v1)):
                got = BT.window(big, at, (T0 + 9) * dh).numpy().reshape(T0 + 9, dh)
                assert np.array_equal(bits(got[:T0]), bits(first[b * T0:(b + 1) * T0, h * dh:(h + 1) * dh])), ("cache rows", b, h)
                assert np.array_equal(bits(got[T0]), bits(last[b, h * dh:(h + 1) * dh])) and np.isnan(got[T0 + 1:]).all(), ("the step's row", b, h)
                assert np.array_equal(bits(got), bits(BT.window(small, h * cap * dh, (T0 + 9) * dh).numpy())), ("B = 1 cache", b, h)
        del K1, V1
        gc.collect()
    tail = BT.window(Kc, total - 64 * dh, 64 * dh).numpy()                 # the last positions of the last head: never written
    assert np.isnan(tail).all()
    del Kc, Vc
    gc.collect()


# ---- KV cache, paged --------------------------------------------------------------------------------------------------------------
def test_kv_cache_paged(dev):
    """Pools of 2^15 + 16 pages of (8, 64, 128) = 2^31 + 2^20 floats each (2^29 + 2^18 units of 16 bytes, inside the vector kernels'
    2^32).  Three samples of 301 positions, five pages each: the table's rows name the last pages of the pool, the pages on both
    sides of elements 2^30 and 2^31, and the first pages; the entries behind a sample's own pages are outside the pool.
    nk_kv_pages_append writes 300 rows and then the step's own; nk_attention_decode_paged_fwd (H = 8 and 16 over Hkv = 8, every key
    and a window of 100) must give the bits of the contiguous entry points on caches of (3, 8, 448, 128) filled by
    nk_kv_cache_append, as tests/test_gpu_attention_paged.py holds it.  Every named page must hold its rows bit for bit and NaN
    behind them; neighbouring pages that no row names, and the guard floats, keep what they held."""
    c = capi()
    B, Hkv, page, dh, T0, max_pages, own = 3, 8, 64, 128, 300, 7, 5
    d, per = Hkv * dh, Hkv * page * dh                                     # floats of a row of K; of a page
    num_pages = (1 << 15) + 16
    total = num_pages * per
    p30, p31 = BT.TWO30 // per, BT.TWO31 // per                            # the pages that begin at elements 2^30 and 2^31
    assert total > BT.TWO31 and num_pages * Hkv * page * (dh // 4) <= 0xffffffff and (T0 + 1 + page - 1) // page == own
    table = np.empty((B, max_pages), np.int32)
    table[0, :own] = [num_pages - 1, num_pages - 3, num_pages - 2, num_pages - 5, num_pages - 4]
    table[1, :own] = [p31, p31 - 1, p30, p30 - 1, 0]
    table[2, :own] = [p31 + 1, 1, num_pages - 6, p30 + 1, p31 - 2]
    table[:, own:] = [[-1, num_pages + 5], [num_pages, -7], [num_pages + 5, -1]]
    named = set(table[:, :own].reshape(-1).tolist())
    assert len(named) == B * own
    quiet = [q for q in (2, p30 + 2, p31 + 2, p31 - 3, num_pages - 7) if q not in named]
    rng = np.random.default_rng(56)
    k0, v0 = (rng.random((B * T0, d), dtype=f32) * f32(2) - f32(1) for _ in range(2))
    k1, v1 = (rng.random((B, d), dtype=f32) * f32(2) - f32(1) for _ in range(2))
    Kp, Vp = BT.guarded(dev, total, NAN), BT.guarded(dev, total, NAN)
    cap = max_pages * page
    Kc, Vc = dev.full((B * Hkv * cap * dh,), NAN), dev.full((B * Hkv * cap * dh,), NAN)
    TAB, ZERO, S = dev.int_array(table), dev.int_array(np.zeros(B, np.int32)), dev.int_array(np.full(B, T0, np.int32))
    K0, V0, K1, V1 = dev.array(k0), dev.array(v0), dev.array(k1), dev.array(v1)
    c.kv_pages_append(dev, Kp, Vp, K0, V0, d, ZERO, TAB, max_pages, B, T0, Hkv, dh, page, num_pages)
    c.kv_pages_append(dev, Kp, Vp, K1, V1, d, S, TAB, max_pages, B, 1, Hkv, dh, page, num_pages)
    c.kv_cache_append(dev, Kc, Vc, K0, V0, d, ZERO, B, T0, Hkv, dh, cap)
    c.kv_cache_append(dev, Kc, Vc, K1, V1, d, S, B, 1, Hkv, dh, cap)
    scale = float(f32(1.0 / np.sqrt(dh)))
    for H in (8, 16):
        Q = dev.array(rng.random((B, H * dh), dtype=f32) * f32(2) - f32(1))
        for W in (0, 100):
            got, want = dev.full((B, H * dh), NAN), dev.full((B, H * dh), NAN)
            ws = dev.full((c.attention_decode_paged_workspace(B, 1, H, dh, max_pages, page, W),), NAN)
            c.attention_decode_paged_fwd(dev, Q, H * dh, Kp, Vp, S, TAB, max_pages, got, ws, B, 1, H, Hkv, dh, page, num_pages, W, scale)
            if W == 0:
                ws = dev.full((c.attention_decode_workspace(B, 1, H, dh, cap),), NAN)
                c.attention_decode_gqa_fwd(dev, Q, H * dh, Kc, Vc, S, want, ws, B, 1, H, Hkv, dh, cap, scale)
            else:
                ws = dev.full((c.attention_decode_window_workspace(B, 1, H, dh, W),), NAN)
                c.attention_decode_window_fwd(dev, Q, H * dh, Kc, Vc, S, want, ws, B, 1, H, Hkv, dh, cap, W, 0, scale)
            got, want = got.numpy(), want.numpy()
            assert np.isfinite(got).all(), ("paged decode", H, W)
            assert np.array_equal(bits(got), bits(want)), ("paged decode against the contiguous twin", H, W, float(np.abs(got - want).max()))
    for pool, first, last in ((Kp, k0, k1), (Vp, v0, v1)):
        for b in range(B):
            rows = np.concatenate([first[b * T0:(b + 1) * T0], last[b:b + 1]]).reshape(T0 + 1, Hkv, dh)     # positions 0 .. 300 of sample b
            for i in range(own):
                got = BT.window(pool, int(table[b, i]) * per, per).numpy().reshape(Hkv, page, dh)
                held = min(page, T0 + 1 - i * page)
                want = rows[i * page:i * page + held].transpose(1, 0, 2)
                assert np.array_equal(bits(got[:, :held]), bits(want)), ("page", b, i, int(table[b, i]))
                assert np.isnan(got[:, held:]).all(), ("slots behind the last row", b, i)
        for q in quiet:
            assert np.isnan(BT.window(pool, q * per, per).numpy()).all(), ("a page that no row names", q)
        assert BT.guard_intact(pool, total)
    del Kp, Vp, Kc, Vc
    gc.collect()


# ---- embedding --------------------------------------------------------------------------------------------------------------------
def test_embedding(dev):
    """2^21 + 3 tokens, D = 1024, V = 50257: the forward's output and the backward's gradient hold 2^31 + 3072 elements.  The ids are
    tiled like the data (id of token r = the tile's id r mod 4099) with ids of their own in the windows' fresh rows.  Forward: a copy,
    window rows bit for bit weight[id].  Backward (assign): dweight against the f64 sum over the tile's rows times their
    multiplicities plus the fresh rows inside the f32 summation bound of its K terms, 48 rows bit for bit in the device's order
    (tests/embedding_oracle.py); rows no id names stay zero."""
    import embedding_oracle as E
    c = capi()
    g = BT.CASES["emb/g"]
    total, D, V = g.total, g.width, 50257
    n = total // D
    rng = np.random.default_rng(66)
    weight = rng.standard_normal((V, D), dtype=f32)
    id_tile = rng.integers(0, V, g.tile_rows)
    ids = id_tile[np.arange(n) % g.tile_rows]
    mult, fresh = BT.multiplicity(g)
    fresh_ids = []
    for lo, data in fresh:
        ids[lo // D:lo // D + data.size // D] = rng.integers(0, V, data.size // D)
        fresh_ids.append(ids[lo // D:lo // D + data.size // D].copy())
    W, I, OUT = dev.array(weight), dev.array(ids.astype(f32)), BT.guarded(dev, total, NAN)
    c.embedding_fwd(dev, W, I, OUT, n, V, D)
    for first, count in BT.marks(total, D):
        got = BT.window(OUT, first * D, count * D).numpy().reshape(count, D)
        assert np.array_equal(bits(got), bits(weight[ids[first:first + count]])), ("embedding forward, tokens %d.." % first)
    assert BT.guard_intact(OUT, total)
    del OUT, W
    gc.collect()
    G, DW = BT.tiled(dev, g), dev.full((V, D), NAN)
    c.embedding_bwd(dev, DW, BT.window(G, 0, total), I, n, V, D, assign=True)
    used, inv = np.unique(np.concatenate([id_tile] + fresh_ids), return_inverse=True)
    acc, mag, terms = np.zeros((used.size, D)), np.zeros((used.size, D)), np.zeros(used.size)
    rows_mult = mult[::D].astype(np.float64)
    tile64 = BT.tile_host(g).reshape(-1, D).astype(np.float64)
    np.add.at(acc, inv[:g.tile_rows], rows_mult[:, None] * tile64)
    np.add.at(mag, inv[:g.tile_rows], rows_mult[:, None] * np.abs(tile64))
    np.add.at(terms, inv[:g.tile_rows], rows_mult)
    at = g.tile_rows
    for (_, data), fi in zip(fresh, fresh_ids):
        d64 = data.reshape(-1, D).astype(np.float64)
        np.add.at(acc, inv[at:at + fi.size], d64)
        np.add.at(mag, inv[at:at + fi.size], np.abs(d64))
        np.add.at(terms, inv[at:at + fi.size], 1.0)
        at += fi.size
    assert int(terms.sum()) == n
    dw = DW.numpy()
    # every named row: an f32 sum of K terms in any order is within (K - 1) * 2^-24 * sum |term| of the exact sum, to first order
    # (the second-order part is below 1e-4 of it at K <= 2^11); a lost or doubled contribution is a whole term, about 1, in 1024 columns
    err, bound = np.abs(dw[used] - acc), (terms[:, None] - 1) * 2.0 ** -24 * mag * (1 + 1e-4)
    assert (err <= bound).all(), ("embedding dweight", float(err.max()), float((err / np.maximum(bound, 1e-30)).max()))
    # 48 named rows, the fresh rows' ids among them, bit for bit in the device's order (the family's tolerance): the tokens that name
    # them, in ascending position, through embedding_oracle.row_sums with the ids renumbered 0 .. 47
    some = np.unique(np.concatenate([fresh_ids[1][:8], fresh_ids[2][:8], id_tile[:32]]))
    tokens = np.flatnonzero(np.isin(ids, some))
    g_sub = BT.expect_at(g, tokens[:, None] * D + np.arange(D, dtype=np.int64)[None, :])
    want, touched = E.row_sums(g_sub, np.searchsorted(some, ids[tokens]).astype(f32), some.size)
    assert touched.all() and np.array_equal(bits(dw[some]), bits(want)), "embedding dweight: the device's summation order"
    rest = np.ones(V, bool)
    rest[used] = False
    assert not dw[rest].any(), "rows that no id names"
    assert BT.guard_intact(G, total)
    del G, DW, I
    gc.collect()


# ---- sampling ---------------------------------------------------------------------------------------------------------------------
def test_sampling(dev):
    """2049 rows of V = ld = 2^20 logits (2^31 + 2^20 floats), `dominant` rows of tests/sampling_cases.py: greedy, and temperature 1
    with one Philox draw per row.  The id of every window row must equal the id of the same row drawn alone as row r of a call whose
    other rows are zeros (tests/test_gpu_sampling.py::test_a_row_keeps_its_id_whatever_surrounds_it); greedy is also the host's argmax.
    A row offset r * ld that wraps reads zeros there and other logits here."""
    c = capi()
    x = BT.CASES["sampling/x"]
    n, V = x.total, x.width
    rows = n // V
    X, ALONE = BT.tiled(dev, x), BT.alloc(dev, n)
    seed, offset = 0xABCDEF0123, 2 ** 33 + 7
    picked = [r for first, count in BT.marks(n, V) for r in range(first, first + count)]
    host = {r: BT.expect_host(x, r * V, V) for r in picked}
    for name, T, k, p in (("greedy", 0.0, 0, 1.0), ("T1", 1.0, 0, 1.0)):
        IDS = dev.full((rows,), NAN)
        c.sample_fwd(dev, BT.window(X, 0, n), V, rows, V, IDS, T, k, p, seed, offset)
        ids = IDS.numpy()
        assert not np.isnan(ids).any()
        for r in picked:
            row = BT.window(ALONE, r * V, V)
            c.check(c.lib.nk_copy(dev.h, row.p, BT.window(X, r * V, V).p, V))
            ONE = dev.full((r + 1,), NAN)
            c.sample_fwd(dev, ALONE, V, r + 1, V, ONE, T, k, p, seed, offset)
            assert ONE.numpy()[r] == ids[r], (name, r, ONE.numpy()[r], ids[r])
            if name == "greedy":
                assert ids[r] == np.argmax(host[r]), (name, r)
            row.fill(0.0)
    assert BT.guard_intact(X, n)
    del X, ALONE, IDS, ONE
    gc.collect()


# ---- transpose --------------------------------------------------------------------------------------------------------------------
def test_transpose_2d(dev):
    """(2^16 + 1) x 2^15 -> 2^15 x (2^16 + 1): 2^31 + 32768 elements; window rows of the output against the host image of the input's
    columns (a copy: bit for bit)"""
    c = capi()
    x = BT.CASES["transpose/x"]
    n, C = x.total, x.width
    R = n // C
    X, OUT = build(dev, n, x), build(dev, n, NAN)
    c.transpose_fwd(dev, shaped(BT.window(X, 0, n), R, C), shaped(BT.window(OUT, 0, n), C, R))
    for first, count in BT.marks(n, R):                                     # rows of the output hold R floats
        got = BT.window(OUT, first * R, count * R).numpy().reshape(count, R)
        want = BT.expect_at(x, np.arange(R, dtype=np.int64)[None, :] * C + np.arange(first, first + count, dtype=np.int64)[:, None])
        assert np.array_equal(bits(got), bits(want)), ("transpose, output rows %d.." % first)
    assert BT.guard_intact(OUT, n) and BT.guard_intact(X, n)
    del X, OUT
    gc.collect()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _refused(call):
    c = capi()
    with pytest.raises(c.NeuronikaHipError) as e:
        call()
    assert e.value.code == 1, e.value                                       # NK_ERR_INVALID


def test_refusals_one_past_the_limit(dev):
    """GLU (rows * 2 H <= 2^31 - 1 elements), rope (B * T <= 2^31 - 1 rows; max_pos * rot <= 2^31 - 1 table entries), cross entropy
    (2^31 - 1 positions), batch norm (N * L <= 2^31 - 1 values per channel) and pooling (a plane of at most 2^31 - 1 elements), each one
    past its limit with small real buffers: NK_ERR_INVALID and the marked outputs untouched."""
    c = capi()
    mark = np.full(4096, 3.25, f32)
    A, OUT = dev.array(np.ones(4096, f32)), dev.array(mark)

    def untouched(what):
        assert np.array_equal(OUT.numpy(), mark), what

    # GLU: GLU_MAX_ELEMS = 2^31 - 1 elements of x; (2^20, 2 * 1024) is 2^31
    for H, rows in ((1024, 1 << 20), (1, 1 << 30)):
        _refused(lambda: c.glu_fwd(dev, "silu", A, OUT, rows, H))
        untouched("glu_fwd")
        for assign in (False, True):
            _refused(lambda: c.glu_bwd(dev, "silu", OUT, A, A, rows, H, assign=assign))
            untouched("glu_bwd")
    # rope: B * T = 2^31 rows
    table = dev.zeros((4, 4, 2))
    c.rope_table(dev, table, 4, 8)
    st = dev.int_array(np.zeros(4, np.int32))
    _refused(lambda: c.rope_fwd(dev, A, 8, OUT, 8, table, st, 1 << 16, 1 << 15, 1, 8, 8, 4, False))
    untouched("rope_fwd")
    for assign in (False, True):
        _refused(lambda: c.rope_bwd(dev, OUT, 8, A, 8, table, st, 1 << 16, 1 << 15, 1, 8, 8, 4, False, assign=assign))
        untouched("rope_bwd")
    _refused(lambda: c.rope_table(dev, OUT, 1 << 30, 2))                    # 2^31 entries
    untouched("rope_table")
    # cross entropy: N * inner = 2^31 positions
    LSE = dev.array(mark)
    _refused(lambda: c.cross_entropy_fwd(dev, A, A, LSE, OUT, (1 << 16, 2, 1 << 15), "mean"))
    untouched("cross_entropy_fwd")
    assert np.array_equal(LSE.numpy(), mark)
    for assign in (False, True):
        _refused(lambda: c.cross_entropy_bwd(dev, OUT, A, A, A, LSE, (1 << 16, 2, 1 << 15), "mean", assign=assign))
        untouched("cross_entropy_bwd")
    # batch norm: N * L = 2^31 values per channel
    P = dev.array(np.ones(8, f32))
    _refused(lambda: c.batch_norm_fwd(dev, A, P, P, OUT, None, None, None, 1 << 16, 1, 1 << 15))
    untouched("batch_norm_fwd")
    _refused(lambda: c.batch_norm_infer_fwd(dev, A, P, P, P, P, OUT, None, 1 << 16, 1, 1 << 15))
    untouched("batch_norm_infer_fwd")
    _refused(lambda: c.batch_norm_bwd(dev, OUT, A, None, P, P, None, 1 << 16, 1, 1 << 15))
    untouched("batch_norm_bwd")
    # pooling: a plane of 2^31 elements
    plane = (1, 1, 1 << 16, 1 << 15)
    IDX = dev.int_array(np.full(4096, 5, np.int32))
    _refused(lambda: c.max_pool_fwd(dev, A, plane, OUT, IDX, (2, 2), (2, 2), (0, 0)))
    untouched("max_pool_fwd")
    assert (IDX.numpy() == 5).all()
    _refused(lambda: c.avg_pool_fwd(dev, A, plane, OUT, (2, 2), (2, 2), (0, 0)))
    untouched("avg_pool_fwd")
    for assign in (False, True):
        _refused(lambda: c.max_pool_bwd(dev, OUT, plane, A, IDX, (2, 2), (2, 2), (0, 0), assign=assign))
        untouched("max_pool_bwd")
        _refused(lambda: c.avg_pool_bwd(dev, OUT, plane, A, (2, 2), (2, 2), (0, 0), assign=assign))
        untouched("avg_pool_bwd")
    del A, OUT, LSE, table, st, P, IDX
    gc.collect()


def test_refusals_decode_and_paged(dev):
    """The decode family's limits, one past each with small real buffers.  B * T * H = 2^24 problems (the limit is below 2^24) and
    H * dh = 2^31 (it must fit 31 bits) through both appends, the three contiguous attention entries, the paged append and the paged
    attention; H * dh = 2^31 through nk_kv_pages_copy, which has that limit alone.  The paged attention's vector kernels keep a key's
    pool offset in 32 bits of 16-byte units: 2^18 pages of (8, 64, 128) are 2^32 units, one past.  NK_ERR_INVALID every time, the
    marked outputs, caches and workspace untouched."""
    c = capi()
    mark = np.full(4096, 3.25, f32)
    A, OUT, WS, KC, VC = dev.array(np.ones(4096, f32)), dev.array(mark), dev.array(mark), dev.array(mark), dev.array(mark)
    ST, TAB = dev.int_array(np.zeros(4096, np.int32)), dev.int_array(np.zeros(4096, np.int32))

    def untouched(what):
        for a in (OUT, WS, KC, VC):
            assert np.array_equal(a.numpy(), mark), what

    for what, (B, T, H, dh) in (("B*T*H", (1 << 12, 1 << 6, 1 << 6, 4)), ("H*dh", (1, 1, 1 << 16, 1 << 15))):
        for append in (c.kv_cache_append, c.kv_cache_append_ring):
            _refused(lambda: append(dev, KC, VC, A, A, 8, ST, B, T, H, dh, 64))
            untouched(what + " append")
        _refused(lambda: c.attention_decode_fwd(dev, A, 8, KC, VC, ST, OUT, WS, B, T, H, dh, 64, 0.5))
        untouched(what + " decode")
        _refused(lambda: c.attention_decode_gqa_fwd(dev, A, 8, KC, VC, ST, OUT, WS, B, T, H, H // 2, dh, 64, 0.5))
        untouched(what + " gqa decode")
        _refused(lambda: c.attention_decode_window_fwd(dev, A, 8, KC, VC, ST, OUT, WS, B, T, H, H // 2, dh, 64, 16, 0, 0.5))
        untouched(what + " window decode")
        _refused(lambda: c.kv_pages_append(dev, KC, VC, A, A, 8, ST, TAB, 4, B, T, H, dh, 16, 8))
        untouched(what + " paged append")
        _refused(lambda: c.attention_decode_paged_fwd(dev, A, 8, KC, VC, ST, TAB, 4, OUT, WS, B, T, H, H // 2, dh, 16, 8, 0, 0.5))
        untouched(what + " paged decode")
    src, dst = dev.int_array(np.array([0], np.int32)), dev.int_array(np.array([1], np.int32))
    _refused(lambda: c.kv_pages_copy(dev, KC, VC, src, dst, 1, 1 << 16, 1 << 15, 16, 8))
    untouched("H*dh pages copy")
    # the pool: num_pages * Hkv * page * (dh / 4) = 2^18 * 8 * 64 * 32 = 2^32 units; everything else about the call is in order
    B, H, Hkv, dh, page, max_pages = 1, 8, 8, 128, 64, 4
    assert (1 << 18) * Hkv * page * (dh // 4) == 1 << 32 and B * H * dh <= A.size
    for W in (0, 16):
        _refused(lambda: c.attention_decode_paged_fwd(dev, A, H * dh, KC, VC, ST, TAB, max_pages, OUT, WS, B, 1, H, Hkv, dh, page, 1 << 18, W, 0.5))
        untouched("a pool of 2^32 units, window %d" % W)
    del A, OUT, WS, KC, VC, ST, TAB, src, dst
    gc.collect()

"""nk_layer_norm_* through the C ABI (`capi`) against tests/layernorm_oracle.py.  y, stats and dx under the suite's rule
err_gpu <= max(2 * err_cpu32, 1e-6 * scale) against the f64 oracle (margins recorded as `layernorm:*`); dgamma and dbeta, sums
over the rows, through tolerance.assert_contraction with K = rows."""
import numpy as np
import pytest

import layernorm_oracle as LN
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu

EPS = 1e-5


def _check(got, want, want32, what, scale=None):
    from conftest import record_margin
    scale = float(np.abs(want).max()) if scale is None else scale
    err_gpu, err_cpu = float(np.abs(got - want).max()), float(np.abs(want32 - want).max())
    record_margin("layernorm:" + what, err_gpu, err_cpu, 1e-6 * scale)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)


def _inputs(rows, D, seed, affine=True):
    """Rows of a known spread (a shuffled ramp over [-1, 1] plus noise): the conditioning of a row is its own subject below."""
    rng = np.random.default_rng(seed)
    ramp = np.linspace(-1.0, 1.0, D) if D > 1 else np.zeros(1)
    x = (rng.permuted(np.tile(ramp, (rows, 1)), axis=1) + 0.25 * rng.standard_normal((rows, D)) + rng.standard_normal((rows, 1))).astype(np.float32)
    g = rng.standard_normal((rows, D)).astype(np.float32)
    gamma = (1.0 + 0.5 * rng.standard_normal(D)).astype(np.float32) if affine else None
    beta = rng.standard_normal(D).astype(np.float32) if affine else None
    return x, g, gamma, beta


def _device_run(dev, c, x, g, gamma, beta, assign, init, eps=EPS):
    """forward, dx, parameter gradients; `init` = (dx0, dgamma0, dbeta0) the outputs hold before the call"""
    rows, D = x.shape
    X, G = dev.array(x), dev.array(g)
    W, B = (dev.array(gamma) if gamma is not None else None), (dev.array(beta) if beta is not None else None)
    Y, S = dev.full((rows, D), np.nan), dev.full((rows, 2), np.nan)
    c.layer_norm_fwd(dev, X, W, B, Y, S, rows, D, eps)
    DX, DG, DB = (dev.array(a) for a in init)
    c.layer_norm_bwd(dev, DX, G, X, W, S, rows, D, assign=assign)
    c.layer_norm_bwd_params(dev, DG, DB, G, X, S, rows, D, assign=assign)
    return dict(y=Y.numpy(), stats=S.numpy(), dx=DX.numpy(), dgamma=DG.numpy(), dbeta=DB.numpy())


ROWS = (1, 3, 64, 1000, 4097)
DS = (1, 2, 3, 4, 5, 31, 64, 100, 256, 260, 512, 768, 1024, 1027, 2048, 2052, 4096, 8192, 16384, 20000)
# the product, thinned: every D at 3 and 64 rows, the other row counts at the D that change the kernel or the row split
EXTRA = {1: (1, 4, 1027, 16384), 1000: (5, 64, 768, 1024, 2048, 4096, 20000), 4097: (3, 256, 1024, 1027, 4096)}
GRID = [(r, D) for D in DS for r in ROWS if r in (3, 64) or D in EXTRA[r]]


@pytest.mark.parametrize("rows,D", GRID)
def test_parity_grid(dev, rows, D):
    from neuronika_amd import capi as c
    for affine in (True, False):
        x, g, gamma, beta = _inputs(rows, D, rows * 100003 + D, affine)
        o64, o32 = LN.both(x, gamma, beta, g, EPS)
        rng = np.random.default_rng(7)
        for assign in (False, True):
            # accumulate into data, assign over NaN
            init = [np.full(s, np.nan, np.float32) if assign else rng.standard_normal(s).astype(np.float32) for s in ((rows, D), (D,), (D,))]
            got = _device_run(dev, c, x, g, gamma, beta, assign, init)
            tag = "%s/%s" % ("affine" if affine else "plain", "assign" if assign else "accumulate")
            _check(got["y"], o64["y"], o32["y"], "y " + tag)
            _check(got["stats"], o64["stats"], o32["stats"], "stats " + tag)
            base = [np.zeros_like(a) if assign else a for a in init]
            _check(got["dx"], base[0] + o64["dx"], base[0] + o32["dx"], "dx " + tag)
            for name, b in (("dgamma", base[1]), ("dbeta", base[2])):
                assert_contraction("layernorm:%s %s" % (name, tag), got[name], b + o64[name], rows, np.abs(g).max(),
                                   max(1.0, np.abs(o64["y"]).max()) if name == "dgamma" else 1.0, cpu32=b + o32[name], epilogue=not assign)


def test_offset_rows_need_the_centred_second_pass(dev):
    """x = 1e4 + noise: E[x^2] - mean^2 in f32 loses the variance entirely (x^2 ~ 1e8 at an ulp of 8); the centred second pass
    keeps it.  The absolute term is taken at the inputs' magnitude, 1e-6 * max|x|: centring rounds at ulp(|x|)."""
    from neuronika_amd import capi as c
    for rows, D in ((64, 1024), (16, 4096), (9, 1027)):
        rng = np.random.default_rng(D)
        x = (1e4 + rng.standard_normal((rows, D))).astype(np.float32)
        g = rng.standard_normal((rows, D)).astype(np.float32)
        gamma, beta = (1.0 + 0.5 * rng.standard_normal(D)).astype(np.float32), rng.standard_normal(D).astype(np.float32)
        o64, o32 = LN.both(x, gamma, beta, g, EPS)
        got = _device_run(dev, c, x, g, gamma, beta, True, [np.zeros((rows, D), np.float32), np.zeros(D, np.float32), np.zeros(D, np.float32)])
        assert np.abs(o64["stats"][:, 1] - 1.0).max() < 0.2                        # the rows' deviation is 1: rstd near 1
        for name in ("y", "stats", "dx"):
            _check(got[name], o64[name], o32[name], "offset " + name, scale=float(np.abs(x).max()))


def test_constant_row_and_single_element_rows(dev):
    from neuronika_amd import capi as c
    for D in (8, 100, 1024, 4096):
        x = np.full((3, D), -7.25, np.float32)
        g = np.random.default_rng(D).standard_normal((3, D)).astype(np.float32)
        gamma, beta = np.full(D, 2.0, np.float32), np.full(D, 0.5, np.float32)
        got = _device_run(dev, c, x, g, gamma, beta, True, [np.zeros((3, D), np.float32), np.zeros(D, np.float32), np.zeros(D, np.float32)])
        assert np.array_equal(got["y"], np.full((3, D), 0.5, np.float32))         # xhat = 0 exactly: y = beta
        assert np.array_equal(got["stats"][:, 0], np.full(3, -7.25, np.float32))
        np.testing.assert_allclose(got["stats"][:, 1], 1.0 / np.sqrt(EPS), rtol=1e-6)
        assert np.isfinite(got["dx"]).all() and np.array_equal(got["dgamma"], np.zeros(D, np.float32))
    # D = 1: y = beta, dx += 0, dbeta = sum of g
    rows = 1000
    x, g, gamma, beta = _inputs(rows, 1, 11)
    dx0 = np.random.default_rng(3).standard_normal((rows, 1)).astype(np.float32)
    got = _device_run(dev, c, x, g, gamma, beta, False, [dx0, np.zeros(1, np.float32), np.zeros(1, np.float32)])
    assert np.array_equal(got["y"], np.full((rows, 1), beta[0], np.float32))
    assert np.array_equal(got["dx"], dx0) and got["dgamma"][0] == 0.0
    assert_contraction("layernorm:dbeta D=1", got["dbeta"], g.astype(np.float64).sum(0), rows, np.abs(g).max(), 1.0, cpu32=g.sum(0, dtype=np.float32))


@pytest.mark.parametrize("D", [100, 256, 2048, 4096, 20000])
def test_nan_row_stays_inside_its_row(dev, D):
    """a NaN in one row: that row's results are NaN, its neighbours' are bit for bit what they are without it"""
    from neuronika_amd import capi as c
    rows = 9
    x, g, gamma, beta = _inputs(rows, D, D)
    zero = [np.zeros((rows, D), np.float32), np.zeros(D, np.float32), np.zeros(D, np.float32)]
    clean = _device_run(dev, c, x, g, gamma, beta, True, zero)
    xn = x.copy()
    xn[4, D // 2] = np.nan
    got = _device_run(dev, c, xn, g, gamma, beta, True, zero)
    keep = np.arange(rows) != 4
    for name in ("y", "stats", "dx"):
        assert np.array_equal(got[name][keep], clean[name][keep]), name
        assert np.isnan(got[name][4]).all(), name
    assert np.isnan(got["dgamma"]).all()                                           # every column sums over the NaN row's xhat
    assert np.array_equal(got["dbeta"], clean["dbeta"])                            # dbeta does not read x


@pytest.mark.parametrize("rows,D,lead", [(5, 1027, 4), (64, 5, 4), (3, 31, 3), (7, 1024, 4), (7, 1024, 1), (4, 4096, 2), (3, 20000, 4)])
def test_guard_words_stay_intact(dev, rows, D, lead):
    """`lead` guard floats before and 5 after every output (lead = 4 keeps 16-byte alignment, other values take it away: the
    row-in-registers kernels must not be chosen then)"""
    from neuronika_amd import capi as c
    x, g, gamma, beta = _inputs(rows, D, 99)
    o64, o32 = LN.both(x, gamma, beta, g, EPS)
    GUARD = np.float32(-12345.5)

    def guarded(n):
        buf = dev.full((lead + n + 5,), float(GUARD))
        return buf, buf.view_offset(lead)

    X, G, W, B = dev.array(x), dev.array(g), dev.array(gamma), dev.array(beta)
    bufs = {name: guarded(n) for name, n in (("y", rows * D), ("stats", rows * 2), ("dx", rows * D), ("dgamma", D), ("dbeta", D))}
    c.layer_norm_fwd(dev, X, W, B, bufs["y"][1], bufs["stats"][1], rows, D, EPS)
    c.layer_norm_bwd(dev, bufs["dx"][1], G, X, W, bufs["stats"][1], rows, D, assign=True)
    c.layer_norm_bwd_params(dev, bufs["dgamma"][1], bufs["dbeta"][1], G, X, bufs["stats"][1], rows, D, assign=True)
    for name, (buf, _) in bufs.items():
        h = buf.numpy()
        assert (h[:lead] == GUARD).all() and (h[-5:] == GUARD).all(), name
        body = h[lead:-5].reshape(o64[name].shape)
        if name in ("y", "stats", "dx"):
            _check(body, o64[name], o32[name], "guarded " + name)
        else:
            assert_contraction("layernorm:guarded " + name, body, o64[name], rows, np.abs(g).max(), max(1.0, np.abs(o64["y"]).max()), cpu32=o32[name])


def test_optional_pointers_and_empty_input(dev):
    from neuronika_amd import capi as c
    rows, D = 37, 768
    x, g, gamma, beta = _inputs(rows, D, 5)
    X, G, W, B = dev.array(x), dev.array(g), dev.array(gamma), dev.array(beta)
    full = _device_run(dev, c, x, g, gamma, beta, True, [np.zeros((rows, D), np.float32), np.zeros(D, np.float32), np.zeros(D, np.float32)])
    S = dev.array(full["stats"])
    # no stats: the same y
    Y = dev.zeros((rows, D))
    c.layer_norm_fwd(dev, X, W, B, Y, None, rows, D, EPS)
    assert np.array_equal(Y.numpy(), full["y"])
    # gamma alone, beta alone, neither: y = xhat * gamma, xhat + beta, xhat
    xhat = dev.zeros((rows, D)); c.layer_norm_fwd(dev, X, None, None, xhat, None, rows, D, EPS)
    o64, o32 = LN.both(x, None, None, g, EPS)
    _check(xhat.numpy(), o64["y"], o32["y"], "y no affine")
    c.layer_norm_fwd(dev, X, W, None, Y, None, rows, D, EPS)
    assert np.array_equal(Y.numpy(), xhat.numpy() * gamma)
    c.layer_norm_fwd(dev, X, None, B, Y, None, rows, D, EPS)
    np.testing.assert_allclose(Y.numpy(), xhat.numpy() + beta, rtol=1e-6, atol=1e-6)   # (the device may fuse the multiply and the add)
    # dx without gamma
    DX = dev.full((rows, D), np.nan); c.layer_norm_bwd(dev, DX, G, X, None, S, rows, D, assign=True)
    _check(DX.numpy(), o64["dx"], o32["dx"], "dx no affine")
    # one parameter output at a time: the same bits as both together, the other buffer untouched
    DG, DB = dev.full((D,), np.nan), dev.full((D,), 3.0)
    c.layer_norm_bwd_params(dev, DG, None, G, X, S, rows, D, assign=True)
    assert np.array_equal(DG.numpy(), full["dgamma"])
    c.layer_norm_bwd_params(dev, None, DB, G, X, S, rows, D, assign=False)
    assert np.array_equal(DB.numpy(), np.float32(3.0) + full["dbeta"])
    # rows = 0: NK_OK, nothing written
    Y.fill(5.0); DG.fill(5.0)
    c.layer_norm_fwd(dev, X, W, B, Y, S, 0, D, EPS)
    c.layer_norm_bwd(dev, Y, G, X, W, S, 0, D, assign=True)
    c.layer_norm_bwd_params(dev, DG, DB, G, X, S, 0, D, assign=True)
    assert (Y.numpy() == 5.0).all() and (DG.numpy() == 5.0).all()


def test_rejections(dev):
    from neuronika_amd import capi as c
    A = dev.zeros((4, 8))
    S, P = dev.zeros((4, 2)), dev.zeros((8,))
    bad = [lambda: c.layer_norm_fwd(dev, A, P, P, A, S, 4, 0, EPS), lambda: c.layer_norm_fwd(dev, A, P, P, A, S, 4, -8, EPS),
           lambda: c.layer_norm_fwd(dev, A, P, P, A, S, -1, 8, EPS), lambda: c.layer_norm_fwd(dev, A, P, P, A, S, 4, 8, -1e-5),
           lambda: c.layer_norm_fwd(dev, A, P, P, A, S, 4, 8, float("nan")), lambda: c.layer_norm_fwd(dev, A, P, P, A, S, 4, 8, float("inf")),
           lambda: c.layer_norm_fwd(dev, None, P, P, A, S, 4, 8, EPS), lambda: c.layer_norm_fwd(dev, A, P, P, None, S, 4, 8, EPS)]
    for assign in (False, True):
        bad += [lambda a=assign: c.layer_norm_bwd(dev, None, A, A, P, S, 4, 8, assign=a), lambda a=assign: c.layer_norm_bwd(dev, A, None, A, P, S, 4, 8, assign=a),
                lambda a=assign: c.layer_norm_bwd(dev, A, A, None, P, S, 4, 8, assign=a), lambda a=assign: c.layer_norm_bwd(dev, A, A, A, P, None, 4, 8, assign=a),
                lambda a=assign: c.layer_norm_bwd(dev, A, A, A, P, S, 4, 0, assign=a), lambda a=assign: c.layer_norm_bwd(dev, A, A, A, P, S, -2, 8, assign=a),
                lambda a=assign: c.layer_norm_bwd_params(dev, None, None, A, A, S, 4, 8, assign=a), lambda a=assign: c.layer_norm_bwd_params(dev, P, P, None, A, S, 4, 8, assign=a),
                lambda a=assign: c.layer_norm_bwd_params(dev, P, P, A, None, S, 4, 8, assign=a), lambda a=assign: c.layer_norm_bwd_params(dev, P, P, A, A, None, 4, 8, assign=a),
                lambda a=assign: c.layer_norm_bwd_params(dev, P, P, A, A, S, 4, 0, assign=a), lambda a=assign: c.layer_norm_bwd_params(dev, P, P, A, A, S, -1, 8, assign=a)]
    for call in bad:
        with pytest.raises(c.NeuronikaHipError) as e:
            call()
        assert str(e.value)                                                        # nk_last_error says why
    dev.sync()


@pytest.mark.parametrize("rows,D", [(32768, 1024), (1000, 1027)])
def test_results_repeat_bit_for_bit(dev, rows, D):
    from neuronika_amd import capi as c
    rng = np.random.default_rng(1)
    x, g = rng.standard_normal((rows, D), dtype=np.float32), rng.standard_normal((rows, D), dtype=np.float32)
    gamma, beta = rng.standard_normal(D, dtype=np.float32), rng.standard_normal(D, dtype=np.float32)
    X, G, W, B = dev.array(x), dev.array(g), dev.array(gamma), dev.array(beta)
    runs = []
    for _ in range(3):
        Y, S, DX, DG, DB = dev.zeros((rows, D)), dev.zeros((rows, 2)), dev.zeros((rows, D)), dev.zeros((D,)), dev.zeros((D,))
        c.layer_norm_fwd(dev, X, W, B, Y, S, rows, D, EPS)
        c.layer_norm_bwd(dev, DX, G, X, W, S, rows, D, assign=True)
        c.layer_norm_bwd_params(dev, DG, DB, G, X, S, rows, D, assign=True)
        runs.append([a.numpy() for a in (Y, S, DX, DG, DB)])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b)
    assert np.isfinite(runs[0][3]).all() and np.abs(runs[0][3]).max() > 0

"""nk_batch_norm_* through the C ABI (`capi`) against tests/batchnorm_oracle.py, over the three layout classes (planes, columns,
generic).  y, stats, the running statistics and dx under the suite's rule err_gpu <= max(2 * err_cpu32, 1e-6 * scale) against
the f64 oracle (margins recorded as `batchnorm:*`); the channel sums, dgamma and dbeta through tolerance.assert_contraction with
K = N * L."""
import numpy as np
import pytest

import batchnorm_oracle as BN
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1


def _check(got, want, want32, what, scale=None):
    from conftest import record_margin
    scale = float(np.abs(want).max()) if scale is None else scale
    err_gpu, err_cpu = float(np.abs(got - want).max()), float(np.abs(want32 - want).max())
    record_margin("batchnorm:" + what, err_gpu, err_cpu, 1e-6 * scale)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)


def _inputs(N, C, L, seed, affine=True):
    """channels of a known spread (unit noise) around their own offset and scale"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, C, L)) * (0.5 + rng.random((1, C, 1))) + rng.standard_normal((1, C, 1))).astype(np.float32)
    g = rng.standard_normal((N, C, L)).astype(np.float32)
    gamma = (1.0 + 0.5 * rng.standard_normal(C)).astype(np.float32) if affine else None
    beta = rng.standard_normal(C).astype(np.float32) if affine else None
    running = (rng.standard_normal(C).astype(np.float32), (0.5 + rng.random(C)).astype(np.float32))
    return x, g, gamma, beta, running


def _opt(dev, a):
    return dev.array(a) if a is not None else None


def _device_run(dev, c, x, g, gamma, beta, running, assign, init, training=True, eps=EPS):
    """forward, sums, dx, parameter gradients; `init` = (dx0, dgamma0, dbeta0) the outputs hold before the call"""
    N, C, L = x.shape
    X, G, W, B = dev.array(x), dev.array(g), _opt(dev, gamma), _opt(dev, beta)
    RM, RV = dev.array(running[0]), dev.array(running[1])
    Y, S, SUMS = dev.full((N, C, L), np.nan), dev.full((C, 2), np.nan), dev.full((C, 2), np.nan)
    if training:
        c.batch_norm_fwd(dev, X, W, B, Y, S, RM, RV, N, C, L, eps, MOM)
    else:
        c.batch_norm_infer_fwd(dev, X, W, B, RM, RV, Y, S, N, C, L, eps)
    DX, DG, DB = (dev.array(a) for a in init)
    c.batch_norm_bwd_sums(dev, SUMS, G, X, S, N, C, L)
    c.batch_norm_bwd(dev, DX, G, X, W, S, SUMS if training else None, N, C, L, assign=assign)
    c.batch_norm_bwd_params(dev, DG, DB, SUMS, C, assign=assign)
    return dict(y=Y.numpy(), stats=S.numpy(), running_mean=RM.numpy(), running_var=RV.numpy(), sums=SUMS.numpy(), dx=DX.numpy(),
                dgamma=DG.numpy(), dbeta=DB.numpy())


def _compare(got, o64, o32, x, g, gamma, tag, base=None, epilogue=False, training=True):
    N, C, L = x.shape
    base = base or [0.0, 0.0, 0.0]
    _check(got["y"], o64["y"], o32["y"], "y " + tag)
    _check(got["stats"][:, 0], o64["stats"][:, 0], o32["stats"][:, 0], "mean " + tag, scale=float(np.abs(x).max()))
    _check(got["stats"][:, 1], o64["stats"][:, 1], o32["stats"][:, 1], "rstd " + tag)
    for name in ("running_mean", "running_var"):
        _check(got[name], o64[name], o32[name], name + " " + tag, scale=max(1.0, float(np.abs(o64[name]).max())))
    ch = lambda v: np.asarray(v, np.float64).reshape(1, C, 1)
    xh = (x - ch(o64["stats"][:, 0])) * ch(o64["stats"][:, 1])
    xhat = max(1.0, float(np.abs(xh).max()))
    # dx is a difference of three terms (two elements of a channel of two cancel almost entirely): its scale is the terms' magnitude
    gr = ch(o64["stats"][:, 1]) * (np.abs(ch(gamma)) if gamma is not None else 1.0)
    terms = np.abs(g) + (np.abs(ch(o64["sums"][:, 0])) + np.abs(xh) * np.abs(ch(o64["sums"][:, 1]))) / (N * L) if training else np.abs(g)
    dx_scale = float((gr * terms).max())
    gmax = float(np.abs(g).max())
    assert_contraction("batchnorm:s0 " + tag, got["sums"][:, 0], o64["sums"][:, 0], N * L, gmax, 1.0, cpu32=o32["sums"][:, 0])
    assert_contraction("batchnorm:s1 " + tag, got["sums"][:, 1], o64["sums"][:, 1], N * L, gmax, xhat, cpu32=o32["sums"][:, 1])
    _check(got["dx"], base[0] + o64["dx"], base[0] + o32["dx"], "dx " + tag, scale=dx_scale)
    assert_contraction("batchnorm:dgamma " + tag, got["dgamma"], base[1] + o64["dgamma"], N * L, gmax, xhat, cpu32=base[1] + o32["dgamma"], epilogue=epilogue)
    assert_contraction("batchnorm:dbeta " + tag, got["dbeta"], base[2] + o64["dbeta"], N * L, gmax, 1.0, cpu32=base[2] + o32["dbeta"], epilogue=epilogue)


# planes: L % 4 == 0, L >= 256; columns: L == 1 (C % 4 == 0 vectorised, else scalar); generic: the rest
GRID = [(64, 256, 1), (1, 8, 4096), (8, 3, 49), (5, 7, 3), (16, 64, 3136), (4, 1, 1024), (1, 5, 300), (2, 1, 1), (3, 6, 1), (1000, 7, 1),
        (37, 260, 1), (300, 4, 256), (2, 2, 260), (9, 2, 5000), (2, 3, 1200000), (4097, 128, 1), (3, 2, 252)]


@pytest.mark.parametrize("N,C,L", GRID)
def test_parity_grid(dev, N, C, L):
    from neuronika_amd import capi as c
    for affine in (True, False):
        x, g, gamma, beta, running = _inputs(N, C, L, N * 100003 + C * 101 + L, affine)
        o64, o32 = BN.both(x, gamma, beta, g, EPS, MOM, running)
        rng = np.random.default_rng(7)
        for assign in (False, True):
            # accumulate into data, assign over NaN
            init = [np.full(s, np.nan, np.float32) if assign else rng.standard_normal(s).astype(np.float32) for s in ((N, C, L), (C,), (C,))]
            got = _device_run(dev, c, x, g, gamma, beta, running, assign, init)
            tag = "%s/%s" % ("affine" if affine else "plain", "assign" if assign else "accumulate")
            _compare(got, o64, o32, x, g, gamma, tag, [np.zeros_like(a) if assign else a for a in init], epilogue=not assign)


@pytest.mark.parametrize("N,C,L", [(16, 8, 3136), (8, 3, 49), (64, 256, 1), (5, 7, 3), (3, 4, 1024)])
def test_pointers_offset_by_one_float_and_guard_words(dev, N, C, L):
    """every tensor starts one float past a 16-byte boundary (the float4 kernels must not be chosen), with guard floats before
    and after every output"""
    from neuronika_amd import capi as c
    x, g, gamma, beta, running = _inputs(N, C, L, 99)
    o64, o32 = BN.both(x, gamma, beta, g, EPS, MOM, running)
    GUARD = np.float32(-12345.5)
    lead = 5                                                                       # 4 guard floats keep alignment, the fifth takes it away

    def guarded(n, fill=None):
        buf = dev.full((lead + n + 5,), float(GUARD))
        if fill is not None:
            h = buf.numpy(); h[lead:lead + n] = fill.ravel(); buf = dev.array(h)
        return buf, buf.view_offset(lead)

    X, G = guarded(x.size, x), guarded(g.size, g)
    W, B = dev.array(gamma), dev.array(beta)
    outs = {name: guarded(n, fill) for name, n, fill in (("y", x.size, None), ("stats", 2 * C, None), ("sums", 2 * C, None), ("dx", x.size, None),
                                                         ("dgamma", C, None), ("dbeta", C, None), ("running_mean", C, running[0]),
                                                         ("running_var", C, running[1]))}
    v = {k: b[1] for k, b in outs.items()}
    c.batch_norm_fwd(dev, X[1], W, B, v["y"], v["stats"], v["running_mean"], v["running_var"], N, C, L, EPS, MOM)
    c.batch_norm_bwd_sums(dev, v["sums"], G[1], X[1], v["stats"], N, C, L)
    c.batch_norm_bwd(dev, v["dx"], G[1], X[1], W, v["stats"], v["sums"], N, C, L, assign=True)
    c.batch_norm_bwd_params(dev, v["dgamma"], v["dbeta"], v["sums"], C, assign=True)
    got = {}
    for name, (buf, _) in outs.items():
        h = buf.numpy()
        assert (h[:lead] == GUARD).all() and (h[-5:] == GUARD).all(), name
        got[name] = h[lead:-5].reshape(o64[name].shape)
    _compare(got, o64, o32, x, g, gamma, "offset pointers")


def test_large_mean_small_spread_needs_the_centred_variance(dev):
    """a channel at 1e4 with a spread of 1e-2: E[x^2] - mean^2 in f32 loses the variance entirely (x^2 ~ 1e8 at an ulp of 8 against a
    variance of 1e-4); the centred sums keep it to the resolution of the f32 mean, ulp(1e4) / 2 ~ 5e-4 against the spread of 1e-2,
    a few 1e-3 of the variance.  The neighbouring channel (mean 0, spread 1) is held to the suite's rule."""
    from neuronika_amd import capi as c
    for N, C, L in ((16, 2, 3136), (4096, 2, 1), (32, 2, 49)):
        rng = np.random.default_rng(L)
        x = rng.standard_normal((N, C, L))
        x[:, 0] = 1e4 + 1e-2 * x[:, 0]
        x = x.astype(np.float32)
        g = rng.standard_normal((N, C, L)).astype(np.float32)
        running = (np.zeros(C, np.float32), np.ones(C, np.float32))
        o64, o32 = BN.both(x, None, None, g, 0.0, MOM, running)
        got = _device_run(dev, c, x, g, None, None, running, True, [np.zeros((N, C, L), np.float32), np.zeros(C, np.float32), np.zeros(C, np.float32)], eps=0.0)
        assert 50.0 < o64["stats"][0, 1] < 200.0                                   # the channel's deviation is about 1e-2
        assert abs(got["stats"][0, 0] - o64["stats"][0, 0]) <= 2e-3
        assert abs(got["stats"][0, 1] / o64["stats"][0, 1] - 1.0) < 1e-2
        np.testing.assert_allclose(got["y"][:, 0], o64["y"][:, 0], atol=0.1)       # xhat of order 1, x resolved to a tenth of the spread
        np.testing.assert_allclose(got["running_var"][0], o64["running_var"][0], rtol=1e-2)
        _check(got["y"][:, 1], o64["y"][:, 1], o32["y"][:, 1], "neighbour of the offset channel y")
        _check(got["stats"][1], o64["stats"][1], o32["stats"][1], "neighbour of the offset channel stats")


def test_constant_channel(dev):
    from neuronika_amd import capi as c
    for N, C, L in ((8, 3, 1024), (64, 8, 1), (6, 3, 10)):
        x, g, gamma, beta, running = _inputs(N, C, L, 3)
        x[:, 1] = -7.25
        got = _device_run(dev, c, x, g, gamma, beta, running, True, [np.zeros((N, C, L), np.float32), np.zeros(C, np.float32), np.zeros(C, np.float32)])
        assert np.array_equal(got["y"][:, 1], np.full((N, L), beta[1], np.float32))  # xhat = 0 exactly: y = beta
        assert got["stats"][1, 0] == np.float32(-7.25)
        np.testing.assert_allclose(got["stats"][1, 1], 1.0 / np.sqrt(EPS), rtol=1e-6)
        assert np.isfinite(got["dx"]).all() and got["dgamma"][1] == 0.0
        np.testing.assert_allclose(got["running_var"][1], (1 - MOM) * running[1][1], rtol=1e-6)


@pytest.mark.parametrize("N,C,L", [(8, 5, 1024), (64, 8, 1), (6, 5, 10), (100, 7, 1)])
def test_nan_stays_inside_its_channel(dev, N, C, L):
    """a NaN in one channel: that channel's results are NaN, its neighbours' are bit for bit what they are without it"""
    from neuronika_amd import capi as c
    x, g, gamma, beta, running = _inputs(N, C, L, L)
    zero = [np.zeros((N, C, L), np.float32), np.zeros(C, np.float32), np.zeros(C, np.float32)]
    clean = _device_run(dev, c, x, g, gamma, beta, running, True, zero)
    xn = x.copy()
    xn[N // 2, 2, L // 2] = np.nan
    got = _device_run(dev, c, xn, g, gamma, beta, running, True, zero)
    keep = np.arange(C) != 2
    for name in ("y", "dx"):
        assert np.array_equal(got[name][:, keep], clean[name][:, keep]), name
        assert np.isnan(got[name][:, 2]).all(), name
    for name in ("stats", "running_mean", "running_var", "dgamma", "sums"):
        assert np.array_equal(got[name][keep], clean[name][keep]), name
        assert np.isnan(got[name][2]).any(), name
    assert np.array_equal(got["dbeta"], clean["dbeta"])                            # dbeta does not read x


@pytest.mark.parametrize("N,C,L", [(16, 8, 3136), (64, 256, 1), (8, 3, 49)])
def test_assign_equals_accumulate_on_zeros(dev, N, C, L):
    from neuronika_amd import capi as c
    x, g, gamma, beta, running = _inputs(N, C, L, 17)
    for training in (True, False):
        acc = _device_run(dev, c, x, g, gamma, beta, running, False, [np.zeros((N, C, L), np.float32), np.zeros(C, np.float32), np.zeros(C, np.float32)], training)
        asg = _device_run(dev, c, x, g, gamma, beta, running, True, [np.full((N, C, L), np.nan, np.float32), np.full(C, np.nan, np.float32), np.full(C, np.nan, np.float32)], training)
        for name in ("dx", "dgamma", "dbeta"):
            assert np.array_equal(acc[name], asg[name]), (name, training)
            assert np.isfinite(asg[name]).all()


@pytest.mark.parametrize("N,C,L", [(16, 8, 3136), (64, 256, 1), (8, 3, 49), (5, 7, 3)])
def test_inference_form(dev, N, C, L):
    from neuronika_amd import capi as c
    x, g, gamma, beta, running = _inputs(N, C, L, 23)
    o64, o32 = BN.both(x, gamma, beta, g, EPS, MOM, running, training=False)
    rng = np.random.default_rng(5)
    init = [rng.standard_normal(s).astype(np.float32) for s in ((N, C, L), (C,), (C,))]
    got = _device_run(dev, c, x, g, gamma, beta, running, False, init, training=False)
    assert np.array_equal(got["running_mean"], running[0]) and np.array_equal(got["running_var"], running[1])   # nothing is updated
    _compare(got, o64, o32, x, g, gamma, "inference", init, epilogue=True, training=False)
    # stats are optional: the same y without them
    X, W, B, RM, RV, Y = dev.array(x), dev.array(gamma), dev.array(beta), dev.array(running[0]), dev.array(running[1]), dev.zeros((N, C, L))
    c.batch_norm_infer_fwd(dev, X, W, B, RM, RV, Y, None, N, C, L, EPS)
    assert np.array_equal(Y.numpy(), got["y"])
    # training without stats and without running statistics: the same y as with them
    full = _device_run(dev, c, x, g, gamma, beta, running, True, init)
    c.batch_norm_fwd(dev, X, W, B, Y, None, None, None, N, C, L, EPS, MOM)
    assert np.array_equal(Y.numpy(), full["y"])
    # one parameter output at a time: the same bits as both together, the other buffer untouched
    SUMS, DG, DB = dev.array(full["sums"]), dev.full((C,), np.nan), dev.full((C,), 3.0)
    c.batch_norm_bwd_params(dev, DG, None, SUMS, C, assign=True)
    assert np.array_equal(DG.numpy(), full["sums"][:, 1])
    c.batch_norm_bwd_params(dev, None, DB, SUMS, C, assign=False)
    assert np.array_equal(DB.numpy(), np.float32(3.0) + full["sums"][:, 0])


def test_empty_input_writes_nothing(dev):
    from neuronika_amd import capi as c
    C = 8
    A, P, S = dev.full((4, C, 4), 5.0), dev.full((C,), 5.0), dev.full((C, 2), 5.0)
    for N, L in ((0, 4), (4, 0), (0, 0)):
        c.batch_norm_fwd(dev, A, P, P, A, S, P, P, N, C, L, EPS, MOM)
        c.batch_norm_infer_fwd(dev, A, P, P, P, P, A, S, N, C, L, EPS)
        c.batch_norm_bwd_sums(dev, S, A, A, S, N, C, L)
        for assign in (False, True):
            c.batch_norm_bwd(dev, A, A, A, P, S, S, N, C, L, assign=assign)
            c.batch_norm_bwd(dev, A, A, A, P, S, None, N, C, L, assign=assign)
    assert (A.numpy() == 5.0).all() and (P.numpy() == 5.0).all() and (S.numpy() == 5.0).all()


def test_rejections(dev):
    from neuronika_amd import capi as c
    N, C, L = 4, 8, 4
    A, P, S = dev.zeros((N, C, L)), dev.zeros((C,)), dev.zeros((C, 2))
    bad = [lambda: c.batch_norm_fwd(dev, A, P, P, A, S, P, P, 1, C, 1, EPS, MOM),       # one value per channel has no variance
           lambda: c.batch_norm_fwd(dev, A, P, P, A, S, P, P, N, 0, L, EPS, MOM), lambda: c.batch_norm_fwd(dev, A, P, P, A, S, P, P, N, -3, L, EPS, MOM),
           lambda: c.batch_norm_fwd(dev, A, P, P, A, S, P, P, -1, C, L, EPS, MOM), lambda: c.batch_norm_fwd(dev, A, P, P, A, S, P, P, N, C, -2, EPS, MOM),
           lambda: c.batch_norm_fwd(dev, A, P, P, A, S, P, P, N, C, L, -1e-5, MOM), lambda: c.batch_norm_fwd(dev, A, P, P, A, S, P, P, N, C, L, float("nan"), MOM),
           lambda: c.batch_norm_fwd(dev, A, P, P, A, S, P, P, N, C, L, EPS, -0.1), lambda: c.batch_norm_fwd(dev, A, P, P, A, S, P, P, N, C, L, EPS, 1.5),
           lambda: c.batch_norm_fwd(dev, A, P, P, A, S, P, P, N, C, L, EPS, float("nan")),
           lambda: c.batch_norm_fwd(dev, None, P, P, A, S, P, P, N, C, L, EPS, MOM), lambda: c.batch_norm_fwd(dev, A, P, P, None, S, P, P, N, C, L, EPS, MOM),
           lambda: c.batch_norm_fwd(dev, A, P, P, A, S, P, P, 1 << 20, C, 1 << 12, EPS, MOM),
           lambda: c.batch_norm_infer_fwd(dev, A, P, P, None, P, A, S, N, C, L, EPS), lambda: c.batch_norm_infer_fwd(dev, A, P, P, P, None, A, S, N, C, L, EPS),
           lambda: c.batch_norm_infer_fwd(dev, A, P, P, P, P, A, S, N, 0, L, EPS), lambda: c.batch_norm_infer_fwd(dev, A, P, P, P, P, A, S, N, C, L, -1.0),
           lambda: c.batch_norm_bwd_sums(dev, None, A, A, S, N, C, L), lambda: c.batch_norm_bwd_sums(dev, S, None, A, S, N, C, L),
           lambda: c.batch_norm_bwd_sums(dev, S, A, None, S, N, C, L), lambda: c.batch_norm_bwd_sums(dev, S, A, A, None, N, C, L),
           lambda: c.batch_norm_bwd_sums(dev, S, A, A, S, N, 0, L)]
    for assign in (False, True):
        bad += [lambda a=assign: c.batch_norm_bwd(dev, None, A, A, P, S, S, N, C, L, assign=a), lambda a=assign: c.batch_norm_bwd(dev, A, None, A, P, S, S, N, C, L, assign=a),
                lambda a=assign: c.batch_norm_bwd(dev, A, A, None, P, S, S, N, C, L, assign=a), lambda a=assign: c.batch_norm_bwd(dev, A, A, A, P, None, S, N, C, L, assign=a),
                lambda a=assign: c.batch_norm_bwd(dev, A, A, A, P, S, S, N, 0, L, assign=a),
                lambda a=assign: c.batch_norm_bwd_params(dev, None, None, S, C, assign=a), lambda a=assign: c.batch_norm_bwd_params(dev, P, P, None, C, assign=a),
                lambda a=assign: c.batch_norm_bwd_params(dev, P, P, S, 0, assign=a)]
    for call in bad:
        with pytest.raises(c.NeuronikaHipError) as e:
            call()
        assert str(e.value)                                                        # nk_last_error says why
    # one value per channel is fine in inference
    c.batch_norm_infer_fwd(dev, A, P, P, P, dev.full((C,), 1.0), A, S, 1, C, 1, EPS)
    dev.sync()


@pytest.mark.parametrize("N,C,L", [(32, 64, 3136), (65536, 256, 1), (1000, 13, 49)])
def test_results_repeat_bit_for_bit(dev, N, C, L):
    from neuronika_amd import capi as c
    rng = np.random.default_rng(1)
    x, g = rng.standard_normal((N, C, L), dtype=np.float32), rng.standard_normal((N, C, L), dtype=np.float32)
    gamma, beta = rng.standard_normal(C, dtype=np.float32), rng.standard_normal(C, dtype=np.float32)
    running = (np.zeros(C, np.float32), np.ones(C, np.float32))
    zero = [np.zeros((N, C, L), np.float32), np.zeros(C, np.float32), np.zeros(C, np.float32)]
    runs = [_device_run(dev, c, x, g, gamma, beta, running, True, zero) for _ in range(3)]
    for other in runs[1:]:
        for name, a in runs[0].items():
            assert np.array_equal(a, other[name]), name
    assert np.isfinite(runs[0]["dgamma"]).all() and np.abs(runs[0]["dgamma"]).max() > 0

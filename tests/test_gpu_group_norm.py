"""nk_group_norm_* through the C ABI (`capi`) against tests/group_norm_oracle.py, over the three kernel classes (the row in
registers, chunked, generic).  y, mean, rstd and dx under the suite's rule err_gpu <= max(2 * err_cpu32, 1e-6 * scale) against
the f64 oracle (margins recorded as `groupnorm:*`); mean with scale = max |x|; dx, a difference of three terms that can cancel
almost entirely (D = 1 or 2), with the scale of the terms' magnitude, as tests/test_gpu_batchnorm.py does and for its reason;
dgamma and dbeta through tolerance.assert_contraction with K = N * L."""
import numpy as np
import pytest

import group_norm_oracle as GN
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu

EPS = 1e-5


def _check(got, want, want32, what, scale=None):
    from conftest import record_margin
    scale = float(np.abs(want).max()) if scale is None else scale
    err_gpu, err_cpu = float(np.abs(got - want).max()), float(np.abs(want32 - want).max())
    print("groupnorm:%s err_gpu=%.3e err_cpu32=%.3e abs=%.3e" % (what, err_gpu, err_cpu, 1e-6 * scale))
    record_margin("groupnorm:" + what, err_gpu, err_cpu, 1e-6 * scale)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)


def _inputs(N, C, L, seed, affine=True):
    """channels of a known spread (unit noise) around their own offset and scale, as test_gpu_batchnorm._inputs"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, C, L)) * (0.5 + rng.random((1, C, 1))) + rng.standard_normal((1, C, 1))).astype(np.float32)
    g = rng.standard_normal((N, C, L)).astype(np.float32)
    gamma = (1.0 + 0.5 * rng.standard_normal(C)).astype(np.float32) if affine else None
    beta = rng.standard_normal(C).astype(np.float32) if affine else None
    return x, g, gamma, beta


def _opt(dev, a):
    return dev.array(a) if a is not None else None


def _shapes(N, C, L):
    return ((N, C, L), (C,), (C,))


def _zeros(N, C, L):
    return [np.zeros(s, np.float32) for s in _shapes(N, C, L)]


def _device_run(dev, c, x, G, g, gamma, beta, assign, init, eps=EPS, params=True):
    """forward, dx, parameter gradients; `init` = (dx0, dgamma0, dbeta0) the outputs hold before the call"""
    N, C, L = x.shape
    X, GR, W, B = dev.array(x), dev.array(g), _opt(dev, gamma), _opt(dev, beta)
    Y, S = dev.full((N, C, L), np.nan), dev.full((N * G, 2), np.nan)
    c.group_norm_fwd(dev, X, W, B, Y, S, N, C, L, G, eps)
    DX = dev.array(init[0])
    c.group_norm_bwd(dev, DX, GR, X, W, S, N, C, L, G, assign=assign)
    out = dict(y=Y.numpy(), stats=S.numpy(), dx=DX.numpy())
    if params:
        DG, DB = dev.array(init[1]), dev.array(init[2])
        c.group_norm_bwd_params(dev, DG, DB, GR, X, S, N, C, L, G, assign=assign)
        out.update(dgamma=DG.numpy(), dbeta=DB.numpy())
    return out


def _compare(got, o64, o32, x, G, g, gamma, tag, base=None, epilogue=False):
    N, C, L = x.shape
    base = base or [0.0, 0.0, 0.0]
    _check(got["y"], o64["y"], o32["y"], "y " + tag)
    _check(got["stats"][:, 0], o64["stats"][:, 0], o32["stats"][:, 0], "mean " + tag, scale=float(np.abs(x).max()))
    _check(got["stats"][:, 1], o64["stats"][:, 1], o32["stats"][:, 1], "rstd " + tag)
    rows = lambda a: np.asarray(a, np.float64).reshape(N * G, -1)
    mean, rstd = o64["stats"][:, :1], o64["stats"][:, 1:]
    xh = (rows(x) - mean) * rstd
    gh = rows(g * (gamma.astype(np.float64).reshape(1, C, 1) if gamma is not None else 1.0))
    # dx = rstd * (gh - c1 - xhat * c2) is a difference of three terms (a row of one element cancels entirely, one of two almost):
    # its last roundings happen at the terms' magnitude, which is its scale
    c1, c2 = gh.mean(axis=1, keepdims=True), (gh * xh).mean(axis=1, keepdims=True)
    dx_scale = float((rstd * (np.abs(gh) + np.abs(c1) + np.abs(xh) * np.abs(c2))).max())
    _check(got["dx"], base[0] + o64["dx"], base[0] + o32["dx"], "dx " + tag, scale=dx_scale)
    if "dgamma" in got:
        gmax, xhat = float(np.abs(g).max()), max(1.0, float(np.abs(xh).max()))
        assert_contraction("groupnorm:dgamma " + tag, got["dgamma"], base[1] + o64["dgamma"], N * L, gmax, xhat, cpu32=base[1] + o32["dgamma"], epilogue=epilogue)
        assert_contraction("groupnorm:dbeta " + tag, got["dbeta"], base[2] + o64["dbeta"], N * L, gmax, 1.0, cpu32=base[2] + o32["dbeta"], epilogue=epilogue)


# (N, C, L, G)
GRID = [(4, 8, 16, 2),         # wave class
        (3, 6, 4, 3),          # D = 8
        (2, 4, 256, 4),        # G = C
        (2, 16, 256, 2),       # D = 2048, the wave limit
        (2, 3, 684, 1),        # D = 2052, the first block row
        (2, 32, 1024, 2),      # D = 16384, the block limit
        (2, 8, 4100, 2),       # D = 16400, the first chunked row, with a last chunk of 16 floats
        (1, 64, 4096, 2),      # D = 131072, one sample, many chunks
        (2, 64, 49, 8),        # D = 392, L % 4 != 0: quads straddle channels
        (5, 6, 7, 3), (3, 7, 5, 7), (2, 4, 1, 2),   # generic class
        (2, 3, 1, 3),          # D = 1, y = beta
        (3, 5, 9999, 1),       # generic class with a long row
        (4097, 4, 4, 2)]       # 8194 rows of D = 8.  The launches cap their grids at 2^20 blocks (of four rows each in the wave class),
                               # which this size does not reach: every row has its own wave and the `row += step` loop runs once.


@pytest.mark.parametrize("N,C,L,G", GRID)
def test_parity_grid(dev, N, C, L, G):
    from neuronika_amd import capi as c
    for affine in (True, False):
        x, g, gamma, beta = _inputs(N, C, L, N * 100003 + C * 101 + L + 7 * G, affine)
        o64, o32 = GN.both(x, G, gamma, beta, g, EPS)
        rng = np.random.default_rng(7)
        for assign in (False, True):
            # accumulate into data, assign over NaN
            init = [np.full(s, np.nan, np.float32) if assign else rng.standard_normal(s).astype(np.float32) for s in _shapes(N, C, L)]
            got = _device_run(dev, c, x, G, g, gamma, beta, assign, init)
            tag = "%s/%s" % ("affine" if affine else "plain", "assign" if assign else "accumulate")
            _compare(got, o64, o32, x, G, g, gamma, tag, [np.zeros_like(a) if assign else a for a in init], epilogue=not assign)
    if (C // G) * L == 1:
        assert np.array_equal(got["y"], np.zeros((N, C, L), np.float32))           # plain: y = xhat = 0 exactly
        x, g, gamma, beta = _inputs(N, C, L, 3)
        y = _device_run(dev, c, x, G, g, gamma, beta, True, _zeros(N, C, L))["y"]
        assert np.array_equal(y, np.broadcast_to(beta.reshape(1, C, 1), (N, C, L)))  # D = 1: y = beta


def _offset_rows(N, C, L, seed):
    rng = np.random.default_rng(seed)
    x = (1000.0 + 0.1 * rng.standard_normal((N, C, L))).astype(np.float32)
    g = rng.standard_normal((N, C, L)).astype(np.float32)
    return x, g, (1.0 + 0.5 * rng.standard_normal(C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)


OFFSET_SHAPES = [(2, 8, 256, 2), (1, 8, 4100, 1)]


def _offset_rows_case(dev, N, C, L, G):
    """every value 1000 + 0.1 * noise: the variance (1e-2) is 1e-8 of the mean square.  E[x^2] - mean^2 in f32 loses it entirely
    (ulp(1e6) = 0.06); chunk means merged without an anchor carry ulp(1000) / 2 = 3e-5 each against a true difference of
    0.1 / sqrt(8192) = 1e-3 between chunks, a part in 10^5 of the variance.  The two-pass f32 twin stays within 1e-6 of rstd
    (checked here on the CPU, so that the rule's bound is the stated one and not a lax twin's), and so must the device."""
    from neuronika_amd import capi as c
    x, g, gamma, beta = _offset_rows(N, C, L, L)
    o64, o32 = GN.both(x, G, gamma, beta, g, EPS)
    rstd64, rstd32 = o64["stats"][:, 1], o32["stats"][:, 1]
    assert float(np.abs(rstd32 - rstd64).max()) <= 1e-6 * float(rstd64.max())
    assert 5.0 < rstd64.min() and rstd64.max() < 20.0
    got = _device_run(dev, c, x, G, g, gamma, beta, True, [np.full(s, np.nan, np.float32) for s in _shapes(N, C, L)])
    _compare(got, o64, o32, x, G, g, gamma, "offset rows")


def test_offset_rows(dev):
    for shape in OFFSET_SHAPES:
        _offset_rows_case(dev, *shape)


# one shape of each class: registers (wave and block), chunked, generic
CLASS_SHAPES = [(3, 8, 64, 2), (2, 6, 2048, 3), (2, 8, 4100, 2), (3, 6, 7, 3)]


def _pointers_one_float_past_a_boundary_and_guard_words_case(dev, N, C, L, G):
    """every tensor starts one float past a 16-byte boundary (the float4 kernels must not be chosen), with guard floats before
    and after every output"""
    from neuronika_amd import capi as c
    x, g, gamma, beta = _inputs(N, C, L, 99)
    o64, o32 = GN.both(x, G, gamma, beta, g, EPS)
    GUARD = np.float32(-12345.5)
    lead = 5                                                                       # 4 guard floats keep alignment, the fifth takes it away

    def guarded(n, fill=None):
        buf = dev.full((lead + n + 5,), float(GUARD))
        if fill is not None:
            h = buf.numpy(); h[lead:lead + n] = fill.ravel(); buf = dev.array(h)
        return buf, buf.view_offset(lead)

    X, GR, W, B = guarded(x.size, x), guarded(g.size, g), guarded(C, gamma), guarded(C, beta)
    outs = {name: guarded(n) for name, n in (("y", x.size), ("stats", 2 * N * G), ("dx", x.size), ("dgamma", C), ("dbeta", C))}
    v = {k: b[1] for k, b in outs.items()}
    c.group_norm_fwd(dev, X[1], W[1], B[1], v["y"], v["stats"], N, C, L, G, EPS)
    c.group_norm_bwd(dev, v["dx"], GR[1], X[1], W[1], v["stats"], N, C, L, G, assign=True)
    c.group_norm_bwd_params(dev, v["dgamma"], v["dbeta"], GR[1], X[1], v["stats"], N, C, L, G, assign=True)
    got = {}
    for name, (buf, _) in outs.items():
        h = buf.numpy()
        assert (h[:lead] == GUARD).all() and (h[-5:] == GUARD).all(), name
        got[name] = h[lead:-5].reshape(o64[name].shape)
    _compare(got, o64, o32, x, G, g, gamma, "offset pointers")


def test_pointers_one_float_past_a_boundary_and_guard_words(dev):
    for shape in CLASS_SHAPES:
        _pointers_one_float_past_a_boundary_and_guard_words_case(dev, *shape)


def _results_repeat_bit_for_bit_case(dev, N, C, L, G):
    from neuronika_amd import capi as c
    x, g, gamma, beta = _inputs(N, C, L, 1)
    runs = [_device_run(dev, c, x, G, g, gamma, beta, True, _zeros(N, C, L)) for _ in range(2)]
    for name, a in runs[0].items():
        assert np.array_equal(a, runs[1][name]), name
    assert np.isfinite(runs[0]["dgamma"]).all() and np.abs(runs[0]["dgamma"]).max() > 0


def test_results_repeat_bit_for_bit(dev):
    for shape in CLASS_SHAPES + [(37, 64, 49, 8)]:
        _results_repeat_bit_for_bit_case(dev, *shape)


def _a_row_alone_has_the_bits_it_has_in_the_batch_case(dev, N, C, L, G):
    """row (n, j): (a) its sample run alone - N = 1, the same C, L, G, every pointer moved to sample n - gives the bits of y, stats
    and dx it has inside the batch; (b) with x, g, gamma and beta of every other group set to NaN they do not change either"""
    from neuronika_amd import capi as c
    x, g, gamma, beta = _inputs(N, C, L, 5)
    Cg = C // G
    whole = _device_run(dev, c, x, G, g, gamma, beta, True, _zeros(N, C, L), params=False)
    X, GR, W, B = dev.array(x), dev.array(g), dev.array(gamma), dev.array(beta)
    n = N - 1
    Y, S, DX = dev.full((N, C, L), np.nan), dev.full((N * G, 2), np.nan), dev.full((N, C, L), np.nan)
    at, st = n * C * L, n * G * 2
    c.group_norm_fwd(dev, X.view_offset(at), W, B, Y.view_offset(at), S.view_offset(st), 1, C, L, G, EPS)
    c.group_norm_bwd(dev, DX.view_offset(at), GR.view_offset(at), X.view_offset(at), W, S.view_offset(st), 1, C, L, G, assign=True)
    for name, a in (("y", Y.numpy()), ("stats", S.numpy()), ("dx", DX.numpy())):
        assert np.array_equal(a[n:] if name != "stats" else a[n * G:], whole[name][n:] if name != "stats" else whole[name][n * G:]), name
        assert np.isnan(a[:n] if name != "stats" else a[:n * G]).all(), name            # nothing before the sample was written
    j = G - 1
    mine = np.zeros((N, C, L), bool)
    mine[n, j * Cg:(j + 1) * Cg] = True
    xn, gn = np.where(mine, x, np.nan).astype(np.float32), np.where(mine, g, np.nan).astype(np.float32)
    ch = np.arange(C) // Cg == j
    alone = _device_run(dev, c, xn, G, gn, np.where(ch, gamma, np.nan).astype(np.float32), np.where(ch, beta, np.nan).astype(np.float32), True,
                        _zeros(N, C, L), params=False)
    for name in ("y", "dx"):
        assert np.array_equal(alone[name][mine], whole[name][mine]), name
        assert np.isnan(alone[name][~mine]).all(), name
    assert np.array_equal(alone["stats"][n * G + j], whole["stats"][n * G + j])


def test_a_row_alone_has_the_bits_it_has_in_the_batch(dev):
    for shape in CLASS_SHAPES:
        _a_row_alone_has_the_bits_it_has_in_the_batch_case(dev, *shape)


def _one_group_has_the_statistics_of_layer_norm_bit_for_bit_case(dev, D):
    """G = 1: `stats` is what nk_layer_norm_fwd(rows = N, D = C * L) writes for the same x (the same row_stats on the same quads)"""
    from neuronika_amd import capi as c
    N, C = 5, 4
    L = D // C
    x, g, gamma, beta = _inputs(N, C, L, D)
    X, Y = dev.array(x), dev.zeros((N, C, L))
    S, SL = dev.full((N, 2), np.nan), dev.full((N, 2), np.nan)
    c.group_norm_fwd(dev, X, dev.array(gamma), dev.array(beta), Y, S, N, C, L, 1, EPS)
    c.layer_norm_fwd(dev, X, None, None, Y, SL, N, D, EPS)
    assert np.isfinite(S.numpy()).all() and np.array_equal(S.numpy(), SL.numpy())


def test_one_group_has_the_statistics_of_layer_norm_bit_for_bit(dev):
    for shape in (64, 2048, 2052, 16384):
        _one_group_has_the_statistics_of_layer_norm_bit_for_bit_case(dev, shape)


def test_constant_row_and_optional_outputs(dev):
    from neuronika_amd import capi as c
    for N, C, L, G in CLASS_SHAPES:
        x, g, gamma, beta = _inputs(N, C, L, 3)
        Cg = C // G
        x[0, Cg:2 * Cg] = -7.25                                                     # row (0, 1)
        got = _device_run(dev, c, x, G, g, gamma, beta, True, _zeros(N, C, L))
        assert np.array_equal(got["y"][0, Cg:2 * Cg], np.broadcast_to(beta[Cg:2 * Cg, None], (Cg, L)))  # xhat = 0 exactly: y = beta
        assert got["stats"][1, 0] == np.float32(-7.25)
        np.testing.assert_allclose(got["stats"][1, 1], 1.0 / np.sqrt(EPS), rtol=1e-6)
        assert np.isfinite(got["dx"]).all()
        # stats are optional: the same y without them; one parameter output at a time: the same bits, the other buffer untouched
        X, GR, Y = dev.array(x), dev.array(g), dev.zeros((N, C, L))
        c.group_norm_fwd(dev, X, dev.array(gamma), dev.array(beta), Y, None, N, C, L, G, EPS)
        assert np.array_equal(Y.numpy(), got["y"])
        S, DG, DB = dev.array(got["stats"]), dev.full((C,), np.nan), dev.full((C,), 3.0)
        c.group_norm_bwd_params(dev, DG, None, GR, X, S, N, C, L, G, assign=True)
        assert np.array_equal(DG.numpy(), got["dgamma"])
        c.group_norm_bwd_params(dev, None, DB, GR, X, S, N, C, L, G, assign=False)
        assert np.array_equal(DB.numpy(), np.float32(3.0) + got["dbeta"])


def test_refusals_and_empty_inputs_write_nothing(dev):
    from neuronika_amd import capi as c
    N, C, L, G = 4, 8, 4, 2
    A, P, S = dev.full((N, C, L), np.nan), dev.full((C,), np.nan), dev.full((N * G, 2), np.nan)
    X = dev.zeros((N, C, L))
    bad = []
    for n, ch, l, grp, eps in ((N, C, L, 3, EPS), (N, C, L, 0, EPS), (N, C, L, -2, EPS), (N, 0, L, G, EPS), (N, C, L, G, -1e-5), (N, C, L, G, float("nan")),
                               (N, C, L, G, float("inf")), (-1, C, L, G, EPS), (N, C, -4, G, EPS), (N, C, 1 << 40, G, EPS), (1 << 40, C, L, G, EPS)):
        bad.append(lambda a=(n, ch, l, grp, eps): c.group_norm_fwd(dev, X, P, P, A, S, *a))
        if eps == EPS:
            for assign in (False, True):
                bad.append(lambda a=(n, ch, l, grp), s=assign: c.group_norm_bwd(dev, A, X, X, P, S, *a, assign=s))
                bad.append(lambda a=(n, ch, l, grp), s=assign: c.group_norm_bwd_params(dev, P, P, X, X, S, *a, assign=s))
    bad += [lambda: c.group_norm_fwd(dev, None, P, P, A, S, N, C, L, G, EPS), lambda: c.group_norm_fwd(dev, X, P, P, None, S, N, C, L, G, EPS),
            lambda: c.group_norm_bwd(dev, A, X, X, P, None, N, C, L, G), lambda: c.group_norm_bwd_params(dev, None, None, X, X, S, N, C, L, G)]
    for call in bad:
        with pytest.raises(c.NeuronikaHipError) as e:
            call()
        assert str(e.value)                                                        # nk_last_error says why
    for n, l in ((0, L), (N, 0), (0, 0)):                                          # NK_OK, nothing written
        c.group_norm_fwd(dev, X, P, P, A, S, n, C, l, G, EPS)
        for assign in (False, True):
            c.group_norm_bwd(dev, A, X, X, P, S, n, C, l, G, assign=assign)
            c.group_norm_bwd_params(dev, P, P, X, X, S, n, C, l, G, assign=assign)
    assert np.isnan(A.numpy()).all() and np.isnan(P.numpy()).all() and np.isnan(S.numpy()).all()

"""nk_rms_norm_* through the C ABI (`capi`) against tests/rms_norm_oracle.py.  y, stats and dx under the suite's rule
err_gpu <= max(2 * err_cpu32, 1e-6 * scale) against the f64 oracle (margins recorded as `rmsnorm:*`); dgamma, a sum over the
rows, through tolerance.assert_contraction with K = rows.

`scale` of the rule is the largest magnitude the compared quantity is rounded at.  For y and stats that is max |oracle|.  dx is
the difference rstd * (gh - xhat * c): its last rounding happens at the magnitude of the two terms, not of their difference, and
for D = 1 (xhat^2 = x^2 / (x^2 + eps), the terms cancel to a part in 10^6) or D = 2, 3 the difference is far smaller than either.
So dx takes scale = max(max |oracle dx|, max |rstd * gh|), both from the f64 oracle (`_dx_scale`); for rows of tens of elements
and more the two agree to a small factor."""
import numpy as np
import pytest

import rms_norm_oracle as RN
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu

EPS = 1e-6


def _check(got, want, want32, what, scale=None):
    from conftest import record_margin
    scale = float(np.abs(want).max()) if scale is None else scale
    err_gpu, err_cpu = float(np.abs(got - want).max()), float(np.abs(want32 - want).max())
    print("rmsnorm:%s err_gpu=%.3e err_cpu32=%.3e abs=%.3e" % (what, err_gpu, err_cpu, 1e-6 * scale))
    record_margin("rmsnorm:" + what, err_gpu, err_cpu, 1e-6 * scale)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)


def _dx_scale(o64, g, gamma, base=0.0):
    gh = g.astype(np.float64) * (gamma.astype(np.float64) if gamma is not None else 1.0)
    return max(float(np.abs(base + o64["dx"]).max()), float(np.abs(o64["stats"][:, None] * gh).max()))


def _inputs(rows, D, seed, affine=True):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, D), dtype=np.float32)
    x *= (0.5 + rng.random((rows, 1), dtype=np.float32) * 4)                      # rows of different magnitude
    g = rng.standard_normal((rows, D), dtype=np.float32)
    gamma = (1.0 + 0.5 * rng.standard_normal(D)).astype(np.float32) if affine else None
    return x, g, gamma


def _device_run(dev, c, x, g, gamma, assign, init, eps=EPS, dgamma=True):
    """forward, dx, dgamma; `init` = (dx0, dgamma0) the outputs hold before the call"""
    rows, D = x.shape
    X, G = dev.array(x), dev.array(g)
    W = dev.array(gamma) if gamma is not None else None
    Y, S = dev.full((rows, D), np.nan), dev.full((rows,), np.nan)
    c.rms_norm_fwd(dev, X, W, Y, S, rows, D, eps)
    DX = dev.array(init[0])
    c.rms_norm_bwd(dev, DX, G, X, W, S, rows, D, assign=assign)
    out = dict(y=Y.numpy(), stats=S.numpy(), dx=DX.numpy())
    if dgamma:
        DG = dev.array(init[1])
        c.rms_norm_bwd_gamma(dev, DG, G, X, S, rows, D, assign=assign)
        out["dgamma"] = DG.numpy()
    return out


def _zeros(rows, D):
    return [np.zeros((rows, D), np.float32), np.zeros(D, np.float32)]


DS = (1, 2, 3, 4, 5, 31, 64, 100, 256, 260, 512, 768, 1024, 1027, 2048, 2052, 4096, 8192, 16384, 20000)
# the D on each side of a dispatch bracket (V = 1 | 2 | 4 | 8 per lane of a wave, 4 | 8 | 16 per thread of a block, general; the
# wave / general seam at 1024 | 1027): these run at every row count, the others at 3 and 64 rows
BRACKET = (256, 260, 512, 768, 1024, 1027, 2048, 2052, 4096, 8192, 16384, 20000)
GRID = [(r, D) for D in DS for r in (1, 3, 5, 64, 1000, 4097) if r in (3, 64) or D in BRACKET]


@pytest.mark.parametrize("rows,D", GRID)
def test_parity_grid(dev, rows, D):
    from neuronika_amd import capi as c
    x, g, weight = _inputs(rows, D, rows * 100003 + D)
    for affine in (True, False):
        gamma = weight if affine else None
        o64, o32 = RN.both(x, gamma, g, EPS)
        rng = np.random.default_rng(7)
        for assign in (False, True):
            # accumulate into data, assign over NaN
            init = [np.full(s, np.nan, np.float32) if assign else rng.standard_normal(s, dtype=np.float32) for s in ((rows, D), (D,))]
            got = _device_run(dev, c, x, g, gamma, assign, init)
            tag = "%s/%s" % ("affine" if affine else "plain", "assign" if assign else "accumulate")
            _check(got["y"], o64["y"], o32["y"], "y " + tag)
            _check(got["stats"], o64["stats"], o32["stats"], "stats " + tag)
            base = 0.0 if assign else init[0]
            _check(got["dx"], base + o64["dx"], base + o32["dx"], "dx " + tag, scale=_dx_scale(o64, g, gamma, base))
            b = 0 if assign else init[1]
            assert_contraction("rmsnorm:dgamma " + tag, got["dgamma"], b + o64["dgamma"], rows, np.abs(g).max(),
                               float((np.abs(x).max(axis=1) * o64["stats"]).max()),   # max |xhat|, the second operand of the sum
                               cpu32=(b + o32["dgamma"]).astype(np.float32), epilogue=not assign)


def test_rows_beyond_one_trip_of_the_wave_kernels(dev):
    """(4 * 2^20 + 5, 4): more rows than 2^20 blocks of four waves hold, so the wave kernels' `row += step` runs; forward and dx"""
    from neuronika_amd import capi as c
    rows, D = 4 * (1 << 20) + 5, 4
    x, g, gamma = _inputs(rows, D, 12)
    o64, o32 = RN.both(x, gamma, g, EPS)
    got = _device_run(dev, c, x, g, gamma, True, [np.full((rows, D), np.nan, np.float32)], dgamma=False)
    for name in ("y", "stats", "dx"):
        scale = _dx_scale(o64, g, gamma) if name == "dx" else None
        _check(got[name], o64[name], o32[name], "long " + name, scale=scale)
        _check(got[name][-8:], o64[name][-8:], o32[name][-8:], "long tail " + name, scale=scale)


@pytest.mark.parametrize("D", [1, 2, 4, 64, 256, 1024, 4096, 16384, 32768])
def test_exact_rows(dev, D):
    """x = +-2^k, D a power of two, eps = 0: the mean square is 2^2k exactly, so rstd = 2^-k and y = sign * gamma bit for bit"""
    from neuronika_amd import capi as c
    rows = 21
    rng = np.random.default_rng(D)
    k = np.arange(rows) - 10
    sign = rng.choice(np.float32([-1.0, 1.0]), size=(rows, D))
    x = (sign * np.exp2(k)[:, None]).astype(np.float32)
    g, gamma = rng.standard_normal((rows, D), dtype=np.float32), rng.standard_normal(D, dtype=np.float32)
    got = _device_run(dev, c, x, g, gamma, True, _zeros(rows, D), eps=0.0)
    assert np.array_equal(got["stats"], np.exp2(-k).astype(np.float32))
    assert np.array_equal(got["y"], sign * gamma)


@pytest.mark.parametrize("D", [5, 256, 2048, 4096, 16384, 20000])
def test_scale_invariance_bit_for_bit(dev, D):
    """y(x * 2^8) and y(x * 2^-8) at eps = 0 equal y(x) bit for bit and their stats are 2^-8 and 2^8 times stats(x): every step
    (square, sum, / D, sqrt, 1 / ., x * rstd) commutes with a power of two while nothing leaves the normal range, given the
    correctly rounded f32 square root and division the build uses"""
    from neuronika_amd import capi as c
    rows = 9
    x, g, gamma = _inputs(rows, D, D + 1)
    x = (x + np.copysign(np.float32(1e-3), x)).astype(np.float32)                  # 1e-3 <= |x| < 30: squares of x * 2^+-8 stay normal
    base = _device_run(dev, c, x, g, gamma, True, _zeros(rows, D), eps=0.0)
    for a in (np.float32(256.0), np.float32(1.0 / 256.0)):
        got = _device_run(dev, c, x * a, g, gamma, True, _zeros(rows, D), eps=0.0)
        assert np.array_equal(got["y"], base["y"]), float(a)
        assert np.array_equal(got["stats"] * a, base["stats"]), float(a)


def test_eps_dominates(dev):
    """rows of magnitude 1e-4 at eps = 1e-5: the mean square (1e-8) is a thousandth of eps"""
    from neuronika_amd import capi as c
    for rows, D in ((16, 1024), (5, 4096), (7, 1027)):
        x, g, gamma = _inputs(rows, D, D)
        x = (x * np.float32(1e-4)).astype(np.float32)
        o64, o32 = RN.both(x, gamma, g, 1e-5)
        got = _device_run(dev, c, x, g, gamma, True, _zeros(rows, D), eps=1e-5)
        assert np.abs(o64["stats"] * np.sqrt(1e-5) - 1.0).max() < 0.01
        for name in ("y", "stats", "dx"):
            _check(got[name], o64[name], o32[name], "eps dominates " + name, scale=_dx_scale(o64, g, gamma) if name == "dx" else None)


@pytest.mark.parametrize("D", [8, 100, 1024, 4096])
def test_zero_row(dev, D):
    from neuronika_amd import capi as c
    rows = 6
    x, g, gamma = _inputs(rows, D, D)
    x[2] = 0.0
    o64, o32 = RN.both(x, gamma, g, EPS)
    got = _device_run(dev, c, x, g, gamma, True, _zeros(rows, D))
    assert np.array_equal(got["y"][2], np.zeros(D, np.float32))
    np.testing.assert_allclose(got["stats"][2], 1.0 / np.sqrt(EPS), rtol=1e-6)
    assert np.isfinite(got["dx"]).all()
    _check(got["dx"][2], o64["stats"][2] * (g[2].astype(np.float64) * gamma), o32["stats"][2] * (g[2] * gamma), "zero row dx = rstd * gh")
    for name in ("y", "stats", "dx"):
        _check(got[name], o64[name], o32[name], "zero row " + name, scale=_dx_scale(o64, g, gamma) if name == "dx" else None)
    # dgamma takes nothing from that row: the same bits as with that row's gradient zeroed
    g0 = g.copy(); g0[2] = 0.0
    assert np.array_equal(got["dgamma"], _device_run(dev, c, x, g0, gamma, True, _zeros(rows, D))["dgamma"])
    assert_contraction("rmsnorm:zero row dgamma", got["dgamma"], o64["dgamma"], rows, np.abs(g).max(), max(1.0, np.abs(o64["y"]).max()), cpu32=o32["dgamma"])


def test_zero_row_at_eps_zero_and_overflowing_row(dev):
    """eps = 0: the zero row is NaN, and only that row.  A row whose sum of squares overflows f32: rstd = 0, y = 0."""
    from neuronika_amd import capi as c
    rows, D = 5, 1024
    x, g, gamma = _inputs(rows, D, 4)
    x[1] = 0.0
    x[3] = 3e19
    clean = _device_run(dev, c, x, g, gamma, True, _zeros(rows, D), eps=EPS)
    got = _device_run(dev, c, x, g, gamma, True, _zeros(rows, D), eps=0.0)
    assert np.isnan(got["y"][1]).all() and np.isinf(got["stats"][1]) and np.isnan(got["dx"][1]).all()
    keep = np.arange(rows) != 1
    assert np.isfinite(got["y"][keep]).all() and np.isfinite(got["dx"][keep]).all()
    for r in (3,):
        assert got["stats"][r] == 0.0 and not got["y"][r].any() and clean["stats"][r] == 0.0


@pytest.mark.parametrize("D", [100, 256, 2048, 4096, 20000])
def test_nan_row_stays_inside_its_row(dev, D):
    """a NaN in one row: that row's results are NaN, its neighbours' are bit for bit what they are without it"""
    from neuronika_amd import capi as c
    rows = 9
    x, g, gamma = _inputs(rows, D, D)
    clean = _device_run(dev, c, x, g, gamma, True, _zeros(rows, D))
    xn = x.copy()
    xn[4, D // 2] = np.nan
    got = _device_run(dev, c, xn, g, gamma, True, _zeros(rows, D))
    keep = np.arange(rows) != 4
    for name in ("y", "stats", "dx"):
        assert np.array_equal(got[name][keep], clean[name][keep]), name
        assert np.isnan(got[name][4]).all(), name
    assert np.isnan(got["dgamma"]).all()                                           # every column sums over the NaN row's xhat


@pytest.mark.parametrize("D", [64, 1024, 2048, 4096, 16384, 1027, 20000])
def test_row_alone_has_the_same_bits(dev, D):
    """row r of a batch equals the same row entered alone: wave (64, 1024, 2048), block (4096, 16384) and general (1027, 20000)"""
    from neuronika_amd import capi as c
    rows, r = 37, 17
    x, g, gamma = _inputs(rows, D, D)
    batch = _device_run(dev, c, x, g, gamma, True, _zeros(rows, D), dgamma=False)
    alone = _device_run(dev, c, x[r:r + 1].copy(), g[r:r + 1].copy(), gamma, True, _zeros(1, D), dgamma=False)
    for name in ("y", "stats", "dx"):
        assert np.array_equal(batch[name][r:r + 1], alone[name]), name


@pytest.mark.parametrize("rows,D,lead", [(5, 1027, 4), (64, 5, 4), (3, 31, 3), (7, 1024, 4), (7, 1024, 1), (4, 4096, 2), (3, 20000, 4)])
def test_guard_words_stay_intact(dev, rows, D, lead):
    """`lead` guard floats before and 5 after every output (lead = 4 keeps 16-byte alignment, other values take it away: the
    row-in-registers kernels must not be chosen then)"""
    from neuronika_amd import capi as c
    x, g, gamma = _inputs(rows, D, 99)
    o64, o32 = RN.both(x, gamma, g, EPS)
    GUARD = np.float32(-12345.5)

    def guarded(n):
        buf = dev.full((lead + n + 5,), float(GUARD))
        return buf, buf.view_offset(lead)

    X, G, W = dev.array(x), dev.array(g), dev.array(gamma)
    bufs = {name: guarded(n) for name, n in (("y", rows * D), ("stats", rows), ("dx", rows * D), ("dgamma", D))}
    c.rms_norm_fwd(dev, X, W, bufs["y"][1], bufs["stats"][1], rows, D, EPS)
    c.rms_norm_bwd(dev, bufs["dx"][1], G, X, W, bufs["stats"][1], rows, D, assign=True)
    c.rms_norm_bwd_gamma(dev, bufs["dgamma"][1], G, X, bufs["stats"][1], rows, D, assign=True)
    for name, (buf, _) in bufs.items():
        h = buf.numpy()
        assert (h[:lead] == GUARD).all() and (h[-5:] == GUARD).all(), name
        body = h[lead:-5].reshape(o64[name].shape)
        if name != "dgamma":
            _check(body, o64[name], o32[name], "guarded " + name, scale=_dx_scale(o64, g, gamma) if name == "dx" else None)
        else:
            assert_contraction("rmsnorm:guarded dgamma", body, o64[name], rows, np.abs(g).max(), max(1.0, np.abs(o64["y"]).max()), cpu32=o32[name])


def test_optional_pointers_and_empty_input(dev):
    from neuronika_amd import capi as c
    rows, D = 37, 768
    x, g, gamma = _inputs(rows, D, 5)
    X, G, W = dev.array(x), dev.array(g), dev.array(gamma)
    full = _device_run(dev, c, x, g, gamma, True, _zeros(rows, D))
    S = dev.array(full["stats"])
    # no stats: the same y
    Y = dev.zeros((rows, D))
    c.rms_norm_fwd(dev, X, W, Y, None, rows, D, EPS)
    assert np.array_equal(Y.numpy(), full["y"])
    # no gamma: y = xhat, and y with gamma is xhat * gamma
    xhat = dev.zeros((rows, D)); c.rms_norm_fwd(dev, X, None, xhat, None, rows, D, EPS)
    o64, o32 = RN.both(x, None, g, EPS)
    _check(xhat.numpy(), o64["y"], o32["y"], "y no gamma")
    assert np.array_equal(full["y"], xhat.numpy() * gamma)
    DX = dev.full((rows, D), np.nan); c.rms_norm_bwd(dev, DX, G, X, None, S, rows, D, assign=True)
    _check(DX.numpy(), o64["dx"], o32["dx"], "dx no gamma", scale=_dx_scale(o64, g, None))
    # rows = 0: NK_OK, nothing written
    DG = dev.full((D,), 5.0)
    Y.fill(5.0)
    c.rms_norm_fwd(dev, X, W, Y, S, 0, D, EPS)
    for assign in (False, True):
        c.rms_norm_bwd(dev, Y, G, X, W, S, 0, D, assign=assign)
        c.rms_norm_bwd_gamma(dev, DG, G, X, S, 0, D, assign=assign)
    assert (Y.numpy() == 5.0).all() and (DG.numpy() == 5.0).all() and np.array_equal(S.numpy(), full["stats"])


def test_rejections(dev):
    from neuronika_amd import capi as c
    A = dev.zeros((4, 8))
    S, P = dev.zeros((4,)), dev.zeros((8,))
    bad = [lambda: c.rms_norm_fwd(dev, A, P, A, S, 4, 0, EPS), lambda: c.rms_norm_fwd(dev, A, P, A, S, 4, -8, EPS),
           lambda: c.rms_norm_fwd(dev, A, P, A, S, -1, 8, EPS), lambda: c.rms_norm_fwd(dev, A, P, A, S, 4, 8, -1e-6),
           lambda: c.rms_norm_fwd(dev, A, P, A, S, 4, 8, float("nan")), lambda: c.rms_norm_fwd(dev, A, P, A, S, 4, 8, float("inf")),
           lambda: c.rms_norm_fwd(dev, None, P, A, S, 4, 8, EPS), lambda: c.rms_norm_fwd(dev, A, P, None, S, 4, 8, EPS)]
    for assign in (False, True):
        bad += [lambda a=assign: c.rms_norm_bwd(dev, None, A, A, P, S, 4, 8, assign=a), lambda a=assign: c.rms_norm_bwd(dev, A, None, A, P, S, 4, 8, assign=a),
                lambda a=assign: c.rms_norm_bwd(dev, A, A, None, P, S, 4, 8, assign=a), lambda a=assign: c.rms_norm_bwd(dev, A, A, A, P, None, 4, 8, assign=a),
                lambda a=assign: c.rms_norm_bwd(dev, A, A, A, P, S, 4, 0, assign=a), lambda a=assign: c.rms_norm_bwd(dev, A, A, A, P, S, -2, 8, assign=a),
                lambda a=assign: c.rms_norm_bwd_gamma(dev, None, A, A, S, 4, 8, assign=a), lambda a=assign: c.rms_norm_bwd_gamma(dev, P, None, A, S, 4, 8, assign=a),
                lambda a=assign: c.rms_norm_bwd_gamma(dev, P, A, None, S, 4, 8, assign=a), lambda a=assign: c.rms_norm_bwd_gamma(dev, P, A, A, None, 4, 8, assign=a),
                lambda a=assign: c.rms_norm_bwd_gamma(dev, P, A, A, S, 4, 0, assign=a), lambda a=assign: c.rms_norm_bwd_gamma(dev, P, A, A, S, -1, 8, assign=a)]
    for call in bad:
        with pytest.raises(c.NeuronikaHipError) as e:
            call()
        assert "rms_norm" in str(e.value)                                          # nk_last_error says why and where
    dev.sync()


@pytest.mark.parametrize("rows,D", [(32768, 1024), (1000, 1027)])
def test_results_repeat_bit_for_bit(dev, rows, D):
    from neuronika_amd import capi as c
    rng = np.random.default_rng(1)
    x, g = rng.standard_normal((rows, D), dtype=np.float32), rng.standard_normal((rows, D), dtype=np.float32)
    gamma = rng.standard_normal(D, dtype=np.float32)
    X, G, W = dev.array(x), dev.array(g), dev.array(gamma)
    runs = []
    for _ in range(2):
        Y, S, DX, DG = dev.zeros((rows, D)), dev.zeros((rows,)), dev.zeros((rows, D)), dev.zeros((D,))
        c.rms_norm_fwd(dev, X, W, Y, S, rows, D, EPS)
        c.rms_norm_bwd(dev, DX, G, X, W, S, rows, D, assign=True)
        c.rms_norm_bwd_gamma(dev, DG, G, X, S, rows, D, assign=True)
        runs.append([a.numpy() for a in (Y, S, DX, DG)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert np.isfinite(runs[0][3]).all() and np.abs(runs[0][3]).max() > 0

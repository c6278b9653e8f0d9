"""The `nt` forms of the HBM-bound kernels: every call site of `nk_streams_past_cache` that tests/streaming_sites.py shows uncrossed by
the rest of the suite, at the smallest shape of the vector family whose bytes expression exceeds 384 MiB.  Every test takes its
shape's crossing from the ledger's expression and asserts it before it launches.

Row-local and elementwise passes (norm dx, rope, activation backward, AdamW, the attention-probability backward): the switch changes
cache hints only, so the whole call must equal BIT FOR BIT the same buffers processed as two row-range calls that the ledger's
expression puts below the threshold (`view_offset` on rows); 64 sampled rows are also held against the family's f64 oracle under the
family's own rule and labels, which pins the small calls.  Reductions whose order depends on the shape (the norms' parameter
gradients, the clip's norm): the f64 oracle through the family's check, and two runs with the same bits.

The norm forwards take no switch (nk_norm.hip: the single-input forward loses with `nt` loads); they run here to produce the stats."""
import gc

import numpy as np
import pytest

import layernorm_oracle as LN
import rms_norm_oracle as RN
import rope_oracle as RO
import streaming_sites as SS
import tolerance
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(got, want, what):
    got, want = bits(got).reshape(-1), bits(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:8])


def rows_of(arr, first, count, width):
    """`count` rows of `width` floats of a device array from row `first` on, as a non-owning (count, width) view"""
    v = arr.view_offset(first * width)
    v.shape, v.size = (count, width), count * width
    return v


def sample_rows(rows, cut, seed):
    """64 rows: the ends, both sides of the split, the rest drawn"""
    fixed = [0, 1, cut - 1, cut, rows - 2, rows - 1]
    return np.array(fixed + list(np.random.default_rng(seed).integers(0, rows, 64 - len(fixed))))


# ---- LayerNorm and RMSNorm ---------------------------------------------------------------------------------------------------------
D_NORM = 1024                                                              # V = 4 float4 per lane of a wave, four rows a block


@pytest.fixture(scope="module")
def norm_data():
    """x, g, dx0 of the largest norm case (49153 rows), gamma and beta; the cases take leading rows.  Never written."""
    rng = np.random.default_rng(31)
    rows = SS.site("nk_layer_norm_bwd_params").shape["rows"]
    x = rng.standard_normal((rows, D_NORM), dtype=f32) * f32(1.5) + rng.standard_normal((rows, 1), dtype=f32)
    g, dx0 = rng.standard_normal((rows, D_NORM), dtype=f32), rng.standard_normal((rows, D_NORM), dtype=f32)
    gamma, beta = (1.0 + 0.5 * rng.standard_normal(D_NORM)).astype(f32), rng.standard_normal(D_NORM).astype(f32)
    for a in (x, g, dx0, gamma, beta):
        a.flags.writeable = False
    yield dict(x=x, g=g, dx0=dx0, gamma=gamma, beta=beta)


def _norm_fwd(dev, c, norm, X, W, B, Y, S, rows):
    if norm == "layer":
        c.layer_norm_fwd(dev, X, W, B, Y, S, rows, D_NORM, 1e-5)
    else:
        c.rms_norm_fwd(dev, X, W, Y, S, rows, D_NORM, 1e-6)


@pytest.mark.parametrize("assign", [False, True], ids=["accumulate", "assign"])
@pytest.mark.parametrize("norm", ["layer", "rms"])
def test_norm_dx(dev, norm_data, norm, assign):
    """dx of the row-in-registers kernels with bit 1 of `flags` set: rows * D * (assign ? 12 : 16) > 384 MiB at 32769 (assign) and 24577
    (`+=`) rows of 1024; one row fewer is the fullsize tests' shape, exactly on the threshold."""
    from neuronika_amd import capi as c
    site = SS.site("nk_layer_norm_bwd /")
    D, W = D_NORM, 1 if norm == "rms" else 2                               # floats of stats per row
    rows = SS.THRESHOLD // (D * (12 if assign else 16)) + 1
    cut = (rows // 2 + 3) // 4 * 4
    assert SS.crosses(site, rows=rows, D=D, assign=assign) and not SS.crosses(site, rows=rows - 1, D=D, assign=assign)
    assert not SS.crosses(site, rows=cut, D=D, assign=assign) and not SS.crosses(site, rows=rows - cut, D=D, assign=assign)
    x, g, gamma, beta = norm_data["x"][:rows], norm_data["g"][:rows], norm_data["gamma"], norm_data["beta"]
    init = np.full((rows, D), np.nan, f32) if assign else norm_data["dx0"][:rows]
    X, G, Wt, B = dev.array(x), dev.array(g), dev.array(gamma), dev.array(beta)
    Y, S = dev.full((rows, D), np.nan), dev.full((rows, W), np.nan)
    _norm_fwd(dev, c, norm, X, Wt, B, Y, S, rows)
    bwd = c.layer_norm_bwd if norm == "layer" else c.rms_norm_bwd
    whole, parts = dev.array(init), dev.array(init)
    bwd(dev, whole, G, X, Wt, S, rows, D, assign=assign)
    for first, count in ((0, cut), (cut, rows - cut)):
        bwd(dev, rows_of(parts, first, count, D), rows_of(G, first, count, D), rows_of(X, first, count, D), Wt, rows_of(S, first, count, W),
            count, D, assign=assign)
    dx = whole.numpy()
    same_bits(dx, parts.numpy(), "%s norm dx: the whole call against two row ranges below the threshold" % norm)
    same_bits(X.numpy(), x, "x is read only")
    pick = sample_rows(rows, cut, rows)
    y, st = Y.numpy()[pick], S.numpy()[pick]
    tag = "affine/" + ("assign" if assign else "accumulate")
    base = 0.0 if assign else init[pick]
    if norm == "layer":
        from test_gpu_layernorm import _check
        o64, o32 = LN.both(x[pick], gamma, beta, g[pick], 1e-5)
        _check(y, o64["y"], o32["y"], "y " + tag)
        _check(st, o64["stats"], o32["stats"], "stats " + tag)
        _check(dx[pick], base + o64["dx"], base + o32["dx"], "dx " + tag)
    else:
        from test_gpu_rms_norm import _check, _dx_scale
        o64, o32 = RN.both(x[pick], gamma, g[pick], 1e-6)
        _check(y, o64["y"], o32["y"], "y " + tag)
        _check(st.reshape(-1), o64["stats"], o32["stats"], "stats " + tag)
        _check(dx[pick], base + o64["dx"], base + o32["dx"], "dx " + tag, scale=_dx_scale(o64, g[pick], gamma, base))
    del X, G, Wt, B, Y, S, whole, parts, dx
    gc.collect()


@pytest.mark.parametrize("norm", ["layer", "rms"])
def test_norm_params(dev, norm_data, norm):
    """Stage 1 of the parameter gradients with `nt` loads: rows * D * 8 > 384 MiB at 49153 rows of 1024.  The oracle walks the rows in
    blocks (its f64 copies stay small); the bound is the fullsize tests', tolerance.assert_contraction with K = rows, the f32 twin
    left out (the absolute term alone: the narrower bound).  `+=` adds onto the assign result's inputs; two runs give the same bits."""
    from neuronika_amd import capi as c
    site = SS.site("nk_layer_norm_bwd_params")
    rows, D, W = site.shape["rows"], D_NORM, 1 if norm == "rms" else 2
    assert SS.crosses(site, rows=rows, D=D) and not SS.crosses(site, rows=rows - 1, D=D)
    x, g, gamma, beta = norm_data["x"][:rows], norm_data["g"][:rows], norm_data["gamma"], norm_data["beta"]
    dg64, db64, ymax, xhat_max = np.zeros(D), np.zeros(D), 0.0, 0.0
    for lo in range(0, rows, 4096):
        xs, gs = x[lo:lo + 4096].astype(np.float64), g[lo:lo + 4096].astype(np.float64)
        if norm == "layer":
            yb, st = LN.forward(xs, gamma.astype(np.float64), beta.astype(np.float64), 1e-5)
            _, dg, db = LN.backward(gs, xs, gamma.astype(np.float64), st)
            db64 += db
            ymax = max(ymax, float(np.abs(yb).max()))
        else:
            _, st = RN.forward(xs, gamma.astype(np.float64), 1e-6)
            _, dg = RN.backward(gs, xs, gamma.astype(np.float64), st)
            xhat_max = max(xhat_max, float((np.abs(xs).max(axis=1) * st).max()))
        dg64 += dg
    X, G, Wt, B = dev.array(x), dev.array(g), dev.array(gamma), dev.array(beta)
    Y, S = dev.full((rows, D), np.nan), dev.full((rows, W), np.nan)
    _norm_fwd(dev, c, norm, X, Wt, B, Y, S, rows)
    del Y
    gmax = float(np.abs(g).max())
    runs = []
    for _ in range(2):
        DG, DB = dev.full((D,), np.nan), dev.full((D,), np.nan)
        if norm == "layer":
            c.layer_norm_bwd_params(dev, DG, DB, G, X, S, rows, D, assign=True)
        else:
            c.rms_norm_bwd_gamma(dev, DG, G, X, S, rows, D, assign=True)
        runs.append((DG.numpy(), DB.numpy()))
    same_bits(runs[0][0], runs[1][0], "dgamma: two runs")
    base = np.random.default_rng(5).standard_normal(D).astype(f32)
    DG, DB = dev.array(base), dev.array(base)
    if norm == "layer":
        same_bits(runs[0][1], runs[1][1], "dbeta: two runs")
        assert_contraction("layernorm:fullsize dgamma", runs[0][0], dg64, rows, gmax, ymax)
        assert_contraction("layernorm:fullsize dbeta", runs[0][1], db64, rows, gmax, 1.0)
        c.layer_norm_bwd_params(dev, DG, DB, G, X, S, rows, D)
        same_bits(DB.numpy(), base + runs[0][1], "dbeta += is the assign result added once")
    else:
        assert_contraction("rmsnorm:fullsize dgamma", runs[0][0], dg64, rows, gmax, xhat_max)
        c.rms_norm_bwd_gamma(dev, DG, G, X, S, rows, D)
    same_bits(DG.numpy(), base + runs[0][0], "dgamma += is the assign result added once")
    del X, G, Wt, B, S, DG, DB
    gc.collect()


# ---- rope --------------------------------------------------------------------------------------------------------------------------
ROPE = dict(NH=16, dh=128, rot=128)
MAX_POS = 200


@pytest.fixture(scope="module")
def rope_data(dev):
    from neuronika_amd import capi as c
    rng = np.random.default_rng(41)
    rows, w = 24577, ROPE["NH"] * ROPE["dh"]
    host = [(rng.random((rows, w), dtype=f32) * f32(6) - f32(3)) for _ in range(3)]
    for a in host:
        a.flags.writeable = False
    table = dev.zeros((MAX_POS, ROPE["rot"] // 2, 2))
    c.rope_table(dev, table, MAX_POS, ROPE["rot"])
    data = dict(x=host[0], g=host[1], dx0=host[2], table=table, table64=RO.table(MAX_POS, ROPE["rot"]))
    yield data
    data.clear()                                                            # the device table goes with the module's last test
    del table
    gc.collect()


@pytest.mark.parametrize("form", ["fwd", "bwd_assign", "bwd"])
@pytest.mark.parametrize("il", [False, True], ids=["half-split", "interleaved"])
def test_rope(dev, rope_data, il, form):
    """The six NT = true instantiations of rope_vec_kernel<IL, INV, ACC, NT>.  items * (il ? 16 : 32) * (ACC ? 3 : 2) > 384 MiB with 16
    heads of 128: 24577 rows (3511 samples of 7 positions) for the forward and the assign backward, 16385 rows (3277 samples of 5) for
    `+=`.  The two row ranges are whole samples with their own slices of `start`."""
    from neuronika_amd import capi as c
    from test_gpu_rope import margin, pair_sum
    site = SS.site("nk_rope_fwd")
    NH, dh, rot = ROPE["NH"], ROPE["dh"], ROPE["rot"]
    acc = form == "bwd"
    B, T = (3277, 5) if acc else (3511, 7)
    rows, w = B * T, NH * dh
    geo = dict(NH=NH, dh=dh, rot=rot, il=il, acc=acc)
    assert SS.crosses(site, rows=rows, **geo) and not SS.crosses(site, rows=rows - 1, **geo)
    B1 = B // 2
    assert not SS.crosses(site, rows=B1 * T, **geo) and not SS.crosses(site, rows=(B - B1) * T, **geo)
    start = ((np.arange(B) * 37) % (MAX_POS - T + 1)).astype(np.int32)      # every position of the table, none clamped
    src = rope_data["g" if form != "fwd" else "x"][:rows]
    init = rope_data["dx0"][:rows] if acc else np.full((rows, w), np.nan, f32)
    SRC, whole, parts = dev.array(src), dev.array(init), dev.array(init)
    tab = rope_data["table"]

    def launch(dst, s, st, b):
        tail = (tab, st, b, T, NH, dh, rot, MAX_POS, il)
        if form == "fwd":
            c.rope_fwd(dev, s, w, dst, w, *tail)
        else:
            c.rope_bwd(dev, dst, w, s, w, *tail, assign=not acc)

    launch(whole, SRC, dev.int_array(start), B)
    launch(rows_of(parts, 0, B1 * T, w), rows_of(SRC, 0, B1 * T, w), dev.int_array(start[:B1]), B1)
    launch(rows_of(parts, B1 * T, (B - B1) * T, w), rows_of(SRC, B1 * T, (B - B1) * T, w), dev.int_array(start[B1:]), B - B1)
    got = whole.numpy()
    same_bits(got, parts.numpy(), "rope %s: the whole call against two sample ranges below the threshold" % form)
    same_bits(SRC.numpy(), src, "the source is read only")
    pick = sample_rows(rows, B1 * T, rows + il)
    pos = RO.positions(start, B, T, MAX_POS)[pick]
    s64 = src[pick].astype(np.float64)
    want = RO.rope(s64, pos, 1, NH, dh, rot, il, rope_data["table64"], inverse=form != "fwd")
    bound = 2.0 ** -22 * pair_sum(src[pick], NH, dh, rot, il)
    if acc:
        want = init[pick].astype(np.float64) + want
        bound = bound * (1 + 2.0 ** -24) + 2.0 ** -24 * np.abs(want)
    assert margin(form, np.abs(got[pick] - want), bound) <= 1.0
    del SRC, whole, parts, got
    gc.collect()


# ---- activation backward, assign ---------------------------------------------------------------------------------------------------
def test_activation_bwd_assign(dev):
    """nk_activation_bwd_assign past n * 12 > 384 MiB: the fullsize test's 8192 x 4096 is 2^25 * 12, the threshold itself, so only its
    `+=` form ran with `nt` loads.  n = 2^25 + 7 (a scalar tail of 3); the ranges split on a quad."""
    from neuronika_amd import capi as c
    import activation_oracle as A
    from test_gpu_activation import within
    site = SS.site("nk_activation_bwd")
    n = site.shape["n"]
    cut = n // 2 // 4 * 4
    assert SS.crosses(site, n=n, assign=True) and not SS.crosses(site, n=1 << 25, assign=True)
    assert not SS.crosses(site, n=cut, assign=True) and not SS.crosses(site, n=n - cut, assign=True)
    rng = np.random.default_rng(9)
    x, g = rng.random(n, dtype=f32) * f32(12) - f32(6), rng.random(n, dtype=f32) * f32(2) - f32(1)
    X, G = dev.array(x), dev.array(g)
    pick = np.concatenate([[0, 1, cut - 1, cut, n - 4, n - 3, n - 2, n - 1], rng.integers(0, n, 56)])
    for act in ("gelu", "silu"):
        whole, parts = dev.full((n,), np.nan), dev.full((n,), np.nan)
        c.activation_bwd(dev, act, whole, G, X, assign=True)
        c.activation_bwd(dev, act, rows_of(parts, 0, cut, 1), rows_of(G, 0, cut, 1), rows_of(X, 0, cut, 1), n=cut, assign=True)
        c.activation_bwd(dev, act, rows_of(parts, cut, n - cut, 1), rows_of(G, cut, n - cut, 1), rows_of(X, cut, n - cut, 1), n=n - cut, assign=True)
        got = whole.numpy()
        same_bits(got, parts.numpy(), act + " backward assign: the whole call against two ranges below the threshold")
        _, d = A.value_and_derivative(act, x[pick])
        within(got[pick], g[pick].astype(np.float64) * d, "%s backward assign past the cache switch" % act)
        del whole, parts, got
    del X, G
    gc.collect()


# ---- the fused attention-probability backward --------------------------------------------------------------------------------------
@pytest.mark.parametrize("assign", [False, True], ids=["accumulate", "assign"])
def test_attention_probs_bwd(dev, assign):
    """nk_scale_softmax_dropout_bwd (stored probabilities) and _from_scores (recomputed) past rows * L * 12 > 384 MiB: (32769, 1024), the
    mask regenerated from Philox.  A row range that starts at row r continues the whole call's mask at offset + r * L / 8."""
    from neuronika_amd import capi as c
    from oracle import neuronika_oracle as O
    site = SS.site("nk_scale_softmax_dropout_bwd")
    rows, L = site.shape["rows"], site.shape["L"]
    cut = 16384
    assert SS.crosses(site, rows=rows, L=L) and not SS.crosses(site, rows=rows - 1, L=L)
    assert not SS.crosses(site, rows=cut, L=L) and not SS.crosses(site, rows=rows - cut, L=L)
    scale, p, seed, offset = 0.125, 0.1, 77, 1000
    rng = np.random.default_rng(13)
    s, g = rng.random((rows, L), dtype=f32) * f32(16) - f32(8), rng.random((rows, L), dtype=f32) * f32(2) - f32(1)
    init = np.full((rows, L), np.nan, f32) if assign else rng.random((rows, L), dtype=f32)
    S, G, P, OUT = dev.array(s), dev.array(g), dev.full((rows, L), np.nan), dev.full((rows, L), np.nan)
    c.scale_softmax_dropout_fwd(dev, S, P, OUT, None, scale, p, True, seed, offset)
    del OUT
    whole, parts, again = dev.array(init), dev.array(init), dev.array(init)
    c.scale_softmax_dropout_bwd(dev, whole, G, P, None, scale, p, True, seed, offset, assign=assign)
    c.scale_softmax_dropout_bwd_from_scores(dev, again, G, S, None, scale, p, True, seed, offset, assign=assign)
    for first, count in ((0, cut), (cut, rows - cut)):
        c.scale_softmax_dropout_bwd(dev, rows_of(parts, first, count, L), rows_of(G, first, count, L), rows_of(P, first, count, L), None, scale, p, True,
                                    seed, offset + first * L // 8, assign=assign)
    got = whole.numpy()
    same_bits(got, parts.numpy(), "probability backward: the whole call against two row ranges below the threshold")
    same_bits(got, again.numpy(), "stored against recomputed probabilities")
    pick = sample_rows(rows, cut, 3)
    pk = P.numpy()[pick].astype(np.float64)
    noise = np.stack([O.dropout_noise(L, p, seed, offset + int(r) * L // 8) for r in pick]).astype(np.float64)
    gp = g[pick].astype(np.float64) * noise                                # the reference's dropout backward does not divide by 1 - p
    inc = pk * (gp - (gp * pk).sum(axis=1, keepdims=True)) * scale
    ref = inc if assign else init[pick].astype(np.float64) + inc
    tolerance.assert_contraction("dispatch/attn_probs/L1024/bwd", got[pick], ref, L, float(np.abs(g).max()), float(pk.max()), epilogue=True)
    del S, G, P, whole, parts, again, got
    gc.collect()


# ---- AdamW and the clip ------------------------------------------------------------------------------------------------------------
def test_adamw_step(dev):
    """One parameter of 14 380 475 elements: n * 28 > 384 MiB (n % 4 == 3: a partial last chunk).  The step is elementwise, so the whole
    call equals two ranges cut on a chunk boundary, each a parameter of its own call below the threshold; 64 elements against
    tests/adamw_oracle.py inside optim_trajectory.check."""
    from neuronika_amd import capi as c
    import adamw_oracle as A
    import optim_trajectory as T
    site = SS.site("nk_adamw_step_multi")
    n = site.shape["n"]
    cut = n // 2 // 4096 * 4096
    assert SS.crosses(site, n=n, amsgrad=False) and not SS.crosses(site, n=n - 7, amsgrad=False)
    assert not SS.crosses(site, n=cut, amsgrad=False) and not SS.crosses(site, n=n - cut, amsgrad=False)
    hyper = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1)
    rng = np.random.default_rng(17)
    w, g = rng.random(n, dtype=f32) * f32(2) - f32(1), rng.random(n, dtype=f32) * f32(2) - f32(1)
    m, v = (rng.random(n, dtype=f32) - f32(0.5)) * f32(0.2), rng.random(n, dtype=f32) * f32(0.1)
    G = dev.array(g)
    whole, parts = [dev.array(a) for a in (w, m, v)], [dev.array(a) for a in (w, m, v)]
    c.adamw_step(dev, whole[0], G, whole[1], whole[2], None, step=3, **hyper)
    for first, count in ((0, cut), (cut, n - cut)):
        r = [rows_of(a, first, count, 1) for a in parts]
        c.adamw_step(dev, r[0], rows_of(G, first, count, 1), r[1], r[2], None, step=3, **hyper)
    same_bits(G.numpy(), g, "the gradient is read only")
    pick = np.concatenate([[0, 1, cut - 1, cut, n - 4, n - 3, n - 2, n - 1], rng.integers(0, n, 56)])
    ref = []
    for dt in (f32, np.float64):
        r = [a[pick].astype(dt) for a in (w, g, m, v)]
        A.adamw_step(r[0], r[1], r[2], r[3], hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"], 3, hyper["weight_decay"], None)
        ref.append(r)
    for j, (what, a, b) in enumerate(zip(("w", "m", "v"), whole, parts)):
        got = a.numpy()
        same_bits(got, b.numpy(), "adamw %s: the whole call against two ranges below the threshold" % what)
        T.check("adamw_grid/" + what, got[pick], ref[0][(0, 2, 3)[j]], ref[1][(0, 2, 3)[j]])
        del got
    del G, whole, parts
    gc.collect()


def test_clip_grad_norm(dev):
    """One gradient of 50 331 655 elements: elems * 8 > 384 MiB switches the scale pass.  total_norm against the f64 norm at
    ELEMENTWISE_RTOL and two runs with the same bits, as the family's test_clip_grid; the scaled gradient is g * coef, one f32 product
    per element (scale_one), so it equals the host's product with the device's own coef bit for bit - the form a call below the
    threshold would give with that coef, which no smaller call can be made to compute."""
    from neuronika_amd import capi as c
    site = SS.site("nk_clip_grad_norm_multi")
    n = site.shape["elems"]
    assert SS.crosses(site, elems=n) and not SS.crosses(site, elems=n - 7)
    g = np.random.default_rng(19).standard_normal(n, dtype=f32)
    norm64 = float(np.sqrt(np.dot(g.astype(np.float64), g.astype(np.float64))))
    max_norm = 20.0
    runs = []
    for _ in range(2):
        G, out = dev.array(g), dev.full((2,), 7.0)
        c.clip_grad_norm_multi(dev, [G], max_norm, out)
        runs.append((G.numpy(), out.numpy()))
        del G
    same_bits(runs[0][1], runs[1][1], "{total_norm, coef}: two runs")
    same_bits(runs[0][0], runs[1][0], "the scaled gradient: two runs")
    total, coef = runs[0][1]
    assert abs(float(total) - norm64) <= tolerance.ELEMENTWISE_RTOL * norm64
    want = max_norm / (norm64 + 1e-6)
    assert coef < 1 and abs(float(coef) - want) <= tolerance.ELEMENTWISE_RTOL * want
    same_bits(runs[0][0], g * f32(coef), "g * coef")
    del runs
    gc.collect()

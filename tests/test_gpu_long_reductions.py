"""Weight and bias gradients over 32768 rows (the benchmark's attention workload, C5 at B = 32: B * S = 32768) against an oracle,
at the plans `gemm_plan` takes BY RULE at that length: split K with no split longer than 128 k-tiles - a slab is one f32 chain of
up to 4096 products.  The cases, their plans (asserted from a restatement of the rule), the operands and the model of one launch
live in tests/test_oracle_long_k.py, which also shows without a GPU that the asserts below have teeth.

Per case (`c.sgemm` with no tune knob set) and data kind:
  * f64 oracle on sampled rows of C (the seams of the 128-row tiles, random rows) under the suite's one contraction policy;
  * integer data: exactly NumPy's product - a dropped, doubled or misplaced k-range cannot hide in a rounding bound;
  * the rule's bits = the bits of its forced twin (the table of test_oracle_long_k.CASES): bits are a function of the shape;
  * c5_dw, small_64tiles: the bits of the device-order model, slab by slab - and not those of chains of 2048;
  * the writer forms of `first_write(dw, beta)`: beta = 0 into NaN = beta = 1 into zeros; beta = 1 on a random C; ldc > N.
Bias gradients (`unbroadcast_add`, both forms) over the same 32768 rows, and one `nn.Linear` through the tape, once and with its
weights shared by two calls (the second LinearBwd accumulates)."""
import types

import numpy as np
import pytest

import test_oracle_long_k as L
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu


def capi():
    from neuronika_amd import capi as c
    return c


@pytest.fixture(scope="module")
def nk():
    import neuronika_amd
    return neuronika_amd.tape


@pytest.fixture(scope="module")
def tdev(nk):
    return nk.Device(0)


RUNS = [(case, layout, kind) for case, (layouts, *_) in L.CASES.items() for layout in layouts for kind in L.KINDS]
RUN_IDS = ["%s-%s-%s" % r for r in RUNS]


def stored(case, layout, kind):
    """(ta, tb, a, b, rows -> those rows of op(A), op(B)): a and b as the layout stores them; the TN pair is the one LinearBwd
    passes, the other layouts hold the same product"""
    at, b = L.stored_tn(case, kind)
    ta, tb = {"tn": (1, 0), "nn": (0, 0), "nt": (0, 1)}[layout]
    a = at if ta else np.ascontiguousarray(at.T)
    bs = np.ascontiguousarray(b.T) if tb else b
    return ta, tb, a, bs, (lambda rows: np.ascontiguousarray(at[:, rows].T)), b


@pytest.fixture(scope="module", params=RUNS, ids=RUN_IDS)
def run(request, dev):
    """One rule-planned launch per (case, layout, kind): operands on the device, the result of beta = 0 into a NaN-filled C, and
    the oracles of the sampled rows.  Module scope: pytest runs every test of one parameter together; the device buffers go
    when the parameter changes."""
    case, layout, kind = request.param
    c = capi()
    _, M, N, K, _ = L.CASES[case]
    ta, tb, a, b, opa_of, opb = stored(case, layout, kind)
    A, B, Cd = dev.array(a), dev.array(b), dev.full((M, N), np.nan)
    dev.gemm_force(None); dev.gemm_kpair(None)
    c.sgemm(dev, ta, tb, M, N, K, 1.0, A, a.shape[1], B, b.shape[1], 0.0, Cd, N)
    got = Cd.numpy()
    del Cd
    rows = L.sample_rows(M)
    opa = opa_of(rows)
    ref64 = opa.astype(np.float64) @ opb.astype(np.float64)
    cpu32 = opa @ opb
    for t in (got, opa, ref64, cpu32):
        t.setflags(write=False)
    yield types.SimpleNamespace(case=case, layout=layout, kind=kind, M=M, N=N, K=K, ta=ta, tb=tb, a=a, b=b, A=A, B=B, got=got,
                                rows=rows, opa=opa, opb=opb, ref64=ref64, cpu32=cpu32, label="long_k:%s:%s" % (case, kind),
                                amax=float(np.abs(a).max()), bmax=float(np.abs(b).max()))
    del A, B


def launch(dev, r, beta, Cd, ldc):
    capi().sgemm(dev, r.ta, r.tb, r.M, r.N, r.K, 1.0, r.A, r.a.shape[1], r.B, r.b.shape[1], beta, Cd, ldc)


def test_oracle_on_sampled_rows_and_integers_exactly(run):
    r = run
    assert np.isfinite(r.got).all()
    ratio = assert_contraction(r.label, r.got[r.rows], r.ref64, r.K, r.amax, r.bmax, cpu32=r.cpu32)
    print("%s err/bound %.4f" % (r.label, ratio))
    if r.kind != "int":
        return
    # integers: NumPy's f32 product is exact and so must the device's be - every element, not a bound
    assert np.abs(r.ref64).max() < 2 ** 24 and np.array_equal(r.cpu32, r.ref64)
    bad = np.argwhere(r.got[r.rows] != r.cpu32)
    assert bad.size == 0, (r.case, len(bad), bad[:4], (r.got[r.rows] - r.cpu32)[tuple(bad[:4].T)])
    opa_full = r.a.T if r.ta else r.a
    if r.case == "c5_dw_packed":        # the full CPU product is 206 GFLOP: the sampled rows above and a band across a column seam
        cols = slice(448, 576)
        want, have = opa_full @ r.opb[:, cols], r.got[:, cols]
    else:
        want, have = opa_full @ r.opb, r.got
    bad = np.argwhere(have != want)
    assert bad.size == 0, (r.case, len(bad), bad[:4], (have - want)[tuple(bad[:4].T)])


def test_the_bits_are_the_forced_twins_and_the_models(dev, run):
    r = run
    try:
        dev.gemm_force(L.twin(r.case)); dev.gemm_kpair(0)
        Cd = dev.full((r.M, r.N), np.nan)
        launch(dev, r, 0.0, Cd, r.N)
        forced = Cd.numpy()
    finally:
        dev.gemm_force(None); dev.gemm_kpair(None)
    bad = np.argwhere(forced != r.got)
    assert bad.size == 0 and np.isfinite(forced).all(), (r.case, L.twin(r.case), len(bad), bad[:4])
    if r.case in ("c5_dw", "small_64tiles") and r.kind != "int":
        # the device-order model slab by slab: splits x one chain of kts * 32 products, the slabs added in split order
        _, _, splits, kts = L.CASES[r.case][4]
        want = L.slab_model(r.opa, r.opb, splits, kts)
        assert np.array_equal(r.got[r.rows], want), (r.case, r.layout, float(np.abs(r.got[r.rows] - want).max()))
        if r.case == "c5_dw":           # teeth: slabs folded every 2048 products are other bits
            assert not np.array_equal(r.got[r.rows], L.slab_model(r.opa, r.opb, splits, kts, kc=2048))


def test_accumulation_forms(dev, run):
    r = run
    # the later writer, beta = 1: on zeros it is the first writer's value ...
    Cd = dev.zeros((r.M, r.N))
    launch(dev, r, 1.0, Cd, r.N)
    assert np.array_equal(Cd.numpy(), r.got), r.case
    # ... and on a gradient that is already there, a contraction followed by one elementwise add
    c0 = L.operand("signed", 77, (r.M, r.N))
    Cd.upload(c0)
    launch(dev, r, 1.0, Cd, r.N)
    acc = Cd.numpy()
    del Cd
    c0r = c0[r.rows].astype(np.float64)
    assert_contraction(r.label + ":beta1", acc[r.rows], r.ref64 + c0r, r.K, r.amax, r.bmax, cpu32=r.cpu32 + c0[r.rows], epilogue=True)
    if r.kind == "int":                 # exact product + one rounding of the sum
        assert np.array_equal(acc[r.rows], (r.ref64 + c0r).astype(np.float32))
    # ldc > N: the second pass that is not one dense block (splitk_reduce_kernel); same bits, the padding untouched
    pad = L.operand("signed", 78, (r.M, r.N + 4))
    Cp = dev.array(pad)
    launch(dev, r, 0.0, Cp, r.N + 4)
    out = Cp.numpy()
    del Cp
    assert np.array_equal(out[:, r.N:], pad[:, r.N:]), r.case
    assert np.array_equal(out[:, :r.N], r.got), r.case


# ---- bias gradients: column sums over 32768 rows ---------------------------------------------------------------------------
BIAS = {1024: "c5_dw", 3072: "c5_dw_packed", 64: "one_tile"}   # o -> the case whose A operand is the (32768, o) gradient
# (bwd_dispatch's chunk rule: o = 1024 -> 256 chunks of 128 rows, 3072 -> 86 of 382, 64 -> 1024 of 32)


@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("o", sorted(BIAS))
def test_bias_gradient_over_32768_rows(dev, o, kind):
    c = capi()
    g, _ = L.stored_tn(BIAS[o], kind)
    assert g.shape == (L.K_LONG, o)
    ref64 = g.sum(0, dtype=np.float64)
    gmax = float(np.abs(g).max())
    label = "long_k:db:%d:%s" % (o, kind)
    G = dev.array(g)
    d = dev.full((o,), np.nan)
    c.unbroadcast_add(dev, d, G, assign=True)
    first = d.numpy()
    d.fill(np.nan)
    c.unbroadcast_add(dev, d, G, assign=True)
    assert np.array_equal(first, d.numpy()) and np.isfinite(first).all()            # two runs, the same bits
    assert_contraction(label, first, ref64, L.K_LONG, gmax, 1.0)                     # no CPU f32 term: the absolute term alone
    d0 = L.operand("signed", 79, (o,))
    d.upload(d0)
    c.unbroadcast_add(dev, d, G)
    later = d.numpy()
    assert_contraction(label + ":add", later, ref64 + d0, L.K_LONG, gmax, 1.0, epilogue=True)
    if kind == "int":
        assert np.abs(ref64).max() < 2 ** 24
        assert np.array_equal(first, ref64) and np.array_equal(later, (ref64 + d0).astype(np.float32))
    else:
        assert np.array_equal(later, first + d0)                                     # d + sum: one add on the finished sum
    del G, d


# ---- the tape: nn.Linear 1024 -> 1024 on 32768 rows -------------------------------------------------------------------------
@pytest.mark.parametrize("calls", [1, 2])
def test_linear_backward_over_32768_rows(nk, tdev, calls):
    """`backward_from` a one-signed gradient G: dW = G^T x (TN, K = 32768: the c5_dw plan), db = the column sums of G, dx = G W
    (NN, K = 1024).  calls = 2: the same layer applied to two inputs and the outputs added - both LinearBwd nodes receive G, the
    second one is the accumulating writer of dW and db: a contraction over the 65536 stacked rows."""
    n, d = L.K_LONG, 1024
    lin = nk.nn.Linear(tdev, d, d, 7)
    xs = [L.operand("one_signed", 41 + i, (n, d)) for i in range(calls)]
    g = L.operand("one_signed", 40, (n, d))
    X = [nk.from_ndarray(tdev, x).requires_grad() for x in xs]
    out = lin.forward(X[0])
    for Xi in X[1:]:
        out = out + lin.forward(Xi)
    out.forward(); out.backward_from(nk.from_ndarray(tdev, g))
    w = lin.weight.data()
    gmax, xmax, wmax = float(np.abs(g).max()), max(float(np.abs(x).max()) for x in xs), float(np.abs(w).max())
    tag = "long_k:tape:%s" % ("first_writer" if calls == 1 else "shared_weights")
    # dW[o, m] = sum_i G[i, o] x[i, m]: sampled rows of the (o, m) gradient, every column
    rows = L.sample_rows(d, seed=calls)
    dw = lin.weight.grad()
    gr = np.ascontiguousarray(g[:, rows].T)
    dw64 = sum(gr.astype(np.float64) @ x.astype(np.float64) for x in xs)
    dw32 = gr @ xs[0] if calls == 1 else (gr @ xs[0]) + (gr @ xs[1])
    assert_contraction(tag + ":dW", dw[rows], dw64, n * calls, gmax, xmax, cpu32=dw32)
    db64 = calls * g.sum(0, dtype=np.float64)
    assert_contraction(tag + ":db", lin.bias.grad(), db64, n * calls, gmax, 1.0)
    # dx = G W on sampled rows of the 32768, each input's own gradient
    xrows = L.sample_rows(n, seed=calls)
    dx64 = g[xrows].astype(np.float64) @ w.astype(np.float64)
    dx32 = g[xrows] @ w
    for Xi in X:
        assert_contraction(tag + ":dx", Xi.grad()[xrows], dx64, d, gmax, wmax, cpu32=dx32)

"""`VarDiff::cross_entropy` / `nn::CrossEntropyLoss` through the tape (`_tape`) against NumPy (tests/cross_entropy_oracle.py): a token
classifier (Embedding -> Linear -> cross_entropy -> backward -> SGD), logits with a second consumer, the `Var` form, ignore_index as
padding together with Embedding's padding_idx, the captured step, and the history length (one node, not two)."""
import numpy as np
import pytest

import cross_entropy_oracle as X

pytestmark = pytest.mark.gpu

V_, D_, C_, N_ = 53, 24, 301, 96


@pytest.fixture(scope="module")
def nk():
    import neuronika_amd
    return neuronika_amd.tape


@pytest.fixture(scope="module")
def tdev(nk):
    return nk.Device(0)


def _data(seed, pad=False):
    rng = np.random.default_rng(seed)
    ids = rng.integers(1 if pad else 0, V_, N_).astype(np.float32)
    tgt = rng.integers(1 if pad else 0, C_, N_).astype(np.float32)
    if pad:
        ids[::5] = 0.0
        tgt[::5] = 0.0
    return ids, tgt


def _model(nk, tdev, ids, tgt, red, ignore=-1, eps=0.0, padding_idx=-1):
    emb = nk.nn.Embedding(tdev, V_, D_, padding_idx=padding_idx, seed=21)
    head = nk.nn.Linear(tdev, D_, C_, 6)
    logits = head.forward(emb.forward(nk.from_ndarray(tdev, ids)))
    loss = nk.nn.CrossEntropyLoss(red, ignore, eps).forward(logits, nk.from_ndarray(tdev, tgt))
    return dict(emb=emb, head=head, logits=logits, loss=loss, params=[emb.weight, head.weight, head.bias])


def _numpy_step(table, W, b, ids, tgt, red, ignore, eps, padding_idx=-1):
    """loss and gradients in f64"""
    idx = ids.astype(np.int64)
    x = table.astype(np.float64)[idx]
    logits = x @ W.astype(np.float64).T + b.astype(np.float64)
    loss, lse = X.forward(logits, tgt, red, ignore, eps)
    dl = X.backward(logits, tgt, lse, 1.0, red, ignore, eps)
    dtable = np.zeros(table.shape)
    keep = idx != padding_idx
    np.add.at(dtable, idx[keep], (dl @ W.astype(np.float64))[keep])
    return loss, logits, dtable, dl.T @ x, dl.sum(0)


@pytest.mark.parametrize("red,ignore,eps", [("Mean", -1, 0.0), ("Sum", -1, 0.1), ("Mean", 7, 0.1)])
def test_token_classifier_step_against_numpy(nk, tdev, red, ignore, eps):
    ids, tgt = _data(1)
    tgt[::9] = 7.0
    m = _model(nk, tdev, ids, tgt, getattr(nk.Reduction, red), ignore, eps)
    before = [p.data().copy() for p in m["params"]]
    opt = nk.optim.SGD(0.25)
    for p in m["params"]:
        opt.register(p)
    m["loss"].forward(); m["loss"].backward(1.0)
    loss, logits, *grads = _numpy_step(*before, ids, tgt, red.lower(), ignore, eps)
    assert abs(m["loss"].item() - loss) <= 1e-5 * abs(loss)
    np.testing.assert_allclose(m["logits"].data(), logits, rtol=1e-4, atol=1e-5)
    scale = max(np.abs(g).max() for g in grads)
    for p, g in zip(m["params"], grads):
        np.testing.assert_allclose(p.grad(), g, rtol=1e-4, atol=1e-5 * scale)
    dl = m["logits"].grad()
    if ignore >= 0:
        assert not dl[tgt == ignore].any() and dl[tgt != ignore].any()
    opt.step()
    for p, w0, g in zip(m["params"], before, grads):
        np.testing.assert_allclose(p.data(), w0 - 0.25 * g, rtol=1e-4, atol=1e-5 * max(scale, 1.0))


@pytest.mark.parametrize("ce_first", [True, False])
def test_logits_with_a_second_consumer_accumulate(nk, tdev, ce_first):
    """two backward writers into the logits' gradient: whichever runs first assigns, the other adds"""
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((N_, C_)) * 2).astype(np.float32)
    tgt = rng.integers(0, C_, N_).astype(np.float32)
    other = rng.standard_normal((N_, C_)).astype(np.float32)
    leaf = nk.from_ndarray(tdev, x).requires_grad()
    ce = lambda: leaf.cross_entropy(nk.from_ndarray(tdev, tgt), nk.Reduction.Mean, 3, 0.1)
    mse = lambda: leaf.mse(nk.from_ndarray(tdev, other), nk.Reduction.Sum)
    total = ce() + mse() if ce_first else mse() + ce()
    total.forward(); total.backward(1.0)
    loss, lse = X.forward(x, tgt, "mean", 3, 0.1)
    want = X.backward(x, tgt, lse, 1.0, "mean", 3, 0.1) + 2.0 * (x.astype(np.float64) - other)
    assert abs(total.item() - (loss + ((x.astype(np.float64) - other) ** 2).sum())) <= 1e-5 * abs(total.item())
    np.testing.assert_allclose(leaf.grad(), want, rtol=1e-5, atol=1e-5)


def test_the_var_form_and_the_history_length(nk, tdev):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((8, 11, 3)).astype(np.float32)
    tgt = rng.integers(0, 11, (8, 3)).astype(np.float32)
    t = nk.from_ndarray(tdev, tgt)
    plain = nk.from_ndarray(tdev, x).cross_entropy(t, nk.Reduction.Sum)
    assert not hasattr(plain, "backward") or not hasattr(plain, "grad")          # a Var: nothing to differentiate
    plain.forward()
    leaf = nk.from_ndarray(tdev, x).requires_grad()
    fused = leaf.cross_entropy(t, nk.Reduction.Sum)
    composed = leaf.log_softmax(1).nll(t, nk.Reduction.Sum)
    assert fused.history_len() == 1 and composed.history_len() == 2 and tuple(fused.shape) == ()
    fused.forward()
    assert plain.item() == fused.item() and abs(fused.item() - X.forward(x, tgt, "sum")[0]) <= 1e-5 * abs(fused.item())
    crit = nk.nn.CrossEntropyLoss(nk.Reduction.Sum)
    v = crit.forward(nk.from_ndarray(tdev, x), t)
    v.forward()
    assert v.item() == fused.item()


def test_bad_shapes_are_refused_when_the_graph_is_built(nk, tdev):
    leaf = nk.from_ndarray(tdev, np.zeros((4, 5), np.float32)).requires_grad()
    for tshape in ((5,), (4, 5), (4, 1)):
        with pytest.raises(Exception, match="cross_entropy: target must have shape"):
            leaf.cross_entropy(nk.from_ndarray(tdev, np.zeros(tshape, np.float32)), nk.Reduction.Mean)
    with pytest.raises(Exception, match="cross_entropy: input of shape"):
        nk.from_ndarray(tdev, np.zeros(4, np.float32)).requires_grad().cross_entropy(nk.from_ndarray(tdev, np.zeros((), np.float32)), nk.Reduction.Mean)
    with pytest.raises(Exception, match="label_smoothing"):
        leaf.cross_entropy(nk.from_ndarray(tdev, np.zeros(4, np.float32)), nk.Reduction.Mean, -1, 1.5)


def test_ignore_index_as_padding_with_the_embeddings_padding_idx(nk, tdev):
    """token 0 pads inputs and targets: padded positions add nothing to the loss, the divisor is the number of real tokens, the
    logits' gradient rows of padded positions and the table's padding row are zero"""
    ids, tgt = _data(4, pad=True)
    m = _model(nk, tdev, ids, tgt, nk.Reduction.Mean, ignore=0, padding_idx=0)
    before = [p.data().copy() for p in m["params"]]
    assert not before[0][0].any()
    m["loss"].forward(); m["loss"].backward(1.0)
    loss, _, dtable, dW, db = _numpy_step(*before, ids, tgt, "mean", 0, 0.0, padding_idx=0)
    real = tgt != 0
    per = X.pieces(m["logits"].data(), tgt, 0)[1]
    assert abs(m["loss"].item() - loss) <= 1e-5 * abs(loss) and abs(loss - per[real].sum() / real.sum()) <= 1e-5 * abs(loss)
    dl = m["logits"].grad()
    assert not dl[~real].any() and dl[real].any()
    assert not m["emb"].weight.grad()[0].any()
    for p, g in zip(m["params"], (dtable, dW, db)):
        np.testing.assert_allclose(p.grad(), g, rtol=1e-4, atol=1e-6)


def _make_step(nk, tdev, ids, tgt, opt):
    m = _model(nk, tdev, ids, tgt, nk.Reduction.Mean, ignore=0, eps=0.1, padding_idx=0)
    for p in m["params"]:
        opt.register(p)
    loss = m["loss"]

    def step():
        loss.forward()
        loss.no_grad(); loss.with_grad()
        loss.backward(1.0)
        opt.step()
        opt.zero_grad()
    return m, step


def test_captured_step_equals_eager_step(nk, tdev):
    """forward (loss sum, active count), backward (count again, gradient) and SGD captured into a graph: nothing synchronises, reads
    the count on the host or allocates; the replayed steps equal the eager ones bit for bit"""
    ids, tgt = _data(5, pad=True)
    me, step_e = _make_step(nk, tdev, ids, tgt, nk.optim.SGD(0.5))
    w0 = [p.data().copy() for p in me["params"]]
    for _ in range(6):
        step_e()
    want = [p.data().copy() for p in me["params"]]
    mg, step_g = _make_step(nk, tdev, ids, tgt, nk.optim.SGD(0.5))
    step_g(); step_g()                       # warm the allocator / workspace, reach the steady state
    tdev.graph_begin()
    step_g()
    graph = tdev.graph_end()
    for _ in range(4):                       # the captured call records, it does not run: 2 + 4 = the 6 eager steps
        graph.launch()
    for p, w in zip(mg["params"], want):
        assert np.array_equal(p.data(), w)
    assert mg["loss"].item() == me["loss"].item() and np.isfinite(me["loss"].item())
    assert all((a != b).any() for a, b in zip(want, w0))
    del graph


ROWS_C = 4099
ROWS_KINDS = ("climbing", "falling", "lifted", "masked_inf", "peaked:slot3", "peaked:last_wave")


def _shift_rows(masked="masked_inf"):
    """(6, 4099) logits of tests/cross_entropy_rows.py - rows that move the running maximum of the block kernel, each at the offset
    from a 16-byte boundary it has in an aligned leaf - and targets alternating between the row's maximum and its lowest live class"""
    import cross_entropy_rows as R
    kinds = tuple(masked if k == "masked_inf" else k for k in ROWS_KINDS)
    made = [R.make_row(k, R.family(ROWS_C, 1), ROWS_C, (r * ROWS_C) % 4, 900 + r) for r, k in enumerate(kinds)]
    x = np.stack([m[0] for m in made])
    live = np.stack([m[1] for m in made])
    hi, lo = np.where(live, x, -np.inf).argmax(1), np.where(live, x, np.inf).argmin(1)
    return x, live, np.where(np.arange(len(kinds)) % 2 == 0, hi, lo).astype(np.float32)


@pytest.mark.parametrize("red", ["Mean", "Sum"])
def test_rows_that_move_the_running_maximum_through_the_tape(nk, tdev, red):
    """nn::CrossEntropyLoss over a leaf of climbing, falling, lifted, masked and peaked rows: loss and leaf gradient against the f64
    oracle within its bounds, finite throughout (the N(0, 2^2) logits of the tests above leave any shift, or none, unnoticed)"""
    x, _, tgt = _shift_rows()
    leaf = nk.from_ndarray(tdev, x).requires_grad()
    loss = nk.nn.CrossEntropyLoss(getattr(nk.Reduction, red)).forward(leaf, nk.from_ndarray(tdev, tgt))
    loss.forward(); loss.backward(1.0)
    want_loss, lse = X.forward(x, tgt, red.lower())
    want = X.backward(x, tgt, lse, 1.0, red.lower())
    n = x.shape[0]
    b = X.bounds(ROWS_C, float(np.abs(x[np.isfinite(x)]).max()), n, 0.0, 1.0, 1.0 / n if red == "Mean" else 1.0)
    assert np.isfinite(want_loss) and want_loss > 100.0                    # the targets on low classes: a large finite loss
    assert np.isfinite(loss.item()) and abs(loss.item() - want_loss) <= b["loss"] * (n if red == "Sum" else 1), (loss.item(), want_loss)
    grad = leaf.grad()
    assert np.isfinite(grad).all() and np.abs(grad - want).max() <= b["dx"], np.abs(grad - want).max()


@pytest.mark.parametrize("ce_first", [True, False])
def test_rows_that_move_the_running_maximum_with_a_second_consumer(nk, tdev, ce_first):
    """as test_logits_with_a_second_consumer_accumulate, on the same rows (the mask value -1e9 in place of -inf, which a squared
    error cannot take): whichever writer runs first assigns, the other adds"""
    x, live, tgt = _shift_rows("masked_1e9")
    noise = np.round(np.random.default_rng(5).standard_normal(x.shape) * 8.0) / 8.0
    other = np.where(live, x.astype(np.float64) + noise, x).astype(np.float32)
    diff = x.astype(np.float64) - other
    assert np.array_equal(diff, np.where(live, -noise, 0.0))               # exact on the 1/8 grid
    leaf = nk.from_ndarray(tdev, x).requires_grad()
    ce = lambda: leaf.cross_entropy(nk.from_ndarray(tdev, tgt), nk.Reduction.Mean)
    mse = lambda: leaf.mse(nk.from_ndarray(tdev, other), nk.Reduction.Sum)
    total = ce() + mse() if ce_first else mse() + ce()
    total.forward(); total.backward(1.0)
    want_loss, lse = X.forward(x, tgt, "mean")
    want = X.backward(x, tgt, lse, 1.0, "mean") + 2.0 * diff
    n = x.shape[0]
    b = X.bounds(ROWS_C, float(np.abs(x[live]).max()), n, 0.0, 1.0, 1.0 / n)
    sq = (diff ** 2).sum()
    assert abs(total.item() - (want_loss + sq)) <= b["loss"] + 1e-5 * sq
    grad = leaf.grad()
    assert np.isfinite(grad).all() and (np.abs(grad - want) <= b["dx"] + 2 * X.U * np.abs(want)).all()

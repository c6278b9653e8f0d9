"""`nn::Embedding` and `VarDiff::embedding` through the tape (`_tape`) against tests/embedding_oracle.py, bit for bit: the module
alone, and a token model (Embedding -> causal MultiheadAttention -> LayerNorm -> Linear -> log_softmax -> nll) whose table
gradient is the oracle's ordered sum of the gradient that reaches the embedding's output; the captured step, tied weights, SGD,
Adam and serde."""
import numpy as np
import pytest

import embedding_oracle as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nk():
    import neuronika_amd
    return neuronika_amd.tape


@pytest.fixture(scope="module")
def tdev(nk):
    return nk.Device(0)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what


def test_module_forward_and_backward_equal_the_oracle(nk, tdev):
    rng = np.random.default_rng(0)
    V, D = 97, 40
    emb = nk.nn.Embedding(tdev, V, D, padding_idx=5, seed=3)
    assert (emb.num_embeddings, emb.embedding_dim, emb.padding_idx) == (V, D, 5)
    w = emb.weight.data()
    assert w.shape == (V, D) and not w[5].any() and w[4].any() and abs(float(w.std()) - 1.0) < 0.1
    idx = rng.integers(0, V, (6, 11)).astype(np.float32)
    idx[0, :4] = 5.0
    y = emb.forward(nk.from_ndarray(tdev, idx))
    assert tuple(y.shape) == (6, 11, D) and y.history_len() == 1
    g = rng.standard_normal((6, 11, D)).astype(np.float32)
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    same_bits(y.data(), E.forward(w, idx), "forward")
    want = E.backward_assign(g, idx, V, 5)
    same_bits(emb.weight.grad(), want, "first writer: the assign form")
    assert not emb.weight.grad()[5].any()
    y.backward_from(nk.from_ndarray(tdev, g))                                  # no zero_grad in between: the += form
    same_bits(emb.weight.grad(), E.backward(want, g, idx, 5), "accumulated")


def test_bad_geometry_is_refused_when_the_graph_is_built(nk, tdev):
    with pytest.raises(Exception):
        nk.nn.Embedding(tdev, 10, 4, padding_idx=10)
    with pytest.raises(Exception):
        nk.nn.Embedding(tdev, 0, 4)
    vec = nk.from_ndarray(tdev, np.zeros(8, np.float32)).requires_grad()
    with pytest.raises(Exception):
        vec.embedding(nk.from_ndarray(tdev, np.zeros(3, np.float32)))


B_, S_, D_, H_, V_ = 2, 64, 64, 2, 211


def _tokens(seed):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, V_ + 1)
    ids = rng.choice(V_, size=B_ * S_, p=p / p.sum()).astype(np.float32)       # skewed: many rows repeat, many are never selected
    tgt = rng.integers(0, V_, B_ * S_).astype(np.float32)
    return ids, tgt


def _model(nk, tdev, ids, tgt, first=None, tied=False):
    """logits = head(ln(mha(x))), x = emb(ids) (or the leaf `first` in its place); loss = nll(log_softmax(logits), tgt).  `tied`: the
    head is a second embedding-shaped use of the table: x2 = emb(tgt) joins the input, so the table has two backward writers"""
    nk.manual_seed(9)
    emb = nk.nn.Embedding(tdev, V_, D_, seed=21)
    mha = nk.nn.MultiheadAttention(tdev, D_, H_, 0.0, 4)
    mha.causal = True
    ln = nk.nn.LayerNorm(tdev, [D_])
    head = nk.nn.Linear(tdev, D_, V_, 6)
    x = emb.forward(nk.from_ndarray(tdev, ids)) if first is None else first
    if tied:
        x = x + nk.nn.Embedding(emb.weight).forward(nk.from_ndarray(tdev, tgt))
    logits = head.forward(ln.forward(mha.forward(x, B_)))
    loss = logits.log_softmax(1).nll(nk.from_ndarray(tdev, tgt), nk.Reduction.Mean)
    params = [emb.weight, ln.weight, ln.bias, head.weight, head.bias] + [getattr(getattr(mha, n), p) for n in "qkvo" for p in ("weight", "bias")]
    return dict(emb=emb, loss=loss, params=params, x=x)


def test_token_model_table_gradient_is_the_ordered_sum_of_what_reaches_the_embedding(nk, tdev):
    ids, tgt = _tokens(1)
    m = _model(nk, tdev, ids, tgt)
    m["loss"].forward(); m["loss"].backward(1.0)
    w = m["emb"].weight.data()
    same_bits(m["x"].data(), E.forward(w, ids), "embedding output")
    # the same graph with the embedding's output as a leaf: its gradient is what the embedding's backward node received
    leaf = nk.from_ndarray(tdev, E.forward(w, ids)).requires_grad()
    r = _model(nk, tdev, ids, tgt, first=leaf)
    r["loss"].forward(); r["loss"].backward(1.0)
    assert r["loss"].item() == m["loss"].item() and np.isfinite(m["loss"].item())
    g = leaf.grad()
    assert np.abs(g).max() > 0
    same_bits(m["emb"].weight.grad(), E.backward_assign(g, ids, V_), "table gradient")
    never = np.setdiff1d(np.arange(V_), ids.astype(np.int64))
    assert never.size > 0 and not m["emb"].weight.grad()[never].any()


def test_tied_tables_take_the_accumulating_form(nk, tdev):
    ids, tgt = _tokens(2)
    m = _model(nk, tdev, ids, tgt, tied=True)
    m["loss"].forward(); m["loss"].backward(1.0)
    w = m["emb"].weight.data()
    leaf = nk.from_ndarray(tdev, E.forward(w, ids) + E.forward(w, tgt)).requires_grad()
    r = _model(nk, tdev, ids, tgt, first=leaf)
    r["loss"].forward(); r["loss"].backward(1.0)
    g = leaf.grad()
    got = m["emb"].weight.grad()
    # two writers into one gradient: the first assigns, the second adds; the tape runs them in reverse order of construction
    a = E.backward(E.backward_assign(g, tgt, V_), g, ids)
    b = E.backward(E.backward_assign(g, ids, V_), g, tgt)
    assert np.array_equal(got.view(np.uint32), a.view(np.uint32)) or np.array_equal(got.view(np.uint32), b.view(np.uint32))
    both = np.intersect1d(ids.astype(np.int64), tgt.astype(np.int64))
    assert both.size > 0


def _make_step(nk, tdev, ids, tgt, opt):
    m = _model(nk, tdev, ids, tgt)
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
    """forward, backward (index build, ordered sum) and SGD captured into a graph: nothing synchronises, allocates or leaves the stream"""
    ids, tgt = _tokens(3)
    me, step_e = _make_step(nk, tdev, ids, tgt, nk.optim.SGD(0.5))
    w0 = me["emb"].weight.data().copy()
    for _ in range(6):
        step_e()
    want = [p.data().copy() for p in me["params"]]
    mg, step_g = _make_step(nk, tdev, ids, tgt, nk.optim.SGD(0.5))
    step_g(); step_g()                       # warm the allocator / workspace, reach the steady state
    tdev.graph_begin()
    step_g()
    graph = tdev.graph_end()
    for _ in range(4):
        graph.launch()
    for p, w in zip(mg["params"], want):
        assert np.array_equal(p.data(), w)
    assert mg["loss"].item() == me["loss"].item() and np.isfinite(me["loss"].item())
    moved = np.flatnonzero((want[0] != w0).any(axis=1))
    assert np.array_equal(moved, np.unique(ids.astype(np.int64)))              # SGD moved the selected rows and no other
    del graph


def test_adam_updates_the_table(nk, tdev):
    ids, tgt = _tokens(4)
    m, step = _make_step(nk, tdev, ids, tgt, nk.optim.Adam(1e-2))
    w0 = m["emb"].weight.data().copy()
    m["loss"].forward(); first = m["loss"].item()
    for _ in range(5):
        step()
    m["loss"].forward()
    w1 = m["emb"].weight.data()
    assert np.isfinite(w1).all() and m["loss"].item() < first
    assert np.array_equal(np.flatnonzero((w1 != w0).any(axis=1)), np.unique(ids.astype(np.int64)))


def test_padding_row_stays_zero_under_sgd(nk, tdev):
    rng = np.random.default_rng(5)
    emb = nk.nn.Embedding(tdev, 20, 8, padding_idx=0, seed=1)
    idx = rng.integers(0, 20, 50).astype(np.float32)
    idx[::3] = 0.0
    loss = emb.forward(nk.from_ndarray(tdev, idx)).mse(nk.from_ndarray(tdev, rng.standard_normal((50, 8)).astype(np.float32)), nk.Reduction.Mean)
    opt = nk.optim.SGD(0.1)
    opt.register(emb.weight)
    w0 = emb.weight.data().copy()
    loss.forward(); loss.backward(1.0); opt.step()
    w1 = emb.weight.data()
    assert not w1[0].any() and (w1[1:] != w0[1:]).any()


def test_serde_round_trip_is_bit_exact(nk, tdev):
    emb = nk.nn.Embedding(tdev, 33, 12, padding_idx=2, seed=8)
    back = nk.serde.embedding_from_json(tdev, nk.serde.to_json(emb), 2)
    assert (back.num_embeddings, back.embedding_dim, back.padding_idx) == (33, 12, 2)
    same_bits(back.weight.data(), emb.weight.data(), "table")
    idx = np.arange(40, dtype=np.float32)
    a, c = emb.forward(nk.from_ndarray(tdev, idx)), back.forward(nk.from_ndarray(tdev, idx))
    a.forward(); c.forward()
    same_bits(a.data(), c.data(), "forward of the copy")

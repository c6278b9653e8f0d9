"""`nn::LayerNorm` and `Var / VarDiff::layer_norm` through the tape (`_tape`) against tests/layernorm_oracle.py: the module on
2-D and 4-D input, every differentiability combination, the graph size, SGD, serde, and a pre-LN transformer block (LayerNorm ->
causal attention -> residual -> LayerNorm -> MLP -> residual -> MSE) against the oracles' chain, eager and captured."""
import numpy as np
import pytest

from oracle import neuronika_oracle as O
import causal_oracle as CO
import layernorm_oracle as LN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nk():
    import neuronika_amd
    return neuronika_amd.tape


@pytest.fixture(scope="module")
def tdev(nk):
    return nk.Device(0)


def rnd(seed, shape, lo=-1.0, hi=1.0):
    a = np.random.default_rng(seed).random(shape, dtype=np.float32)
    return np.asarray(a * np.float32(hi - lo) + np.float32(lo), dtype=np.float32).reshape(shape)


def _check(got, want, want32, what, floor=0.0):
    from conftest import record_margin
    got, want, want32 = (np.asarray(a).reshape(np.shape(want)) for a in (got, want, want32))
    scale = max(np.abs(want).max(), floor)
    err_gpu, err_cpu = np.abs(got - want).max(), np.abs(want32 - want).max()
    record_margin("layernorm:tape " + what, err_gpu, err_cpu, 1e-6 * scale)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)


def _param_check(got, want, want32, what, rows, gmax, ymax):
    from tolerance import assert_contraction
    assert_contraction("layernorm:tape " + what, np.asarray(got).reshape(np.shape(want)), want, rows, gmax, ymax, cpu32=want32)


def _set_params(ln, seed):
    shape = tuple(ln.normalized_shape)
    w, b = 1.0 + 0.5 * rnd(seed, shape), rnd(seed + 1, shape)
    ln.weight.set_data(w); ln.bias.set_data(b)
    return w, b


@pytest.mark.parametrize("shape,normalized", [((96, 256), (256,)), ((37, 100), (100,)), ((3, 5, 8, 16), (8, 16)), ((4, 3000), (3000,))])
def test_module_equals_oracle(nk, tdev, shape, normalized):
    D = int(np.prod(normalized)); rows = int(np.prod(shape)) // D
    x, g = rnd(1, shape), rnd(2, shape)
    ln = nk.nn.LayerNorm(tdev, list(normalized))
    assert ln.eps == 1e-5 and ln.elementwise_affine and list(ln.normalized_shape) == list(normalized)
    assert np.array_equal(ln.weight.data(), np.ones(normalized, np.float32)) and np.array_equal(ln.bias.data(), np.zeros(normalized, np.float32))
    w, b = _set_params(ln, 10)
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = ln.forward(X)
    assert tuple(y.shape) == shape
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    o64, o32 = LN.both(x.reshape(rows, D), w.reshape(D), b.reshape(D), g.reshape(rows, D), 1e-5)
    _check(y.data(), o64["y"], o32["y"], "y")
    _check(X.grad(), o64["dx"], o32["dx"], "dx")
    _param_check(ln.weight.grad(), o64["dgamma"], o32["dgamma"], "dgamma", rows, np.abs(g).max(), np.abs(o64["y"]).max())
    _param_check(ln.bias.grad(), o64["dbeta"], o32["dbeta"], "dbeta", rows, np.abs(g).max(), 1.0)
    # a second backward() on the same graph accumulates into the leaves; the node's own gradient is re-seeded
    first = [X.grad().copy(), ln.weight.grad().copy(), ln.bias.grad().copy()]
    y.backward_from(nk.from_ndarray(tdev, g))
    for got, one in zip((X.grad(), ln.weight.grad(), ln.bias.grad()), first):
        np.testing.assert_allclose(got, 2 * one, rtol=1e-6, atol=1e-6)


def test_without_affine_and_var_forms(nk, tdev):
    rows, D = 50, 192
    x, g = rnd(3, (rows, D)), rnd(4, (rows, D))
    o64, o32 = LN.both(x, None, None, g, 1e-3)
    ln = nk.nn.LayerNorm(tdev, [D], eps=1e-3, elementwise_affine=False)
    assert ln.weight is None and ln.bias is None and not ln.elementwise_affine
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = ln.forward(X); y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    _check(y.data(), o64["y"], o32["y"], "y plain")
    _check(X.grad(), o64["dx"], o32["dx"], "dx plain")
    with pytest.raises(RuntimeError):
        ln.forward(nk.from_ndarray(tdev, x))                                       # nothing to differentiate
    # the Var forms: no gradient, no statistics kept
    v = nk.from_ndarray(tdev, x).layer_norm([D], 1e-3); v.forward()
    assert np.array_equal(v.data(), y.data())
    w, b = 1.0 + 0.5 * rnd(5, (D,)), rnd(6, (D,))
    a64, a32 = LN.both(x, w, b, g, 1e-5)
    v = nk.from_ndarray(tdev, x).layer_norm(nk.from_ndarray(tdev, w), nk.from_ndarray(tdev, b)); v.forward()
    _check(v.data(), a64["y"], a32["y"], "y Var form")
    # shapes that do not fit
    with pytest.raises(RuntimeError):
        nk.from_ndarray(tdev, x).layer_norm([D + 1], 1e-5)
    with pytest.raises(RuntimeError):
        nk.from_ndarray(tdev, x).layer_norm(nk.from_ndarray(tdev, w), nk.from_ndarray(tdev, b[:-1].copy()))
    with pytest.raises(RuntimeError):
        nk.from_ndarray(tdev, x).layer_norm([D], -1.0)


def test_gradients_flow_to_each_differentiable_operand_alone(nk, tdev):
    rows, D = 64, 512
    x, g = rnd(7, (rows, D)), rnd(8, (rows, D))
    w, b = 1.0 + 0.5 * rnd(9, (D,)), rnd(10, (D,))
    o64, o32 = LN.both(x, w, b, g, 1e-5)
    G = nk.from_ndarray(tdev, g)
    # x is a plain Var: only the parameter gradients run
    W, B = nk.from_ndarray(tdev, w).requires_grad(), nk.from_ndarray(tdev, b).requires_grad()
    y = nk.from_ndarray(tdev, x).layer_norm(W, B, 1e-5)
    assert y.history_len() == 1
    y.forward(); y.backward_from(G)
    _check(y.data(), o64["y"], o32["y"], "y params only")
    _param_check(W.grad(), o64["dgamma"], o32["dgamma"], "dgamma params only", rows, np.abs(g).max(), np.abs(o64["y"]).max())
    _param_check(B.grad(), o64["dbeta"], o32["dbeta"], "dbeta params only", rows, np.abs(g).max(), 1.0)
    # the parameters are plain Vars: only dx runs
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = X.layer_norm(nk.from_ndarray(tdev, w), nk.from_ndarray(tdev, b), 1e-5)
    assert y.history_len() == 1
    y.forward(); y.backward_from(G)
    _check(X.grad(), o64["dx"], o32["dx"], "dx only")
    # one parameter shared by two layers: the second writer accumulates (first writer assigns, per gradient)
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = X.layer_norm(W, B, 1e-5) + X.layer_norm(W, B, 1e-5)
    W.zero_grad(); B.zero_grad()
    y.forward(); y.backward_from(G)
    _param_check(W.grad(), 2 * o64["dgamma"], 2 * o32["dgamma"], "dgamma shared", 2 * rows, np.abs(g).max(), np.abs(o64["y"]).max())
    _check(X.grad(), 2 * o64["dx"], 2 * o32["dx"], "dx shared")


def test_the_node_adds_one_forward_and_one_backward_entry(nk, tdev):
    x = nk.from_ndarray(tdev, rnd(1, (8, 32))).requires_grad()
    ln = nk.nn.LayerNorm(tdev, [32])
    base = x.relu()
    y = ln.forward(base)
    assert y.history_len() == base.history_len() + 1                               # dx, dgamma and dbeta leave ONE backward entry
    assert y.forward_history_len() == base.forward_history_len() + 1
    assert nk.from_ndarray(tdev, rnd(1, (8, 32))).layer_norm([32]).history_len() == 1


def test_sgd_step_moves_weight_and_bias_as_the_oracle_says(nk, tdev):
    rows, D, lr = 40, 128, 0.1
    x, t = rnd(11, (rows, D)), rnd(12, (rows, D))
    ln = nk.nn.LayerNorm(tdev, [D])
    w, b = _set_params(ln, 20)
    loss = ln.forward(nk.from_ndarray(tdev, x)).mse(nk.from_ndarray(tdev, t), nk.Reduction.Mean)
    opt = nk.optim.SGD(lr)
    opt.register(ln.weight); opt.register(ln.bias)
    loss.forward(); loss.backward(1.0); opt.step()
    want = []
    for dt in (np.float64, np.float32):
        y, st = LN.forward(x.astype(dt), w.astype(dt), b.astype(dt), 1e-5)
        g = (2 * (y - t.astype(dt))) / dt(y.size)
        _, dg, db = LN.backward(g, x.astype(dt), w.astype(dt), st)
        want.append((w.astype(dt) - dt(lr) * dg, b.astype(dt) - dt(lr) * db))
    assert not np.array_equal(ln.weight.data(), w) and not np.array_equal(ln.bias.data(), b)
    _check(ln.weight.data(), want[0][0], want[1][0], "sgd weight")
    _check(ln.bias.data(), want[0][1], want[1][1], "sgd bias")


def test_serde_round_trip_is_bit_exact(nk, tdev):
    ln = nk.nn.LayerNorm(tdev, [4, 6])
    w, b = _set_params(ln, 30)
    text = nk.serde.to_json(ln)
    assert text.startswith('{"weight":{"v":1,"dim":[4,6],"data":[') and '"bias":{"v":1,"dim":[4,6]' in text
    back = nk.serde.layer_norm_from_json(tdev, text)
    assert list(back.normalized_shape) == [4, 6] and back.eps == 1e-5 and back.elementwise_affine
    assert np.array_equal(back.weight.data(), w) and np.array_equal(back.bias.data(), b)
    x = rnd(2, (5, 4, 6))
    a, c = ln.forward(nk.from_ndarray(tdev, x)), back.forward(nk.from_ndarray(tdev, x))
    a.forward(); c.forward()
    assert np.array_equal(a.data(), c.data())
    with pytest.raises(RuntimeError):
        nk.serde.to_json(nk.nn.LayerNorm(tdev, [4], elementwise_affine=False))


# ---- a pre-LN transformer block ---------------------------------------------------------------------------------------------------
B_, S_, D_, H_, HID = 2, 64, 128, 2, 256


def _block(nk, tdev, x, t, lr=None):
    """h = x + mha(ln1(x)), causal; out = h + lin2(lin1(ln2(h)).relu()); loss = MSE(out, t)"""
    nk.manual_seed(5)
    ln1, ln2 = nk.nn.LayerNorm(tdev, [D_]), nk.nn.LayerNorm(tdev, [D_])
    _set_params(ln1, 40); _set_params(ln2, 50)
    mha = nk.nn.MultiheadAttention(tdev, D_, H_, 0.0, 3)
    mha.causal = True
    lin1, lin2 = nk.nn.Linear(tdev, D_, HID, 1), nk.nn.Linear(tdev, HID, D_, 2)
    X = nk.from_ndarray(tdev, x).requires_grad()
    h = X + mha.forward(ln1.forward(X), B_)
    out = h + lin2.forward(lin1.forward(ln2.forward(h)).relu())
    loss = out.mse(nk.from_ndarray(tdev, t), nk.Reduction.Mean)
    return dict(X=X, ln1=ln1, ln2=ln2, mha=mha, lin1=lin1, lin2=lin2, out=out, loss=loss)


def _block_oracle(m, x, t, dt):
    c = lambda v: v.data().astype(dt)
    x, t = x.astype(dt), t.astype(dt)
    w1, b1, w2, b2 = c(m["ln1"].weight), c(m["ln1"].bias), c(m["ln2"].weight), c(m["ln2"].bias)
    proj = [c(getattr(getattr(m["mha"], n), p)) for n in "qkvo" for p in ("weight", "bias")]
    W1, B1, W2, B2 = c(m["lin1"].weight), c(m["lin1"].bias), c(m["lin2"].weight), c(m["lin2"].bias)
    ones = np.ones((B_ * H_, S_, S_), dt)
    a1, st1 = LN.forward(x, w1, b1, 1e-5)
    att, _ = CO.mha_forward_backward(a1, *proj, H_, B_, 0.0, ones, np.zeros_like(x), causal=True)
    h = x + att
    a2, st2 = LN.forward(h, w2, b2, 1e-5)
    z1 = O.linear_forward(a2, W1, B1)
    r = np.zeros_like(z1); O.relu_forward(z1, r)
    out = h + O.linear_forward(r, W2, B2)
    loss = np.zeros((), dt); O.squared_error_forward(out, t, loss, "mean")
    dout = np.zeros_like(out); O.squared_error_backward(dout, np.ones((), dt), out, t, "mean")
    dr = np.zeros_like(r); O.mm_t_backward_left(dr, dout, W2)
    dz1 = np.zeros_like(z1); O.relu_backward(dz1, dr, z1)
    da2 = np.zeros_like(a2); O.mm_t_backward_left(da2, dz1, W1)
    dh2, dw2, db2 = LN.backward(da2, h, w2, st2)
    dh = dout + dh2
    _, grads = CO.mha_forward_backward(a1, *proj, H_, B_, 0.0, ones, dh, causal=True)
    dx1, dw1, db1 = LN.backward(grads["x"], x, w1, st1)
    return dict(loss=loss, out=out, dx=dh + dx1, dw1=dw1, db1=db1, dw2=dw2, db2=db2, g1=grads["x"], g2=da2, a1=a1, a2=a2)


def test_pre_ln_block_equals_the_oracles_chain(nk, tdev):
    x, t = rnd(60, (B_ * S_, D_)), rnd(61, (B_ * S_, D_))
    m = _block(nk, tdev, x, t)
    m["loss"].forward(); m["loss"].backward(1.0)
    o64, o32 = _block_oracle(m, x, t, np.float64), _block_oracle(m, x, t, np.float32)
    _check(m["loss"].item(), o64["loss"], o32["loss"], "block loss")
    _check(m["out"].data(), o64["out"], o32["out"], "block out")
    _check(m["X"].grad(), o64["dx"], o32["dx"], "block dx")
    rows = B_ * S_
    for ln, k, g, a in ((m["ln1"], "1", "g1", "a1"), (m["ln2"], "2", "g2", "a2")):
        _param_check(ln.weight.grad(), o64["dw" + k], o32["dw" + k], "block dgamma" + k, rows, np.abs(o64[g]).max(), np.abs(o64[a]).max())
        _param_check(ln.bias.grad(), o64["db" + k], o32["db" + k], "block dbeta" + k, rows, np.abs(o64[g]).max(), 1.0)


def test_pre_ln_block_step_captured_equals_eager(nk, tdev):
    """The training step of the block (forward, backward, SGD) captured into a graph and replayed gives the parameters the same
    steps give eagerly, bit for bit: nothing in the layer synchronises, allocates or leaves the compute stream."""
    x, t = rnd(60, (B_ * S_, D_)), rnd(61, (B_ * S_, D_))

    def make():
        m = _block(nk, tdev, x, t)
        params = [p for l in (m["ln1"], m["ln2"], m["lin1"], m["lin2"]) for p in (l.weight, l.bias)]
        params += [getattr(getattr(m["mha"], n), p) for n in "qkvo" for p in ("weight", "bias")]
        opt = nk.optim.SGD(0.05)
        for p in params:
            opt.register(p)
        loss = m["loss"]

        def step():
            loss.forward()
            loss.no_grad(); loss.with_grad()
            loss.backward(1.0)
            opt.step()
            opt.zero_grad()
        return m, params, step

    me, pe, step_e = make()
    for _ in range(6):
        step_e()
    want = [p.data().copy() for p in pe]
    mg, pg, step_g = make()
    step_g(); step_g()                       # warm the allocator / workspace, reach the steady state
    tdev.graph_begin()
    step_g()
    graph = tdev.graph_end()                 # capturing records the step, it does not run it
    for _ in range(4):
        graph.launch()
    for p, w in zip(pg, want):
        assert np.array_equal(p.data(), w)
    assert np.isfinite(mg["loss"].item()) and mg["loss"].item() == me["loss"].item()
    assert not np.array_equal(pg[0].data(), 1.0 + 0.5 * rnd(40, (D_,)))           # ln1.weight moved
    del graph

"""`nn::RMSNorm` and `Var / VarDiff::rms_norm` through the tape (`_tape`) against tests/rms_norm_oracle.py: the module on 2-D, 3-D
and 4-D input, every differentiability combination, the graph size, the input used twice, SGD and AdamW, serde, and a pre-norm
block (RMSNorm -> Linear -> SwiGLU -> Linear -> + h -> MSE) against the oracles' chain, eager and captured.  The last test pins
`nn::LayerNorm`: the same entry counts and, on one small case, the bits recorded before this layer existed."""
import os

import numpy as np
import pytest

import activation_oracle as ACT
import adamw_oracle as AW
import layernorm_oracle as LN
import rms_norm_oracle as RN

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layernorm_small_bits.npy")


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
    print("rmsnorm:tape %s err_gpu=%.3e err_cpu32=%.3e abs=%.3e" % (what, err_gpu, err_cpu, 1e-6 * scale))
    record_margin("rmsnorm:tape " + what, err_gpu, err_cpu, 1e-6 * scale)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)


def _param_check(got, want, want32, what, rows, gmax, xhatmax):
    from tolerance import assert_contraction
    assert_contraction("rmsnorm:tape " + what, np.asarray(got).reshape(np.shape(want)), want, rows, gmax, xhatmax, cpu32=want32)


def _xhat_max(x, D, eps):
    return float(np.abs(RN.forward(x.reshape(-1, D).astype(np.float64), None, eps)[0]).max())


def _set_weight(rn, seed):
    w = 1.0 + 0.5 * rnd(seed, tuple(rn.normalized_shape))
    rn.weight.set_data(w)
    return w


@pytest.mark.parametrize("shape,normalized", [((96, 256), (256,)), ((37, 100), (100,)), ((4, 9, 64), (64,)), ((3, 5, 8, 16), (8, 16)), ((4, 3000), (3000,))])
def test_module_equals_oracle(nk, tdev, shape, normalized):
    D = int(np.prod(normalized)); rows = int(np.prod(shape)) // D
    x, g = rnd(1, shape), rnd(2, shape)
    rn = nk.nn.RMSNorm(tdev, list(normalized))
    assert rn.eps == 1e-6 and rn.elementwise_affine and list(rn.normalized_shape) == list(normalized)
    assert np.array_equal(rn.weight.data(), np.ones(normalized, np.float32))
    w = _set_weight(rn, 10)
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = rn.forward(X)
    assert tuple(y.shape) == shape
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    o64, o32 = RN.both(x.reshape(rows, D), w.reshape(D), g.reshape(rows, D), 1e-6)
    _check(y.data(), o64["y"], o32["y"], "y")
    _check(X.grad(), o64["dx"], o32["dx"], "dx")
    _param_check(rn.weight.grad(), o64["dgamma"], o32["dgamma"], "dgamma", rows, np.abs(g).max(), _xhat_max(x, D, 1e-6))
    # a second backward() on the same graph accumulates into the leaves; the node's own gradient is re-seeded
    first = [X.grad().copy(), rn.weight.grad().copy()]
    y.backward_from(nk.from_ndarray(tdev, g))
    for got, one in zip((X.grad(), rn.weight.grad()), first):
        np.testing.assert_allclose(got, 2 * one, rtol=1e-6, atol=1e-6)


def test_without_affine_and_var_forms(nk, tdev):
    rows, D = 50, 192
    x, g = rnd(3, (rows, D)), rnd(4, (rows, D))
    o64, o32 = RN.both(x, None, g, 1e-3)
    rn = nk.nn.RMSNorm(tdev, [D], eps=1e-3, elementwise_affine=False)
    assert rn.weight is None and not rn.elementwise_affine
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = rn.forward(X); y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    _check(y.data(), o64["y"], o32["y"], "y plain")
    _check(X.grad(), o64["dx"], o32["dx"], "dx plain")
    with pytest.raises(RuntimeError):
        rn.forward(nk.from_ndarray(tdev, x))                                       # nothing to differentiate
    # the Var forms: no gradient, no statistics kept
    v = nk.from_ndarray(tdev, x).rms_norm([D], 1e-3); v.forward()
    assert np.array_equal(v.data(), y.data())
    w = 1.0 + 0.5 * rnd(5, (D,))
    a64, a32 = RN.both(x, w, g, 1e-6)
    v = nk.from_ndarray(tdev, x).rms_norm(nk.from_ndarray(tdev, w)); v.forward()   # eps defaults to 1e-6
    _check(v.data(), a64["y"], a32["y"], "y Var form")
    # shapes that do not fit, a negative eps
    with pytest.raises(RuntimeError):
        nk.from_ndarray(tdev, x).rms_norm([D + 1], 1e-6)
    with pytest.raises(RuntimeError):
        nk.from_ndarray(tdev, x).rms_norm(nk.from_ndarray(tdev, w[:-1].copy()))
    with pytest.raises(RuntimeError):
        nk.from_ndarray(tdev, x).rms_norm([D], -1.0)


def test_gradients_flow_to_each_differentiable_operand_alone(nk, tdev):
    rows, D = 64, 512
    x, g = rnd(7, (rows, D)), rnd(8, (rows, D))
    w = 1.0 + 0.5 * rnd(9, (D,))
    o64, o32 = RN.both(x, w, g, 1e-6)
    G = nk.from_ndarray(tdev, g)
    xm = _xhat_max(x, D, 1e-6)
    # x is a plain Var: only dgamma runs
    W = nk.from_ndarray(tdev, w).requires_grad()
    y = nk.from_ndarray(tdev, x).rms_norm(W, 1e-6)
    assert y.history_len() == 1
    y.forward(); y.backward_from(G)
    _check(y.data(), o64["y"], o32["y"], "y gamma only")
    _param_check(W.grad(), o64["dgamma"], o32["dgamma"], "dgamma only", rows, np.abs(g).max(), xm)
    # gamma is a plain Var: only dx runs
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = X.rms_norm(nk.from_ndarray(tdev, w), 1e-6)
    assert y.history_len() == 1
    y.forward(); y.backward_from(G)
    _check(X.grad(), o64["dx"], o32["dx"], "dx only")
    # one weight shared by two layers: the second writer accumulates (first writer assigns, per gradient)
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = X.rms_norm(W, 1e-6) + X.rms_norm(W, 1e-6)
    W.zero_grad()
    y.forward(); y.backward_from(G)
    _param_check(W.grad(), 2 * o64["dgamma"], 2 * o32["dgamma"], "dgamma shared", 2 * rows, np.abs(g).max(), xm)
    _check(X.grad(), 2 * o64["dx"], 2 * o32["dx"], "dx shared")


def test_the_node_adds_one_forward_and_one_backward_entry(nk, tdev):
    x = nk.from_ndarray(tdev, rnd(1, (8, 32))).requires_grad()
    rn = nk.nn.RMSNorm(tdev, [32])
    base = x.relu()
    y = rn.forward(base)
    assert y.history_len() == base.history_len() + 1                               # dx and dgamma leave ONE backward entry
    assert y.forward_history_len() == base.forward_history_len() + 1
    assert nk.from_ndarray(tdev, rnd(1, (8, 32))).rms_norm([32]).history_len() == 1


@pytest.mark.parametrize("norm_writes_first", [False, True])
def test_input_used_twice(nk, tdev, norm_writes_first):
    """y = rms(h).mm(W) + other(h): h's gradient is the sum of both uses, whether the norm's backward entry is the first writer of
    it (the other use, a ReLU, was recorded before the norm and so runs after it) or a later one (the residual `+ h` itself)."""
    rows, D = 48, 64
    h, g, w, m = rnd(1, (rows, D)), rnd(2, (rows, D)), 1.0 + 0.5 * rnd(3, (D,)), rnd(4, (D, D)) * 0.2
    H, W = nk.from_ndarray(tdev, h).requires_grad(), nk.from_ndarray(tdev, w).requires_grad()
    other = H.relu() if norm_writes_first else H
    y = H.rms_norm(W, 1e-6).mm(nk.from_ndarray(tdev, m)) + other
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    want = []
    for dt in (np.float64, np.float32):
        c = lambda a: a.astype(dt)
        a, st = RN.forward(c(h), c(w), 1e-6)
        out = a @ c(m) + (np.maximum(c(h), 0) if norm_writes_first else c(h))
        da = c(g) @ c(m).T
        dx, dg = RN.backward(da, c(h), c(w), st)
        want.append(dict(y=out, dh=dx + (c(g) * (c(h) > 0) if norm_writes_first else c(g)), dg=dg, da=da))
    _check(y.data(), want[0]["y"], want[1]["y"], "twice y")
    _check(H.grad(), want[0]["dh"], want[1]["dh"], "twice dh")
    _param_check(W.grad(), want[0]["dg"], want[1]["dg"], "twice dgamma", rows, np.abs(want[0]["da"]).max(), _xhat_max(h, D, 1e-6))


def _one_step_oracles(x, t, w, dt):
    y, st = RN.forward(x.astype(dt), w.astype(dt), 1e-6)
    g = (2 * (y - t.astype(dt))) / dt(y.size)
    return RN.backward(g, x.astype(dt), w.astype(dt), st)[1]


def test_sgd_step_moves_weight_as_the_oracle_says(nk, tdev):
    rows, D, lr = 40, 128, 0.1
    x, t = rnd(11, (rows, D)), rnd(12, (rows, D))
    rn = nk.nn.RMSNorm(tdev, [D])
    w = _set_weight(rn, 20)
    loss = rn.forward(nk.from_ndarray(tdev, x)).mse(nk.from_ndarray(tdev, t), nk.Reduction.Mean)
    opt = nk.optim.SGD(lr)
    opt.register(rn.weight)
    loss.forward(); loss.backward(1.0); opt.step()
    want = [w.astype(dt) - dt(lr) * _one_step_oracles(x, t, w, dt) for dt in (np.float64, np.float32)]
    assert not np.array_equal(rn.weight.data(), w)
    _check(rn.weight.data(), want[0], want[1], "sgd weight")


def test_adamw_step_moves_weight_as_the_oracle_says(nk, tdev):
    rows, D = 40, 128
    hp = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
    x, t = rnd(13, (rows, D)), rnd(14, (rows, D))
    rn = nk.nn.RMSNorm(tdev, [D])
    w = _set_weight(rn, 21)
    loss = rn.forward(nk.from_ndarray(tdev, x)).mse(nk.from_ndarray(tdev, t), nk.Reduction.Mean)
    opt = nk.optim.AdamW(**hp)
    opt.register(rn.weight)
    loss.forward(); loss.backward(1.0); opt.step()
    f = lambda v: float(np.float32(v))                                             # the host class stores f32
    want = []
    for dt in (np.float64, np.float32):
        ww = w.astype(dt)
        AW.adamw_step(ww, _one_step_oracles(x, t, w, dt), np.zeros(D, dt), np.zeros(D, dt), f(hp["lr"]), f(hp["beta1"]), f(hp["beta2"]), f(hp["eps"]), 1,
                      f(hp["weight_decay"]))
        want.append(ww)
    assert np.abs(rn.weight.data() - w).max() > 0.5 * hp["lr"]                     # the first AdamW step moves every weight by about lr
    _check(rn.weight.data(), want[0], want[1], "adamw weight")


def test_serde_round_trip_is_bit_exact(nk, tdev):
    rn = nk.nn.RMSNorm(tdev, [4, 6])
    w = _set_weight(rn, 30)
    text = nk.serde.to_json(rn)
    assert text.startswith('{"weight":{"v":1,"dim":[4,6],"data":[') and "bias" not in text
    back = nk.serde.rms_norm_from_json(tdev, text)
    assert list(back.normalized_shape) == [4, 6] and back.eps == 1e-6 and back.elementwise_affine
    assert np.array_equal(back.weight.data(), w)
    assert nk.serde.rms_norm_from_json(tdev, text, eps=1e-5).eps == 1e-5
    x = rnd(2, (5, 4, 6))
    a, c = rn.forward(nk.from_ndarray(tdev, x)), back.forward(nk.from_ndarray(tdev, x))
    a.forward(); c.forward()
    assert np.array_equal(a.data(), c.data())
    with pytest.raises(RuntimeError):
        nk.serde.to_json(nk.nn.RMSNorm(tdev, [4], elementwise_affine=False))


# ---- a pre-norm gated block ---------------------------------------------------------------------------------------------------
N_, D_, HID = 96, 128, 192


def _block(nk, tdev, x, t):
    """out = h + lin2(glu_silu(lin1(rms(h)))); loss = MSE(out, t)"""
    rn = nk.nn.RMSNorm(tdev, [D_])
    _set_weight(rn, 40)
    lin1, lin2 = nk.nn.Linear(tdev, D_, 2 * HID, 1), nk.nn.Linear(tdev, HID, D_, 2)
    X = nk.from_ndarray(tdev, x).requires_grad()
    out = lin2.forward(lin1.forward(rn.forward(X)).glu(nk.Activation.Silu)) + X
    loss = out.mse(nk.from_ndarray(tdev, t), nk.Reduction.Mean)
    return dict(X=X, rn=rn, lin1=lin1, lin2=lin2, out=out, loss=loss)


def _swiglu(z, dt):
    """(a * silu(b), silu(b), silu'(b)) for z = [a | b], in dtype dt (tests/activation_oracle.py is f64 only; the f64 pass is
    compared with it below)"""
    a, b = z[:, :HID], z[:, HID:]
    s = dt(1) / (dt(1) + np.exp(-b))
    return a * (b * s), b * s, s * (dt(1) + b * (dt(1) - s))


def _block_oracle(m, x, t, dt):
    c = lambda v: v.data().astype(dt)
    x, t = x.astype(dt), t.astype(dt)
    w, W1, B1, W2, B2 = c(m["rn"].weight), c(m["lin1"].weight), c(m["lin1"].bias), c(m["lin2"].weight), c(m["lin2"].bias)
    a, st = RN.forward(x, w, 1e-6)
    z = a @ W1.T + B1
    u, v, d = _swiglu(z, dt)
    out = u @ W2.T + B2 + x
    diff = out - t
    loss = (diff * diff).mean(dtype=dt)
    dout = dt(2) * diff / dt(diff.size)
    du = dout @ W2
    dz = np.concatenate([du * v, du * z[:, :HID] * d], axis=1)
    da = dz @ W1
    dx, dw = RN.backward(da, x, w, st)
    if dt is np.float64:
        assert np.abs(u - ACT.glu_forward("silu", z, HID)).max() <= 1e-12 and np.abs(dz - ACT.glu_backward("silu", z, du, HID)).max() <= 1e-12
    return dict(loss=loss, out=out, dx=dout + dx, dw=dw, da=da, a=a)


def test_pre_norm_block_equals_the_oracles_chain(nk, tdev):
    x, t = rnd(60, (N_, D_)), rnd(61, (N_, D_))
    m = _block(nk, tdev, x, t)
    m["loss"].forward(); m["loss"].backward(1.0)
    o64, o32 = _block_oracle(m, x, t, np.float64), _block_oracle(m, x, t, np.float32)
    _check(m["loss"].item(), o64["loss"], o32["loss"], "block loss")
    _check(m["out"].data(), o64["out"], o32["out"], "block out")
    _check(m["X"].grad(), o64["dx"], o32["dx"], "block dx")
    _param_check(m["rn"].weight.grad(), o64["dw"], o32["dw"], "block dgamma", N_, np.abs(o64["da"]).max(), _xhat_max(x, D_, 1e-6))


def test_pre_norm_block_step_captured_equals_eager(nk, tdev):
    """The training step of the block (forward, backward, SGD) captured into a graph and replayed gives the parameters the same
    steps give eagerly, bit for bit: nothing in the layer synchronises, allocates or leaves the compute stream."""
    x, t = rnd(60, (N_, D_)), rnd(61, (N_, D_))

    def make():
        m = _block(nk, tdev, x, t)
        params = [m["rn"].weight] + [p for l in (m["lin1"], m["lin2"]) for p in (l.weight, l.bias)]
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
    assert not np.array_equal(pg[0].data(), 1.0 + 0.5 * rnd(40, (D_,)))           # the norm's weight moved
    del graph


def test_layer_norm_graphs_are_unchanged(nk, tdev):
    """nn::LayerNorm beside the new layer: one forward and one backward entry as before, and on one small case the bits of y, dx,
    dgamma and dbeta recorded with the LayerNorm kernels as they were before this layer was added (tests/golden)."""
    rows, D = 8, 32
    x, g = rnd(1, (rows, D)), rnd(2, (rows, D))
    ln = nk.nn.LayerNorm(tdev, [D])
    w, b = 1.0 + 0.5 * rnd(10, (D,)), rnd(11, (D,))
    ln.weight.set_data(w); ln.bias.set_data(b)
    X = nk.from_ndarray(tdev, x).requires_grad()
    base = X.relu()
    y = ln.forward(base)
    assert y.history_len() == base.history_len() + 1 and y.forward_history_len() == base.forward_history_len() + 1
    assert nk.from_ndarray(tdev, x).layer_norm([D]).history_len() == 1
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    got = np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in (y.data(), X.grad(), ln.weight.grad(), ln.bias.grad())])
    o64, o32 = LN.both(np.maximum(x, 0), w, b, g, 1e-5)
    _check(got[:rows * D], o64["y"].reshape(-1), o32["y"].reshape(-1), "layernorm y beside rmsnorm")
    want = np.load(GOLDEN)
    assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))

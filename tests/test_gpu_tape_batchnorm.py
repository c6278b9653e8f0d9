"""`nn::BatchNorm1d / 2d / 3d` and `Var / VarDiff::batch_norm` through the tape (`_tape`) against tests/batchnorm_oracle.py: each
module, the train / eval switch, the running statistics over three steps, every differentiability combination, the graph size,
serde, and a Conv2d -> BatchNorm2d -> ReLU -> MSE step with SGD against the oracles' chain, eager and captured."""
import numpy as np
import pytest

from oracle import neuronika_oracle as O
import batchnorm_oracle as BN

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1


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
    record_margin("batchnorm:tape " + what, err_gpu, err_cpu, 1e-6 * scale)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)


def _param_check(got, want, want32, what, K, gmax, ymax):
    from tolerance import assert_contraction
    assert_contraction("batchnorm:tape " + what, np.asarray(got).reshape(np.shape(want)), want, K, gmax, ymax, cpu32=want32)


def _ncl(a):
    return a.reshape(a.shape[0], a.shape[1], -1)


def _set_params(bn, seed):
    C = bn.num_features
    w, b = 1.0 + 0.5 * rnd(seed, (C,)), rnd(seed + 1, (C,))
    bn.weight.set_data(w); bn.bias.set_data(b)
    return w, b


def _compare(bn_out, X, bn, o64, o32, x, g, tag):
    K = x.size // x.shape[1]
    _check(bn_out.data(), o64["y"], o32["y"], "y " + tag)
    _check(X.grad(), o64["dx"], o32["dx"], "dx " + tag, floor=1.0)
    _param_check(bn.weight.grad(), o64["dgamma"], o32["dgamma"], "dgamma " + tag, K, np.abs(g).max(), max(1.0, np.abs(o64["y"]).max()))
    _param_check(bn.bias.grad(), o64["dbeta"], o32["dbeta"], "dbeta " + tag, K, np.abs(g).max(), 1.0)


@pytest.mark.parametrize("cls,shape", [("BatchNorm1d", (64, 24)), ("BatchNorm1d", (12, 6, 50)), ("BatchNorm2d", (4, 8, 16, 16)),
                                       ("BatchNorm2d", (3, 5, 7, 7)), ("BatchNorm3d", (2, 4, 3, 8, 16))])
def test_module_equals_oracle(nk, tdev, cls, shape):
    C = shape[1]
    x, g = rnd(1, shape, -2.0, 3.0), rnd(2, shape)
    bn = getattr(nk.nn, cls)(tdev, C)
    assert bn.eps == 1e-5 and bn.momentum == 0.1 and bn.affine and bn.track_running_stats and bn.num_features == C and bn.training
    assert np.array_equal(bn.weight.data(), np.ones(C, np.float32)) and np.array_equal(bn.bias.data(), np.zeros(C, np.float32))
    assert np.array_equal(bn.running_mean.data(), np.zeros(C, np.float32)) and np.array_equal(bn.running_var.data(), np.ones(C, np.float32))
    w, b = _set_params(bn, 10)
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = bn.forward(X)
    assert tuple(y.shape) == shape
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    o64, o32 = BN.both(_ncl(x), w, b, _ncl(g), EPS, MOM, (np.zeros(C, np.float32), np.ones(C, np.float32)))
    _compare(y, X, bn, o64, o32, x, g, cls)
    _check(bn.running_mean.data(), o64["running_mean"], o32["running_mean"], "running_mean " + cls, floor=1.0)
    _check(bn.running_var.data(), o64["running_var"], o32["running_var"], "running_var " + cls, floor=1.0)


def test_train_eval_train_and_three_steps_of_running_statistics(nk, tdev):
    shape, C = (6, 5, 12, 12), 5
    bn = nk.nn.BatchNorm2d(tdev, C, eps=1e-3, momentum=0.25)
    w, b = _set_params(bn, 20)
    xs = [rnd(30 + i, shape, -1.0 - i, 2.0) for i in range(4)]
    g = rnd(29, shape)
    X = nk.from_ndarray(tdev, xs[0]).requires_grad()
    y = bn.forward(X)
    running = [(np.zeros(C, np.float32), np.ones(C, np.float32))] * 2               # f64 and f32 histories
    for i in range(3):                                                             # three training steps on the same graph
        X.set_data(xs[i])
        y.forward()
        o64, o32 = BN.both(_ncl(xs[i]), w, b, _ncl(g), 1e-3, 0.25, running[0])
        _, o32 = BN.both(_ncl(xs[i]), w, b, _ncl(g), 1e-3, 0.25, running[1])
        running = [(o64["running_mean"], o64["running_var"]), (o32["running_mean"], o32["running_var"])]
        _check(y.data(), o64["y"], o32["y"], "y step %d" % i)
    _check(bn.running_mean.data(), running[0][0], running[1][0], "running_mean after three steps", floor=1.0)
    _check(bn.running_var.data(), running[0][1], running[1][1], "running_var after three steps", floor=1.0)
    # eval: the running statistics normalise, nothing is updated, the gradient takes the inference form
    bn.eval()
    assert not bn.training
    rm, rv = bn.running_mean.data().copy(), bn.running_var.data().copy()
    X.set_data(xs[3]); X.zero_grad(); bn.weight.zero_grad(); bn.bias.zero_grad()
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    assert np.array_equal(bn.running_mean.data(), rm) and np.array_equal(bn.running_var.data(), rv)
    e64, e32 = BN.both(_ncl(xs[3]), w, b, _ncl(g), 1e-3, 0.25, (rm, rv), training=False)
    _compare(y, X, bn, e64, e32, xs[3], g, "eval")
    # and back: the batch statistics again, the running ones move again
    bn.train()
    X.zero_grad(); bn.weight.zero_grad(); bn.bias.zero_grad()
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    t64, t32 = BN.both(_ncl(xs[3]), w, b, _ncl(g), 1e-3, 0.25, (rm, rv))
    _compare(y, X, bn, t64, t32, xs[3], g, "train again")
    _check(bn.running_mean.data(), t64["running_mean"], t32["running_mean"], "running_mean train again", floor=1.0)


def test_without_affine_without_tracking_and_var_forms(nk, tdev):
    shape, C = (8, 6, 30), 6
    x, g = rnd(3, shape), rnd(4, shape)
    o64, o32 = BN.both(_ncl(x), None, None, _ncl(g), 1e-3, MOM, None)
    bn = nk.nn.BatchNorm1d(tdev, C, eps=1e-3, affine=False, track_running_stats=False)
    assert bn.weight is None and bn.bias is None and bn.running_mean is None and bn.running_var is None
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = bn.forward(X); y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    _check(y.data(), o64["y"], o32["y"], "y plain")
    _check(X.grad(), o64["dx"], o32["dx"], "dx plain", floor=1.0)
    bn.eval()                                                                      # no running statistics: the batch's in both modes
    first = y.data().copy()
    y.forward()
    assert np.array_equal(y.data(), first)
    with pytest.raises(RuntimeError):
        bn.forward(nk.from_ndarray(tdev, x))                                       # nothing to differentiate
    # the Var form: no gradient, no statistics kept
    st = nk.Status(True)
    v = nk.from_ndarray(tdev, x).batch_norm(None, None, None, None, MOM, 1e-3, st); v.forward()
    assert np.array_equal(v.data(), first)
    w, b = 1.0 + 0.5 * rnd(5, (C,)), rnd(6, (C,))
    rm, rv = rnd(7, (C,)), 0.5 + rnd(8, (C,), 0.0, 1.0)
    RM, RV = nk.from_ndarray(tdev, rm), nk.from_ndarray(tdev, rv)
    st.set(False)
    v = nk.from_ndarray(tdev, x).batch_norm(nk.from_ndarray(tdev, w), nk.from_ndarray(tdev, b), RM, RV, MOM, EPS, st); v.forward()
    i64, i32 = BN.both(_ncl(x), w, b, _ncl(g), EPS, MOM, (rm, rv), training=False)
    _check(v.data(), i64["y"], i32["y"], "y Var form, inference")
    st.set(True)
    v.forward()
    a64, a32 = BN.both(_ncl(x), w, b, _ncl(g), EPS, MOM, (rm, rv))
    _check(v.data(), a64["y"], a32["y"], "y Var form, training")
    _check(RM.data(), a64["running_mean"], a32["running_mean"], "running_mean Var form", floor=1.0)


def test_wrong_inputs_panic_with_a_message(nk, tdev):
    x4, x2 = nk.from_ndarray(tdev, rnd(1, (2, 3, 4, 4))).requires_grad(), nk.from_ndarray(tdev, rnd(1, (2, 3))).requires_grad()
    for layer, bad in ((nk.nn.BatchNorm1d(tdev, 3), x4), (nk.nn.BatchNorm2d(tdev, 3), x2), (nk.nn.BatchNorm3d(tdev, 3), x4), (nk.nn.BatchNorm2d(tdev, 4), x4)):
        with pytest.raises(RuntimeError) as e:
            layer.forward(bad)
        assert "BatchNorm" in str(e.value)
    with pytest.raises(RuntimeError):
        nk.nn.BatchNorm2d(tdev, 0)
    st = nk.Status(True)
    p3, p4 = nk.from_ndarray(tdev, rnd(2, (3,))), nk.from_ndarray(tdev, rnd(2, (4,)))
    for call in (lambda: x4.batch_norm(p4, p3, None, None, MOM, EPS, st), lambda: x4.batch_norm(p3, p3, p3, None, MOM, EPS, st),
                 lambda: x4.batch_norm(p3, p3, None, None, 1.5, EPS, st), lambda: x4.batch_norm(p3, p3, None, None, MOM, -1.0, st)):
        with pytest.raises(RuntimeError):
            call()
    # one value per channel has no variance: training panics when the node runs, inference does not
    one = nk.from_ndarray(tdev, rnd(3, (1, 3))).requires_grad()
    bn = nk.nn.BatchNorm1d(tdev, 3)
    y = bn.forward(one)
    with pytest.raises(RuntimeError) as e:
        y.forward()
    assert "variance" in str(e.value)
    bn.eval()
    y.forward()


def test_gradients_flow_to_each_differentiable_operand_alone(nk, tdev):
    shape, C = (8, 16, 10, 10), 16
    x, g = rnd(7, shape), rnd(8, shape)
    w, b = 1.0 + 0.5 * rnd(9, (C,)), rnd(10, (C,))
    o64, o32 = BN.both(_ncl(x), w, b, _ncl(g), EPS, MOM, None)
    G, st, K = nk.from_ndarray(tdev, g), nk.Status(True), x.size // C
    # x is a plain Var: only the parameter gradients run
    W, B = nk.from_ndarray(tdev, w).requires_grad(), nk.from_ndarray(tdev, b).requires_grad()
    y = nk.from_ndarray(tdev, x).batch_norm(W, B, None, None, MOM, EPS, st)
    assert y.history_len() == 1
    y.forward(); y.backward_from(G)
    _check(y.data(), o64["y"], o32["y"], "y params only")
    _param_check(W.grad(), o64["dgamma"], o32["dgamma"], "dgamma params only", K, np.abs(g).max(), np.abs(o64["y"]).max())
    _param_check(B.grad(), o64["dbeta"], o32["dbeta"], "dbeta params only", K, np.abs(g).max(), 1.0)
    # the parameters are plain Vars: only dx runs
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = X.batch_norm(nk.from_ndarray(tdev, w), nk.from_ndarray(tdev, b), None, None, MOM, EPS, st)
    assert y.history_len() == 1
    y.forward(); y.backward_from(G)
    _check(X.grad(), o64["dx"], o32["dx"], "dx only", floor=1.0)
    # one parameter pair shared by two layers: the second writer accumulates (first writer assigns, per gradient)
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = X.batch_norm(W, B, None, None, MOM, EPS, st) + X.batch_norm(W, B, None, None, MOM, EPS, st)
    W.zero_grad(); B.zero_grad()
    y.forward(); y.backward_from(G)
    _param_check(W.grad(), 2 * o64["dgamma"], 2 * o32["dgamma"], "dgamma shared", 2 * K, np.abs(g).max(), np.abs(o64["y"]).max())
    _check(X.grad(), 2 * o64["dx"], 2 * o32["dx"], "dx shared", floor=1.0)


def test_the_node_adds_one_forward_and_one_backward_entry(nk, tdev):
    x = nk.from_ndarray(tdev, rnd(1, (8, 4, 6, 6))).requires_grad()
    bn = nk.nn.BatchNorm2d(tdev, 4)
    base = x.relu()
    y = bn.forward(base)
    assert y.history_len() == base.history_len() + 1                               # sums, dx, dgamma and dbeta leave ONE backward entry
    assert y.forward_history_len() == base.forward_history_len() + 1


def test_serde_round_trip(nk, tdev):
    bn = nk.nn.BatchNorm2d(tdev, 7)
    _set_params(bn, 50)
    X = nk.from_ndarray(tdev, rnd(51, (4, 7, 5, 5), -3.0, 1.0)).requires_grad()
    bn.forward(X).forward()                                                        # running statistics that are not 0 and 1
    text = nk.serde.to_json(bn)
    for cls in (nk.nn.BatchNorm2d, nk.nn.BatchNorm1d):                             # the wire format does not name the rank
        back = cls(tdev, 7)
        nk.serde.batch_norm_load_json(back, text)
        for name in ("weight", "bias", "running_mean", "running_var"):
            assert np.array_equal(getattr(back, name).data(), getattr(bn, name).data()), name
        assert nk.serde.to_json(back) == text
    assert not np.array_equal(bn.running_mean.data(), np.zeros(7, np.float32))
    with pytest.raises(RuntimeError):
        nk.serde.batch_norm_load_json(nk.nn.BatchNorm2d(tdev, 8), text)


# ---- Conv2d -> BatchNorm2d -> ReLU -> MSE ---------------------------------------------------------------------------------------
N_, CI_, CO_, H_, W_ = 8, 4, 16, 16, 16
LR_ = 0.05


def _model(nk, tdev, x, t):
    conv = nk.nn.Conv2d(tdev, CI_, CO_, [3, 3], [1, 1], nk.PaddingMode.zero(), [1, 1], [1, 1], 3)
    bn = nk.nn.BatchNorm2d(tdev, CO_)
    bn.weight.set_data(1.0 + 0.5 * rnd(40, (CO_,))); bn.bias.set_data(0.2 * rnd(41, (CO_,)))
    X = nk.from_ndarray(tdev, x).requires_grad()
    loss = bn.forward(conv.forward(X)).relu().mse(nk.from_ndarray(tdev, t), nk.Reduction.Mean)
    return dict(conv=conv, bn=bn, X=X, loss=loss, params=[conv.weight, conv.bias, bn.weight, bn.bias])


def _oracle_step(x, t, p, running, dt):
    """one training step of the chain in dtype `dt`: the loss, the gradients of (conv weight, conv bias, gamma, beta), the new
    running statistics"""
    w, cb, gamma, beta = (np.asarray(a, dt) for a in p)
    xp = np.zeros((N_, CI_, H_ + 2, W_ + 2), dt); O.pad_constant_forward(np.asarray(x, dt), xp, (1, 1), 0.0)
    z = np.zeros((N_, CO_, H_, W_), dt); O.convolution_forward(xp, w, z, (1, 1), (1, 1), 1)
    z = z + cb
    st, var = BN.batch_stats(_ncl(z), EPS)
    rm, rv = BN.running_update(np.asarray(running[0], dt), np.asarray(running[1], dt), st, var, N_ * H_ * W_, MOM)
    y = BN.normalise(_ncl(z), st, gamma, beta).reshape(z.shape)
    a = np.maximum(y, 0)
    d = a - np.asarray(t, dt)
    loss = (d * d).mean(dtype=dt)
    ga = (2 * d / dt(d.size)) * (y > 0)
    _, dz, dgamma, dbeta = BN.backward(_ncl(ga), _ncl(z), gamma, st)
    dz = dz.reshape(z.shape)
    dw = np.zeros_like(w); O.convolution_backward_kernel(dw, np.ascontiguousarray(dz), xp, (1, 1), (1, 1), 1)
    return loss, [dw, dz.sum((0, 2, 3)).reshape(cb.shape), dgamma, dbeta], (rm, rv)


def test_conv_bn_relu_step_equals_the_oracles_chain(nk, tdev):
    x, t = rnd(60, (N_, CI_, H_, W_)), rnd(61, (N_, CO_, H_, W_), 0.0, 1.0)
    m = _model(nk, tdev, x, t)
    opt = nk.optim.SGD(LR_)
    for p in m["params"]:
        opt.register(p)
    p64 = [p.data().astype(np.float64) for p in m["params"]]
    running = (np.zeros(CO_), np.ones(CO_))
    for step in range(3):
        m["loss"].forward()
        m["loss"].no_grad(); m["loss"].with_grad()                                 # the intermediate gradients start from zero again
        m["loss"].backward(1.0)
        loss, grads, running = _oracle_step(x, t, p64, running, np.float64)
        np.testing.assert_allclose(m["loss"].item(), loss, rtol=2e-5)
        for p, gr, name in zip(m["params"], grads, ("conv weight", "conv bias", "gamma", "beta")):
            np.testing.assert_allclose(p.grad().reshape(gr.shape), gr, rtol=2e-3, atol=2e-6, err_msg="%s, step %d" % (name, step))
        opt.step(); opt.zero_grad()
        p64 = [a - LR_ * gr for a, gr in zip(p64, grads)]
        for p, a in zip(m["params"], p64):
            np.testing.assert_allclose(p.data(), a, rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(m["bn"].running_mean.data(), running[0], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(m["bn"].running_var.data(), running[1], rtol=1e-4, atol=1e-6)


def test_conv_bn_relu_step_captured_equals_eager(nk, tdev):
    """The training step (forward, backward, SGD) captured into a graph and replayed gives the parameters AND the running statistics
    the same steps give eagerly, bit for bit: nothing in the layer synchronises, allocates or leaves the compute stream, and the
    in-place update of the running statistics is part of the captured work."""
    x, t = rnd(60, (N_, CI_, H_, W_)), rnd(61, (N_, CO_, H_, W_), 0.0, 1.0)

    def make():
        m = _model(nk, tdev, x, t)
        opt = nk.optim.SGD(LR_)
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

    me, step_e = make()
    for _ in range(5):
        step_e()
    mg, step_g = make()
    step_g(); step_g()                       # eager steps first: the workspace has its size before capture begins
    tdev.graph_begin()
    step_g()
    graph = tdev.graph_end()                 # capturing records the step, it does not run it
    for _ in range(3):
        graph.launch()
    for pe, pg in zip(me["params"], mg["params"]):
        assert np.array_equal(pe.data(), pg.data())
    for name in ("running_mean", "running_var"):
        assert np.array_equal(getattr(me["bn"], name).data(), getattr(mg["bn"], name).data()), name
    assert np.isfinite(mg["loss"].item()) and mg["loss"].item() == me["loss"].item()
    assert not np.array_equal(mg["bn"].running_mean.data(), np.zeros(CO_, np.float32))
    del graph

"""`nn::GroupNorm`, `nn::InstanceNorm1d / 2d / 3d` and `Var / VarDiff::group_norm` through the tape (`_tape`) against
tests/group_norm_oracle.py: a small Conv2d -> GroupNorm -> SiLU -> sum graph, the node as first and as later writer of a gradient,
a parameter shared by two layers, the forms without parameters, serde, the captured step, and the refusals.  The norm's own
outputs are held to the suite's rule on the device's own input of the norm (the convolution's output, read back)."""
import numpy as np
import pytest

import group_norm_oracle as GN

pytestmark = pytest.mark.gpu

EPS = 1e-5
N_, CI_, C_, H_, W_, G_ = 2, 3, 8, 6, 6, 4


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


def _ncl(a):
    return np.asarray(a).reshape(a.shape[0], a.shape[1], -1)


def _check(got, want, want32, what, scale=None):
    from conftest import record_margin
    got, want, want32 = (np.asarray(a).reshape(np.shape(want)) for a in (got, want, want32))
    scale = float(np.abs(want).max()) if scale is None else scale
    err_gpu, err_cpu = float(np.abs(got - want).max()), float(np.abs(want32 - want).max())
    print("groupnorm:tape %s err_gpu=%.3e err_cpu32=%.3e abs=%.3e" % (what, err_gpu, err_cpu, 1e-6 * scale))
    record_margin("groupnorm:tape " + what, err_gpu, err_cpu, 1e-6 * scale)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)


def _dx_scale(o64, x, G, g, gamma):
    """the magnitude of the three terms of dx (tests/test_gpu_group_norm.py)"""
    N, C, L = x.shape
    rows = lambda a: np.asarray(a, np.float64).reshape(N * G, -1)
    mean, rstd = o64["stats"][:, :1], o64["stats"][:, 1:]
    xh = (rows(x) - mean) * rstd
    gh = rows(g * (np.asarray(gamma, np.float64).reshape(1, C, 1) if gamma is not None else 1.0))
    return float((rstd * (np.abs(gh) + np.abs(gh.mean(axis=1, keepdims=True)) + np.abs(xh) * np.abs((gh * xh).mean(axis=1, keepdims=True)))).max())


def _params_check(layer, o64, o32, g, x, G, what, times=1):
    from tolerance import assert_contraction
    N, C, L = x.shape
    xh = np.abs((x.reshape(N * G, -1) - o64["stats"][:, :1]) * o64["stats"][:, 1:]).max()
    assert_contraction("groupnorm:tape dgamma " + what, layer.weight.grad().reshape(C), times * o64["dgamma"], times * N * L, np.abs(g).max(), max(1.0, xh),
                       cpu32=times * o32["dgamma"])
    assert_contraction("groupnorm:tape dbeta " + what, layer.bias.grad().reshape(C), times * o64["dbeta"], times * N * L, np.abs(g).max(), 1.0,
                       cpu32=times * o32["dbeta"])


def _silu_grad(y):
    s = 1.0 / (1.0 + np.exp(-y.astype(np.float64)))
    return (s * (1.0 + y * (1.0 - s))).astype(np.float32)


def _set_affine(layer, C, seed):
    w, b = 1.0 + 0.5 * rnd(seed, (C,)), rnd(seed + 1, (C,))
    layer.weight.set_data(w); layer.bias.set_data(b)
    return w, b


def test_conv_group_norm_silu_sum_equals_the_oracle(nk, tdev):
    x = rnd(1, (N_, CI_, H_, W_))
    conv = nk.nn.Conv2d(tdev, CI_, C_, [3, 3], [1, 1], nk.PaddingMode.zero(), [1, 1], [1, 1], 3)
    gn = nk.nn.GroupNorm(tdev, G_, C_)
    assert gn.eps == 1e-5 and gn.affine and gn.num_groups == G_ and gn.num_channels == C_
    assert np.array_equal(gn.weight.data(), np.ones(C_, np.float32)) and np.array_equal(gn.bias.data(), np.zeros(C_, np.float32))
    w, b = _set_affine(gn, C_, 10)
    z = conv.forward(nk.from_ndarray(tdev, x).requires_grad())
    y = gn.forward(z)
    assert tuple(y.shape) == (N_, C_, H_, W_)
    assert y.history_len() == z.history_len() + 1 and y.forward_history_len() == z.forward_history_len() + 1   # ONE entry each way
    loss = y.silu().sum()
    loss.forward(); loss.backward(1.0)
    zd, yd = _ncl(z.data()), _ncl(y.data())
    g = _silu_grad(yd)                                                             # d sum(silu(y)) / dy on the device's own y
    o64, o32 = GN.both(zd, G_, w, b, g, EPS)
    _check(yd, o64["y"], o32["y"], "graph y")
    _check(_ncl(z.grad()), o64["dx"], o32["dx"], "graph dx", scale=_dx_scale(o64, zd, G_, g, w))
    _params_check(gn, o64, o32, g, zd, G_, "graph")
    s = 1.0 / (1.0 + np.exp(-o64["y"]))
    np.testing.assert_allclose(loss.item(), (o64["y"] * s).sum(), rtol=1e-5)
    assert np.abs(conv.weight.grad()).max() > 0                                    # the gradient went on through the norm


@pytest.mark.parametrize("nd,shape", [(1, (3, 5, 12)), (2, (2, 4, 6, 6)), (3, (2, 3, 2, 3, 4))])
def test_instance_norm_layers_are_one_channel_per_group(nk, tdev, nd, shape):
    layer_t = getattr(nk.nn, "InstanceNorm%dd" % nd)
    C = shape[1]
    x, g = rnd(2, shape), rnd(3, shape)
    plain = layer_t(tdev, C)
    assert plain.weight is None and plain.bias is None and not plain.affine and plain.eps == 1e-5   # torch's default: no parameters
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = plain.forward(X); y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    o64, o32 = GN.both(_ncl(x), C, None, None, _ncl(g), EPS)
    _check(y.data(), o64["y"].reshape(shape), o32["y"].reshape(shape), "instance%dd y" % nd)
    _check(X.grad(), o64["dx"].reshape(shape), o32["dx"].reshape(shape), "instance%dd dx" % nd, scale=_dx_scale(o64, _ncl(x), C, _ncl(g), None))
    with pytest.raises(RuntimeError):
        plain.forward(nk.from_ndarray(tdev, x))                                    # nothing to differentiate
    aff = layer_t(tdev, C, affine=True)
    w, b = _set_affine(aff, C, 20)
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = aff.forward(X); y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    o64, o32 = GN.both(_ncl(x), C, w, b, _ncl(g), EPS)
    _check(y.data(), o64["y"].reshape(shape), o32["y"].reshape(shape), "instance%dd affine y" % nd)
    _check(X.grad(), o64["dx"].reshape(shape), o32["dx"].reshape(shape), "instance%dd affine dx" % nd, scale=_dx_scale(o64, _ncl(x), C, _ncl(g), w))
    _params_check(aff, o64, o32, _ncl(g), _ncl(x), C, "instance%dd" % nd)
    with pytest.raises(RuntimeError):                                              # the rank is checked, as BatchNormNd does
        aff.forward(nk.from_ndarray(tdev, rnd(4, shape[:-1])).requires_grad())
    with pytest.raises(RuntimeError):
        aff.forward(nk.from_ndarray(tdev, rnd(4, (shape[0], C + 1) + shape[2:])).requires_grad())


def test_variable_forms_and_the_layer_without_parameters(nk, tdev):
    shape = (N_, C_, H_, W_)
    x, g = rnd(5, shape), rnd(6, shape)
    w, b = 1.0 + 0.5 * rnd(7, (C_,)), rnd(8, (C_,))
    o64, o32 = GN.both(_ncl(x), G_, w, b, _ncl(g), EPS)
    p64, p32 = GN.both(_ncl(x), G_, None, None, _ncl(g), EPS)
    Gv = nk.from_ndarray(tdev, g)
    # affine = false: no parameters
    gn = nk.nn.GroupNorm(tdev, G_, C_, affine=False)
    assert gn.weight is None and gn.bias is None and not gn.affine
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = gn.forward(X); y.forward(); y.backward_from(Gv)
    _check(y.data(), p64["y"].reshape(shape), p32["y"].reshape(shape), "plain y")
    _check(X.grad(), p64["dx"].reshape(shape), p32["dx"].reshape(shape), "plain dx", scale=_dx_scale(p64, _ncl(x), G_, _ncl(g), None))
    with pytest.raises(RuntimeError):
        gn.forward(nk.from_ndarray(tdev, x))
    # Var forms: no gradient, one forward entry, nothing kept
    v = nk.from_ndarray(tdev, x).group_norm(G_); v.forward()
    assert v.history_len() == 1 and np.array_equal(v.data(), y.data())
    v = nk.from_ndarray(tdev, x).group_norm(G_, nk.from_ndarray(tdev, w), nk.from_ndarray(tdev, b)); v.forward()
    _check(v.data(), o64["y"].reshape(shape), o32["y"].reshape(shape), "Var form y")
    # x a plain Var, differentiable parameters: only the parameter gradients run
    W, B = nk.from_ndarray(tdev, w).requires_grad(), nk.from_ndarray(tdev, b).requires_grad()
    y = nk.from_ndarray(tdev, x).group_norm(G_, W, B)
    assert y.history_len() == 1
    y.forward(); y.backward_from(Gv)
    assert np.array_equal(y.data(), v.data())
    from tolerance import assert_contraction
    xh = float(np.abs((x.reshape(N_ * G_, -1) - o64["stats"][:, :1]) * o64["stats"][:, 1:]).max())
    assert_contraction("groupnorm:tape dgamma alone", W.grad(), o64["dgamma"], N_ * H_ * W_, np.abs(g).max(), max(1.0, xh), cpu32=o32["dgamma"])
    assert_contraction("groupnorm:tape dbeta alone", B.grad(), o64["dbeta"], N_ * H_ * W_, np.abs(g).max(), 1.0, cpu32=o32["dbeta"])
    # plain parameters, differentiable x: only dx runs
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = X.group_norm(G_, nk.from_ndarray(tdev, w), nk.from_ndarray(tdev, b))
    assert y.history_len() == 1
    y.forward(); y.backward_from(Gv)
    _check(X.grad(), o64["dx"].reshape(shape), o32["dx"].reshape(shape), "dx alone", scale=_dx_scale(o64, _ncl(x), G_, _ncl(g), w))


@pytest.mark.parametrize("norm_writes_first", [False, True])
def test_input_used_twice_and_a_parameter_shared_by_two_layers(nk, tdev, norm_writes_first):
    """y = gn1(h) + gn2(h) + other(h) with gn2 built on gn1's parameters: h's gradient is the sum of its uses, whether a norm's
    backward entry is the first writer of it (the other use, a ReLU, was recorded before the norms and so runs after them) or a
    later one (`+ h` itself), and the shared weight and bias take both layers' sums (the first writer assigns, the second adds)."""
    shape = (N_, C_, H_, W_)
    h, g = rnd(11, shape), rnd(12, shape)
    gn1 = nk.nn.GroupNorm(tdev, G_, C_)
    w, b = _set_affine(gn1, C_, 30)
    gn2 = nk.nn.GroupNorm(G_, gn1.weight, gn1.bias)                                  # the constructor from existing parameters
    assert gn2.num_channels == C_ and gn2.num_groups == G_ and gn2.affine
    H = nk.from_ndarray(tdev, h).requires_grad()
    other = H.relu() if norm_writes_first else H
    y = gn1.forward(H) + gn2.forward(H) + other
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    o64, o32 = GN.both(_ncl(h), G_, w, b, _ncl(g), EPS)
    extra = [(g * (h > 0) if norm_writes_first else g).astype(dt) for dt in (np.float64, np.float32)]
    o_other = [np.maximum(h, 0) if norm_writes_first else h for _ in range(2)]
    _check(y.data(), 2 * o64["y"].reshape(shape) + o_other[0], np.float32(2) * o32["y"].reshape(shape) + o_other[1], "twice y")
    _check(H.grad(), 2 * o64["dx"].reshape(shape) + extra[0], np.float32(2) * o32["dx"].reshape(shape) + extra[1], "twice dh",
           scale=2 * _dx_scale(o64, _ncl(h), G_, _ncl(g), w))
    _params_check(gn1, o64, o32, _ncl(g), _ncl(h), G_, "shared", times=2)
    assert np.array_equal(gn1.weight.grad(), gn2.weight.grad())


def test_serde_round_trip_is_bit_exact(nk, tdev):
    gn = nk.nn.GroupNorm(tdev, 2, 6)
    w, b = _set_affine(gn, 6, 40)
    text = nk.serde.to_json(gn)
    assert text.startswith('{"weight":{"v":1,"dim":[6],"data":[') and '"bias":{' in text      # LayerNorm's wire form
    back = nk.serde.group_norm_from_json(tdev, text, 2)
    assert back.num_groups == 2 and back.num_channels == 6 and back.eps == 1e-5 and back.affine
    assert np.array_equal(back.weight.data(), w) and np.array_equal(back.bias.data(), b)
    assert nk.serde.to_json(back) == text
    assert nk.serde.group_norm_from_json(tdev, text, 3, eps=1e-3).eps == 1e-3
    x = rnd(2, (3, 6, 5))
    a, c = gn.forward(nk.from_ndarray(tdev, x).requires_grad()), back.forward(nk.from_ndarray(tdev, x).requires_grad())
    a.forward(); c.forward()
    assert np.array_equal(a.data(), c.data())
    with pytest.raises(RuntimeError):
        nk.serde.to_json(nk.nn.GroupNorm(tdev, 2, 6, affine=False))
    with pytest.raises(RuntimeError):
        nk.serde.group_norm_from_json(tdev, text, 4)                               # 6 channels in 4 groups


def test_step_captured_into_a_graph_replays_to_the_eager_bits(nk, tdev):
    """the training step of Conv2d -> GroupNorm -> SiLU -> sum (forward, backward, SGD) captured after one eager call of the same
    sizes and replayed gives the parameters the same steps give eagerly, bit for bit: nothing in the node synchronises, allocates
    or leaves the compute stream"""
    x = rnd(1, (N_, CI_, H_, W_))

    def make():
        conv = nk.nn.Conv2d(tdev, CI_, C_, [3, 3], [1, 1], nk.PaddingMode.zero(), [1, 1], [1, 1], 3)
        gn = nk.nn.GroupNorm(tdev, G_, C_)
        _set_affine(gn, C_, 10)
        loss = gn.forward(conv.forward(nk.from_ndarray(tdev, x))).silu().sum()
        params = [conv.weight, conv.bias, gn.weight, gn.bias]
        opt = nk.optim.SGD(0.01)
        for p in params:
            opt.register(p)

        def step():
            loss.forward()
            loss.no_grad(); loss.with_grad()
            loss.backward(1.0)
            opt.step()
            opt.zero_grad()
        return loss, params, step

    le, pe, step_e = make()
    start = [p.data().copy() for p in pe]
    for _ in range(4):
        step_e()
    lg, pg, step_g = make()
    step_g()                                 # one eager call of the same sizes: the workspace has its size before capture begins
    tdev.graph_begin()
    step_g()
    graph = tdev.graph_end()                 # capturing records the step, it does not run it
    for _ in range(3):
        graph.launch()
    for a, b, s0 in zip(pe, pg, start):
        assert np.array_equal(a.data(), b.data())
        assert not np.array_equal(a.data(), s0)                                    # every parameter moved, the norm's among them
    assert np.isfinite(lg.item()) and lg.item() == le.item()
    del graph


def test_refusals_come_before_any_launch(nk, tdev):
    v = nk.from_ndarray(tdev, rnd(1, (12,)))
    with pytest.raises(RuntimeError):
        v.group_norm(2)                                                            # a rank-1 input
    with pytest.raises(RuntimeError):
        nk.from_ndarray(tdev, rnd(1, (12,))).requires_grad().group_norm(2)
    x = nk.from_ndarray(tdev, rnd(1, (2, 6, 4))).requires_grad()
    for groups in (4, 0, -1):
        with pytest.raises(RuntimeError):
            x.group_norm(groups)                                                   # 6 channels in 4 groups, no groups
    with pytest.raises(RuntimeError):
        nk.nn.GroupNorm(tdev, 4, 6)                                                # num_channels % num_groups != 0
    with pytest.raises(RuntimeError):
        nk.nn.GroupNorm(tdev, 3, 6).forward(nk.from_ndarray(tdev, rnd(1, (2, 5, 4))).requires_grad())   # the wrong channel count
    with pytest.raises(RuntimeError):
        x.group_norm(2, -1.0)                                                      # a negative eps
    w = nk.from_ndarray(tdev, rnd(2, (5,)))
    with pytest.raises(RuntimeError):
        x.group_norm(2, w, w)                                                      # parameters that are not (C)
    tdev.sync()

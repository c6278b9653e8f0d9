"""`Var / VarDiff::max_pool / avg_pool / global_avg_pool / flatten` and `nn::MaxPool / AvgPool 1d, 2d, 3d` through the tape (`_tape`): a
small ResNet-shaped graph (Conv2d -> BatchNorm2d -> relu -> MaxPool2d(3, 2, 1) -> Conv2d -> relu -> global_avg_pool -> flatten -> Linear ->
loss) against the same graph in torch f64, eager and captured; an activation that feeds a pool and a second consumer; the modules
of the other ranks and the `Var` path against tests/pooling_oracle.py; the build-time panics."""
import numpy as np
import pytest

import pooling_oracle as P

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


def _check(got, want, want32, what, floor=1e-30):
    from conftest import record_margin
    got, want32 = np.asarray(got).reshape(np.shape(want)), np.asarray(want32).reshape(np.shape(want))
    scale = max(float(np.abs(want).max()), floor)
    err_gpu, err_cpu = float(np.abs(got - want).max()), float(np.abs(want32.astype(np.float64) - want).max())
    record_margin("pooling:tape " + what, err_gpu, err_cpu, 1e-6 * scale)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)


# ---- the ResNet-shaped graph ----------------------------------------------------------------------------------------------------
N_, C0_, C1_, C2_, H_, F_ = 4, 3, 8, 16, 16, 5
LR_ = 0.05


def _model(nk, tdev, x, t):
    conv1 = nk.nn.Conv2d(tdev, C0_, C1_, [3, 3], [1, 1], nk.PaddingMode.zero(), [1, 1], [1, 1], 3)
    bn = nk.nn.BatchNorm2d(tdev, C1_)
    bn.weight.set_data(1.0 + 0.5 * rnd(40, (C1_,))); bn.bias.set_data(0.2 * rnd(41, (C1_,)))
    pool = nk.nn.MaxPool2d([3, 3], [2, 2], [1, 1])
    conv2 = nk.nn.Conv2d(tdev, C1_, C2_, [3, 3], [1, 1], nk.PaddingMode.zero(), [1, 1], [1, 1], 4)
    fc = nk.nn.Linear(tdev, C2_, F_, 5)
    X = nk.from_ndarray(tdev, x).requires_grad()
    a = pool.forward(bn.forward(conv1.forward(X)).relu())
    feat = conv2.forward(a).relu().global_avg_pool().flatten()
    loss = fc.forward(feat).mse(nk.from_ndarray(tdev, t), nk.Reduction.Mean)
    params = [conv1.weight, conv1.bias, bn.weight, bn.bias, conv2.weight, conv2.bias, fc.weight, fc.bias]
    return dict(X=X, pooled=a, feat=feat, loss=loss, params=params, bn=bn)


# torch runs in a child process: a process that has loaded the HIP library must not import torch as well
_TORCH_STEP = r"""
import sys
import numpy as np
import torch
F = torch.nn.functional
d = np.load(sys.argv[1])
X = torch.tensor(d["x"], dtype=torch.float64, requires_grad=True)
p = [torch.tensor(d["p%d" % i].astype(np.float64), requires_grad=True) for i in range(8)]
z = F.conv2d(X, p[0], p[1].reshape(-1), padding=1)
z = F.batch_norm(z, None, None, p[2], p[3], training=True, eps=1e-5)
a = F.max_pool2d(torch.relu(z), 3, 2, 1)
f = torch.relu(F.conv2d(a, p[4], p[5].reshape(-1), padding=1))
feat = torch.flatten(F.adaptive_avg_pool2d(f, 1), 1)
loss = F.mse_loss(F.linear(feat, p[6], p[7]), torch.tensor(d["t"], dtype=torch.float64))
loss.backward()
np.savez(sys.argv[2], a=a.detach().numpy(), feat=feat.detach().numpy(), loss=loss.item(), dx=X.grad.numpy(),
         **{"g%d" % i: q.grad.numpy() for i, q in enumerate(p)})
"""


def _torch_step(x, t, params, tmp_path):
    import subprocess
    import sys
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, x=x, t=t, **{"p%d" % i: np.asarray(a) for i, a in enumerate(params)})
    r = subprocess.run([sys.executable, "-c", _TORCH_STEP, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    d = np.load(dst)
    return d["a"], d["feat"], float(d["loss"]), d["dx"], [d["g%d" % i] for i in range(8)]


def test_resnet_shaped_graph_equals_torch(nk, tdev, tmp_path):
    x, t = rnd(60, (N_, C0_, H_, H_)), rnd(61, (N_, F_))
    m = _model(nk, tdev, x, t)
    m["loss"].forward()
    m["loss"].backward(1.0)
    a, feat, loss, dx, grads = _torch_step(x, t, [p.data() for p in m["params"]], tmp_path)
    assert m["pooled"].data().shape == (N_, C1_, H_ // 2, H_ // 2) and m["feat"].data().shape == (N_, C2_)
    np.testing.assert_allclose(m["pooled"].data(), a, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(m["feat"].data(), feat, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(m["loss"].item(), loss, rtol=2e-5)
    np.testing.assert_allclose(m["X"].grad(), dx, rtol=2e-3, atol=2e-6)
    for p, gr, name in zip(m["params"], grads, ("conv1 weight", "conv1 bias", "gamma", "beta", "conv2 weight", "conv2 bias", "fc weight", "fc bias")):
        np.testing.assert_allclose(p.grad().reshape(gr.shape), gr, rtol=2e-3, atol=2e-6, err_msg=name)


def test_resnet_shaped_step_captured_equals_eager(nk, tdev):
    """forward, backward and SGD captured into a graph and replayed leave the parameters the same eager steps leave, bit for bit:
    the pooling entries neither synchronise nor allocate, and the offsets buffer of the max pool is part of the captured work"""
    x, t = rnd(60, (N_, C0_, H_, H_)), rnd(61, (N_, F_))

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
    graph = tdev.graph_end()
    for _ in range(3):
        graph.launch()
    for pe, pg in zip(me["params"], mg["params"]):
        assert np.array_equal(pe.data(), pg.data())
    assert np.isfinite(mg["loss"].item()) and mg["loss"].item() == me["loss"].item()
    del graph


@pytest.mark.parametrize("order", ["pool-first", "pool-second"])
@pytest.mark.parametrize("kind", ["max", "avg", "global"])
def test_activation_with_a_second_consumer(nk, tdev, kind, order):
    """the activation's lazily zeroed gradient gets one assign and one add, whichever node runs first"""
    x = rnd(70, (2, 3, 12, 16))
    X = nk.from_ndarray(tdev, x).requires_grad()
    A = X.tanh()
    pooled = {"max": lambda: A.max_pool([3, 3], [2, 2], [1, 1]), "avg": lambda: A.avg_pool([3, 3], [2, 2], [1, 1], False),
              "global": lambda: A.global_avg_pool()}[kind]
    if order == "pool-first":
        loss = pooled().sum() + A.relu().sum()
    else:
        other = A.relu().sum()
        loss = other + pooled().sum()
    loss.forward()
    loss.backward(1.0)

    def want(dt):
        a = np.tanh(x.astype(dt))
        if kind == "max":
            y, idx = P.max_pool_fwd(a, (3, 3), (2, 2), (1, 1))
            da = P.max_pool_bwd(np.ones(y.shape, dt), idx, a.shape)
        elif kind == "avg":
            y = P.avg_pool_fwd(a, (3, 3), (2, 2), (1, 1), False)
            da = P.avg_pool_bwd(np.ones(y.shape, dt), a.shape, (3, 3), (2, 2), (1, 1), False)
        else:
            y = P.global_avg_pool_fwd(a)
            da = P.avg_pool_bwd(np.ones(y.shape, dt), a.shape, a.shape[2:], a.shape[2:], (0, 0), True)
        da = da + (a > 0)
        return y.sum(dtype=dt) + np.maximum(a, 0).sum(dtype=dt), da * (1 - a * a)
    (l64, d64), (l32, d32) = want(np.float64), want(np.float32)
    np.testing.assert_allclose(loss.item(), l64, rtol=1e-5)
    _check(X.grad(), d64, d32, "dx second consumer %s %s" % (kind, order), floor=1.0)


MODULES = {
    "MaxPool1d": ((2, 3, 40), lambda nn: nn.MaxPool1d(3, 2, 1), (3,), (2,), (1,), None),
    "MaxPool3d": ((2, 2, 6, 8, 8), lambda nn: nn.MaxPool3d([2, 2, 2]), (2, 2, 2), (2, 2, 2), (0, 0, 0), None),
    "MaxPool2d-default-stride": ((2, 3, 9, 12), lambda nn: nn.MaxPool2d([3, 3]), (3, 3), (3, 3), (0, 0), None),
    "AvgPool1d": ((2, 3, 19), lambda nn: nn.AvgPool1d(4, 3, 2), (4,), (3,), (2,), True),
    "AvgPool2d-exclude-pad": ((2, 3, 12, 16), lambda nn: nn.AvgPool2d([3, 3], [2, 2], [1, 1], False), (3, 3), (2, 2), (1, 1), False),
    "AvgPool3d": ((1, 2, 5, 7, 9), lambda nn: nn.AvgPool3d([3, 2, 3], [2, 1, 2], [1, 1, 0]), (3, 2, 3), (2, 1, 2), (1, 1, 0), True),
}


@pytest.mark.parametrize("name", list(MODULES))
def test_modules_forward_and_backward(nk, tdev, name):
    shape, make, k, s, p, cip = MODULES[name]
    layer = make(nk.nn)
    x = rnd(80, shape)
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = layer.forward(X)
    g = rnd(81, P.out_shape(shape, k, s, p))
    loss = (y * nk.from_ndarray(tdev, g)).sum()
    loss.forward()
    loss.backward(1.0)
    plain = layer.forward(nk.from_ndarray(tdev, x))                           # the Var path: no offsets are kept
    plain.forward()
    if cip is None:
        want, idx = P.max_pool_fwd(x, k, s, p)
        assert np.array_equal(y.data(), want) and np.array_equal(plain.data(), want)
        _check(X.grad(), P.max_pool_bwd(g.astype(np.float64), idx, shape), P.max_pool_bwd(g, idx, shape), "dx " + name, floor=1.0)
    else:
        w64, w32 = P.avg_pool_fwd(x.astype(np.float64), k, s, p, cip), P.avg_pool_fwd(x, k, s, p, cip)
        _check(y.data(), w64, w32, "y " + name, floor=1.0)
        assert np.array_equal(plain.data(), y.data())
        _check(X.grad(), P.avg_pool_bwd(g.astype(np.float64), shape, k, s, p, cip), P.avg_pool_bwd(g, shape, k, s, p, cip), "dx " + name, floor=1.0)


def test_var_path_global_pool_and_flatten(nk, tdev):
    x = rnd(90, (3, 5, 7, 7))
    v = nk.from_ndarray(tdev, x).global_avg_pool()
    f = v.flatten()
    f.forward()
    assert v.data().shape == (3, 5, 1, 1) and f.data().shape == (3, 5)
    _check(f.data(), x.astype(np.float64).mean(axis=(2, 3)), P.flatten(P.global_avg_pool_fwd(x)), "global avg Var", floor=1.0)
    X = nk.from_ndarray(tdev, x).requires_grad()
    g = rnd(91, (3, 5 * 7 * 7))
    loss = (X.flatten() * nk.from_ndarray(tdev, g)).sum()
    loss.forward()
    loss.backward(1.0)
    assert np.array_equal(X.grad(), P.flatten_bwd(g, x.shape))
    m = nk.from_ndarray(tdev, x).max_pool([7, 7])                            # the whole plane through the pair reduction
    m.forward()
    assert np.array_equal(m.data().reshape(3, 5), x.max(axis=(2, 3)))


def test_build_time_panics_name_the_axis(nk, tdev):
    X = nk.from_ndarray(tdev, rnd(95, (2, 3, 8, 10))).requires_grad()
    V = nk.from_ndarray(tdev, rnd(95, (2, 3, 8, 10)))
    for v in (X, V):
        with pytest.raises(RuntimeError, match="kernel has 1 entries for 2 spatial axes"):
            v.max_pool([3], [2, 2], [1, 1])
        with pytest.raises(RuntimeError, match="stride has 3 entries"):
            v.avg_pool([3, 3], [2, 2, 2], [1, 1])
        with pytest.raises(RuntimeError, match="padding 2 of spatial axis 1"):
            v.max_pool([3, 3], [2, 2], [1, 2])
        with pytest.raises(RuntimeError, match="stride 0 of spatial axis 0"):
            v.max_pool([3, 3], [0, 2], [1, 1])
        with pytest.raises(RuntimeError, match="window 0 of spatial axis 1"):
            v.avg_pool([3, 0], [1, 1], [0, 0])
        with pytest.raises(RuntimeError, match="window 9 exceeds the padded extent 8 .* of spatial axis 0"):
            v.max_pool([9, 3], [1, 1], [0, 0])
    with pytest.raises(RuntimeError, match="1 to 3 spatial axes"):
        nk.from_ndarray(tdev, rnd(96, (4, 6))).global_avg_pool()
    with pytest.raises(RuntimeError, match="at least two dimensions"):
        nk.from_ndarray(tdev, rnd(96, (6,))).flatten()
    with pytest.raises(RuntimeError, match="expected 4-dimensional input"):
        nk.nn.MaxPool2d([2, 2]).forward(nk.from_ndarray(tdev, rnd(96, (2, 3, 8))))

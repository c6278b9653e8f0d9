"""`Var / VarDiff::upsample` and `nn::Upsample` through the tape (`_tape`) against tests/upsample_oracle.py, bit for bit: by `size`
and by `scale_factor` (integer and 1.5), the node as first and as later writer of its input's gradient, the gradient through a
two-node graph, the refusals, and a small U-Net up-block (Upsample -> Conv2d -> GroupNorm -> SiLU) whose upsample gradient is the
oracle's backward of the gradient the convolution left on the tape.  Two test ids: the first walks the forms case by case, runs every
one of them and names the ones that failed."""
import numpy as np
import pytest

import upsample_oracle as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nk():
    import neuronika_amd
    return neuronika_amd.tape


@pytest.fixture(scope="module")
def tdev(nk):
    return nk.Device(0)


def rnd(seed, shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _each(cases, check, nk, tdev):
    failed = []
    for case in cases:
        try:
            check(nk, tdev, *case)
        except AssertionError as e:
            failed.append("%s%r: %s" % (check.__name__, case, str(e)[:300]))
    assert not failed, "\n".join(failed)


def _same(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), float(np.abs(got - want).max())


METHODS = [((2, 3, 5), (8,), "linear", True), ((2, 3, 4, 4), (8, 8), "nearest", False), ((1, 2, 6, 8), (9, 20), "bilinear", False),
           ((1, 2, 3, 4, 4), (6, 8, 8), "trilinear", True), ((1, 2, 3, 4, 4), (6, 8, 8), "nearest", False)]


def _variable_methods_equal_the_oracle(nk, tdev, shape, size, mode, align):
    omode = "nearest" if mode == "nearest" else "linear"
    x, g = rnd(1, shape), rnd(2, shape[:2] + size)
    v = nk.from_ndarray(tdev, x).upsample(list(size), mode, align)                  # Var: no gradient, one forward entry
    v.forward()
    assert tuple(v.shape) == shape[:2] + size and v.history_len() == 1
    _same(v.data(), U.forward(x, size, omode, align))
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = X.upsample(list(size), mode, align)
    assert y.history_len() == 1 and y.forward_history_len() == 1                    # ONE entry each way
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    _same(y.data(), v.data())
    _same(X.grad(), U.backward(g, shape, omode, align))


LAYERS = [({"size": [9, 20]}, (1, 2, 6, 8), "bilinear"), ({"size": 8}, (2, 3, 5), "linear"), ({"scale_factor": 2}, (2, 3, 4, 4), "nearest"),
          ({"scale_factor": 2.0}, (1, 2, 3, 4, 4), "trilinear"), ({"scale_factor": 1.5}, (1, 2, 6, 8), "bilinear"),
          ({"scale_factor": 1.5}, (2, 3, 5), "nearest"), ({"scale_factor": [1.5, 2.5]}, (1, 2, 6, 8), "nearest")]


def _layer_by_size_and_by_scale_factor(nk, tdev, kw, shape, mode):
    from neuronika_amd import capi
    layer = nk.nn.Upsample(mode=mode, **kw)
    assert layer.mode == mode and not layer.align_corners
    if "size" in kw:
        size = tuple(np.atleast_1d(kw["size"]).tolist())
        assert list(layer.size) == list(size) and list(layer.scale_factor) == []
    else:
        size = capi.upsample_out_size(shape, kw["scale_factor"])                   # the extents are nk_upsample_out_size's
        assert size == U.out_size(shape, kw["scale_factor"]) and list(layer.size) == []
    assert tuple(layer.output_size(list(shape))) == size
    with pytest.raises(AttributeError):
        layer.mode = "nearest"                                                     # read-only fields
    omode = "nearest" if mode == "nearest" else "linear"
    x, g = rnd(3, shape), rnd(4, shape[:2] + size)
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = layer.forward(X)
    assert tuple(y.shape) == shape[:2] + size
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    _same(y.data(), U.forward(x, size, omode))
    _same(X.grad(), U.backward(g, shape, omode))
    v = layer.forward(nk.from_ndarray(tdev, x)); v.forward()                        # the form without gradient
    _same(v.data(), y.data())


def _gradient_through_a_two_node_graph(nk, tdev, mode, align):
    """loss = sum(upsample(x) * t): the gradient that reaches the node is read from the tape, dx is the oracle's backward of it"""
    shape, size = (2, 3, 4, 4), (8, 8)
    x, t = rnd(5, shape), rnd(6, shape[:2] + size)
    X = nk.from_ndarray(tdev, x).requires_grad()
    u = X.upsample(list(size), mode, align)
    loss = (u * nk.from_ndarray(tdev, t)).sum()
    loss.forward(); loss.backward(1.0)
    omode = "nearest" if mode == "nearest" else "linear"
    _same(u.grad(), t)
    _same(X.grad(), U.backward(u.grad(), shape, omode, align))
    y = U.forward(x, size, omode, align)
    np.testing.assert_allclose(loss.item(), (y.astype(np.float64) * t).sum(), rtol=1e-5, atol=1e-5)


def _first_and_later_writer_of_the_inputs_gradient(nk, tdev, mode, upsample_writes_first):
    """h feeds the upsample and one more node: its gradient is the sum of both uses - one f32 add - whether the upsample's entry is the
    first writer (the other use, a ReLU recorded before it, runs after it: `_assign`, then the ReLU adds) or a later one (`+=`)"""
    shape, size = (2, 3, 4, 4), (8, 8)
    h, t, s = rnd(7, shape), rnd(8, shape[:2] + size), rnd(9, shape)
    H = nk.from_ndarray(tdev, h).requires_grad()
    other = H.relu() if upsample_writes_first else H
    u = H.upsample(list(size), mode)
    loss = (u * nk.from_ndarray(tdev, t)).sum() + (other * nk.from_ndarray(tdev, s)).sum()
    loss.forward(); loss.backward(1.0)
    omode = "nearest" if mode == "nearest" else "linear"
    extra = (s * (h > 0)).astype(np.float32) if upsample_writes_first else s
    _same(H.grad(), U.backward(u.grad(), shape, omode) + extra)


def _refusals_come_when_the_graph_is_built(nk, tdev):
    x4 = nk.from_ndarray(tdev, rnd(1, (2, 3, 4, 4)))
    x3 = nk.from_ndarray(tdev, rnd(1, (2, 3, 5))).requires_grad()
    with pytest.raises(RuntimeError):
        nk.nn.Upsample(size=[8, 8], scale_factor=2.0)                              # both
    with pytest.raises(RuntimeError):
        nk.nn.Upsample()                                                           # neither
    with pytest.raises(RuntimeError):
        nk.nn.Upsample(scale_factor=2.0, mode="bicubic")
    with pytest.raises(RuntimeError):
        nk.nn.Upsample(scale_factor=2.0, mode="nearest", align_corners=True)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            nk.nn.Upsample(scale_factor=bad)
    with pytest.raises(RuntimeError):
        nk.nn.Upsample(scale_factor=2.0, mode="linear").forward(x4)                # the wrong mode for the rank
    with pytest.raises(RuntimeError):
        nk.nn.Upsample(scale_factor=2.0, mode="bilinear").forward(x3)
    with pytest.raises(RuntimeError):
        x4.upsample([8, 8], "trilinear")
    with pytest.raises(RuntimeError):
        x4.upsample([8], "nearest")                                                # one extent for two axes
    with pytest.raises(RuntimeError):
        nk.nn.Upsample(size=[8]).forward(x4)
    with pytest.raises(RuntimeError):
        nk.nn.Upsample(scale_factor=[2.0, 2.0, 2.0]).forward(x4)
    with pytest.raises(RuntimeError):
        x4.upsample([8, 0], "nearest")
    with pytest.raises(RuntimeError):
        x3.upsample([8], "nearest", True)
    with pytest.raises(RuntimeError):
        nk.nn.Upsample(scale_factor=0.1).forward(x4)                               # floor(4 * 0.1) = 0
    with pytest.raises(RuntimeError):
        nk.from_ndarray(tdev, rnd(1, (12,))).upsample([24], "nearest")             # no (N, C, spatial...) input


def test_variable_methods_the_layer_writers_and_refusals(nk, tdev):
    """`Var / VarDiff::upsample` and `nn.Upsample` by `size` and by `scale_factor` (integer and 1.5; the extents are
    nk_upsample_out_size's) equal the oracle bit for bit; the gradient through a two-node graph; the node as first (`_assign`) and as
    later (`+=`) writer of its input's gradient; the wrong mode for the rank, `size` together with `scale_factor` and the other bad
    arguments raise when the graph is built"""
    _each(METHODS, _variable_methods_equal_the_oracle, nk, tdev)
    _each(LAYERS, _layer_by_size_and_by_scale_factor, nk, tdev)
    _each([("nearest", False), ("bilinear", False), ("bilinear", True)], _gradient_through_a_two_node_graph, nk, tdev)
    _each([(m, f) for m in ("nearest", "bilinear") for f in (False, True)], _first_and_later_writer_of_the_inputs_gradient, nk, tdev)
    _refusals_come_when_the_graph_is_built(nk, tdev)


def test_unet_up_block_runs_and_the_upsample_gradient_is_the_oracles(nk, tdev):
    """Upsample(2, nearest) -> Conv2d 3x3 -> GroupNorm -> SiLU at (2, 8, 8, 8): forward and backward run, and the gradient of the
    block's input is the oracle's backward applied to the gradient the convolution left on the upsample's output"""
    N, C, H, W, CO = 2, 8, 8, 8, 8
    x = rnd(10, (N, C, H, W))
    up = nk.nn.Upsample(scale_factor=2, mode="nearest")
    conv = nk.nn.Conv2d(tdev, C, CO, [3, 3], [1, 1], nk.PaddingMode.zero(), [1, 1], [1, 1], 1)
    gn = nk.nn.GroupNorm(tdev, 4, CO)
    X = nk.from_ndarray(tdev, x).requires_grad()
    u = up.forward(X)
    y = gn.forward(conv.forward(u)).silu()
    assert tuple(u.shape) == (N, C, 2 * H, 2 * W) and tuple(y.shape) == (N, CO, 2 * H, 2 * W)
    loss = y.sum()
    loss.forward(); loss.backward(1.0)
    _same(u.data(), U.forward(x, (2 * H, 2 * W), "nearest"))
    gu = u.grad()
    assert np.isfinite(loss.item()) and np.isfinite(gu).all() and np.abs(gu).max() > 0
    _same(X.grad(), U.backward(gu, (N, C, H, W), "nearest"))
    assert np.abs(conv.weight.grad()).max() > 0 and np.abs(gn.weight.grad()).max() > 0

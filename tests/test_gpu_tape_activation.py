"""`Var / VarDiff::gelu / silu / glu` and `nn::GELU / SiLU / GLU` through the tape (`_tape`) against tests/activation_oracle.py (f64):
every node as the first and as a later writer of one gradient, the `Var` forms, the modules, a gated MLP and a GELU MLP with the loss
and every parameter gradient, and a second backward after `zero_grad` reproducing the first bit for bit."""
import itertools

import numpy as np
import pytest

import activation_oracle as A
import tolerance
from tolerance import ELEMENTWISE_ATOL, ELEMENTWISE_RTOL

pytestmark = pytest.mark.gpu

ROWS, H_ = 37, 52                                            # x is (ROWS, 2 H_): the 16-byte gated kernels; H_ = 7: the scalar ones


@pytest.fixture(scope="module")
def nk():
    import neuronika_amd
    return neuronika_amd.tape


@pytest.fixture(scope="module")
def tdev(nk):
    return nk.Device(0)


def nodes(nk):
    """name -> (how to apply it to a Var or VarDiff, oracle name, gated)"""
    Act = nk.Activation
    return {"gelu": (lambda v: v.gelu(), "gelu", False), "gelu_tanh": (lambda v: v.gelu(True), "gelu_tanh", False),
            "silu": (lambda v: v.silu(), "silu", False), "glu": (lambda v: v.glu(), "sigmoid", True),
            "geglu": (lambda v: v.glu(Act.Gelu), "gelu", True), "geglu_tanh": (lambda v: v.glu(Act.GeluTanh), "gelu_tanh", True),
            "swiglu": (lambda v: v.glu(Act.Silu), "silu", True)}


def oracle(act, gated, x, w, H):
    """value of the node and the gradient of sum(w * node(x)) with respect to x, f64"""
    if gated:
        return A.glu_forward(act, x, H), A.glu_backward(act, x, w, H)
    return A.forward(act, x), A.backward(act, x, w)


def elementwise_close(got, ref, what, parts=1, scale=None):
    """|got - ref| <= parts * ATOL + RTOL * scale (+ one f32 rounding of the sum when two writers met); scale = |ref| by default"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref) if scale is None else scale
    bound = parts * ELEMENTWISE_ATOL + ELEMENTWISE_RTOL * scale + (2.0 ** -24 * np.abs(ref) if parts > 1 else 0.0)
    ratio = np.abs(got - ref) / bound
    print("%-40s worst error / bound %.4f" % (what, float(ratio.max())))
    assert got.shape == ref.shape and np.isfinite(got).all() and ratio.max() <= 1.0, (what, float(ratio.max()))


@pytest.mark.parametrize("H", [H_, 7])
def test_every_node_as_first_and_as_later_writer(nk, tdev, H):
    """sum(w1 * f(x)) + sum(w2 * h(x)) for every ordered pair (f, h) of distinct nodes: the later node on the tape writes x's gradient
    first (the assign form), the other adds; `x.gelu() + x.silu()` is the pair (gelu, silu) with unit weights"""
    rng = np.random.default_rng(H)
    x = rng.uniform(-4, 4, (ROWS, 2 * H)).astype(np.float32)
    table = nodes(nk)
    for (nf, (f, af, gf)), (nh, (h, ah, gh)) in itertools.permutations(table.items(), 2):
        leaf = nk.from_ndarray(tdev, x).requires_grad()
        w1 = rng.uniform(-1, 1, (ROWS, H if gf else 2 * H)).astype(np.float32)
        w2 = rng.uniform(-1, 1, (ROWS, H if gh else 2 * H)).astype(np.float32)
        a, b = f(leaf), h(leaf)
        assert a.history_len() == 1 and b.history_len() == 1                     # one node each
        total = (a * nk.from_ndarray(tdev, w1)).sum() + (b * nk.from_ndarray(tdev, w2)).sum()
        total.forward(); total.backward(1.0)
        (va, ga), (vb, gb) = oracle(af, gf, x, w1, H), oracle(ah, gh, x, w2, H)
        elementwise_close(a.data(), va, nf + " value")
        elementwise_close(b.data(), vb, nh + " value")
        elementwise_close(leaf.grad(), (ga + gb).reshape(x.shape), "%s + %s gradient" % (nf, nh), parts=2,
                          scale=(np.abs(ga) + np.abs(gb)).reshape(x.shape))
    leaf = nk.from_ndarray(tdev, x).requires_grad()
    total = (leaf.gelu() + leaf.silu()).sum()
    total.forward(); total.backward(1.0)
    one = np.ones(x.shape)
    ga, gb = A.backward("gelu", x, one), A.backward("silu", x, one)
    elementwise_close(leaf.grad(), ga + gb, "x.gelu() + x.silu()", parts=2, scale=np.abs(ga) + np.abs(gb))


def test_the_var_forms_and_the_modules(nk, tdev):
    rng = np.random.default_rng(3)
    x = rng.uniform(-4, 4, (ROWS, 2 * H_)).astype(np.float32)
    Act = nk.Activation
    modules = {"gelu": nk.nn.GELU(), "gelu_tanh": nk.nn.GELU(True), "silu": nk.nn.SiLU(), "glu": nk.nn.GLU(), "geglu": nk.nn.GLU(Act.Gelu),
               "geglu_tanh": nk.nn.GLU(Act.GeluTanh), "swiglu": nk.nn.GLU(Act.Silu)}
    for name, (f, act, gated) in nodes(nk).items():
        plain = f(nk.from_ndarray(tdev, x))
        assert not hasattr(plain, "grad")                                        # a Var: nothing to differentiate
        diff = f(nk.from_ndarray(tdev, x).requires_grad())
        by_module = modules[name].forward(nk.from_ndarray(tdev, x))
        by_module_diff = modules[name].forward(nk.from_ndarray(tdev, x).requires_grad())
        assert hasattr(by_module_diff, "grad") and not hasattr(by_module, "grad")
        for v in (plain, diff, by_module, by_module_diff):
            v.forward()
            assert tuple(v.shape) == (ROWS, H_ if gated else 2 * H_) and v.history_len() == 1
        elementwise_close(plain.data(), A.glu_forward(act, x, H_) if gated else A.forward(act, x), name + " Var form")
        for v in (diff, by_module, by_module_diff):
            assert np.array_equal(v.data().view(np.uint32), plain.data().view(np.uint32)), name


def test_glu_needs_an_even_last_extent(nk, tdev):
    for shape in ((4, 5), (3,), (2, 3, 1)):
        v = nk.from_ndarray(tdev, np.zeros(shape, np.float32))
        for bad in (lambda: v.glu(), lambda: v.requires_grad().glu(nk.Activation.Silu), lambda: nk.nn.GLU().forward(v)):
            with pytest.raises(Exception, match="glu: the last axis must have an even extent"):
                bad()
    nk.from_ndarray(tdev, np.zeros((3, 4, 6), np.float32)).glu().forward()


def _mlp(nk, tdev, gated, H, seed):
    """Linear(D, 2 H or H) -> glu(SiLU) or gelu -> Linear(H, D) -> mse(Mean); returns the tape objects and the f64 reference"""
    N, D = 64, 48
    rng = np.random.default_rng(seed)
    x, t = rng.uniform(-1, 1, (N, D)).astype(np.float32), rng.uniform(-1, 1, (N, D)).astype(np.float32)
    l1, l2 = nk.nn.Linear(tdev, D, 2 * H if gated else H, seed + 1), nk.nn.Linear(tdev, H, D, seed + 2)
    z = l1.forward(nk.from_ndarray(tdev, x))
    h = z.glu(nk.Activation.Silu) if gated else z.gelu()
    y = l2.forward(h)
    loss = y.mse(nk.from_ndarray(tdev, t), nk.Reduction.Mean)
    W1, b1, W2, b2 = (p.data().astype(np.float64) for p in (l1.weight, l1.bias, l2.weight, l2.bias))
    z64 = x.astype(np.float64) @ W1.T + b1
    h64 = A.glu_forward("silu", z64, H) if gated else A.forward("gelu", z64)
    y64 = h64 @ W2.T + b2
    diff = y64 - t
    dy = 2.0 * diff / diff.size
    dh = dy @ W2
    dz = A.glu_backward("silu", z64, dh, H) if gated else A.backward("gelu", z64, dh)
    ref = dict(loss=float((diff ** 2).mean()), x=x, h=h64, dy=dy, dz=dz, dW2=dy.T @ h64, db2=dy.sum(0), dW1=dz.T @ x.astype(np.float64), db1=dz.sum(0))
    return dict(loss=loss, nodes=[z, h, y, loss], params=[l1.weight, l1.bias, l2.weight, l2.bias]), ref


@pytest.mark.parametrize("gated,H", [(True, 80), (True, 30), (False, 80), (False, 30)])
def test_mlp_loss_and_parameter_gradients_against_the_oracle(nk, tdev, gated, H):
    m, ref = _mlp(nk, tdev, gated, H, 11)
    m["loss"].forward(); m["loss"].backward(1.0)
    assert abs(m["loss"].item() - ref["loss"]) <= ELEMENTWISE_ATOL + ELEMENTWISE_RTOL * abs(ref["loss"]), (m["loss"].item(), ref["loss"])
    N = ref["x"].shape[0]
    tag = ("swiglu" if gated else "gelu") + "_mlp_H%d_" % H
    l1w, l1b, l2w, l2b = m["params"]
    amax = lambda a: float(np.abs(a).max())
    tolerance.assert_contraction(tag + "dW2", l2w.grad(), ref["dW2"], N, amax(ref["dy"]), amax(ref["h"]), epilogue=True)
    tolerance.assert_contraction(tag + "db2", l2b.grad(), ref["db2"], N, amax(ref["dy"]), 1.0, epilogue=True)
    tolerance.assert_contraction(tag + "dW1", l1w.grad(), ref["dW1"], N, amax(ref["dz"]), amax(ref["x"]), epilogue=True)
    tolerance.assert_contraction(tag + "db1", l1b.grad(), ref["db1"], N, amax(ref["dz"]), 1.0, epilogue=True)
    assert all(np.abs(p.grad()).max() > 0 for p in m["params"])


@pytest.mark.parametrize("gated", [True, False])
def test_zero_grad_and_a_second_backward_reproduce_the_first(nk, tdev, gated):
    m, _ = _mlp(nk, tdev, gated, 80, 13)
    m["loss"].forward(); m["loss"].backward(1.0)
    first = [p.grad().copy() for p in m["params"]]
    for v in m["nodes"] + m["params"]:
        v.zero_grad()
    m["loss"].forward(); m["loss"].backward(1.0)
    for p, g in zip(m["params"], first):
        assert np.array_equal(p.grad().view(np.uint32), g.view(np.uint32))

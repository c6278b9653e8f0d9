"""The four attention nodes of the tape (`_tape`) hold ONE description of a fused-core call; these are the facts its single call site
could break, per form of the core (full, causal, band, packed sequences, packed sequences under a band), all exact:

  * the packed node's forward equals the strided `heads_attention` path bit for bit at p = 0;
  * a second backward without zeroing doubles dq, dk, dv and the packed parameter gradients (g + g is exact): the assign /
    accumulate flags reach the kernels;
  * in training at p = 0.1 two forwards of one graph differ (the Philox offset advances); in evaluation the output is the p = 0 one;
  * a graph without gradients gives the differentiable graph's forward.

test_gpu_tape_causal.py, test_gpu_tape_band.py and test_gpu_tape_segments.py hold the last fact for the causal, band and segment
forms; the full form and segments under a band are the cells they leave out, and none of them holds the first three."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, H, DH, W = 2, 2, 32, 40
D = H * DH
SCALE = float(np.float32(1 / np.sqrt(DH)))
SIZES = [128, 160]                        # 160: ragged, two 128-row query blocks
DOCS = {128: [[70, 58], [30, 70, 28]], 160: [[70, 70, 20], [60, 70, 30]]}   # max_len = 70 < S
# form: (causal, window, with segments)
FORMS = {"full": (False, 0, False), "causal": (True, 0, False), "band": (True, W, False), "segments": (True, 0, True),
         "segments, band": (True, W, True)}
CELLS = [(S, form) for S in SIZES for form in FORMS]
IDS = ["S %d, %s" % c for c in CELLS]


@pytest.fixture(scope="module")
def nk():
    import neuronika_amd
    return neuronika_amd.tape


@pytest.fixture(scope="module")
def tdev(nk):
    return nk.Device(0)


def rnd(seed, shape):
    a = np.random.default_rng(seed).random(shape, dtype=np.float32)
    return np.asarray(a * np.float32(2) - np.float32(1), dtype=np.float32).reshape(shape)


@pytest.fixture(scope="module")
def inputs():
    return {S: tuple(rnd(s, (B * S, D)) for s in (1, 2, 3, 4)) for S in SIZES}      # q (also the module's x), k, v, dO


def _segments(nk, tdev, S, form):
    if not FORMS[form][2]:
        return None
    seg = nk.nn.Segments(tdev, B, S, DOCS[S])
    assert seg.max_len == 70
    return seg


def _core(Q, K, V, S, form, p, status, seg):
    causal, window, _ = FORMS[form]
    if seg is None:
        return Q.heads_attention(K, V, B, S, H, DH, SCALE, p, status, causal, window)
    return Q.heads_attention(K, V, B, S, H, DH, SCALE, p, status, causal, window, seg)


def _module(nk, tdev, form, p, packed):
    causal, window, _ = FORMS[form]
    mha = nk.nn.MultiheadAttention(tdev, D, H, p, 3)
    mha.causal, mha.window, mha.packed_qkv = causal, window, packed
    return mha


def _forward(mha, X, seg):
    return mha.forward(X, B) if seg is None else mha.forward(X, B, seg)


@pytest.mark.parametrize("S,form", CELLS, ids=IDS)
def test_the_packed_node_is_the_strided_path_bit_for_bit(nk, tdev, inputs, S, form):
    x = inputs[S][0]
    seg = _segments(nk, tdev, S, form)
    mha = _module(nk, tdev, form, 0.0, True)
    outs, nodes = [], []
    for packed in (True, False):
        mha.packed_qkv = packed
        y = _forward(mha, nk.from_ndarray(tdev, x).requires_grad(), seg)
        y.forward()
        outs.append(y.data().copy()); nodes.append(y.history_len())
    assert nodes == [2, 5]                                                 # [projections + core], out | q, k, v, core, out
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0
    print(form, S, "packed - strided: max |diff| %.3g" % np.abs(outs[0] - outs[1]).max())
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("S,form", CELLS, ids=IDS)
def test_a_second_backward_without_zeroing_doubles_every_gradient(nk, tdev, inputs, S, form):
    q, k, v, g = inputs[S]
    seg = _segments(nk, tdev, S, form)
    G = nk.from_ndarray(tdev, g)
    # the strided node: dq, dk, dv
    leaves = [nk.from_ndarray(tdev, t).requires_grad() for t in (q, k, v)]
    y = _core(*leaves, S, form, 0.0, nk.Status(False), seg)
    y.forward(); y.backward_from(G)
    first = [leaf.grad().copy() for leaf in leaves]
    y.backward_from(G)
    for name, leaf, one in zip(("dq", "dk", "dv"), leaves, first):
        assert np.isfinite(one).all() and np.abs(one).max() > 0, name
        print(form, S, name, "second - 2 * first: max |diff| %.3g" % np.abs(leaf.grad() - (one + one)).max())
        assert np.array_equal(leaf.grad(), one + one), name
    # the packed node: the input and the packed parameters (views of one storage, written by one kernel each)
    mha = _module(nk, tdev, form, 0.0, True)
    X = nk.from_ndarray(tdev, q).requires_grad()
    y = _forward(mha, X, seg)
    named = [("x", X)] + [(n + "." + w, getattr(getattr(mha, n), w)) for n in "qkv" for w in ("weight", "bias")]
    for _, leaf in named:
        leaf.zero_grad()
    y.forward(); y.backward_from(G)
    first = [leaf.grad().copy() for _, leaf in named]
    y.no_grad(); y.with_grad()                                             # the inner gradients start again, the leaves keep theirs
    y.backward_from(G)
    for (name, leaf), one in zip(named, first):
        assert np.isfinite(one).all(), name
        print(form, S, name, "second - 2 * first: max |diff| %.3g" % np.abs(leaf.grad() - (one + one)).max())
        assert np.array_equal(leaf.grad(), one + one), name
    assert all(np.abs(one).max() > 0 for (name, _), one in zip(named, first) if not name.startswith("k.b"))   # (dbk is 0 in exact arithmetic)


@pytest.mark.parametrize("S,form", CELLS, ids=IDS)
def test_training_draws_a_fresh_mask_and_evaluation_is_the_forward_without_dropout(nk, tdev, inputs, S, form):
    q, k, v, _ = inputs[S]
    seg = _segments(nk, tdev, S, form)
    # the strided node, in a graph without gradients
    Q, K, V = (nk.from_ndarray(tdev, t) for t in (q, k, v))
    plain = _core(Q, K, V, S, form, 0.0, nk.Status(False), seg); plain.forward()
    status = nk.Status(True)
    y = _core(Q, K, V, S, form, 0.1, status, seg)
    y.forward(); one = y.data().copy()
    y.forward(); two = y.data().copy()
    assert not np.array_equal(one, two) and not np.array_equal(one, plain.data())
    status.set(False)
    y.forward()
    assert np.array_equal(y.data(), plain.data())
    # the packed node, differentiable
    want = _forward(_module(nk, tdev, form, 0.0, True), nk.from_ndarray(tdev, q).requires_grad(), seg); want.forward()
    mha = _module(nk, tdev, form, 0.1, True)
    mha.drop.train()
    y = _forward(mha, nk.from_ndarray(tdev, q).requires_grad(), seg)
    y.forward(); one = y.data().copy()
    y.forward(); two = y.data().copy()
    assert not np.array_equal(one, two) and not np.array_equal(one, want.data())
    mha.drop.eval()
    y.forward()
    assert np.array_equal(y.data(), want.data())


@pytest.mark.parametrize("S,form", [c for c in CELLS if c[1] in ("full", "segments, band")],
                         ids=[i for c, i in zip(CELLS, IDS) if c[1] in ("full", "segments, band")])
def test_a_graph_without_gradients_gives_the_differentiable_forward(nk, tdev, inputs, S, form):
    q, k, v, _ = inputs[S]
    seg = _segments(nk, tdev, S, form)
    out = _core(*(nk.from_ndarray(tdev, t) for t in (q, k, v)), S, form, 0.0, nk.Status(False), seg)
    out.forward()
    kept = _core(*(nk.from_ndarray(tdev, t).requires_grad() for t in (q, k, v)), S, form, 0.0, nk.Status(False), seg)
    kept.forward()
    assert np.isfinite(out.data()).all() and np.abs(out.data()).max() > 0
    assert np.array_equal(out.data(), kept.data())

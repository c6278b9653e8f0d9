"""nn.Sampler / Var.sample through `neuronika_amd.tape` against tests/sampling_oracle.py: every id equal (the fixed inputs are the
TAPE entries of tests/sampling_cases.py, which tests/test_oracle_sampling.py shows to be unambiguous at EPS on the CPU), the offset
counter, the ids feeding nn.Embedding on the device, the VarDiff overload, the panics, and examples/generate.py with --device-sample."""
import importlib.util
import os

import numpy as np
import pytest

import sampling_cases as SC
import sampling_oracle as SO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nk():
    import neuronika_amd
    return neuronika_amd.tape


@pytest.fixture(scope="module")
def tdev(nk):
    return nk.Device(0)


@pytest.fixture(scope="module")
def generate():
    spec = importlib.util.spec_from_file_location("generate", os.path.join(ROOT, "examples", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("i", range(len(SC.TAPE)))
def test_forward_draws_the_last_row_of_every_sample_and_consumes_offsets(nk, tdev, i):
    batch, T, V, prm, _ = SC.TAPE[i]
    logits, last, seed = SC.tape_input(i)
    sampler = nk.nn.Sampler(tdev, temperature=prm.temperature, top_k=prm.top_k, top_p=prm.top_p, seed=seed)
    assert (sampler.temperature, sampler.top_k, sampler.top_p, sampler.seed, sampler.offset) == (np.float32(prm.temperature), prm.top_k, np.float32(prm.top_p), seed, 0)
    x = nk.from_ndarray(tdev, logits)
    ids = sampler.forward(x, batch)
    assert sampler.offset == 0                                           # building the node draws nothing
    ids.forward()
    assert ids.data().shape == (batch,) and ids.data().dtype == np.float32
    assert (ids.data() == SO.sample(last, prm, seed, 0)).all() and sampler.offset == 1
    ids.forward()                                                        # the second execution draws at offset 1
    assert (ids.data() == SO.sample(last, prm, seed, 1)).all() and sampler.offset == 2
    assert (x.data() == logits).all()
    # Var.sample is the same node; the counter is the sampler's, shared by every node it built
    again = x.sample(sampler, batch)
    again.forward()
    assert (again.data() == SO.sample(last, prm, seed, 2)).all() and sampler.offset == 3
    sampler.offset = 0
    again.forward()
    assert (again.data() == SO.sample(last, prm, seed, 0)).all() and sampler.offset == 1


def test_ids_feed_the_embedding_on_the_device_and_the_vardiff_overload_agrees(nk, tdev):
    batch, T, V, prm, _ = SC.TAPE[1]
    logits, last, seed = SC.tape_input(1)
    want = SO.sample(last, prm, seed, 0)
    emb = nk.nn.Embedding(tdev, V, 24, seed=5)
    table = emb.weight.data()
    sampler = nk.nn.Sampler(tdev, temperature=prm.temperature, top_k=prm.top_k, top_p=prm.top_p, seed=seed)
    rows = emb.forward(sampler.forward(nk.from_ndarray(tdev, logits), batch))
    rows.forward()                                                       # runs the sampling node, then the gather
    assert rows.data().shape == (batch, 24) and (rows.data() == table[want]).all()
    # a differentiable input (what a Linear head returns) enters through its data; the ids carry no gradient
    head = nk.nn.Linear(nk.from_ndarray(tdev, np.eye(V, dtype=np.float32)).requires_grad(), nk.from_ndarray(tdev, np.zeros(V, np.float32)).requires_grad())
    out = head.forward(nk.from_ndarray(tdev, logits))                    # = logits, as a VarDiff
    sampler.offset = 0
    ids = sampler.forward(out, batch)
    assert type(ids) is nk.Var
    ids.forward()
    assert (ids.data() == want).all()


def test_panics(nk, tdev):
    x = nk.from_ndarray(tdev, np.zeros((6, 10), np.float32))
    s = nk.nn.Sampler(tdev)
    assert (s.temperature, s.top_k, s.top_p, s.seed, s.offset) == (1.0, 0, 1.0, 0, 0)
    for batch in (4, 0, -1, 7):
        with pytest.raises(Exception):
            s.forward(x, batch)
    with pytest.raises(Exception):
        nk.from_ndarray(tdev, np.zeros(6, np.float32)).sample(s, 2)      # not (batch*T, V)
    for kw in (dict(temperature=-1.0), dict(temperature=float("inf")), dict(top_p=0.0), dict(top_p=float("nan"))):
        with pytest.raises(Exception):
            nk.nn.Sampler(tdev, **kw)
    s.temperature = -2.0                                                 # a member set to nonsense later is refused when the node is built
    with pytest.raises(Exception):
        s.forward(x, 2)
    assert s.offset == 0


@pytest.mark.parametrize("rope", [False, True])
def test_generate_on_the_device_equals_the_host_path_at_temperature_0(generate, rope):
    host, worst_h = generate.main(16, rope=rope)
    device, worst_d = generate.main(16, rope=rope, device_sample=True)
    assert host.shape == device.shape == (1, 8 + 16) and (host == device).all(), (host, device)
    assert np.isfinite(worst_d) and np.isfinite(worst_h)


def test_generate_with_a_fixed_seed_repeats(generate):
    a, _ = generate.main(16, device_sample=True, temperature=0.8, top_k=8, seed=3)
    b, _ = generate.main(16, device_sample=True, temperature=0.8, top_k=8, seed=3)
    assert (a == b).all() and ((a >= 0) & (a < generate.VOCAB)).all()
    g, _ = generate.main(16, device_sample=True)
    assert (a != g).any()                                                # at this temperature the draws leave the greedy path

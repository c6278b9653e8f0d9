"""nk_embedding_* through the C ABI (`capi`) against tests/embedding_oracle.py, BIT FOR BIT: the forward is a copy and the oracle
restates the backward's summation order (ascending token position, from the first contribution, chunks of 128 added in chunk
order).  Every device array sits between guard bands that must come back intact: out-of-range ids are defined behaviour."""
import numpy as np
import pytest

import embedding_oracle as E

pytestmark = pytest.mark.gpu

GUARD = 37.25  # the value of every guard float


class Guarded:
    """`lead` guard floats, the body, 8 guard floats, in one allocation: lead % 4 != 0 takes the body's 16-byte alignment away"""

    def __init__(self, dev, body, lead=4):
        body = np.ascontiguousarray(body, dtype=np.float32)
        self.shape, self.n, self.lead = body.shape, body.size, lead
        self.whole = dev.array(np.concatenate([np.full(lead, GUARD, np.float32), body.reshape(-1), np.full(8, GUARD, np.float32)]))
        self.body = self.whole.view_offset(lead)

    def numpy(self):
        a = self.whole.numpy()
        assert (a[:self.lead] == GUARD).all() and (a[self.lead + self.n:] == GUARD).all(), "a guard band was overwritten"
        return a[self.lead:self.lead + self.n].reshape(self.shape)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
    assert bad.size == 0, (what, bad.size, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


def uniform_ids(rng, n, V):
    return rng.integers(0, V, n).astype(np.float32)


def zipf_ids(rng, n, V):
    """natural-language shape: rank r with probability ~ 1 / r, ranks scattered over the table"""
    p = 1.0 / np.arange(1, V + 1)
    ranks = rng.choice(V, size=n, p=p / p.sum())
    return rng.permutation(V)[ranks].astype(np.float32)


def run_all(dev, weight, idx, g, dw0, padding_idx=-1, lead=4):
    """forward, `+=` backward onto dw0, assign backward onto NaN garbage; guard bands checked on every array"""
    from neuronika_amd import capi as c
    V, D = weight.shape
    n = idx.size
    W, I, G = Guarded(dev, weight, lead), Guarded(dev, idx, lead), Guarded(dev, g, lead)
    OUT = Guarded(dev, np.full((n, D), np.nan, np.float32), lead)
    DW = Guarded(dev, dw0, lead)
    DA = Guarded(dev, np.full((V, D), np.nan, np.float32), lead)
    c.embedding_fwd(dev, W.body, I.body, OUT.body, n, V, D)
    c.embedding_bwd(dev, DW.body, G.body, I.body, n, V, D, padding_idx)
    c.embedding_bwd(dev, DA.body, G.body, I.body, n, V, D, padding_idx, assign=True)
    for a in (W, I, G):
        a.numpy()  # inputs: guards only
    return OUT.numpy(), DW.numpy(), DA.numpy()


def check_case(dev, V, D, idx, seed=0, padding_idx=-1, lead=4):
    rng = np.random.default_rng(seed)
    idx = np.asarray(idx, np.float32)
    weight = rng.standard_normal((V, D)).astype(np.float32)
    g = rng.standard_normal((idx.size, D)).astype(np.float32)
    dw0 = rng.standard_normal((V, D)).astype(np.float32)
    out, dw, da = run_all(dev, weight, idx, g, dw0, padding_idx, lead)
    same_bits(out, E.forward(weight, idx).reshape(-1, D), "forward")
    same_bits(dw, E.backward(dw0, g, idx, padding_idx), "backward +=")
    same_bits(da, E.backward_assign(g, idx, V, padding_idx), "backward assign")


@pytest.mark.parametrize("D", (1, 3, 4, 64, 100, 768, 1024, 4096))
@pytest.mark.parametrize("lead", (4, 1))
def test_every_width_aligned_and_misaligned(dev, D, lead):
    rng = np.random.default_rng(D)
    check_case(dev, 300, D, uniform_ids(rng, 1000, 300), seed=D, lead=lead)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4096, 100000))
def test_token_counts(dev, n):
    rng = np.random.default_rng(n)
    check_case(dev, 1000, 64, uniform_ids(rng, n, 1000), seed=n)


@pytest.mark.parametrize("V", (1, 2, 50257, 131072))
def test_table_heights(dev, V):
    rng = np.random.default_rng(V)
    check_case(dev, V, 8, uniform_ids(rng, 5000, V), seed=V)


def test_ids_fractional_negative_nan_and_out_of_range(dev):
    V = 50
    idx = np.array([0.0, 0.99, 1.5, 49.0, 49.99, 50.0, 51.0, -1.0, -0.5, -1e30, np.nan, np.inf, -np.inf, 1e9, 1e19, 3.4e38, 7.0, 7.9, 16777216.0,
                    -0.0], np.float32)
    check_case(dev, V, 12, idx)
    check_case(dev, V, 5, np.tile(idx, 40), seed=1, lead=3)
    assert (E.read_ids(idx)[:6] == [0, 0, 1, 49, 49, 50]).all()


def test_all_tokens_on_one_row(dev):
    """one segment far beyond one chunk: the chunked order (partials per chunk, added in chunk order)"""
    n = 20000
    for D in (64, 100):
        check_case(dev, 40, D, np.full(n, 17.0, np.float32), seed=D)
    # CHUNK tokens are still one chunk, one more makes two
    for n in (E.CHUNK, E.CHUNK + 1, 2 * E.CHUNK, 2 * E.CHUNK + 1):
        check_case(dev, 3, 8, np.full(n, 2.0, np.float32), seed=n)


def test_chunked_order_is_not_the_plain_order(dev):
    """the test above would pass with any order if the two agreed on its data: they do not"""
    rng = np.random.default_rng(5)
    g = rng.standard_normal((20000, 4)).astype(np.float32)
    idx = np.zeros(20000, np.float32)
    assert not np.array_equal(E.backward_assign(g, idx, 1), E.backward_assign(g, idx, 1, chunk=1 << 30))


def test_zipf_ids(dev):
    rng = np.random.default_rng(11)
    idx = zipf_ids(rng, 30000, 5000)
    assert np.bincount(idx.astype(np.int64)).max() > 2 * E.CHUNK   # some rows are chunked, most are not
    check_case(dev, 5000, 96, idx, seed=2)


def test_every_id_distinct(dev):
    rng = np.random.default_rng(12)
    check_case(dev, 6000, 32, rng.permutation(6000)[:5000].astype(np.float32), seed=3)


def test_padding_idx_hit_by_many_tokens(dev):
    rng = np.random.default_rng(13)
    idx = uniform_ids(rng, 8000, 200)
    idx[rng.random(8000) < 0.6] = 3.0
    check_case(dev, 200, 48, idx, seed=4, padding_idx=3)
    g = rng.standard_normal((8000, 48)).astype(np.float32)
    assert not E.backward_assign(g, idx, 200, 3)[3].any() and E.backward_assign(g, idx, 200)[3].any()
    check_case(dev, 200, 48, idx, seed=4, padding_idx=0)
    check_case(dev, 200, 48, idx, seed=4, padding_idx=10 ** 12)   # beyond the table: no id equals it


def test_no_tokens(dev):
    from neuronika_amd import capi as c
    V, D = 7, 12
    dw0 = np.arange(V * D, dtype=np.float32).reshape(V, D)
    DW, DA = Guarded(dev, dw0), Guarded(dev, np.full((V, D), np.nan, np.float32))
    c.embedding_fwd(dev, DW.body, None, None, 0, V, D)
    c.embedding_bwd(dev, DW.body, None, None, 0, V, D)
    c.embedding_bwd(dev, DA.body, None, None, 0, V, D, assign=True)
    same_bits(DW.numpy(), dw0, "+= with no tokens")
    same_bits(DA.numpy(), np.zeros((V, D), np.float32), "assign with no tokens covers the table")


def test_four_runs_give_the_same_bits(dev):
    from neuronika_amd import capi as c
    rng = np.random.default_rng(14)
    V, D, n = 3000, 256, 40000
    idx = zipf_ids(rng, n, V)
    G, I = dev.array(rng.standard_normal((n, D)).astype(np.float32)), dev.array(idx)
    runs = []
    for _ in range(4):
        DA = dev.full((V, D), np.nan)
        c.embedding_bwd(dev, DA, G, I, n, V, D, assign=True)
        runs.append(DA.numpy())
    for r in runs[1:]:
        same_bits(r, runs[0], "repeat")


def test_bad_arguments_are_refused(dev):
    from neuronika_amd import capi as c
    a = dev.zeros(16)
    for V, D, n in (((1 << 24) + 1, 1, 1), (0, 4, 1), (4, 0, 1), (4, 4, -1)):
        with pytest.raises(c.NeuronikaHipError):
            c.embedding_fwd(dev, a, a, a, n, V, D)
        for assign in (False, True):
            with pytest.raises(c.NeuronikaHipError):
                c.embedding_bwd(dev, a, a, a, n, V, D, assign=assign)
    same_bits(a.numpy(), np.zeros(16, np.float32), "nothing written")

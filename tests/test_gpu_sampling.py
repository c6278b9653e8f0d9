"""nk_sample_fwd through the C ABI (`capi`) against tests/sampling_oracle.py in f64: EVERY id must equal the oracle's.  Every device
array sits between guard bands that must come back intact (tests/test_gpu_embedding.py's `Guarded`), the logits bit-identical.

Why equality can be demanded.  The device decides on integers (weights truncated to multiples of 2^-40), the oracle in f64; they can
differ only where a decision lies at a boundary: a cumulative mass at a distinct-value level against top_p, or u against a CDF
boundary of the kept set.  The device's normalised CDF differs from the f64 one by
    the rounding of (x - m) * c:   |arg| * 2^-24 * ln 2 relative per weight, under 2e-6 for |x - m| / T <= 40 (beyond it a weight is
                                   below 2^-57 of the maximum's and truncates to 0 either way)
  + the error of the f32 exponential, a few ulp: a few times 6e-8
  + the truncation: at most V * 2^-40 of the maximum's weight, under 1e-6 for V <= 2^20
together below 5e-6.  EPS = 1e-4 has about 20 times that: tests/test_oracle_sampling.py checks ON THE CPU that no fixed input of this
file has a decision within EPS of a boundary (`sampling_oracle.ambiguity` is empty for every case of tests/sampling_cases.py, whose
seeds were chosen on the CPU until that held), so no case is left out here and no id is forgiven.

The equivalences `top_k = 1 == greedy`, `top_p = 1e-6 == greedy` and `temperature = 1e-6 == greedy` are statements about rows with a
UNIQUE maximum: ties at a threshold all stay (section 1 of the header), so a row whose maximum is shared keeps every holder of it and
draws among them - there the test demands a holder of the maximum."""
import numpy as np
import pytest

import sampling_cases as SC
import sampling_oracle as SO
from test_gpu_embedding import GUARD, Guarded, same_bits

pytestmark = pytest.mark.gpu

MARK = np.float32(-7.0)                                                  # what ids hold before a call


@pytest.fixture(scope="module")
def L():
    from neuronika_amd import capi as c
    return c.sample_stage_limit()


def embed(x, ld, seed=0):
    """(rows, V) rows at stride ld in the shortest buffer that holds them: (rows - 1) * ld + V floats, the gaps filled with values
    above every ordinary logit (a kernel that read them would return them)"""
    rows, V = x.shape
    buf = np.full((rows - 1) * ld + V, 29.0, np.float32) + np.random.default_rng(seed).random((rows - 1) * ld + V, dtype=np.float32)
    for r in range(rows):
        buf[r * ld:r * ld + V] = x[r]
    return buf


def run(dev, x, ld, lead, prm, seed, offset):
    """-> ids (rows,) as the device wrote them; checks the guards, that the logits came back bit-identical and that every id is an
    integer in [0, V)"""
    from neuronika_amd import capi as c
    x = np.asarray(x, np.float32)
    rows, V = x.shape
    buf = embed(x, ld)
    X, IDS = Guarded(dev, buf, lead), Guarded(dev, np.full(rows, MARK, np.float32), 4)
    c.sample_fwd(dev, X.body, ld, rows, V, IDS.body, prm.temperature, prm.top_k, prm.top_p, seed, offset)
    ids = IDS.numpy()
    same_bits(X.numpy(), buf, "the logits were written")
    assert ((ids >= 0) & (ids < V) & (ids == np.floor(ids))).all(), ids
    return ids.astype(np.int64)


def test_stage_limit_is_a_constant_within_the_lds(L):
    from neuronika_amd import capi as c
    assert L == c.sample_stage_limit() and 1024 <= L and L * 4 <= 160 * 1024


@pytest.mark.parametrize("tag", SC.V_TAGS, ids=[str(t) for t in SC.V_TAGS])
def test_grid_every_id_equals_the_oracle(dev, L, tag):
    mine = [c for c in SC.cases(L) if c.tag == tag]
    assert {c.mode for c in mine} == {m[0] for m in SC.MODES} and {c.lead for c in mine} == {4, 5, 6, 7}
    assert any(c.lead == 4 and c.ld % 4 == 0 for c in mine) and {c.rows for c in mine} >= {1, 3}
    for case in mine:
        x = SC.logits(case)
        want = SO.sample(x, case.prm, case.seed, case.offset)
        got = run(dev, x, case.ld, case.lead, case.prm, case.seed, case.offset)
        assert (got == want).all(), (case, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])


def special_rows(V):
    """name -> (row, the id every mode must return)"""
    rng = np.random.default_rng(V)
    base = (rng.random(V, dtype=np.float32) * np.float32(16) - np.float32(8)).astype(np.float32)
    out = {}
    if V >= 3:
        a = base.copy(); a[[V // 3, V - 1]] = np.inf
        out["+inf twice"] = (a, V // 3)
        z = -np.abs(base) - np.float32(1); z[V // 2] = -0.0; z[V - 1] = 0.0
        out["-0 before +0"] = (z, V // 2)
        n = np.full(V, np.nan, np.float32); n[V // 2:] = -np.inf
        out["NaN then -inf"] = (n, V // 2)                              # NaN sorts below -inf: the first -inf is the maximum
    out["only -inf"] = (np.full(V, -np.inf, np.float32), 0)
    out["only NaN"] = (np.full(V, np.nan, np.float32), 0)
    return out


@pytest.mark.parametrize("V", [1, 5, 300, 4099, "L", "L+4"])
def test_rows_without_a_finite_maximum_and_signed_zeros(dev, L, V):
    V = SC.resolve(V, L)
    rows = special_rows(V)
    x = np.stack([r for r, _ in rows.values()])
    want = np.array([i for _, i in rows.values()])
    for lead, ld in ((4, (V + 3) // 4 * 4), (5, V + 1)):
        for prm in (SO.Params(0.0, 0, 1.0), SO.Params(1.0, 0, 1.0), SO.Params(0.7, 2, 0.9), SO.Params(1.5, 40, 1.0), SO.Params(1.0, 0, 0.5)):
            got = run(dev, x, ld, lead, prm, 11, 3)
            # greedy returns the lower of the two zeros; a draw sees one value held twice and may return either holder (top_k = 2
            # keeps exactly the two), or, unfiltered, any finite token
            exact = np.array([prm.temperature == 0 or k != "-0 before +0" for k in rows])
            assert (got[exact] == want[exact]).all(), (V, lead, prm, list(rows), got, want)
            if not exact.all() and prm.top_k == 2:
                assert got[~exact][0] in (V // 2, V - 1), (V, lead, prm, got)
    assert (SO.sample(x, SO.Params(0.0, 0, 1.0)) == want).all()


@pytest.mark.parametrize("V", [2, 65, 1025, "L", "L+1", 50257])
def test_equivalences_that_need_no_oracle(dev, L, V):
    V = SC.resolve(V, L)
    greedy = SO.Params(0.0, 0, 1.0)
    for kind, lead, ld in (("uniform", 4, (V + 3) // 4 * 4), ("integers", 5, V), ("masked", 6, V + 3), ("nan", 4, 2 * ((V + 1) // 2 * 2)), ("dominant", 7, V + 1)):
        x = SC.make(kind, 3, V, 17 + V)
        lo = np.where(np.isnan(x), -np.inf, x)
        m = lo.max(axis=1)
        holders = lo == m[:, None]
        second = np.where(holders, -np.inf, lo).max(axis=1)
        unique = holders.sum(axis=1) == 1
        g = run(dev, x, ld, lead, greedy, 0, 0)
        assert (g == holders.argmax(axis=1)).all(), (kind, V)
        for what, prm in (("top_k = 1", SO.Params(1.0, 1, 1.0)), ("top_p = 1e-6", SO.Params(1.0, 0, 1e-6)), ("both", SO.Params(0.7, 1, 1e-6))):
            for seed, offset in ((1, 0), (2 ** 63 + 5, 2 ** 40 + 1)):
                got = run(dev, x, ld, lead, prm, seed, offset)
                assert (got[unique] == g[unique]).all(), (what, kind, V, got, g)
                assert holders[np.arange(3), got].all(), (what, kind, V, got)
        # temperature 1e-6: every other token sits (m - x) * 1.44e6 below the maximum in the exponent; from a gap of 1e-3 on that is
        # beyond -1000 and its weight is 0
        far = m - second >= 1e-3
        clear = unique & far
        got = run(dev, x, ld, lead, SO.Params(1e-6, 0, 1.0), 5, 9)
        assert (got[clear] == g[clear]).all() and holders[np.arange(3), got][far].all(), (kind, V, got, g)
        if kind == "dominant":
            assert clear.all(), (kind, V)
        # a token of weight 0 is never drawn: NaN and -inf tokens whatever the mode
        for prm in (SO.Params(1.5, 0, 1.0), SO.Params(1.0, V - 1, 1.0), SO.Params(1.0, 0, 0.999), SO.Params(1.0, 40, 0.9)):
            for offset in range(4):
                got = run(dev, x, ld, lead, prm, 77, offset)
                assert np.isfinite(x[np.arange(3), got]).all(), (kind, V, prm, offset, got)


@pytest.mark.parametrize("V,prm", [(255, SO.Params(1.0, 0, 1.0)), (4099, SO.Params(0.7, 40, 0.9)), ("L", SO.Params(1.0, 0, 0.9)), ("L-1", SO.Params(1.5, 40, 1.0)),
                                   (1024, SO.Params(1.0, 2, 0.5))])
def test_a_row_keeps_its_id_whatever_surrounds_it(dev, L, V, prm):
    """the id depends on the row's logits and (params, seed, offset, r) only: not on rows, ld, the lead, the other rows, or staging"""
    V = SC.resolve(V, L)
    seed, offset = 0xABCDEF0123, 2 ** 33 + 7
    x17 = SC.make("uniform", 17, V, 5 + V)
    ids17 = run(dev, x17, (V + 3) // 4 * 4, 4, prm, seed, offset)
    assert (run(dev, x17, (V + 3) // 4 * 4, 4, prm, seed, offset) == ids17).all()          # two identical calls
    assert (run(dev, x17, V + 1, 5, prm, seed, offset) == ids17).all()                    # the scalar family, another stride
    for r in (0, 6, 16):
        alone = np.zeros((r + 1, V), np.float32)                        # rows 0 .. r-1 are filler, row r is the row under test
        alone[r] = x17[r]
        assert run(dev, alone, 2 * V, 7, prm, seed, offset)[r] == ids17[r], r
        assert run(dev, alone, (V + 3) // 4 * 4, 4, prm, seed, offset)[r] == ids17[r], r
    if V <= L:
        # the same rows followed by -inf up to L + 8 tokens: the same kept sets, weights and draws, but re-read from memory instead
        # of staged in LDS
        wide = np.full((17, L + 8), -np.inf, np.float32)
        wide[:, :V] = x17
        assert (run(dev, wide, L + 8, 4, prm, seed, offset) == ids17).all()
        assert (run(dev, wide, L + 9, 6, prm, seed, offset) == ids17).all()


def test_offsets_give_the_oracles_draws(dev):
    x, seed = SC.offsets_input()
    prm = SC.OFFSETS["prm"]
    seen = []
    for off in SC.OFFSETS["offsets"]:
        got = run(dev, x, x.shape[1], 4, prm, seed, off)
        assert (got == SO.sample(x, prm, seed, off)).all(), off
        seen.append(tuple(got))
    assert len(set(seen)) > 1                                            # the draws do differ


def test_invalid_arguments_write_nothing(dev):
    from neuronika_amd import capi as c
    V, rows = 40, 3
    X = Guarded(dev, SC.make("uniform", rows, V, 1), 4)
    IDS = Guarded(dev, np.full(rows, MARK, np.float32), 4)
    ok = dict(logits=X.body, ld=V, rows=rows, V=V, ids=IDS.body, temperature=1.0, top_k=0, top_p=1.0)
    bad = [dict(logits=None), dict(ids=None), dict(rows=0), dict(rows=-2), dict(V=0), dict(V=-1), dict(V=2 ** 20 + 1, ld=2 ** 20 + 1), dict(ld=V - 1),
           dict(temperature=-0.5), dict(temperature=float("inf")), dict(temperature=float("nan")), dict(top_p=0.0), dict(top_p=-0.1),
           dict(top_p=float("nan"))]
    for change in bad:
        a = dict(ok, **change)
        with pytest.raises(c.NeuronikaHipError) as e:
            c.sample_fwd(dev, a["logits"], a["ld"], a["rows"], a["V"], a["ids"], a["temperature"], a["top_k"], a["top_p"], 3, 4)
        assert e.value.code == 1, change                                 # NK_ERR_INVALID
        assert (IDS.numpy() == MARK).all(), change
    c.sample_fwd(dev, ok["logits"], V, rows, V, IDS.body, 1.0, -3, 7.0, 3, 4)    # top_k <= 0 and top_p >= 1 only turn the filters off
    assert (IDS.numpy() != MARK).all()
    assert GUARD not in IDS.numpy()

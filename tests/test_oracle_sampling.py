"""tests/sampling_oracle.py pinned without a GPU - greedy, the top-k and top-p sets, the distribution of its draws - and the condition
the GPU tests rest on: no fixed input of tests/test_gpu_sampling.py / tests/test_gpu_tape_sampling.py has a decision within EPS of a
boundary (`ambiguity` is empty for every case of tests/sampling_cases.py), which is why those tests may demand equality of every id."""
import numpy as np
import pytest

import sampling_cases as SC
import sampling_oracle as SO

L = 32768                                                                # nk_sample_stage_limit(); checked below against the library


def test_the_stage_limit_the_cases_were_searched_with():
    from neuronika_amd import capi
    assert capi.sample_stage_limit() == L


def test_greedy_is_argmax():
    rng = np.random.default_rng(1)
    for V in (1, 2, 7, 300):
        x = rng.standard_normal((9, V)).astype(np.float32)
        x[3] = np.round(x[3])                                            # ties: the lowest index
        assert (SO.sample(x, (0.0, 5, 0.3), seed=4, offset=9) == np.argmax(x, axis=1)).all()
    x = np.array([[1, np.inf, 3, np.inf], [-np.inf] * 4, [np.nan] * 4, [np.nan, -np.inf, np.nan, -np.inf], [-1, -0.0, 0.0, -2]], np.float32)
    for prm in ((0.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 2, 0.5)):
        assert list(SO.sample(x, prm)[:4]) == [1, 0, 0, 1]               # a maximum that is not finite: greedy whatever the mode
    assert SO.sample(x, (0.0, 0, 1.0))[4] == 1                           # -0 counts as +0: the lower index


def test_top_k_set_is_the_kth_filter():
    rng = np.random.default_rng(2)
    for V, k in ((10, 3), (64, 1), (64, 40), (257, 256), (33, 33), (33, 40), (33, 0)):
        for x in (rng.standard_normal(V).astype(np.float32), rng.integers(-3, 4, V).astype(np.float32)):
            kept = SO.kept_set(x, (1.0, k, 1.0))
            if k <= 0 or k >= V:
                assert kept.all()
            else:
                kth = np.sort(x)[::-1][k - 1]
                assert (kept == ~(x < kth)).all() and kept.sum() >= k    # ties at the threshold all stay


def test_top_p_set_is_the_smallest_value_closed_set_with_the_mass():
    rng = np.random.default_rng(3)
    for V, p, k in ((10, 0.5, 0), (64, 0.9, 0), (64, 0.999, 0), (257, 1e-6, 0), (40, 0.6, 7), (300, 0.9, 40)):
        for x in (rng.standard_normal(V).astype(np.float32) * 2, rng.integers(-3, 4, V).astype(np.float32)):
            S = SO.kept_set(x, (1.0, k, 1.0))
            kept = SO.kept_set(x, (1.0, k, p))
            w = np.where(S, np.exp(x.astype(np.float64) - x.max()), 0.0)
            assert (kept <= S).all() and w[kept].sum() >= np.float32(p) * w.sum()
            t = x[kept].min()
            assert (kept == (S & (x >= t))).all()                       # value-closed: ties stay
            smaller = S & (x > t)                                        # the next smaller value-closed set misses the mass
            assert w[smaller].sum() < np.float32(p) * w.sum()


def test_draws_follow_the_distribution():
    V, n = 8, 20000
    x = np.array([0.3, -1.0, 2.0, 0.0, -np.inf, 1.1, -0.4, 0.9], np.float32)
    for prm, keep in (((1.0, 0, 1.0), np.ones(V, bool)), ((0.7, 4, 1.0), None), ((1.5, 0, 0.8), None)):
        kept = SO.kept_set(x, prm) if keep is None else keep
        p = np.where(kept & np.isfinite(x), np.exp((x.astype(np.float64) - 2.0) / prm[0]), 0.0)
        p /= p.sum()
        ids = SO.draws(x, prm, 12345, np.arange(n))
        assert all(SO.sample(x[None], prm, seed=12345, offset=o)[0] == ids[o] for o in (0, 1, 777, n - 1))
        counts = np.bincount(ids, minlength=V)
        assert (counts[p == 0] == 0).all()
        live = p > 0
        chi2 = float((((counts - n * p) ** 2)[live] / (n * p[live])).sum())
        # the 1 - 1e-6 quantiles of chi-square with 1 .. 7 degrees of freedom
        q = {1: 23.93, 2: 27.63, 3: 30.66, 4: 33.38, 5: 35.89, 6: 38.26, 7: 40.52}[int(live.sum()) - 1]
        assert chi2 < q, (prm, chi2, q, counts)
    # rows of one call draw from different counters
    u = SO.uniforms(7, 2 ** 40 + 3, 5)
    assert len(set(u)) == 5 and (SO.uniforms(7, 2 ** 40 + 3, 2, row0=3) == u[3:]).all()


def test_ambiguity_sees_a_decision_at_a_boundary():
    x = np.array([[0.0, 0.0, 0.0, 0.0]], np.float32)                     # CDF boundaries at 0.25, 0.5, 0.75
    seeds = [s for s in range(400) if abs(SO.uniforms(s, 0, 1)[0] - 0.5) < 5e-3]
    assert seeds and all(SO.ambiguity(x, (1.0, 0, 1.0), s, 0, 5e-3) == [0] for s in seeds)
    y = np.array([[np.log(3.0), 0.0]], np.float32)                       # masses 0.75, 0.25: the first level sits at top_p = 0.75
    assert SO.ambiguity(y, (1.0, 0, 0.75), 1, 0, 1e-4) == [0] and SO.ambiguity(y, (0.0, 0, 0.75), 1, 0, 1e-4) == []


@pytest.mark.parametrize("tag", SC.V_TAGS, ids=[str(t) for t in SC.V_TAGS])
def test_no_fixed_input_of_the_gpu_grid_is_ambiguous(tag):
    mine = [c for c in SC.cases(L) if c.tag == tag]
    assert len(mine) in (len(SC.MODES), 2 * len(SC.MODES))
    for c in mine:
        assert SO.ambiguity(SC.logits(c), c.prm, c.seed, c.offset, SC.EPS) == [], c


def test_the_grid_covers_what_it_must():
    cs = SC.cases(L)
    assert {c.V for c in cs} == {1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099, L - 1, L, L + 1, L + 4, 50257, 131072}
    assert {c.rows for c in cs} == {1, 3, 17} and {c.lead for c in cs} == {4, 5, 6, 7} and {c.kind for c in cs} == set(SC.KINDS)
    for V in {c.V for c in cs}:
        mine = [c for c in cs if c.V == V]
        assert {c.mode for c in mine} == {m[0] for m in SC.MODES}
        assert {c.ld for c in mine} <= {V, V + 1, V + 3, 2 * V} and len({c.ld for c in mine}) >= 3
        assert any(c.lead == 4 and c.ld % 4 == 0 for c in mine) and any(c.lead != 4 for c in mine)      # both access families
    for V in (L - 1, L, L + 1, L + 4):                                  # both sides of L: every mode in both families
        for fam in (True, False):
            assert {c.mode for c in cs if c.V == V and (c.lead == 4) == fam} == {m[0] for m in SC.MODES}
    big = [c for c in cs if c.V >= L - 1 and c.prm.temperature > 0]
    assert {c.kind for c in big} >= {"ladder", "dominant"}


def test_no_extra_fixed_input_is_ambiguous():
    x, seed = SC.offsets_input()
    for off in SC.OFFSETS["offsets"]:
        assert SO.ambiguity(x, SC.OFFSETS["prm"], seed, off, SC.EPS) == []
    assert len({tuple(SO.sample(x, SC.OFFSETS["prm"], seed, off)) for off in SC.OFFSETS["offsets"]}) > 1
    for i, (batch, T, V, prm, _) in enumerate(SC.TAPE):
        logits, last, seed = SC.tape_input(i)
        assert logits.shape == (batch * T, V) and last.shape == (batch, V)
        for off in (0, 1):
            assert SO.ambiguity(last, prm, seed, off, SC.EPS) == []

"""The score rows of tests/decode_rows.py, checked without a GPU: that their raw scores are exact in f32, that the kinds have the spread
they are built for, that a correct replay of the decode kernels' arithmetic satisfies the bound tests/test_gpu_attention_decode_rows.py
applies to the device, that every wrong one (decode_rows.FLAWS) is far outside it on a named case - and that on `plain` rows, the data
of every other decode test, a wrong SHIFT is not.

The bound.  SURVEY 8c (ii), err <= max(2 * err_cpu32, 1e-6 * yardstick) against the f64 oracle, with err_cpu32 the larger of two plain
f32 references' errors: the oracle in f32 (softmax of scores * scale in nats) and the full-row softmax in the exponent domain
(decode_rows.exponent_softmax: s = f32(d * c1), exp2(s - max s), no chunks).  At dh 64 the first one's scores * scale is EXACT
(scale = 1/8) while any exp2 kernel rounds d * c1 at |s| up to 226: against the first reference alone the correct replay reads up
to 2.65 x the bound at dh 64 (`falling`; `climbing` 1.84 x), 1.56 x at dh 128 and 1.10 x at dh 20.  The second reference carries that
rounding and nothing of the kernel's structure.  The factors 2 and 1e-6 are the project's own.

Measured with the replay, worst err / bound over the 50 cases per kind (the seeds of decode_rows.SEEDS):
  plain 0.03  climbing 0.53  falling 0.56  lifted 0.51  sunk 0.51  peaked 0.33  edge 0.33  edge_in 0.33
Flawed replays, on the cases of TEETH: "no_shift" non-finite on every lifted and sunk row (40 cases); "stale_head_max" non-finite on
every sunk head behind a lifted one (15); "combine_first_m" non-finite on climbing problems of three chunks (20); "wave_local_max"
3.1e4 .. 5.8e5, "combine_no_rescale" 2.7e4 .. 6.1e5 and "combine_l_unscaled" 8.8e3 .. 4.1e5 bounds out on climbing and falling;
"lo_off_by_one" 7.5e5 .. 1.4e6 bounds out on edge.
The control: with every head `plain`, the three flaws that are a consistent wrong shift (decode_rows.SHIFT_FLAWS) stay inside 0.05 of
the bound - that is why the uniform data of the other decode tests cannot see them in the result - while "wave_local_max" and the
two combine flaws, which add partials taken under DIFFERENT shifts without rescaling, are 3e2 .. 2e4 bounds out even there: uniform
data does see those."""
import numpy as np
import pytest

import decode_rows as R

CASES = R.all_cases()
IDS = [R.case_id(c) for c in CASES]
VECTOR = (32, 64, 128)

# flaw -> (case name, kind, head sizes) on which it must show
TEETH = {
    "no_shift": [(name, kind, R.DHS) for name in ("plain-two", "gqa-8x1", "win-linear-1", "win-ring-8") for kind in ("lifted", "sunk")],
    "wave_local_max": [(name, "climbing", R.DHS) for name in ("plain-two", "plain-seam", "gqa-12x1", "win-linear-8", "win-ring-1")],
    "stale_head_max": [(name, "sunk", VECTOR) for name in ("gqa-4x2", "gqa-8x1", "gqa-12x1", "win-linear-8", "win-ring-8")],
    "combine_first_m": [(name, "climbing", R.DHS) for name in ("plain-four", "gqa-8x1", "gqa-12x1", "win-linear-8")],
    "combine_no_rescale": [(name, kind, R.DHS) for name in ("plain-two", "plain-four", "gqa-4x2", "win-linear-1", "win-ring-8")
                           for kind in ("climbing", "falling")],
    "combine_l_unscaled": [(name, kind, R.DHS) for name in ("plain-two", "plain-four", "gqa-4x2", "win-linear-1", "win-ring-8")
                           for kind in ("climbing", "falling")],
    "lo_off_by_one": [(name, "edge", R.DHS) for name in ("win-linear-1", "win-linear-8", "win-ring-1", "win-ring-8")],
}
TEETH_CASES = [(flaw, c, kind) for flaw, where in TEETH.items() for name, kind, dhs in where for c in CASES if c.name == name and c.dh in dhs]


def _ratio(case, ev, out, kind):
    """err / bound of `out` on the heads of `kind`; inf for a non-finite result."""
    m = R.kind_mask(case, kind)
    if not np.isfinite(out[m]).all():
        return float("inf")
    return float(np.abs(out[m] - ev["ref"][m]).max()) / R.bound(ev["ref"], (ev["ref32"], ev["ref32e"]), m, ev["vmax"])[0]


def test_the_chunk_is_the_librarys():
    from neuronika_amd import capi
    for dh in R.DHS + (48, 256):
        assert R.chunk(dh) == capi.attention_decode_chunk(dh), dh


def test_the_seeds_are_what_the_search_finds():
    assert len(R.SEEDS) == len(CASES) and R.search() == R.SEEDS


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_scores_are_exact_and_the_kinds_have_their_spread(case):
    d = R.build(case)
    for b in range(case.B):
        for t in range(case.T):
            lo, n = R.span(case, b, t)
            assert 0 <= lo < n
            for h in range(case.H):
                dots, _ = R.raw_scores(case, d, b, t, h, lo, n)
                assert np.array_equal(dots, dots.astype(np.float32).astype(np.float64)) and np.isfinite(dots).all()
    assert R.conditions(case) == []
    assert np.abs(d["q"]).max() <= 16 and np.abs(d["kl"]).max() <= 16
    # small: at most four chunks per problem, 24 problems per row of the step, nothing beyond 3C + 7 keys
    C = R.chunk(case.dh)
    assert all(len(R.chunks_of(case, *R.span(case, b, t))) <= 4 for b in range(case.B) for t in range(case.T))
    assert case.B * case.H <= 24 and max(case.start) + case.T <= 3 * C + 7


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_correct_replay_is_inside_the_bound(case):
    ev = R.evaluate(case)
    assert np.isfinite(ev["replay"]).all() and np.isfinite(ev["ref32"]).all() and np.isfinite(ev["ref32e"]).all()
    for kind, r in ev["ratios"].items():
        assert r <= 0.6, (kind, r)


@pytest.mark.parametrize("flaw,case,kind", TEETH_CASES, ids=["%s-%s-%s" % (f, R.case_id(c), k) for f, c, k in TEETH_CASES])
def test_a_flawed_replay_is_far_outside(flaw, case, kind):
    ev = R.evaluate(case)
    assert not _ratio(case, ev, R.replay_case(case, ev["d"], (flaw,)), kind) <= 100.0


def test_every_flaw_has_teeth_at_every_head_size_it_applies_to():
    for flaw in R.FLAWS:
        sizes = {c.dh for f, c, _ in TEETH_CASES if f == flaw}
        assert sizes == set(VECTOR if flaw == "stale_head_max" else R.DHS), flaw     # (the generic kernels take one head per block)


def _all_plain(case):
    return case._replace(kinds=tuple(("plain",) * case.H for _ in range(case.B)))


CONTROL = [c for c in CASES if c.name in ("plain-four", "gqa-8x1", "gqa-12x1", "win-linear-8", "win-ring-1")]


@pytest.mark.parametrize("case", CONTROL, ids=[R.case_id(c) for c in CONTROL])
def test_on_plain_rows_a_wrong_shift_is_invisible(case):
    """Why the uniform inputs of the other decode tests were blind: the same geometry with every head `plain`."""
    plain = _all_plain(case)
    ev = R.evaluate(plain, R.seed_of(case))
    assert ev["ratios"]["plain"] <= 0.6
    for flaw in R.SHIFT_FLAWS:
        assert _ratio(plain, ev, R.replay_case(plain, ev["d"], (flaw,)), "plain") <= 1.0, flaw
    for flaw in ("wave_local_max", "combine_no_rescale", "combine_l_unscaled"):      # not a shift: partials under different shifts are mixed
        assert not _ratio(plain, ev, R.replay_case(plain, ev["d"], (flaw,)), "plain") <= 100.0, flaw


def test_off_grid_scores_are_not_exact():
    """The control of the construction: the same rows off the grid lose the exactness the device test relies on."""
    case = CASES[0]
    d = dict(R.build(case))
    d["q"] = d["q"] + np.float32(0.01)
    dots, _ = R.raw_scores(case, d, 0, 0, 0, *R.span(case, 0, 0))
    assert not np.array_equal(dots, dots.astype(np.float32).astype(np.float64))

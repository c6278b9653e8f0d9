"""The score rows of tests/attention_rows.py, checked without a GPU: that their raw scores are exact in f32, that a replay of the
kernel's tile recurrence REACHES the rescale branch on the kinds meant to (and stays out of it on the others), that a correct
recurrence satisfies the parity policy tests/test_gpu_attention_rows.py applies to the device, and that a wrong one does not.

Measured with the replay (worst over geometries, full and causal; err / bound against the f64 oracle):
  out       plain 0.14  climbing 0.28  falling 0.68  mixed 0.23  under 0.12  peaked 0.67  shifted 0.49
  flawed    "no_rescale" >= 7.9e5 x and "no_l_rescale" >= 4.1e5 x the bound on climbing, mixed and peaked
  "row_local_any" changes the stored shift of the carried rows and leaves `out` inside the bound: softmax is invariant to the shift,
  so the wave-uniform coupling shows in the statistics alone (asserted on the device by test_a_row_does_not_depend_on_its_wave)."""
import functools

import numpy as np
import pytest

import attention_rows as R

CASES = [(kind, geometry, causal) for kind in R.KINDS for geometry in R.GEOMETRIES for causal in (False, True)]
IDS = ["%s-%s-%s" % (kind, "x".join(map(str, geometry)), "causal" if causal else "full") for kind, geometry, causal in CASES]


@functools.lru_cache(maxsize=None)
def case(kind, geometry, causal):
    """Inputs, both oracles (dropout inactive), the correct replay and its tile-0 shifts: computed once, shared, read-only."""
    B, S, H, dh = geometry
    q, k, v, g = R.rows(kind, B, S, H, dh)
    ref, ref32 = R.oracle(q, k, v, g, B, H, 0.0, np.ones((B * H, S, S), np.float32), causal)
    out, stats, moved = R.replay_forward(q, k, v, B, H, dh, causal)
    vis = R.visible(S, causal)
    sc2 = R.log2_scores(ref["scores"], dh, vis)
    for t in (out, stats, sc2, *ref.values(), *ref32.values()):
        t.setflags(write=False)
    return dict(q=q, k=k, v=v, g=g, ref=ref, ref32=ref32, out=out, stats=stats, moved=moved, vis=vis, sc2=sc2,
                bound=R.bound(ref["out"], ref32["out"], R.terms(ref, q, k, v, g, 0.0)["out"]))


@pytest.mark.parametrize("kind,geometry,causal", CASES, ids=IDS)
def test_scores_are_exact_and_the_f32_oracle_is_sane(kind, geometry, causal):
    c = case(kind, geometry, causal)
    assert np.array_equal(c["ref32"]["scores"], c["ref"]["scores"]) and c["ref32"]["scores"].dtype == np.float32
    for name, t in c["ref32"].items():
        assert np.isfinite(t).all(), name
    np.testing.assert_allclose(c["ref32"]["probs"].sum(2), 1.0, rtol=0, atol=1e-5)
    assert not c["ref32"]["probs"][:, ~c["vis"]].any()
    assert c["ref"]["probs"][:, c["vis"]].min() >= 1e-30      # nothing an f32 kernel could flush: every `dropped` entry is comparable


@pytest.mark.parametrize("kind,geometry,causal", CASES, ids=IDS)
def test_the_replay_reaches_the_branch_where_it_should(kind, geometry, causal):
    c = case(kind, geometry, causal)
    B, S, H, dh = geometry
    m2 = c["stats"][..., 0].astype(np.float64)
    tile0 = c["sc2"][:, :, :32].max(2)
    must = R.must_move(c["sc2"])
    assert (m2 >= c["sc2"].max(2) - 6.0 - 1e-4).all() and (m2 <= c["sc2"].max(2) + 1e-4).all()
    assert (m2[must] > tile0[must]).all()
    if kind in R.MOVING:
        assert c["moved"] > 0 and must.any()
    if kind in R.STILL:
        assert c["moved"] == 0 and not must.any()
        np.testing.assert_allclose(m2, tile0, rtol=0, atol=1e-4)
    if not causal:      # (causal: a row sees the keys up to its own only)
        assert kind != "climbing" or must.all()
        assert kind != "mixed" or must[:, 1::2].all()
    if kind == "under":     # pinned: the lifted tile stays under the threshold, and not by much
        assert 4.5 <= (c["sc2"].max(2) - m2).max() <= 6.0
    if kind == "mixed":     # an even row that did not have to move (its own lift is below the threshold) and was moved
        carried = ~must[:, 0::2] & (m2[:, 0::2] > tile0[:, 0::2] + 1e-3)
        assert carried.any()


@pytest.mark.parametrize("kind,geometry,causal", CASES, ids=IDS)
def test_a_correct_recurrence_is_inside_the_policy(kind, geometry, causal):
    c = case(kind, geometry, causal)
    assert np.isfinite(c["out"]).all() and np.isfinite(c["stats"]).all()
    assert np.abs(c["out"] - c["ref"]["out"]).max() <= c["bound"]
    # the stored pair reproduces the softmax, as the device test asserts
    soft = np.where(c["vis"], c["ref"]["probs"], 0.0)
    m2, inv = c["stats"][..., 0].astype(np.float64), c["stats"][..., 1].astype(np.float64)
    np.testing.assert_allclose(np.exp2(c["sc2"] - m2[..., None]) * inv[..., None], soft, rtol=2e-5, atol=1e-9)


@pytest.mark.parametrize("kind,geometry,causal", [t for t in CASES if t[0] in R.MOVING], ids=[i for i, t in zip(IDS, CASES) if t[0] in R.MOVING])
@pytest.mark.parametrize("flaw", ["no_rescale", "no_l_rescale"])
def test_a_recurrence_that_does_not_rescale_is_far_outside(kind, geometry, causal, flaw):
    c = case(kind, geometry, causal)
    B, S, H, dh = geometry
    out, _, _ = R.replay_forward(c["q"], c["k"], c["v"], B, H, dh, causal, flaws=(flaw,))
    with np.errstate(invalid="ignore"):
        err = np.abs(out - c["ref"]["out"]).max()
    assert not err <= 10 * c["bound"]       # (a NaN is a failure too)


@pytest.mark.parametrize("geometry,causal", [(g_, c_) for g_ in R.GEOMETRIES for c_ in (False, True)])
def test_a_row_local_trigger_shows_in_the_statistics_only(geometry, causal):
    """"row_local_any" on `mixed`: the even rows are no longer carried - their final shift changes - and `out` stays inside the bound,
    because softmax is invariant to the shift.  `out` cannot catch this flaw; the stored shift can."""
    c = case("mixed", geometry, causal)
    B, S, H, dh = geometry
    out, stats, _ = R.replay_forward(c["q"], c["k"], c["v"], B, H, dh, causal, flaws=("row_local_any",))
    even = (slice(None), slice(0, None, 2))
    assert (stats[..., 0][even] <= c["stats"][..., 0][even]).all() and (stats[..., 0][even] < c["stats"][..., 0][even]).any()
    assert np.abs(out - c["ref"]["out"]).max() <= c["bound"]


def _backward_ratios(c, geometry, causal, out, stats, cancelling):
    """err / bound of the replayed backward per tensor; `cancelling`: dS, dQ, dK measured by attention_rows.cancelling_terms (the
    device test's yardstick) or, False, by the size of the result as in tests/test_gpu_attention.py."""
    B, S, H, dh = geometry
    q, k, v, g, ref, ref32, vis = (c[n] for n in ("q", "k", "v", "g", "ref", "ref32", "vis"))
    terms = R.terms(ref, q, k, v, g, 0.0)
    if cancelling:
        terms.update(R.cancelling_terms(ref, q, k, v, g, B, H, 0.0, None))
    got = R.replay_backward(q, k, v, g, out, stats, B, H, dh, causal)
    ratios = {}
    for name in ("d_scores", "dropped", "dq", "dk", "dv"):
        pick = (lambda t: t[:, vis]) if name in ("d_scores", "dropped") else (lambda t: t)
        with np.errstate(invalid="ignore"):
            ratios[name] = np.abs(pick(got[name]) - pick(ref[name])).max() / R.bound(pick(ref[name]), pick(ref32[name]), terms.get(name, 0.0))
    return ratios


@pytest.mark.parametrize("kind,geometry,causal", CASES, ids=IDS)
def test_the_backward_recomputation_is_inside_the_policy(kind, geometry, causal):
    """The backward's arithmetic - probabilities from the stored (shift, 1 / sum) pair, the softmax dot as dO . O - on the correct
    forward's output and statistics.  Measured by the result's size, dS reads up to 1.86 x the bound on `peaked` (full attention: every
    row's gradient has cancelled to 1e-3 .. 1e-1 of its terms) and 1.08 x on one case of `falling`, as the device does; measured by
    the terms that cancel (attention_rows.cancelling_terms) the worst is 0.15 (dS and dQ, `peaked`)."""
    c = case(kind, geometry, causal)
    for name, r in _backward_ratios(c, geometry, causal, c["out"], c["stats"], True).items():
        assert r <= 1.0, (name, r)


@pytest.mark.parametrize("kind,geometry,causal", [t for t in CASES if t[0] in R.MOVING], ids=[i for i, t in zip(IDS, CASES) if t[0] in R.MOVING])
def test_a_backward_that_reads_a_stale_sum_is_far_outside(kind, geometry, causal):
    """The yardstick of the cancelling terms keeps its teeth: statistics from a forward that did not rescale its running sum put dS, dQ
    and dK at least 10 bounds away."""
    c = case(kind, geometry, causal)
    B, S, H, dh = geometry
    _, stats, _ = R.replay_forward(c["q"], c["k"], c["v"], B, H, dh, causal, flaws=("no_l_rescale",))
    ratios = _backward_ratios(c, geometry, causal, c["out"], stats, True)
    for name in ("d_scores", "dq", "dk"):
        assert not ratios[name] <= 10.0, (name, ratios[name])


def test_off_grid_scores_are_not_exact():
    """The control of the construction: the same rows off the grid lose the exactness the device test relies on."""
    B, S, H, dh = 1, 64, 1, 64
    q, k, v, g = R.rows("climbing", B, S, H, dh)
    q = q + np.float32(0.01)
    ref, ref32 = R.oracle(q, k, v, g, B, H, 0.0, np.ones((B * H, S, S), np.float32), False)
    assert not np.array_equal(ref32["scores"], ref["scores"])

"""The score rows of tests/attention_band_rows.py, checked without a GPU - tests/test_oracle_attention_rows.py for the sliding-window
and packed-sequence walks: that the raw scores are exact in f32 and no allowed probability is below 1e-30 (so the device test leaves
nothing out), that a replay of the kernels' walk REACHES the rescale branch after a row's first finite tile on the kinds meant to, in
left-edge tiles, whole tiles and the diagonal square alike, that a correct recurrence satisfies the parity policy
tests/test_gpu_attention_band_rows.py applies to the device, and that a wrong one does not.

What the moving left edge changes against the causal file: a wave's rows START in different tiles, and a start is an unconditional
move for the whole wave - so a `plain` or `falling` row under a band does not end at the maximum of its first visible tile (it reads several log2
units above it) but at `attention_band_rows.settled_max`, the maximum over the tiles in which a row of its wave starts;
that is what the still kinds are held to, here and on the device, to 1e-4.  "Moves" below are (row, tile) pairs in which a row passes
the test BY ITSELF after its first finite tile: there alpha < 2^-6 multiplies a non-zero sum and accumulator.

Measured with the replay (worst over the geometries; err / bound against the f64 oracle, bound = max(2 err_cpu32, 1e-6 yardstick),
dS, dQ and dK by attention_rows.cancelling_terms):
  band  out   plain 0.13  climbing 0.28  falling 0.59  mixed 0.23  shifted 0.45  peaked_in 0.65
        Pd    plain 0.06  climbing 0.15  falling 0.25  mixed 0.11  shifted 0.29  peaked_in 0.44
        dS    plain 0.03  climbing 0.07  falling 0.10  mixed 0.06  shifted 0.08  peaked_in 0.09
        dQ    plain 0.03  climbing 0.05  falling 0.09  mixed 0.04  shifted 0.09  peaked_in 0.09
        dK    plain 0.02  climbing 0.02  falling 0.01  mixed 0.02  shifted 0.01  peaked_in 0.03
        dV    plain 0.19  climbing 0.21  falling 0.06  mixed 0.33  shifted 0.07  peaked_in 0.28
  seg   out   plain 0.15  climbing 0.28  falling 0.50  mixed 0.23  shifted 0.53  peaked_in 0.61  handover 0.40
        Pd    plain 0.07  climbing 0.15  falling 0.26  mixed 0.11  shifted 0.37  peaked_in 0.44  handover 0.28
        dS    plain 0.06  climbing 0.07  falling 0.07  mixed 0.06  shifted 0.10  peaked_in 0.11  handover 0.08
        dQ    plain 0.05  climbing 0.05  falling 0.08  mixed 0.05  shifted 0.10  peaked_in 0.11  handover 0.07
        dK    plain 0.03  climbing 0.02  falling 0.01  mixed 0.03  shifted 0.01  peaked_in 0.03  handover 0.01
        dV    plain 0.18  climbing 0.21  falling 0.07  mixed 0.29  shifted 0.07  peaked_in 0.22  handover 0.09
  flawed (the SMALLEST ratio over the cases that move)
        "no_rescale" >= 6.4e5, "no_l_rescale" >= 1.7e5 bounds in `out` on climbing, mixed, peaked_in and handover;
        statistics of a "no_l_rescale" forward: dS >= 1.6e3, dQ >= 7.2e3, dK >= 103 bounds (`peaked_in` the lowest, climbing >= 8.7e3)
  moves by (family, class), summed over the geometries
        band  left-edge: climbing 876 mixed 426 peaked_in 255    whole: 302 / 150 / 72     diagonal: 2956 / 1477 / 863
        seg   left-edge: climbing 282 mixed 140 peaked_in 50 handover 274   whole: 1254 / 624 / 315 / 274   diagonal: 3071 / 1546 / 879 / 1301
        `plain` and `falling`: 0 in every class at every geometry"""
import functools

import numpy as np
import pytest

import attention_rows as R
import attention_band_rows as BR

CASES = [(kind, geometry) for geometry in BR.BAND for kind in BR.BAND_KINDS] + [(kind, geometry) for geometry in BR.SEG for kind in BR.SEG_KINDS]
IDS = ["%s-%s" % (kind, BR.gid(geometry)) for kind, geometry in CASES]


def moves_expected(kind, geometry):
    """A moving kind moves wherever it exists: `peaked_in` needs a row with 64 visible keys (W = 40 and span = 48 have none)."""
    B, S, H, dh, lo, span = BR.edges(geometry)
    return kind in BR.MOVING and (kind != "peaked_in" or (np.arange(S) - BR.SO.lo_eff(lo, span) + 1 >= 64).any())


@functools.lru_cache(maxsize=2)
def build(kind, geometry):
    """Inputs, both oracles (dropout inactive), the correct replay: computed once per case, read-only."""
    B, S, H, dh, lo, span = BR.edges(geometry)
    q, k, v, g = BR.rows(kind, geometry)
    ref, ref32 = BR.oracle(q, k, v, g, B, H, 0.0, np.ones((B * H, S, S), np.float32), lo, span)
    out, stats, moves = BR.replay_forward(q, k, v, B, H, dh, lo, span)
    allowed, le = BR.allowed_rows(lo, span, H), BR.lo_eff_rows(lo, span, H)
    sc2 = R.log2_scores(ref["scores"], dh, allowed)
    for t in (out, stats, sc2, *ref.values(), *ref32.values()):
        t.setflags(write=False)
    return dict(kind=kind, geometry=geometry, q=q, k=k, v=v, g=g, ref=ref, ref32=ref32, out=out, stats=stats, moves=moves,
                allowed=allowed, le=le, sc2=sc2, bound=R.bound(ref["out"], ref32["out"], R.terms(ref, q, k, v, g, 0.0)["out"]))


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def case(request):
    """Module-scoped, so that pytest runs every test of one case before the next case is built."""
    return build(*request.param)


@pytest.fixture(scope="module", params=[t for t in CASES if moves_expected(*t)], ids=[i for i, t in zip(IDS, CASES) if moves_expected(*t)])
def moving_case(request):
    return build(*request.param)


@pytest.fixture(scope="module", params=[t for t in CASES if t[0] == "mixed"], ids=[i for i, t in zip(IDS, CASES) if t[0] == "mixed"])
def mixed_case(request):
    return build(*request.param)


def test_scores_are_exact_and_no_probability_can_be_flushed(case):
    c = case
    assert np.array_equal(c["ref32"]["scores"], c["ref"]["scores"]) and c["ref32"]["scores"].dtype == np.float32
    for name, t in c["ref32"].items():
        assert np.isfinite(t).all(), name
    np.testing.assert_allclose(c["ref32"]["probs"].sum(2), 1.0, rtol=0, atol=1e-5)
    assert not c["ref32"]["probs"][~c["allowed"]].any()
    # the share of probabilities the device's `dropped == 0` comparison would have to leave out is a CONDITION: none
    assert c["ref"]["probs"][c["allowed"]].min() >= 1e-30


def test_the_replay_reaches_the_branch_where_it_should(case):
    c, kind = case, case["kind"]
    m2 = c["stats"][..., 0].astype(np.float64)
    first = BR.first_tile_max(c["sc2"], c["le"])
    must = BR.must_move(c["sc2"], c["le"])
    own = sum(c["moves"][name] for name in BR.CLASSES)
    assert (m2 >= c["sc2"].max(2) - 6.0 - 1e-4).all() and (m2 <= c["sc2"].max(2) + 1e-4).all()
    assert (m2[must] > first[must]).all()
    if moves_expected(kind, c["geometry"]):
        assert own > 0 and must.any()
    if kind in BR.STILL:
        assert own == 0 and not must.any()
        assert all(c["moves"][name] == 0 for name in BR.CLASSES)
        np.testing.assert_allclose(m2, BR.settled_max(c["sc2"], c["le"]), rtol=0, atol=1e-4)
    if kind == "climbing":     # every row that sees a whole tile (8 nats) past its first visible tile
        assert must[np.arange(m2.shape[1])[None, :] - c["le"] >= 64].all()
    if kind == "mixed":        # even rows that did not have to move and were moved by an odd neighbour that did
        assert c["moves"]["carried"] > 0
        settled = BR.settled_max(c["sc2"], c["le"])
        assert (~must[:, 0::2] & (m2[:, 0::2] > settled[:, 0::2] + 1e-3)).any()


@pytest.mark.parametrize("name", BR.CLASSES)
@pytest.mark.parametrize("family", ["band", "seg"])
def test_the_moves_cover_every_tile_class(family, name):
    """Both textual copies of each tile body rescale a non-zero sum: the EDGE copy in left-edge tiles and in the diagonal square, the
    whole-tile copy in [left_end, 4 qb) - for the band walk and for the seg walk, on `climbing` alone and over every moving kind."""
    geometries = BR.BAND if family == "band" else BR.SEG
    kinds = [k for k in (BR.BAND_KINDS if family == "band" else BR.SEG_KINDS) if k in BR.MOVING]
    count = {kind: sum(build(kind, geometry)["moves"][name] for geometry in geometries) for kind in kinds}
    print("moves", family, name, count)
    assert count["climbing"] > 0 and count["mixed"] > 0 and count["peaked_in"] > 0
    assert family == "band" or count["handover"] > 0


def test_a_correct_recurrence_is_inside_the_policy(case):
    c = case
    assert np.isfinite(c["out"]).all() and np.isfinite(c["stats"]).all()      # rows that sat at -1e30 through all--inf tiles included
    ratio = np.abs(c["out"] - c["ref"]["out"]).max() / c["bound"]
    print("RATIO out %s %s %.3f" % (c["kind"], BR.gid(c["geometry"]), ratio))
    assert ratio <= 1.0
    soft = np.where(c["allowed"], c["ref"]["probs"], 0.0)
    m2, inv = c["stats"][..., 0].astype(np.float64), c["stats"][..., 1].astype(np.float64)
    np.testing.assert_allclose(np.exp2(c["sc2"] - m2[..., None]) * inv[..., None], soft, rtol=2e-5, atol=1e-9)


@pytest.mark.parametrize("flaw", ["no_rescale", "no_l_rescale"])
def test_a_recurrence_that_does_not_rescale_is_far_outside(moving_case, flaw):
    c = moving_case
    B, S, H, dh, lo, span = BR.edges(c["geometry"])
    out, _, _ = BR.replay_forward(c["q"], c["k"], c["v"], B, H, dh, lo, span, flaws=(flaw,))
    with np.errstate(invalid="ignore"):
        ratio = np.abs(out - c["ref"]["out"]).max() / c["bound"]
    print("RATIO %s %s %s %.3g" % (flaw, c["kind"], BR.gid(c["geometry"]), ratio))
    assert not ratio <= 10.0       # (a NaN is a failure too)


def test_a_row_local_trigger_shows_in_the_statistics_only(mixed_case):
    """"row_local_any" on `mixed`: the even rows are no longer carried - their final shift drops - and `out` stays inside the bound."""
    c = mixed_case
    B, S, H, dh, lo, span = BR.edges(c["geometry"])
    out, stats, _ = BR.replay_forward(c["q"], c["k"], c["v"], B, H, dh, lo, span, flaws=("row_local_any",))
    even = (slice(None), slice(0, None, 2))
    assert (stats[..., 0][even] <= c["stats"][..., 0][even]).all() and (stats[..., 0][even] < c["stats"][..., 0][even]).any()
    assert np.abs(out - c["ref"]["out"]).max() <= c["bound"]


def _backward_ratios(c, out, stats):
    """err / bound of the replayed backward per tensor; dS, dQ and dK by attention_rows.cancelling_terms, the device test's yardstick."""
    B, S, H, dh, lo, span = BR.edges(c["geometry"])
    q, k, v, g, ref, ref32, allowed = (c[n] for n in ("q", "k", "v", "g", "ref", "ref32", "allowed"))
    terms = R.terms(ref, q, k, v, g, 0.0)
    terms.update(R.cancelling_terms(ref, q, k, v, g, B, H, 0.0, None))
    got = BR.replay_backward(q, k, v, g, out, stats, B, H, dh, allowed)
    ratios = {}
    for name in ("d_scores", "dropped", "dq", "dk", "dv"):
        pick = (lambda t: t[allowed]) if name in ("d_scores", "dropped") else (lambda t: t)
        with np.errstate(invalid="ignore"):
            ratios[name] = np.abs(pick(got[name]) - pick(ref[name])).max() / R.bound(pick(ref[name]), pick(ref32[name]), terms.get(name, 0.0))
    return ratios


def test_the_backward_recomputation_is_inside_the_policy(case):
    """Probabilities from the stored (shift, 1 / sum) pair - a shift up to 6 below the row maximum - and the softmax dot as dO . O."""
    c = case
    for name, r in _backward_ratios(c, c["out"], c["stats"]).items():
        print("RATIO %s %s %s %.3f" % (name, c["kind"], BR.gid(c["geometry"]), r))
        assert r <= 1.0, (name, r)


def test_a_backward_that_reads_a_stale_sum_is_far_outside(moving_case):
    """Statistics from a forward that did not rescale its running sum put dS, dQ and dK more than 10 bounds away."""
    c = moving_case
    B, S, H, dh, lo, span = BR.edges(c["geometry"])
    _, stats, _ = BR.replay_forward(c["q"], c["k"], c["v"], B, H, dh, lo, span, flaws=("no_l_rescale",))
    ratios = _backward_ratios(c, c["out"], stats)
    for name in ("d_scores", "dq", "dk"):
        print("RATIO stale_%s %s %s %.3g" % (name, c["kind"], BR.gid(c["geometry"]), ratios[name]))
        assert not ratios[name] <= 10.0, (name, ratios[name])


# ---- a later document's rows in a wave that straddles a boundary ------------------------------------------------------------

STRADDLING = [g_ for g_ in BR.SEG if BR.later_rows(*BR.edges(g_)[4:]).any()]


@pytest.mark.parametrize("geometry", STRADDLING, ids=BR.gid)
def test_later_rows_ask_in_the_diagonal_tile_whatever_their_neighbours_hold(geometry):
    """nk_attention_band.h: "a row of a LATER document of the same wave has all its keys in the wave's diagonal tile, where it asks
    unconditionally (its first finite tile), so what it holds changes no decision".  On `handover`, in both orientations - the earlier
    rows of the wave tens of nats above, and tens of nats below - the replayed shift of every such row is f32(row maximum * c1), the
    value of one unconditional move from -1e30; and with a later document held fixed (`climbing`) while every other document switches
    orientation, its rows' shifts and sums do not change by a bit."""
    B, S, H, dh, lo, span = BR.edges(geometry)
    later = np.repeat(BR.later_rows(lo, span), H, axis=0)                      # (B*H, S)
    allowed = BR.allowed_rows(lo, span, H)
    wave0 = (np.arange(S) // 32 * 32)[None, :, None]
    assert (~allowed | (np.arange(S)[None, None, :] >= wave0))[later].all()    # all their keys are in the diagonal tile
    for orient in (0, 1):
        q, k, v, g = BR.rows("handover", geometry, orient)
        _, stats, _ = BR.replay_forward(q, k, v, B, H, dh, lo, span)
        qh, kh = (BR.O._heads_split(t, B, H) for t in (q, k))
        rowmax = np.where(allowed, np.matmul(qh, kh.transpose(0, 2, 1)), -np.inf).max(2).astype(np.float32)
        assert np.array_equal(stats[..., 0][later], (rowmax * R._c1(dh)).astype(np.float32)[later]), orient
    doc = BR.documents(lo)
    for b in range(B):
        for idx in range(1, doc[b].max() + 1):
            mine = np.repeat((np.arange(B)[:, None] == b) & (doc == idx), H, axis=0) & later
            if not mine.any():
                continue
            a, z = (BR.replay_forward(*BR.kept_document(geometry, (b, idx), variant)[:3], B, H, dh, lo, span) for variant in (0, 1))
            assert np.array_equal(a[1][mine], z[1][mine]), (b, idx)
            kept_rows = BR.kept_document(geometry, (b, idx), 0)[4]
            assert np.array_equal(a[0][kept_rows], z[0][kept_rows]), (b, idx)


def test_handover_holds_both_orientations():
    """Over the layouts, a straddling wave meets a `climbing` document before a `low` one and a `low` one before a `climbing` one."""
    seen = set()
    for geometry in STRADDLING:
        B, S, H, dh, lo, span = BR.edges(geometry)
        doc, later = BR.documents(lo), BR.later_rows(lo, span)
        for b, r in zip(*np.nonzero(later & (np.arange(S)[None, :] % 32 != 0) & (doc != np.roll(doc, 1, axis=1)))):
            seen.add((int(doc[b, r]) + int(b)) % 2)       # parity of the later document: 0 = climbing after low, 1 = low after climbing
    assert seen == {0, 1}


def test_the_walk_without_a_left_edge_is_the_causal_replay():
    """The control of the walk: lo = 0 and span = S give attention_rows.replay_forward(causal=True) bit for bit."""
    B, S, H, dh = 1, 160, 2, 64
    q, k, v, g = R.rows("climbing", B, S, H, dh)
    want = R.replay_forward(q, k, v, B, H, dh, True)
    got = BR.replay_forward(q, k, v, B, H, dh, np.zeros((B, S), np.int32), S)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert sum(got[2][name] for name in BR.CLASSES) > 0 and got[2]["left"] == 0


def test_a_band_row_is_carried_by_its_wave():
    """The replay's twin of the device test of that name: the even rows of `mixed`, once among climbing and once among `plain` odd rows."""
    geometry = BR.BAND[0]
    B, S, H, dh, lo, W = BR.edges(geometry)
    c = build("mixed", geometry)
    calm = np.array(c["q"])
    calm[1::2] = BR.rows("plain", geometry)[0][1::2]
    out, stats, moves = BR.replay_forward(calm, c["k"], c["v"], B, H, dh, lo, W)
    even = slice(0, None, 2)
    assert all(moves[name] == 0 for name in BR.CLASSES)
    ma, mb = c["stats"][:, even, 0], stats[:, even, 0]
    np.testing.assert_allclose(mb, BR.settled_max(c["sc2"], c["le"])[:, even], rtol=0, atol=1e-4)
    assert (ma >= mb).all() and (ma > mb + 1.0).any()
    bound = R.bound(c["ref"]["out"][even], c["ref32"]["out"][even], R.terms(c["ref"], c["q"], c["k"], c["v"], c["g"], 0.0)["out"])
    for t in (out, c["out"]):
        assert np.abs(t[even] - c["ref"]["out"][even]).max() <= bound

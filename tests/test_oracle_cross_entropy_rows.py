"""The logit rows of tests/cross_entropy_rows.py, checked without a GPU: that the restated walk and dispatch are the headers', that the
kinds have the spread they claim and the peaks the role they name, that a correct replay of the forward kernels' arithmetic and the
plain f32 two-pass reference are inside the oracle's bound (the reference inside half of it, the condition under which a kernel can
be held to the whole), and that every wrong shift (cross_entropy_rows.SHIFT_FLAWS) is invisible on the N(0, 3^2) logits of every
other cross-entropy test and non-finite or more than 100 bounds out here.

Measured (all 16 cases at the four leads, bounds per row from the row's live xmax): the two-pass reference's worst err / bound is
0.352 for lse (`climbing` at C = 1100; lifted 0.25, sunk 0.20, every other kind below 0.12) and 0.123 for dx (`climbing`, block
families); the correct replay's worst is the same 0.352: both are dominated by the one rounding of m + log s at |lse| up to 2016.
WORST32_LSE, WORST32_DX and WORST_REPLAY hold those figures, rounded up, and are asserted."""
import os
import re

import numpy as np
import pytest

import cross_entropy_oracle as X
import cross_entropy_rows as R
from test_gpu_cross_entropy import FAMILY_SHAPES, make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [R.case_id(c) for c in R.CASES]

# worst err / bound of the plain f32 two-pass reference and of the correct replay over every committed row, as measured here
WORST32_LSE, WORST32_DX, WORST_REPLAY = 0.36, 0.13, 0.36

# flaw -> the kinds on which it must show, in at least one committed call of every family that can have it
TEETH = {
    "max_skips_edge": ("peaked:head", "peaked:tail"),
    "group_max_of_three": ("peaked:slot3",),
    "partial_trip_no_online": ("climbing", "peaked:partial"),
    "edge_no_online": ("climbing", "peaked:edge_after_body", "peaked:head", "peaked:tail"),
    "wave_merge_first_lane_m": ("climbing", "peaked:last_wave", "peaked:last_quad", "masked_inf"),
    "block_merge_first_wave_m": ("climbing", "peaked:last_wave"),
    "fold_from_zero": ("sunk",),
    "no_shift": ("lifted", "sunk"),
    "no_rescale": ("climbing",),
}


def _src(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_walk_and_family_are_the_headers():
    h = _src("neuronika_amd", "csrc", "nk_cross_entropy.h")
    const = {k: int(v) for k, v in re.findall(r"constexpr int (CE_[A-Z0-9_]+) = (\d+);", h)}
    assert (const["CE_ROW_MAX"], const["CE_BLOCK_512"], const["CE_BLOCK_1024"], const["CE_EDGE_TAIL"]) == \
        (R.ROW_MAX, R.BLOCK_512, R.BLOCK_1024, R.EDGE_TAIL)
    fwd = h[h.index("int nk_cross_entropy_fwd("):]
    rows = [(int(c), int(v)) for c, v in re.findall(r"if \(C <= (\d+)\) CE_ROW\((\d+)\);", fwd)]
    assert rows + [(R.ROW_MAX, int(re.search(r"else CE_ROW\((\d+)\);", fwd).group(1)))] == list(R.ROW_V)
    assert re.findall(r"CE_BLOCK\((\d+)\);", fwd) == ["256", "512", "1024"]
    assert "if (C <= CE_BLOCK_512) CE_BLOCK(256);" in fwd and "else if (C <= CE_BLOCK_1024) CE_BLOCK(512);" in fwd
    assert "#pragma unroll\n        for (int u = 0; u < 4; ++u) r[u] = body[q + u * NT];" in h and "q + 3 * NT < w.nb; q += 4 * NT" in h
    doc = " ".join(_src("include", "neuronika_hip.h").split())
    assert "inner == 1: C <= %d one wave per row" % R.ROW_MAX in doc
    assert "(256 threads up to C = %d, 512 up to %d, 1024 beyond)" % (R.BLOCK_512, R.BLOCK_1024) in doc
    for C, want in ((1, "row1"), (256, "row1"), (257, "row2"), (512, "row2"), (513, "row4"), (1024, "row4"), (1025, "row8"), (2048, "row8"),
                    (2049, "block256"), (16384, "block256"), (16385, "block512"), (65536, "block512"), (65537, "block1024")):
        assert R.family(C, 1) == want and R.family(C, 3) == "generic" and R.family(C, 1, together=False) == "generic"
    for C in (1, 2, 3, 4, 5, 10, 255, 256, 4099):
        for off in range(4):
            head, nb, tail = R.walk(C, off)
            # by hand: scalars until the address is a multiple of four floats, whole quads, the rest
            want_head = next(k for k in range(5) if (off + k) % 4 == 0 or k == C)
            assert head == want_head and nb == (C - head) // 4 and tail == (C - head) % 4 and head + 4 * nb + tail == C


@pytest.mark.parametrize("fam,C", [("row1", 10), ("row2", 300), ("row8", 2048), ("block256", 2049), ("block256", 9001), ("block1024", 70001)])
def test_ownership_is_the_kernels_loop(fam, C):
    """`ownership` against the loops of the kernels written out thread by thread"""
    NT = R.threads_of(fam)
    for off in range(4):
        head, nb, tail = R.walk(C, off)
        own = R.ownership(fam, C, off)
        seen = np.zeros(C, int)
        for tid in range(NT):
            q, trip = tid, 0
            if fam.startswith("block"):
                while q + 3 * NT < nb:
                    for u in range(4):
                        cols = head + 4 * (q + u * NT) + np.arange(4)
                        assert (own.thread[cols] == tid).all() and (own.trip[cols] == trip).all() and (own.u[cols] == u).all() and own.full[cols].all()
                        seen[cols] += 1
                    q, trip = q + 4 * NT, trip + 1
                assert trip == R.full_trips(NT, nb, tid)
            for u in range(4 if fam.startswith("block") else int(fam[3:])):
                if q + u * NT < nb:
                    cols = head + 4 * (q + u * NT) + np.arange(4)
                    assert (own.thread[cols] == tid).all() and (own.slot[cols] == 4 * trip + u).all() and not own.full[cols].any()
                    seen[cols] += 1
            ec = tid if tid < head else head + 4 * nb + tid - R.EDGE_TAIL if 0 <= tid - R.EDGE_TAIL < tail else -1      # ce_edge_col
            if ec >= 0:
                assert own.thread[ec] == tid and own.edge[ec] == (1 if tid < head else 2) and own.slot[ec] == -1
                seen[ec] += 1
        assert (seen == 1).all()


def _check_role(fam, C, off, role, col):
    own = R.ownership(fam, C, off)
    NT = R.threads_of(fam)
    head, nb, tail = R.walk(C, off)
    if role == "head":
        assert own.edge[col] == 1
    elif role == "tail":
        assert own.edge[col] == 2
    elif role == "last_quad":
        assert own.edge[col] == 0 and own.slot[col] == own.slot.max() and (col - head) // 4 == nb - 1
        assert nb % 64 == 0 or own.thread[col] == (nb - 1) % 64            # the lanes beyond it hold nothing in that v[i]
    elif role == "slot3":
        assert own.full[col] and own.u[col] == 3
    elif role == "partial":
        assert own.edge[col] == 0 and not own.full[col] and own.trip[col] == R.full_trips(NT, nb, own.thread[col])
    elif role == "edge_after_body":
        assert own.edge[col] > 0 and own.thread[col] in (0, R.EDGE_TAIL) and nb > own.thread[col]     # the thread has body quads too
    elif role == "last_wave":
        assert own.edge[col] == 0 and own.thread[col] >= NT - 64
    elif role == "wave0":
        assert own.edge[col] == 0 and own.thread[col] < 64
    else:
        raise AssertionError(role)


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_every_kind_has_the_spread_and_every_peak_the_role_it_claims(case):
    C = case.C
    for lead in R.LEADS if case.inner == 1 else (4,):
        d = R.build(case, lead)
        fam, x = d["fam"], d["x"]
        assert x.shape[0] <= 16 and x.shape[0] % case.inner == 0
        for p, kind in enumerate(d["kinds"]):
            xr, live, off, where = x[p].astype(np.float64), d["live"][p], d["offs"][p], (R.case_id(case), lead, p, kind)
            tA, tB = int(d["tA"][p]), int(d["tB"][p])
            assert live[tA] and live[tB] and xr[tA] == xr[live].max() and xr[tB] == xr[live].min(), where
            if case.inner == 1:
                assert off == (lead - 4 + p * C) % 4, where
            if kind in (None, "plain"):
                assert np.abs(xr).max() <= R.NOISE, where
            elif kind in R.SPREAD_KINDS:
                lv, sign = R.level(fam, C, off), 1.0 if kind == "climbing" else -1.0
                assert np.abs(xr - sign * R.GAP * lv).max() <= R.NOISE and np.abs(xr).max() <= 8192, where
                assert lv.max() >= 1 and set(np.unique(lv)) == set(range(lv.max() + 1)), where
                # two columns of different levels: exp of their difference overflows one way and is nothing the other way
                assert R.GAP - 2 * R.NOISE > R.LN_F32_MAX and np.exp(-(R.GAP - 2 * R.NOISE)) < 2.0 ** -138, where
                assert xr[tA] - xr[tB] >= R.GAP, where
                if fam != "generic":
                    own = R.ownership(fam, C, off)
                    body = own.edge == 0
                    assert np.array_equal(lv[body], own.slot[body]) and (lv[~body] == own.slot.max() + 1).all(), where
            elif kind in ("lifted", "sunk"):
                assert (xr >= 8 * R.GAP - R.NOISE).all() if kind == "lifted" else (xr <= -8 * R.GAP + R.NOISE).all(), where
                assert 8 * R.GAP - R.NOISE > -R.LN_F32_DENORM_MIN, where
            elif kind.startswith("peaked:"):
                col = d["cols"][p]
                assert col == tA and (np.delete(xr, col) <= xr[col] - R.GAP).all() and np.abs(np.delete(xr, col)).max() <= R.NOISE, where
                _check_role(fam, C, off, kind[7:], col)
            else:
                assert np.array_equal(xr[~live], np.full((~live).sum(), np.float32(R.MASKED[kind]), np.float64)), where
                assert np.abs(xr[live]).max() <= R.NOISE, where
                if C >= 255:
                    assert 0.8 <= (~live).mean() <= 0.97, (where, (~live).mean())
                if fam != "generic":
                    own = R.ownership(fam, C, off)
                    head, nb, tail = R.walk(C, off)
                    assert live[own.edge > 0].all(), where
                    quads = live[head:head + 4 * nb].reshape(nb, 4)
                    assert (quads.all(1) | ~quads.any(1)).all(), where                           # whole quads
                if fam.startswith("block"):
                    NT = R.threads_of(fam)
                    assert (live & (own.edge == 0) & (own.thread >= NT - 64)).any(), where         # a live quad in the last wave
                    dead = np.array([not live[(own.thread == t) & (own.edge == 0)].any() for t in range(NT)])
                    assert dead.any(), where                                                    # lanes whose m stays f32::MIN
                    if own.full.any():                                                          # full trips whose group maximum is the mask
                        trips = {(t, j) for t, j in zip(own.thread[own.full], own.trip[own.full])}
                        assert any(not live[(own.thread == t) & (own.trip == j) & own.full].any() for t, j in list(trips)[:4096]), where
        xe = d["extra_row"]
        assert np.array_equal(xe, x[d["kinds"].index("masked_inf")]) and xe[int(d["extra_target"])] == -np.inf


def test_every_kind_and_role_is_present_in_every_family_it_is_meaningful_for():
    seen = {}
    for case in R.CASES:
        for lead in R.LEADS:
            d = R.build(case, lead)
            seen.setdefault(d["fam"], set()).update(k for k in d["kinds"] if k)
    assert set(seen) == set(R.FAMILIES)
    for fam in R.FAMILIES:
        assert seen[fam] == set(R.kinds_of(fam)), (fam, set(R.kinds_of(fam)) - seen[fam])
    # the shapes the block families are entered at: partial trip only; one full trip; two full trips and a ragged partial; four full
    assert R.walk(2049, 0)[1] <= 3 * 256 and R.full_trips(256, R.walk(4099, 0)[1], 0) == 1
    assert R.full_trips(256, R.walk(9001, 1)[1], 0) == 2 and R.walk(9001, 1)[1] % 256 != 0
    assert R.full_trips(1024, R.walk(65537, 0)[1], 0) == 4


def _ratios(case, lead):
    ev = R.evaluate(case, lead)
    out = []
    for p, r in enumerate(ev["rows"]):
        b = r["bounds"]
        assert np.isfinite(r["replay"]) and np.isfinite(r["lse32"]) and np.isfinite(r["lse64"])
        out.append((r["kind"], R.ratio(r["replay"], r["lse64"], b["lse"]), r["lse32_err"] / b["lse"],
                    max(r["dx32_err_tA"], r["dx32_err_tB"]) / b["dx"]))
    return out


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_the_replay_and_the_two_pass_reference_are_inside_the_bound(case):
    """The flawless replay within the oracle's bound; the plain f32 two-pass reference within HALF of it, for lse and for dx: a row
    that a plain f32 evaluation handles within 0.5 of the bound is one a kernel must handle within 1.0."""
    for lead in R.LEADS if case.inner == 1 else (4,):
        for kind, rep, lse32, dx32 in _ratios(case, lead):
            where = (R.case_id(case), lead, kind)
            print("%s lead %d %-22s replay %.3f two-pass lse %.3f dx %.3f" % (R.case_id(case), lead, kind, rep, lse32, dx32))
            assert rep <= 1.0 and rep <= WORST_REPLAY, (where, rep)
            assert lse32 <= 0.5 and dx32 <= 0.5, (where, lse32, dx32)
            assert lse32 <= WORST32_LSE and dx32 <= WORST32_DX, (where, lse32, dx32)


# ---- teeth ---------------------------------------------------------------------------------------------------------------------------
def _flawed_ratio(case, lead, p, flaw):
    ev = R.evaluate(case, lead)
    d, r = ev["d"], ev["rows"][p]
    return R.ratio(R.replay(d["x"][p], d["offs"][p], d["fam"], (flaw,)), r["lse64"], r["bounds"]["lse"])


@pytest.mark.parametrize("flaw", R.FLAWS)
def test_a_flawed_replay_is_far_outside_on_the_committed_rows(flaw):
    """non-finite or more than 100 bounds out in at least one committed call of EVERY family the flaw exists in"""
    shown = {}
    for case in R.CASES:
        for lead in R.LEADS if case.inner == 1 else (4,):
            d = R.build(case, lead)
            if flaw not in R.flaws_of(d["fam"]):
                continue
            for p, kind in enumerate(d["kinds"]):
                if kind in TEETH[flaw] and not _flawed_ratio(case, lead, p, flaw) <= 100.0:
                    shown.setdefault(d["fam"], []).append((R.case_id(case), lead, kind))
    want = {f for f in R.FAMILIES if flaw in R.flaws_of(f)}
    assert set(shown) == want, (flaw, want - set(shown))
    print(flaw, {f: sorted({(c, k) for c, _, k in v}) for f, v in shown.items()})


def test_on_the_logits_of_the_other_tests_a_wrong_shift_is_invisible():
    """Why tests/test_gpu_cross_entropy.py (and the fullsize and tape files, which draw the same way) were blind: on `make`'s
    N(0, 3^2) logits, over the shapes of its family test, every flaw of SHIFT_FLAWS stays inside the bound.  `no_rescale`, which
    adds sums taken under different shifts, is far outside even there."""
    worst = dict.fromkeys(R.FLAWS, 0.0)
    for C, inner in FAMILY_SHAPES:
        x, _ = make(C, (5, C) if inner == 1 else (5, C, inner))
        rows = R.as_rows(x, inner)
        fam = R.family(C, inner)
        for p in range(0, rows.shape[0], inner):
            xr, off = rows[p], (p * C) % 4 if inner == 1 else 0
            lse64 = R.oracle_row(xr, 0)[0]
            bound = X.bounds(C, float(np.abs(xr).max()), 1)["lse"]
            assert R.ratio(R.replay(xr, off, fam), lse64, bound) <= 1.0
            for flaw in R.flaws_of(fam):
                worst[flaw] = max(worst[flaw], R.ratio(R.replay(xr, off, fam, (flaw,)), lse64, bound))
    print(worst)
    for flaw in R.SHIFT_FLAWS:
        assert worst[flaw] <= 1.0, (flaw, worst[flaw])
    assert not worst["no_rescale"] <= 100.0


def test_where_a_shift_flaw_leaves_m_at_the_start_value_any_data_sees_it():
    """The two forms of a shift flaw the old data does see.  A partial trip without ce_online on a lane WITHOUT a full trip (nb <= 3
    NT: the partial trip is the lane's first): m is still f32::MIN and exp(x - m) overflows whatever x is - why
    `partial_trip_no_online` spares such lanes.  And `max_skips_edge` on a row with no quad at all (C <= 3, and C = 4 .. 6 at some
    row starts): the same; test_grid has C = 1, 2, 3.  Every row with a quad hides it (the test above, from C = 8)."""
    with np.errstate(all="ignore"):
        assert np.exp(np.float32(-3.0) - np.float32(R.F32_MIN)) == np.inf
    assert R.full_trips(256, R.walk(2049, 0)[1], np.arange(256)).max() == 0
    x, _ = make(3 * 131 + 7 + 1, (1, 3))
    assert R.walk(3, 0)[1] == 0 and R.replay(x[0], 0, "row1", ("max_skips_edge",)) == np.inf and np.isfinite(R.replay(x[0], 0, "row1"))
    assert min(C for C, _ in FAMILY_SHAPES) >= 8

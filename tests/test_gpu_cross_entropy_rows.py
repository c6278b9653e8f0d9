"""GPU parity of nk_cross_entropy_fwd / _bwd / _bwd_assign on logit rows that MOVE the running maximum (tests/cross_entropy_rows.py:
kinds, cases, the 1/8 grid), against tests/cross_entropy_oracle.py in f64, through the C ABI.
tests/test_gpu_cross_entropy.py, tests/test_gpu_fullsize_cross_entropy.py and tests/test_gpu_tape_cross_entropy.py draw every logit
from N(0, 3^2) or N(0, 2^2): lse = m + log(sum exp(x - m)) is the same for any m that neither overflows nor flushes the sum, so a
maximum that leaves out the head / tail scalars or a quad of the four-quad trip, a partial trip or edge element added without
ce_online, a merge against lane 0's or wave 0's m, a fold from 0 and no shift at all read correct values there
(tests/test_oracle_cross_entropy_rows.py shows it on a replay of the kernels' arithmetic, and shows that each is non-finite or more
than 100 bounds out on the rows used here).

Cases (cross_entropy_rows.CASES): row1 at C = 10, 255, 256; row2 300; row4 601; row8 1100, 2048; block256 2049 (partial trip only),
4099 (one full trip), 9001 (two and a ragged partial); block512 16385, 20000; block1024 65537 (four full trips), 70001; generic
(12, 5) and (300, 7); the x / dx pair at different offsets (C = 300, 9001: the backward goes generic).  One call holds every kind
that exists at its geometry, at leads 4, 5, 6, 7; both target sets (the row's maximum; its lowest live class) at every lead.

Tolerance: cross_entropy_oracle.bounds and nothing else - through check_case for the call (xmax over the call's finite logits) and,
per row, with the row's own live xmax (cross_entropy_rows, Bounds): |lse - lse64| <= bounds.lse, |da - dx64| <= bounds.dx.  Margins
are recorded under `cross_entropy_rows:<family>:<kind>` with the oracle's bound in the absolute slot and the plain f32 two-pass
reference's error as err_cpu32.

Bit contracts on these rows: two runs are identical; assign equals `+=` onto zeros; a row's lse and gradient row do not depend on
the rows it shares the call (row kernels: the block) with.  Every case with inner == 1 is also held against the composed device path
(log_softmax + nll, two-pass kernels) under the tolerances of test_fused_against_the_composed_device_path.

Worst err_gpu / bound per family and kind on an MI355X (`vs_abs_1e-6` of the margins file: the slot holds the oracle's bound), kinds
in the order plain, climbing, falling, lifted, sunk, masked_inf, masked_min, masked_1e9; every `peaked` row reads 0.00 (its lse IS the
raised logit and every other softmax entry is 0: a peak is right or non-finite):
  cross_entropy_rows:row1       0.02 0.18 0.02 0.23 0.09 0.08 0.04 0.08
  cross_entropy_rows:row2       0.07 0.16 0.00 0.00 0.01 0.04 0.08 0.02
  cross_entropy_rows:row4       0.01 0.22 0.01 0.05 0.15 0.04 0.07 0.07
  cross_entropy_rows:row8       0.05 0.35 0.01 0.14 0.17 0.04 0.04 0.04
  cross_entropy_rows:block256   0.03 0.20 0.02 0.19 0.04 0.03 0.04 0.03
  cross_entropy_rows:block512   0.01 0.24 0.00 0.19 0.09 0.02 0.02 0.01
  cross_entropy_rows:block1024  0.01 0.19 0.00 0.16 0.15 0.02 0.01 0.02
  cross_entropy_rows:generic    0.07 0.25 0.00 0.25 0.20 0.04 0.09 0.02
The replay and the plain f32 two-pass reference read the same worst figure, 0.35 (tests/test_oracle_cross_entropy_rows.py): what is
left is the one rounding of m + log s at |lse| up to 2016.  No kernel had to change.

Teeth, measured once on the device with three libraries built for the purpose (one flaw each, no flawed source kept), over this
file, tests/test_gpu_cross_entropy.py and tests/test_gpu_fullsize_cross_entropy.py (the tape file binds the library it was linked
with and was not part of it).  The block merge shifting by wave 0's maximum (`red[0][0]`): 22 tests here fail - parity, composed
path and bit contracts of all seven block cases and the offset pair at C = 9001, every failure a non-finite lse - and all 146 other
tests pass, every test of the two older files among them.  The four-quad trip's group maximum over three quads: 19 tests here fail
(the six block cases with a full trip, the pair at 9001) and the two shapes this change adds to
test_non_finite_logits_follow_the_composed_device_path, (5, 4099) and (3, 16385), whose +inf sits in slot 3; everything older
passes.  The row kernels leaving the head / tail scalars out of the maximum: 17 tests here fail (all seven row cases) - and so do the
twelve test_grid cases at C = 1, 2, 3, rows that are ALL edge and overflow on any data; on every row with a quad the older files
pass.  The other flaws of cross_entropy_rows.SHIFT_FLAWS are shown on the replay only."""
import numpy as np
import pytest

import cross_entropy_oracle as X
import cross_entropy_rows as R
from test_gpu_cross_entropy import check_case, composed, run_all
from test_gpu_embedding import same_bits

pytestmark = pytest.mark.gpu

IDS = [R.case_id(c) for c in R.CASES]
FLAT = [c for c in R.CASES if c.inner == 1]


def _built(case, lead):
    blead = lead if case.inner == 1 else 4          # (a strided call has no row starts to rotate)
    return R.build(case, blead), R.evaluate(case, blead)


def _per_row(case, lead, d, ev, tname, t, res, g, w, ignore=-1):
    """the per-row checks on one check_case result: finite where the oracle is, lse and the assign gradient within the ROW's bound"""
    from conftest import record_margin
    _, lse, dx, da = res
    lse, dx, da = lse.reshape(-1), R.as_rows(dx, case.inner), R.as_rows(da, case.inner)
    failed = []
    for p, kind in enumerate(d["kinds"]):
        r, xr = ev["rows"][p], d["x"][p]
        b = X.bounds(case.C, R.row_xmax(xr), 1, 0.0, g, w)
        label = "cross_entropy_rows:%s:%s" % (d["fam"], kind)
        err_lse = abs(float(lse[p]) - r["lse64"])
        ok = np.isfinite(lse[p]) and err_lse <= b["lse"]
        if kind:
            record_margin(label, err_lse, r["lse32_err"], b["lse"])
        err_dx = 0.0
        if int(t.reshape(-1)[p]) != ignore:
            want = g * w * r["dx64_" + tname]
            err_dx = float(np.abs(da[p] - want).max())
            ok = ok and np.isfinite(da[p]).all() and np.isfinite(dx[p]).all() and err_dx <= b["dx"]
            if kind:
                record_margin(label, err_dx, abs(g * w) * r["dx32_err_" + tname], b["dx"])
        print("%s lead %d %s %-22s lse %.3f dx %.3f of the bound" % (R.case_id(case), lead, tname, kind, err_lse / b["lse"], err_dx / b["dx"]))
        if not ok:
            failed.append((p, kind, float(lse[p]), r["lse64"], err_lse, b["lse"], err_dx, b["dx"]))
    assert not failed, (R.case_id(case), lead, tname, failed)


def _three_calls(dev, case, lead, lead_dx=None):
    d, ev = _built(case, lead)
    inner = case.inner
    x = R.as_call(d["x"], inner)
    P = d["x"].shape[0]
    first, second = ("tA", "tB") if lead % 2 == 0 else ("tB", "tA")
    t = R.as_targets(d[first], inner)
    _per_row(case, lead, d, ev, first, t, check_case(dev, x, t, "mean", lead=lead, lead_dx=lead_dx, seed=lead), 0.75, 1.0 / P)
    t = R.as_targets(d[second], inner)
    ignore = int(d[second][0])                      # a class that the targets of some rows hit: theirs are inactive
    hit = int((d[second] == ignore).sum())
    assert 1 <= hit < P
    _per_row(case, lead, d, ev, second, t, check_case(dev, x, t, "sum", ignore=ignore, lead=lead, lead_dx=lead_dx, seed=lead + 8), 0.75, 1.0, ignore)
    # label smoothing needs the mean of the logits: the rows without a mask value
    keep = np.flatnonzero(R.grid_finite(d))
    keep = keep[:keep.size // inner * inner]
    check_case(dev, R.as_call(d["x"][keep], inner), R.as_targets(d[first][keep], inner), "mean", eps=0.1, lead=lead, lead_dx=lead_dx, seed=lead + 16)


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_rows_equal_oracle(dev, case):
    for lead in R.LEADS:
        _three_calls(dev, case, lead)


@pytest.mark.parametrize("C", R.MISALIGNED_PAIR)
def test_rows_equal_oracle_with_x_and_dx_at_different_offsets(dev, C):
    """the backward takes the generic kernels, the forward does not"""
    assert R.family(C, 1, together=False) == "generic" and R.family(C, 1) != "generic"
    _three_calls(dev, R.Case(C, 1), 4, lead_dx=5)


@pytest.mark.parametrize("case", FLAT, ids=[R.case_id(c) for c in FLAT])
def test_rows_equal_the_composed_device_path(dev, case):
    """The independent device twin: log_softmax_fwd + nll_fwd / nll_bwd + log_softmax_bwd, whose kernels are two-pass.  On the
    rows without a finite mask value (finfo.min and -1e9 would make the call's xmax, and so the tolerance, meaningless) under the
    tolerances of test_fused_against_the_composed_device_path; on every row, with the masked_inf row whose target is a -inf class
    (loss = +inf) added, by NaN and inf pattern."""
    C, g = case.C, 0.5
    d, _ = _built(case, 4)
    keep = np.array([k not in ("masked_min", "masked_1e9") for k in d["kinds"]])
    x = np.ascontiguousarray(d["x"][keep])
    xmax = float(np.abs(x[np.isfinite(x)]).max())
    for red, tname in (("mean", "tA"), ("sum", "tB")):
        t = d[tname][keep]
        cout, cdx = composed(dev, x, t, red, g)
        want_loss, want_lse = X.forward(x, t, red)
        want = X.backward(x, t, want_lse, g, red)
        b = X.bounds(C, xmax, t.size, 0.0, g, 1.0 / t.size if red == "mean" else 1.0)
        scale = t.size if red == "sum" else 1
        for lead in (4, 5):
            out, _, _, da = run_all(dev, x, t, red, g=g, lead=lead)
            print("%s %s lead %d loss %.3g composed %.3g bound %.3g dx %.3g composed %.3g bound %.3g" % (
                R.case_id(case), red, lead, abs(out - want_loss), abs(cout - want_loss), b["loss"] * scale, np.abs(da - want).max(),
                np.abs(cdx - want).max(), b["dx"]))
            assert abs(out - cout) <= 2 * b["loss"] * scale and np.abs(da - cdx).max() <= 2 * b["dx"]
            assert abs(out - want_loss) <= max(abs(cout - want_loss), b["loss"] * scale / 8)
            assert np.abs(da - want).max() <= max(np.abs(cdx - want).max(), b["dx"] / 8)
    x = np.concatenate([d["x"], d["extra_row"][None, :]])
    t = np.concatenate([d["tB"], [d["extra_target"]]]).astype(np.float32)
    out, lse, _, da = run_all(dev, x, t, "sum", g=1.0)
    cout, cdx = composed(dev, x, t, "sum", 1.0)
    assert out == np.inf and cout == np.inf and np.isfinite(lse).all()
    assert np.array_equal(np.isnan(da), np.isnan(cdx)) and np.array_equal(np.isinf(da), np.isinf(cdx)) and np.isfinite(da).all()
    live_max = max(R.row_xmax(r) for r in x)
    assert np.abs(da - cdx).max() <= 2 * X.bounds(C, live_max, t.size)["dx"]
    assert da[-1, int(t[-1])] == -1.0                                   # dx_t = -(1 - e) g w on the -inf class


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_bit_contracts(dev, case):
    """two runs are identical; assign equals `+=` onto zeros; a row alone - at the offset from a 16-byte boundary it has in the
    call - gives the bits it gives among the others (a block family's row is its own block, four rows of a row family share one)"""
    lead = 5
    d, _ = _built(case, lead)
    x, t = R.as_call(d["x"], case.inner), R.as_targets(d["tA"], case.inner)
    runs = [run_all(dev, x, t, "sum", g=0.5, dx0=np.zeros(x.shape, np.float32), lead=lead) for _ in range(2)]
    assert runs[0][0] == runs[1][0] and np.isfinite(runs[0][0])
    for a, b, what in zip(runs[0][1:], runs[1][1:], ("lse", "+=", "assign")):
        same_bits(a, b, what)
    _, lse, dx, da = runs[0]
    same_bits(dx, da, "assign against += onto zeros")
    if case.inner > 1:
        return
    for p, kind in enumerate(d["kinds"]):
        _, lse1, _, da1 = run_all(dev, x[p:p + 1], t[p:p + 1], "sum", g=0.5, lead=4 + d["offs"][p])
        same_bits(lse1, lse[p:p + 1], ("lse alone", p, kind))
        same_bits(da1, da[p:p + 1], ("gradient alone", p, kind))

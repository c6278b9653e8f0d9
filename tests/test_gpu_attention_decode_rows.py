"""GPU parity of the decode attention (nk_attention_decode_fwd, nk_attention_decode_gqa_fwd, nk_attention_decode_window_fwd) on score
rows that MOVE the split-KV shift across chunks (tests/decode_rows.py: kinds, cases, the exact-score grid), against
tests/decode_oracle.py, tests/gqa_oracle.py and tests/window_oracle.py in f64, through the C ABI.
tests/test_gpu_attention_decode.py, tests/test_gpu_gqa.py and tests/test_gpu_attention_window.py draw q and k from uniform [-1, 1):
every chunk maximum lies within 2 log2 units of every other and of 0, a softmax is invariant under any shift that neither overflows
nor underflows, and so the first chunk's m in the combine, a `red[]` value left by the previous head of a group or no shift at all
give the same result there (tests/test_oracle_decode_rows.py shows it on a replay, and shows that each is non-finite or more than 100
bounds out on the rows used here).

Cases (decode_rows._cases, per dh in 32, 64, 128 - the vector kernels - and 20, 5 - the generic ones; C = the chunk of dh): lengths
C + 1 (the second chunk holds one key, which carries the `climbing` maximum), 2C + 1, 3C + 7 and T = 4 at start = kC - 2; the plain
form with B = 2, H = 3 and another kind per head; the grouped form at (H, Hkv) = (4, 2), (8, 1), (12, 1) - two blocks of 8 and 4
heads - with `lifted` and `sunk` neighbours inside a block; the window form at W = C - 1 (across one seam, and inside one chunk: the
direct write) and W = C + 5 (three chunks), one head per block and eight, on a linear cache and on rings that have wrapped - lo at
the last slot, a window that wraps, the smallest capacity W + T - 1 - with a dominant key at lo - 1 that must not count (`edge`) and
at lo and n - 1 that must (`edge_in`).  The workspace and every cache slot no position has reached are NaN; every result is finite.

Tolerance: err_gpu <= max(2 * err_cpu32, 1e-6 * yardstick) against the f64 oracle, per kind, yardstick = max(|ref|max, |v|max) as in
tests/test_gpu_attention_decode.py, with err_cpu32 the LARGER of two plain f32 references' errors: the oracle in f32 and the full-row
softmax in the exponent domain (decode_rows.exponent_softmax; why: tests/test_oracle_decode_rows.py).  Margins are recorded under
`attention_decode_rows:<form>:<kind>`.

Bit contracts on these rows: grouped = nk_attention_decode_fwd on the repeated cache; a window that holds every key = the
unwindowed call; grouped window = ungrouped window on the repeated cache; a ring = the linear cache of the same positions.

Worst err_gpu / bound per label on an MI355X (`vs_stated_policy` of the margins file), kinds in the order plain, climbing, falling,
lifted, sunk, peaked (, edge, edge_in):
  attention_decode_rows:plain   0.03 0.51 0.50 0.48 0.46 0.27
  attention_decode_rows:gqa     0.03 0.53 0.51 0.50 0.50 0.33
  attention_decode_rows:window  0.03 0.52 0.56 0.51 0.52 0.21 0.33 0.33
The replay of the kernels' arithmetic reads the same figures to 0.01 (tests/test_oracle_decode_rows.py).  Teeth, measured once on the
device with three libraries built for the purpose.  The combine shifting by the FIRST chunk's m: 20 of the 50 parity cases here fail
(non-finite: every case with a `climbing` problem of three chunks or more), and all 282 decode tests of the three files above pass.
No shift at all in the partials (m = 0 in the exponent and in the workspace): all 50 fail, the same 282 pass.  `red[]` written by a
block's first head only: the 15 grouped vector cases and the three vector cases of the test below fail; in the three files above
every comparison with an oracle still passes and 49 tests fail through their BIT comparisons of grouped against ungrouped alone
(another shift is another rounding) - so that flaw was visible before, the other two were not."""
import numpy as np
import pytest

import decode_rows as R

pytestmark = pytest.mark.gpu

CASES = R.all_cases()
IDS = [R.case_id(c) for c in CASES]


def capi():
    from neuronika_amd import capi as c
    return c


def _run(dev, form, q, kc, vc, start, T, H, W=0, ring=0):
    """One call of the form's entry point on host arrays: q (B*T, H*dh), kc / vc (B, Hkv, cap, dh) -> (B*T, H*dh).  The output and
    the workspace start as NaN."""
    c = capi()
    B, Hkv, cap, dh = kc.shape
    scale = float(R.scale_of(dh))
    Q, Kc, Vc, S = dev.array(q), dev.array(kc), dev.array(vc), dev.int_array(start)
    out = dev.full((B * T, H * dh), np.nan)
    if form == "window":
        ws = dev.full((c.attention_decode_window_workspace(B, T, H, dh, W),), np.nan)
        c.attention_decode_window_fwd(dev, Q, H * dh, Kc, Vc, S, out, ws, B, T, H, Hkv, dh, cap, W, ring, scale)
    else:
        ws = dev.full((c.attention_decode_workspace(B, T, H, dh, cap),), np.nan)
        if form == "gqa":
            c.attention_decode_gqa_fwd(dev, Q, H * dh, Kc, Vc, S, out, ws, B, T, H, Hkv, dh, cap, scale)
        else:
            assert Hkv == H
            c.attention_decode_fwd(dev, Q, H * dh, Kc, Vc, S, out, ws, B, T, H, dh, cap, scale)
    return out.numpy()


def _repeat(a, G):
    return np.ascontiguousarray(np.repeat(a, G, axis=1))


def _check(case, got, ev):
    from conftest import record_margin
    assert np.isfinite(got).all(), R.case_id(case)
    failed = []
    for kind in R.kinds_in(case):
        m = R.kind_mask(case, kind)
        bound, err_cpu, floor = R.bound(ev["ref"], (ev["ref32"], ev["ref32e"]), m, ev["vmax"])
        err_gpu = float(np.abs(got[m] - ev["ref"][m]).max())
        record_margin("attention_decode_rows:%s:%s" % (case.form, kind), err_gpu, err_cpu, floor)
        print("%s %s err_gpu %.3g err_cpu32 %.3g bound %.3g ratio %.2f (replay %.2f)" % (R.case_id(case), kind, err_gpu, err_cpu, bound,
                                                                                      err_gpu / bound, ev["ratios"][kind]))
        if not err_gpu <= bound:
            failed.append((kind, err_gpu, err_cpu, bound))
    assert not failed, (R.case_id(case), failed)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_equal_oracle(dev, case):
    ev = R.evaluate(case)
    d = ev["d"]
    G = case.H // case.Hkv
    W, ring = (case.W, case.ring) if case.form == "window" else (0, 0)
    got = _run(dev, case.form, d["q"], d["kc"], d["vc"], d["start"], case.T, case.H, W, ring)
    _check(case, got, ev)
    if G > 1:            # grouped bits are the ungrouped bits on the repeated cache
        form = "window" if case.form == "window" else "plain"
        assert np.array_equal(got, _run(dev, form, d["q"], _repeat(d["kc"], G), _repeat(d["vc"], G), d["start"], case.T, case.H, W, ring))
    if case.form != "window":   # a window that holds every key gives the bits of the unwindowed call
        for W_all in (max(case.start) + case.T, 100 * case.cap):
            assert np.array_equal(got, _run(dev, "window", d["q"], d["kc"], d["vc"], d["start"], case.T, case.H, W_all, 0)), W_all
    if ring:             # a ring gives the bits of the linear cache that holds the same positions
        assert np.array_equal(got, _run(dev, "window", d["q"], d["kl"], d["vl"], d["start"], case.T, case.H, W, 0))


@pytest.mark.parametrize("dh", R.DHS)
def test_a_head_does_not_depend_on_the_heads_it_shares_a_block_with(dev, dh):
    """The (12, 1) group - blocks of 8 and 4 heads over one read of the chunk, `lifted` and `sunk` side by side - against every head
    ALONE on the same cache (H = Hkv = 1: one head per block, nothing left over in LDS): the same bits."""
    case = next(c for c in CASES if c.name == "gqa-12x1" and c.dh == dh)
    d = R.evaluate(case)["d"]
    together = _run(dev, "gqa", d["q"], d["kc"], d["vc"], d["start"], case.T, case.H)
    for h in range(case.H):
        cols = slice(h * dh, (h + 1) * dh)
        alone = _run(dev, "plain", np.ascontiguousarray(d["q"][:, cols]), d["kc"], d["vc"], d["start"], case.T, 1)
        assert np.array_equal(alone, together[:, cols]), (h, case.kinds[0][h], case.kinds[1][h])

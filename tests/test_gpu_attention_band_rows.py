"""GPU parity of the sliding-window and packed-sequence fused cores (nk_attention_band_* / nk_attention_seg_* and the packed-QKV forms)
on score rows that MOVE the online softmax's lazy shift after a row's first finite tile (tests/attention_band_rows.py: kinds,
geometries, the exact-score grid), against tests/segment_oracle.py's composition, through the C ABI.  tests/test_gpu_attention_band.py,
tests/test_gpu_attention_seg.py and the tape tests draw q and k from uniform [-1, 1): in these kernels' own compiled copies of the tile
body (nk_attention_tile.h, included by attention_band_kernel for edge tiles and for whole tiles) the rescale of the running
sum and of the out accumulator then only ever multiplied zeros.  tests/test_gpu_attention_rows.py covers the causal copy alone.

Tolerance: the rule of tests/test_gpu_attention.py, unchanged - kernels and f32 oracle both measured against the f64 oracle fed the
SAME Philox mask, pass iff err_gpu <= max(2 * err_cpu32, 1e-6 * yardstick) per tensor, yardsticks attention_rows.terms for O, Pd and dV
and attention_rows.cancelling_terms for dS, dQ and dK; margins recorded under `attention_band_rows:<kind>:*` and
`attention_seg_rows:<kind>:*`.  Raw scores are exact on the grid and must EQUAL the f64 oracle's; no allowed probability is below
1e-30 (tests/test_oracle_attention_band_rows.py), so `dropped == 0` is compared everywhere, with no exclusion.

That the branch ran is read off the statistics: a row whose maximum exceeds the maximum of its first visible tile by more than 6 (log2
units) must end with a stored shift above that tile's maximum (attention_band_rows.must_move).  The still kinds are held to
attention_band_rows.settled_max - under a moving left edge a wave's rows start in different tiles, every start moves the whole wave,
and a `plain` row does NOT end at its own first tile's maximum (the CPU file measures that on the replay).

Instantiations.  attention_band_kernel<BWD, MASKED, OCC, DH, RAGGED, SEG>, SEG = false / true: 2 x 2 x 3 x 2 = 24 each (OCC follows).
test_band_rows_equal_oracle[kind-geometry-p] and test_seg_rows_equal_oracle[kind-geometry-p] run forward (BWD = false) and backward
(BWD = true) of every kind, so of `climbing`, `mixed` and (W, span >= 64) `peaked_in`, at p = 0.0 (MASKED = false) and p = 0.2 (MASKED =
true) on every geometry:
  band  DH 64 whole   1x256x2x64-w176 1x384x1x64-w100       DH 64 ragged   2x197x2x64-w40
        DH 32 whole   2x160x2x32-w40                        DH 32 ragged   1x129x1x32-w70
        DH 128 whole  1x256x1x128-w100                      DH 128 ragged  1x300x1x128-w96
  seg   DH 64 whole   1x256x2x64-d40.216 1x320x1x64-d200.120-s48       DH 64 ragged   2x197x2x64-d40.40.117_5.100.92
        DH 32 whole   1x384x2x32-d170.214                              DH 32 ragged   2x129x1x32-d5.124_64.65
        DH 128 whole  1x256x1x128-d96.160                              DH 128 ragged  1x300x2x128-d96.96.108
e.g. attention_band_kernel<true, true, 1, 128, true, true> is test_seg_rows_equal_oracle[climbing-1x300x2x128-d96.96.108-0.2].  Which tile
class (left-edge, whole, diagonal square) the moves of each geometry fall into: tests/test_oracle_attention_band_rows.py.

Worst err_gpu / bound per label on an MI355X (`vs_stated_policy` of the margins file), kinds in the order plain, climbing, falling,
mixed, shifted, peaked_in (, handover):
  attention_band_rows  out 0.13 0.28 0.59 0.25 0.55 0.65      dropped 0.05 0.15 0.28 0.15 0.31 0.44    d_scores 0.04 0.06 0.11 0.06 0.11 0.12
                       dq (accumulated) and dq (assigned) 0.04 0.06 0.11 0.04 0.12 0.12
                       dk 0.02 0.02 0.01 0.03 0.01 0.04       dv 0.19 0.24 0.08 0.27 0.08 0.28
  attention_seg_rows   out 0.14 0.27 0.50 0.23 0.56 0.61 0.59     dropped 0.08 0.15 0.26 0.15 0.37 0.50 0.29
                       d_scores 0.04 0.06 0.10 0.06 0.13 0.11 0.10     dq (accumulated) 0.04 0.05 0.08 0.04 0.14 0.11 0.08
                       dq (assigned) 0.04 0.05 0.08 0.04 0.13 0.10 0.08
                       dk 0.04 0.02 0.01 0.03 0.01 0.03 0.01      dv 0.24 0.24 0.08 0.29 0.07 0.34 0.12
The replay of the kernels' arithmetic reads the same figures (tests/test_oracle_attention_band_rows.py).  Teeth, measured once on the
device with a library built for the purpose: `l_run *= alpha` removed from the band's whole-tile copy alone, and the seg whole-tile copy
rescaling `oacc[0]` alone, fail all 44 cases of the two parity tests whose moving rows (`climbing`, `mixed`, `shifted`, `peaked_in`,
`handover`) cross a whole tile (seg: dh 64 and 128, where oacc has more than one tile) - and none of `plain` or `falling`."""
import functools

import numpy as np
import pytest

from oracle import neuronika_oracle as O
import attention_rows as R
import attention_band_rows as BR
import segment_oracle as SO
from test_gpu_attention_band import _run as band_run
from test_gpu_attention_rows import OFFSET, SEED, _run as causal_run
from test_gpu_attention_seg import SENTINEL, Geometry, _run as seg_run

pytestmark = pytest.mark.gpu

NAMES = ("scores", "stats", "bits", "out", "d_scores", "dropped", "dq", "dk", "dv")      # in the order they are made


def capi():
    from neuronika_amd import capi as c
    return c


def _check(got, want64, want32, what, floor=0.0):
    scale = max(np.abs(want64).max(), floor)
    err_gpu, err_cpu = np.abs(got - want64).max(), np.abs(want32 - want64).max()
    from conftest import record_margin
    record_margin(what, err_gpu, err_cpu, 1e-6 * scale)
    print(what, "err_gpu %.3g err_cpu32 %.3g bound %.3g ratio %.3f" % (err_gpu, err_cpu, max(2 * err_cpu, 1e-6 * scale),
                                                                     err_gpu / max(2 * err_cpu, 1e-6 * scale)))
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


def _run(dev, family, geometry, p, assign, q, k, v, g, dq0):
    """Forward + backward of the band kernels (family "band": the geometry's W) or of the seg kernels on the geometry's edges."""
    B, S, H, dh, lo, span = BR.edges(geometry)
    if family == "band":
        assert BR.is_band(geometry)
        return band_run(dev, B, S, H, dh, span, p, True, SEED, OFFSET, assign, q, k, v, g, dq0)[0]
    return seg_run(dev, B, S, H, dh, lo, span, p, True, SEED, OFFSET, assign, q, k, v, g, dq0)[0]


@functools.lru_cache(maxsize=2)
def _reference(kind, geometry, p):
    """(ref64, ref32, noise (B*H, S, S)): computed once per case, shared by whoever asks next; nobody writes to it."""
    B, S, H, dh, lo, span = BR.edges(geometry)
    q, k, v, g = BR.rows(kind, geometry)
    SP = capi().attention_padded(S)
    noise = (np.ascontiguousarray(O.dropout_noise(B * H * SP * SP, p, SEED, OFFSET).reshape(B * H, SP, SP)[:, :S, :S]) if p != 0.0
             else np.ones((B * H, S, S), np.float32))
    ref, ref32 = BR.oracle(q, k, v, g, B, H, p, noise, lo, span)
    for t in (noise, *ref.values(), *ref32.values()):
        t.setflags(write=False)
    return ref, ref32, noise


def _rows_equal_oracle(dev, family, kind, geometry, p):
    B, S, H, dh, lo, span = BR.edges(geometry)
    q, k, v, g = BR.rows(kind, geometry)
    dq0 = R.uniform(9, (B * S, H * dh))
    ref, ref32, noise = _reference(kind, geometry, p)
    got = _run(dev, family, geometry, p, False, q, k, v, g, dq0)
    geo = Geometry(S, span, lo, H)      # (the band's maps are the seg maps at lo = band_lo)
    label = lambda name: "attention_%s_rows:%s:%s" % (family, kind, name)
    real, allowS = geo.real, geo.allowed[:, :S, :S]
    assert np.array_equal(allowS, BR.allowed_rows(lo, span, H))
    cut = lambda t: t[:, :S, :S]
    # raw scores: exact on the grid, so the MFMA's equal the f64 oracle's bit for bit; -inf at the masked positions of the computed
    # tiles (right of the diagonal, left of the row's edge, padded keys); nothing else was touched
    scores = geo.dense(got["scores"], geo.tile)
    assert np.array_equal(cut(scores)[allowS].astype(np.float64), ref["scores"][allowS])
    assert np.all(np.isneginf(scores[geo.tile & ~geo.allowed & real]))
    assert np.all(geo.untouched(got["scores"], geo.tile) == SENTINEL)
    terms = R.terms(ref, q, k, v, g, p)
    terms.update(R.cancelling_terms(ref, q, k, v, g, B, H, p, noise))
    # dS / Pd: oracle values on the allowed set, exactly 0 at every masked position of a defined block, untouched elsewhere
    dense = {}
    for name in ("dropped", "d_scores"):
        t = dense[name] = geo.dense(got[name], geo.block)
        assert np.isfinite(t[geo.block]).all(), name                     # (padded query rows are copies of row S - 1)
        assert not t[geo.block & ~geo.allowed & real].any(), name
        assert np.all(geo.untouched(got[name], geo.block) == SENTINEL), name
    assert np.array_equal(cut(dense["dropped"])[allowS] == 0, noise[allowS] == 0)      # dropped exactly where the mask says: everywhere
    for name in ("out", "dk", "dv", "dq"):
        assert np.isfinite(got[name]).all(), name       # (rows that sat at -1e30 through all--inf tiles included)
    _check(got["out"], ref["out"], ref32["out"], label("out"), floor=terms["out"])
    for name in ("dropped", "d_scores"):
        _check(cut(dense[name])[allowS], ref[name][allowS], ref32[name][allowS], label(name), floor=terms.get(name, 0.0))
    for name in ("dk", "dv"):
        _check(got[name], ref[name], ref32[name], label(name), floor=terms[name])
    _check(got["dq"] - dq0, ref["dq"], ref32["dq"], label("dq (accumulated)"), floor=max(np.abs(dq0).max(), terms["dq"]))
    # row statistics over the allowed keys: a shift within 2^6 below the maximum, never above; with the scores they reproduce the
    # softmax; the shift of every row that had to rescale lies above its first tile's maximum - the branch ran on the device
    le = BR.lo_eff_rows(lo, span, H)
    sc2 = R.log2_scores(ref["scores"], dh, allowS)
    stats = got["stats"][:, :S]
    m2, inv = stats[..., 0].astype(np.float64), stats[..., 1].astype(np.float64)
    assert np.isfinite(stats).all()
    assert (m2 >= sc2.max(2) - 6.0 - 1e-4).all() and (m2 <= sc2.max(2) + 1e-4).all()
    z = np.where(allowS, ref["scores"] * np.float64(np.float32(1.0 / np.sqrt(dh))), -np.inf)
    soft = np.exp(z - z.max(2, keepdims=True)); soft /= soft.sum(2, keepdims=True)
    np.testing.assert_allclose(np.exp2(sc2 - m2[..., None]) * inv[..., None], soft, rtol=2e-5, atol=1e-9)
    must = BR.must_move(sc2, le)
    assert (m2[must] > BR.first_tile_max(sc2, le)[must]).all()
    if kind in BR.MOVING and (kind != "peaked_in" or span >= 64):
        assert must.any()
    if kind in BR.STILL:
        assert not must.any()
        np.testing.assert_allclose(m2, BR.settled_max(sc2, le), rtol=0, atol=1e-4)
    # first-write form: dQ assigned, whatever the buffer held
    got2 = _run(dev, family, geometry, p, True, q, k, v, g, dq0)
    assert np.array_equal(got2["dq"] + dq0, got["dq"]) or np.abs(got2["dq"] + dq0 - got["dq"]).max() <= 1e-6 * np.abs(dq0).max()
    _check(got2["dq"], ref["dq"], ref32["dq"], label("dq (assigned)"), floor=terms["dq"])


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("geometry", BR.BAND, ids=BR.gid)
@pytest.mark.parametrize("kind", BR.BAND_KINDS)
def test_band_rows_equal_oracle(dev, kind, geometry, p):
    _rows_equal_oracle(dev, "band", kind, geometry, p)


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("geometry", BR.SEG, ids=BR.gid)
@pytest.mark.parametrize("kind", BR.SEG_KINDS)
def test_seg_rows_equal_oracle(dev, kind, geometry, p):
    _rows_equal_oracle(dev, "seg", kind, geometry, p)


# ---- bit contracts on moving rows ---------------------------------------------------------------------------------------------

BITS = [BR.BAND[1], BR.BAND[4], BR.BAND[6]]      # dh 64 whole with kt0 > 0, dh 32 ragged, dh 128 ragged: W >= 64, so `peaked_in` moves


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("geometry", BITS, ids=BR.gid)
@pytest.mark.parametrize("kind", ["climbing", "peaked_in"])
def test_rows_band_edges_give_the_band_core_to_the_bit(dev, kind, geometry, p):
    """lo = max(0, r - W + 1), and every entry -7 (the clamp makes it that), with span = W: the seg kernels' buffers - scores,
    statistics, mask words, out, dS, Pd, dq, dk, dv - are byte-identical to the band kernels', the untouched sentinel included."""
    B, S, H, dh, lo, W = BR.edges(geometry)
    q, k, v, g = BR.rows(kind, geometry)
    dq0 = R.uniform(9, (B * S, H * dh))
    want = _run(dev, "band", geometry, p, False, q, k, v, g, dq0)
    for edge in (SO.band_lo(B, S, W), np.full((B, S), -7, np.int32)):
        got = seg_run(dev, B, S, H, dh, edge, W, p, True, SEED, OFFSET, False, q, k, v, g, dq0)[0]
        for name in NAMES:
            assert got[name].tobytes() == want[name].tobytes(), (name, int(edge[0, 0]))


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("shape", [(1, 160, 2, 64), (2, 100, 2, 32), (1, 129, 1, 128)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["climbing", "peaked_in"])
def test_rows_without_a_left_edge_are_the_causal_core_to_the_bit(dev, kind, shape, p):
    """W in {S, S + 50}, and one document with span in {S, S + 50}: the causal layouts, and the causal entry points' bits in every
    buffer.  The causal kernel's rescale is the verified one (tests/test_gpu_attention_rows.py): this ties both copies to it on rows
    that rescale in every tile."""
    B, S, H, dh = shape
    SP, BH = capi().attention_padded(S), B * H
    q, k, v, g = BR.rows(kind, (B, S, H, dh, S))
    dq0 = R.uniform(9, (B * S, H * dh))
    want = causal_run(dev, B, S, H, dh, p, True, False, q, k, v, g, dq0)
    for width in (S, S + 50):
        runs = {"band": band_run(dev, B, S, H, dh, width, p, True, SEED, OFFSET, False, q, k, v, g, dq0)[0],
                "seg": seg_run(dev, B, S, H, dh, np.zeros((B, S), np.int32), width, p, True, SEED, OFFSET, False, q, k, v, g, dq0)[0]}
        for family, got in runs.items():
            for name in ("out", "dq", "dk", "dv"):
                assert np.array_equal(got[name], want[name]), (family, name, width)
            assert np.array_equal(got["stats"][:, :S], want["stats"]), (family, width)
            for name in ("scores", "d_scores", "dropped"):
                assert np.array_equal(got[name].reshape(BH, SP, SP), want[name], equal_nan=True), (family, name, width)
            assert np.array_equal(got["bits"].reshape(want["bits"].shape), want["bits"]), (family, width)


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("geometry", [BR.BAND[1], BR.BAND[4], BR.SEG[2], BR.SEG[5]], ids=BR.gid)
@pytest.mark.parametrize("kind", ["climbing", "peaked_in"])
def test_rows_packed_qkv_and_a_second_run_bit_for_bit(dev, kind, geometry, p):
    """nk_attention_qkv_band_* / nk_attention_qkv_seg_* on one (B*S, 3*H*dh) array give the bits of the three-array calls, and a second
    run of those gives the first one's bits in every buffer (no atomics; the rescale is a function of the data)."""
    c = capi()
    B, S, H, dh, lo, span = BR.edges(geometry)
    family = "band" if BR.is_band(geometry) else "seg"
    d = H * dh
    q, k, v, g = BR.rows(kind, geometry)
    zero = np.zeros((B * S, d), np.float32)
    ref = _run(dev, family, geometry, p, True, q, k, v, g, zero)
    again = _run(dev, family, geometry, p, True, q, k, v, g, zero)
    for name in NAMES:
        assert ref[name].tobytes() == again[name].tobytes(), name
    geo = Geometry(S, span, lo, H)
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    SP, BH = geo.SP, B * H
    QKV, G, LO = dev.array(np.concatenate([q, k, v], axis=1)), dev.array(g), dev.int_array(lo)
    scores, stats, out = dev.full((BH, geo.ext), SENTINEL), dev.zeros((BH, SP, 2)), dev.zeros((B * S, d))
    bits = dev.zeros((BH, geo.words))
    dS, dropped = dev.full((BH, geo.ext), SENTINEL), dev.full((BH, geo.ext), SENTINEL)
    dQKV = dev.full((B * S, 3 * d), np.nan)
    if family == "band":
        c.attention_qkv_band_fwd(dev, QKV, scores, stats, bits, out, B, S, H, dh, scale, p, True, SEED, OFFSET, window=span)
        c.attention_qkv_band_bwd(dev, dQKV, dS, dropped, G, out, scores, stats, bits, QKV, B, S, H, dh, scale, p, True, assign=True, window=span)
    else:
        c.attention_qkv_seg_fwd(dev, QKV, LO, scores, stats, bits, out, B, S, H, dh, scale, p, True, SEED, OFFSET, span=span)
        c.attention_qkv_seg_bwd(dev, dQKV, dS, dropped, G, out, scores, stats, bits, QKV, LO, B, S, H, dh, scale, p, True, assign=True, span=span)
    packed = dict(scores=scores.numpy(), stats=stats.numpy(), bits=bits.numpy().view(np.uint32), out=out.numpy(), d_scores=dS.numpy(),
                  dropped=dropped.numpy())
    for name, t in packed.items():
        assert np.array_equal(t, ref[name]), name
    dqkv = dQKV.numpy()
    for i, name in enumerate(("dq", "dk", "dv")):
        assert np.array_equal(dqkv[:, i * d:(i + 1) * d], ref[name]), name


# ---- neighbours ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geometry,keep", [(BR.SEG[2], (0, 1)), (BR.SEG[2], (1, 2)), (BR.SEG[5], (0, 1)), (BR.SEG[3], (0, 1)), (BR.SEG[1], (0, 1))],
                         ids=lambda t: BR.gid(t) if len(t) > 2 else "doc%d.%d" % t)
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_a_document_of_moving_rows_does_not_see_its_neighbours(dev, geometry, keep, p):
    """The kept document (sample, index) holds `climbing` rows - its shift moves in every tile - and starts and ends inside 32-row tiles
    it shares with its neighbours (rows 40 .. 79, 105 .. 196, 5 .. 128, 170 .. 383; 96 .. 191, the dh = 128 case, lies on tile edges).  Every OTHER document is switched between
    the two `handover` orientations - the rest of a shared wave tens of nats above the kept rows, then tens of nats below - and
    then to finite values of magnitude up to 1e3: out, dq, dk, dv AND the stored statistics of the kept rows are bit-identical.  (For the
    rows of a later document in a straddling wave that is nk_attention_band.h's claim: they ask unconditionally in the diagonal tile.)"""
    B, S, H, dh, lo, span = BR.edges(geometry)
    zero = np.zeros((B * S, H * dh), np.float32)
    runs, inputs = [], []
    for variant in (0, 1, "far"):
        q, k, v, g, mine = BR.kept_document(geometry, keep, variant)
        inputs.append(q)
        runs.append(seg_run(dev, B, S, H, dh, lo, span, p, True, SEED, OFFSET, True, q, k, v, g, zero)[0])
    assert np.abs(inputs[2]).max() > 900 and not np.array_equal(inputs[0], inputs[1])
    others = np.setdiff1d(np.arange(B * S), mine)
    b = keep[0]
    own = mine - b * S
    assert BR.later_rows(lo, span)[b, own].any() or keep == (0, 1)      # (a later document in a straddling wave, or the earlier one)
    for other in runs[1:]:
        for name in ("out", "dq", "dk", "dv"):
            assert np.isfinite(other[name]).all(), name
            assert np.array_equal(runs[0][name][mine], other[name][mine]), name
            assert not np.array_equal(runs[0][name][others], other[name][others]), name
        assert np.array_equal(runs[0]["stats"][b * H:(b + 1) * H, own], other["stats"][b * H:(b + 1) * H, own])
    assert np.isfinite(runs[0]["stats"][:, :S]).all()


def test_a_band_row_is_carried_by_its_wave(dev):
    """tests/test_gpu_attention_rows.py's test_a_row_does_not_depend_on_its_wave for the band kernel: an even (`plain`) row of `mixed`
    moves with every climbing odd neighbour that passes the test; the same even rows among `plain` odd rows move only where a row of
    their wave starts (attention_band_rows.settled_max).  Outputs inside the bound under two different stored shifts."""
    geometry = BR.BAND[0]
    B, S, H, dh, lo, W = BR.edges(geometry)
    q, k, v, g = BR.rows("mixed", geometry)
    calm = np.array(q)
    calm[1::2] = BR.rows("plain", geometry)[0][1::2]
    zero = np.zeros((B * S, H * dh), np.float32)
    a = _run(dev, "band", geometry, 0.0, True, q, k, v, g, zero)
    b = _run(dev, "band", geometry, 0.0, True, calm, k, v, g, zero)
    ref, ref32, _ = _reference("mixed", geometry, 0.0)
    even = slice(0, None, 2)
    bound = R.bound(ref["out"][even], ref32["out"][even], R.terms(ref, q, k, v, g, 0.0)["out"])
    for t in (a, b):
        assert np.abs(t["out"][even] - ref["out"][even]).max() <= bound
    ma, mb = a["stats"][:, :S][:, even, 0], b["stats"][:, :S][:, even, 0]
    allowed, le = BR.allowed_rows(lo, W, H), BR.lo_eff_rows(lo, W, H)
    settled = BR.settled_max(R.log2_scores(ref["scores"], dh, allowed), le)[:, even]
    np.testing.assert_allclose(mb, settled, rtol=0, atol=1e-4)                # among plain rows: the starts of the wave only
    assert (ma >= mb).all() and (ma > mb + 1.0).any()                         # among climbing rows: carried along

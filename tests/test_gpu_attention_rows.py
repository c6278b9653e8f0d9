"""GPU parity of the fused attention core (nk_attention_fwd / _bwd, the causal pair and the packed-QKV forms) on score rows that MOVE
the online softmax's lazy shift (tests/attention_rows.py: kinds, geometries, the exact-score grid), against the oracle's
node-by-node composition, through the C ABI.  tests/test_gpu_attention.py and tests/test_gpu_attention_causal.py draw q and k from
uniform [-1, 1): the shift never moves after the first key tile there, and the rescale of the running sum and of the out
accumulator, the rows a wave carries along, and a backward pass that reads a shift below the row maximum never ran.

Tolerance: the rule of tests/test_gpu_attention.py, unchanged - kernels and f32 oracle both measured against the f64 oracle fed the
SAME Philox mask, pass iff err_gpu <= max(2 * err_cpu32, 1e-6 * yardstick) per tensor with that file's yardsticks
(attention_rows.terms) for O, Pd and dV, and the summed terms of the cancelling score gradient (`_cancelling_terms`) for dS, dQ and
dK; margins recorded under `attention_rows:<kind>:*`.  The raw scores are exact on the grid and must EQUAL
the f64 oracle's.

That the rescale branch ran is read off the outputs: a row whose maximum exceeds its tile-0 maximum by more than 6 (log2 units)
must end with a stored shift above its tile-0 maximum (attention_rows.must_move); tests/test_oracle_attention_rows.py shows on the
CPU which rows of which kind those are."""
import functools

import numpy as np
import pytest

from oracle import neuronika_oracle as O
import attention_rows as R

pytestmark = pytest.mark.gpu

SEED, OFFSET = 0x1234567890ABCDEF, 4242      # as tests/test_gpu_attention.py
SENTINEL = 7.0


def capi():
    from neuronika_amd import capi as c
    return c


def _check(got, want64, want32, what, floor=0.0):
    scale = max(np.abs(want64).max(), floor)
    err_gpu, err_cpu = np.abs(got - want64).max(), np.abs(want32 - want64).max()
    from conftest import record_margin
    record_margin("attention_rows:" + what.split("[")[0].strip(), err_gpu, err_cpu, 1e-6 * scale)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


# The one yardstick that is not test_gpu_attention.py's: dS (and dQ, dK, which contract it) on rows where the score gradient
# cancels is measured by the terms that cancel - derivation in attention_rows.cancelling_terms and DESIGN.md section 5.  With the
# result's own size as the yardstick the device read up to 1.65 x the bound on `peaked` (dS 4.6e-7 against 2 x 1.4e-7 at
# (1, 160, 2, 64), p = 0, full; dK 1.64 x, dQ 1.65 x there) and 1.04 - 1.34 x for dS on single cases of `falling`, `mixed` and
# `shifted`: the rounding of the softmax dot dO . O (2e-6 on a dot of ~4) times P ~ 1 and the scale, on a dS that has cancelled to
# 1e-3 .. 1e-1 of its terms.  The replay of the kernel's arithmetic reads the same (tests/test_oracle_attention_rows.py).
_cancelling_terms = R.cancelling_terms


def _regions(S, SP):
    """Boolean (SP, SP) maps of the causal kernels' scratch contract (tests/test_gpu_attention_causal.py): `low` key <= query; `tile`
    the 32 x 32 tiles the forward visits; `block` the 128 x 128 blocks on which the backward defines dS / Pd."""
    r, k = np.arange(SP)[:, None], np.arange(SP)[None, :]
    return k <= r, (k // 32) <= (r // 32), (k // 128) <= (r // 128)


def _run(dev, B, S, H, dh, p, causal, assign, q, k, v, g, dq0, keep=True):
    """Forward + backward on three arrays; returns the whole padded (B*H, SP, SP) scratch tensors."""
    c = capi()
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    SP = c.attention_padded(S)
    Q, K, V, G = (dev.array(t) for t in (q, k, v, g))
    scores, stats, out = dev.full((B * H, SP, SP), SENTINEL), dev.zeros((B * H, SP, 2)), dev.zeros((B * S, H * dh))
    bits = dev.zeros((B * H, SP, SP // 32))
    c.attention_fwd(dev, Q, K, V, scores, stats, bits, out, B, S, H, dh, scale, p, True, SEED, OFFSET, causal=causal)
    dS, dropped, dQ = dev.full((B * H, SP, SP), SENTINEL), dev.full((B * H, SP, SP), SENTINEL), dev.array(dq0)
    dK, dV = dev.full((B * S, H * dh), np.nan), dev.full((B * S, H * dh), np.nan)
    c.attention_bwd(dev, dQ, dK, dV, dS, dropped, G, out, scores, stats, bits, Q, K, V, B, S, H, dh, scale, p, True,
                    assign=(assign, True, True), causal=causal)
    return dict(scores=scores.numpy(), stats=stats.numpy()[:, :S], out=out.numpy(), bits=bits.numpy().view(np.uint32), d_scores=dS.numpy(),
                dropped=dropped.numpy(), dq=dQ.numpy(), dk=dK.numpy(), dv=dV.numpy())


@functools.lru_cache(maxsize=None)
def _reference(kind, B, S, H, dh, p, causal):
    """(ref64, ref32, noise (B*H, S, S)): computed once per case and shared; nobody writes to it."""
    q, k, v, g = R.rows(kind, B, S, H, dh)
    SP = capi().attention_padded(S)
    noise = (np.ascontiguousarray(O.dropout_noise(B * H * SP * SP, p, SEED, OFFSET).reshape(B * H, SP, SP)[:, :S, :S]) if p != 0.0
             else np.ones((B * H, S, S), np.float32))
    ref, ref32 = R.oracle(q, k, v, g, B, H, p, noise, causal)
    for t in (noise, *ref.values(), *ref32.values()):
        t.setflags(write=False)
    return ref, ref32, noise


def _id(geometry):
    return "x".join(str(n) for n in geometry)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("geometry", R.GEOMETRIES, ids=_id)
@pytest.mark.parametrize("kind", R.KINDS)
def test_rows_equal_oracle(dev, kind, geometry, p, causal):
    """Entries the `dropped == 0` comparison leaves out because the f64 probability is below 1e-30 (an f32 kernel may flush it): none,
    for every kind at these geometries - the smallest probability is 3e-22 (`falling` at S = 160); asserted for `plain`, `under` and
    `shifted`, where anything else would mean wrong inputs, and printed for the others."""
    B, S, H, dh = geometry
    c = capi()
    SP = c.attention_padded(S)
    q, k, v, g = R.rows(kind, B, S, H, dh)
    dq0 = R.uniform(9, (B * S, H * dh))
    ref, ref32, noise = _reference(kind, B, S, H, dh, p, causal)
    got = _run(dev, B, S, H, dh, p, causal, False, q, k, v, g, dq0)
    label = lambda name: kind + ":" + name
    vis = R.visible(S, causal)
    low, tile, block = _regions(S, SP) if causal else (np.ones((SP, SP), bool),) * 3
    cut = lambda t: t[:, :S, :S]
    padk = np.zeros((SP, SP), bool); padk[:S, S:] = True
    # raw scores: exact on the grid, so the MFMA's equal the f64 oracle's bit for bit; -inf at masked and padded keys of visited tiles
    assert np.array_equal(cut(got["scores"])[:, vis].astype(np.float64), ref["scores"][:, vis])
    assert np.all(np.isneginf(got["scores"][:, tile & ~low])) and np.all(got["scores"][:, ~tile] == SENTINEL)
    assert np.all(np.isneginf(got["scores"][:, padk & tile]))
    # dS / Pd: oracle values at the visible positions, exactly 0 at masked and padded keys of a defined block, untouched elsewhere
    for name in ("dropped", "d_scores"):
        assert np.isfinite(got[name]).all(), name
        assert not got[name][:, block & ~low].any() and not got[name][:, padk & block].any(), name
        assert np.all(got[name][:, ~block] == SENTINEL), name
    # dropped exactly where the mask says, wherever the probability cannot underflow
    sure = ref["probs"] >= 1e-30
    left_out = int((vis & ~sure).sum())
    print(f"attention_rows {kind} {geometry} p={p} causal={causal}: {left_out} probabilities below 1e-30 left out")
    if kind in ("plain", "under", "shifted"):
        assert left_out == 0
    assert np.array_equal((cut(got["dropped"]) == 0)[:, vis][sure[:, vis]], (noise == 0)[:, vis][sure[:, vis]])
    assert (np.abs(cut(got["dropped"])[:, vis][~sure[:, vis]]) <= 1e-30).all()
    terms = R.terms(ref, q, k, v, g, p)
    terms.update(_cancelling_terms(ref, q, k, v, g, B, H, p, noise))
    for name in ("out", "dk", "dv", "dq"):
        assert np.isfinite(got[name]).all(), name
    _check(got["out"], ref["out"], ref32["out"], label("out"), floor=terms["out"])
    for name in ("dropped", "d_scores"):
        _check(cut(got[name])[:, vis], ref[name][:, vis], ref32[name][:, vis], label(name), floor=terms.get(name, 0.0))
    for name in ("dk", "dv"):
        _check(got[name], ref[name], ref32[name], label(name), floor=terms[name])
    _check(got["dq"] - dq0, ref["dq"], ref32["dq"], label("dq (accumulated)"), floor=max(np.abs(dq0).max(), terms["dq"]))
    # row statistics over the visible keys: a shift within 2^6 below the maximum, never above; with the scores they reproduce the
    # softmax; and the shift of every row that had to rescale lies above its tile-0 maximum - the branch ran on the device
    sc2 = R.log2_scores(ref["scores"], dh, vis)
    m2, inv = got["stats"][..., 0].astype(np.float64), got["stats"][..., 1].astype(np.float64)
    assert np.isfinite(got["stats"]).all()
    assert (m2 >= sc2.max(2) - 6.0 - 1e-4).all() and (m2 <= sc2.max(2) + 1e-4).all()
    z = np.where(vis, ref["scores"] * np.float64(np.float32(1.0 / np.sqrt(dh))), -np.inf)
    soft = np.exp(z - z.max(2, keepdims=True)); soft /= soft.sum(2, keepdims=True)
    np.testing.assert_allclose(np.exp2(sc2 - m2[..., None]) * inv[..., None], soft, rtol=2e-5, atol=1e-9)
    must = R.must_move(sc2)
    assert (m2[must] > sc2[:, :, :32].max(2)[must]).all()
    if not causal:   # which rows those are is fixed by the construction (tests/test_oracle_attention_rows.py): every row / every odd row
        assert kind != "climbing" or must.all()
        assert kind != "mixed" or must[:, 1::2].all()
        assert kind not in R.STILL or not must.any()
    # first-write form: dQ assigned, whatever the buffer held
    got2 = _run(dev, B, S, H, dh, p, causal, True, q, k, v, g, dq0)
    assert np.array_equal(got2["dq"] + dq0, got["dq"]) or np.abs(got2["dq"] + dq0 - got["dq"]).max() <= 1e-6 * np.abs(dq0).max()
    _check(got2["dq"], ref["dq"], ref32["dq"], label("dq (assigned)"), floor=terms["dq"])


TWO = [(1, 160, 2, 64), (2, 100, 2, 32)]


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("geometry", TWO, ids=_id)
@pytest.mark.parametrize("kind", R.MOVING)
def test_rows_inference_form_is_the_same_forward(dev, kind, geometry, causal):
    """scores = stats = mask_bits = NULL: the output bits are the kept-state form's, on rows that rescale."""
    c = capi()
    B, S, H, dh = geometry
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    Q, K, V = (dev.array(t) for t in R.rows(kind, B, S, H, dh)[:3])
    SP = c.attention_padded(S)
    for p in (0.0, 0.2):
        scores, stats, bits = dev.zeros((B * H, SP, SP)), dev.zeros((B * H, SP, 2)), dev.zeros((B * H, SP, SP // 32))
        kept, lean = dev.zeros((B * S, H * dh)), dev.zeros((B * S, H * dh))
        c.attention_fwd(dev, Q, K, V, scores, stats, bits, kept, B, S, H, dh, scale, p, True, SEED, OFFSET, causal=causal)
        c.attention_fwd(dev, Q, K, V, None, None, None, lean, B, S, H, dh, scale, p, True, SEED, OFFSET, causal=causal)
        assert np.array_equal(kept.numpy(), lean.numpy()), p


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("geometry", TWO, ids=_id)
@pytest.mark.parametrize("kind", ["climbing", "peaked"])
def test_rows_packed_qkv_bit_for_bit(dev, kind, geometry, causal):
    """nk_attention_qkv_fwd / _bwd and the causal pair on one (B*S, 3*H*dh) array give the bits of the three-array calls."""
    c = capi()
    B, S, H, dh = geometry
    d, p = H * dh, 0.2
    q, k, v, g = R.rows(kind, B, S, H, dh)
    ref = _run(dev, B, S, H, dh, p, causal, True, q, k, v, g, np.zeros((B * S, d), np.float32))
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    SP = c.attention_padded(S)
    QKV, G = dev.array(np.concatenate([q, k, v], axis=1)), dev.array(g)
    scores, stats, out = dev.full((B * H, SP, SP), SENTINEL), dev.zeros((B * H, SP, 2)), dev.zeros((B * S, d))
    bits = dev.zeros((B * H, SP, SP // 32))
    c.attention_qkv_fwd(dev, QKV, scores, stats, bits, out, B, S, H, dh, scale, p, True, SEED, OFFSET, causal=causal)
    dS, dropped = dev.full((B * H, SP, SP), SENTINEL), dev.full((B * H, SP, SP), SENTINEL)
    dQKV = dev.full((B * S, 3 * d), np.nan)
    c.attention_qkv_bwd(dev, dQKV, dS, dropped, G, out, scores, stats, bits, QKV, B, S, H, dh, scale, p, True, assign=True, causal=causal)
    assert np.array_equal(out.numpy(), ref["out"]) and np.array_equal(scores.numpy(), ref["scores"])
    assert np.array_equal(stats.numpy()[:, :S], ref["stats"]) and np.array_equal(bits.numpy().view(np.uint32), ref["bits"])
    assert np.array_equal(dS.numpy(), ref["d_scores"]) and np.array_equal(dropped.numpy(), ref["dropped"])
    dqkv = dQKV.numpy()
    for i, name in enumerate(("dq", "dk", "dv")):
        assert np.array_equal(dqkv[:, i * d:(i + 1) * d], ref[name]), name


def test_rows_repeat_bit_for_bit(dev):
    """Two runs of forward and backward on `mixed` agree in every output (no atomics; the rescale is a function of the data)."""
    B, S, H, dh = 1, 160, 2, 64
    q, k, v, g = R.rows("mixed", B, S, H, dh)
    for causal in (False, True):
        a, b = (_run(dev, B, S, H, dh, 0.2, causal, True, q, k, v, g, np.zeros((B * S, H * dh), np.float32)) for _ in range(2))
        for name in a:
            assert np.array_equal(a[name], b[name]), (name, causal)


def test_a_row_does_not_depend_on_its_wave(dev):
    """The trigger is uniform over a wave's 32 queries: an even (`plain`) row of `mixed` takes max(shift, tile maximum) in every tile
    in which a climbing odd neighbour passes the test.  The same even rows among `plain` odd rows see no trigger after tile 0 and keep
    their tile-0 shift.  Their outputs agree within the policy bound - the same softmax under two shifts - and their stored shifts
    differ: the coupling is a documented property of the statistics, invisible in the output (the device-side twin of the
    "row_local_any" replay in tests/test_oracle_attention_rows.py)."""
    B, S, H, dh = 1, 64, 1, 64
    q, k, v, g = R.rows("mixed", B, S, H, dh)
    calm = np.array(q)
    calm[1::2] = R.rows("plain", B, S, H, dh)[0][1::2]
    zero = np.zeros((B * S, H * dh), np.float32)
    a = _run(dev, B, S, H, dh, 0.0, False, True, q, k, v, g, zero)
    b = _run(dev, B, S, H, dh, 0.0, False, True, calm, k, v, g, zero)
    ref, ref32, _ = _reference("mixed", B, S, H, dh, 0.0, False)
    even = slice(0, None, 2)
    assert np.array_equal(a["scores"][:, even], b["scores"][:, even])
    bound = R.bound(ref["out"][even], ref32["out"][even], R.terms(ref, q, k, v, g, 0.0)["out"])
    for t in (a, b):
        assert np.abs(t["out"][even] - ref["out"][even]).max() <= bound
    ma, mb = a["stats"][0, even, 0], b["stats"][0, even, 0]
    sc2 = R.log2_scores(ref["scores"], dh, R.visible(S, False))[0, even]
    np.testing.assert_allclose(mb, sc2[:, :32].max(1), rtol=0, atol=1e-4)     # alone: the tile-0 maximum
    assert (ma >= mb).all() and (ma > mb).any()                               # carried: moved with the wave
    np.testing.assert_allclose(ma, sc2.max(1), rtol=0, atol=1e-4)             # S = 64: to max(tile 0, tile 1)

"""The sliding-window oracle (tests/window_oracle.py) pinned without a GPU: against an independent per-row loop (no oracle node,
no mask: a plain softmax over the rows a query may see), against tests/causal_oracle.py and tests/decode_oracle.py for W >= S, ring
against linear storage, the banded module's gradients against torch autograd (in a child process), and the workspace bound (W + C - 2) / C + 1 against a
brute-force count of the position-aligned chunks a window touches, over all lo."""
import numpy as np
import pytest

import causal_oracle as CO
import decode_oracle as DO
import gqa_oracle as GO
import window_oracle as WO


def rnd(seed, shape, lo=-1.0, hi=1.0):
    a = np.random.default_rng(seed).random(shape)
    return a * (hi - lo) + lo


def _rows(t, B, S, lo, hi):
    return np.ascontiguousarray(np.concatenate([t[b * S + lo:b * S + hi] for b in range(B)]))


def _per_row(q, k, v, B, S, H, Hkv, dh, W):
    """Independent restatement: row i of sample b, head h, over keys max(0, i - W + 1) .. i of kv head h // G, exp / sum by hand."""
    G = H // Hkv
    out = np.zeros((B * S, H * dh))
    for b in range(B):
        for i in range(S):
            lo = max(0, i - W + 1)
            for h in range(H):
                kv = h // G
                qr = q[b * S + i, h * dh:(h + 1) * dh]
                s = np.array([qr @ k[b * S + j, kv * dh:(kv + 1) * dh] for j in range(lo, i + 1)]) / np.sqrt(dh)
                e = np.exp(s - s.max())
                p = e / e.sum()
                out[b * S + i, h * dh:(h + 1) * dh] = sum(p[j - lo] * v[b * S + j, kv * dh:(kv + 1) * dh] for j in range(lo, i + 1))
    return out


@pytest.mark.parametrize("W", [1, 2, 5, 11, 12, 30])
@pytest.mark.parametrize("B,S,H,Hkv,dh", [(2, 12, 2, 2, 8), (1, 9, 4, 2, 5), (2, 7, 4, 1, 4)])
def test_banded_core_equals_a_per_row_loop(B, S, H, Hkv, dh, W):
    q, k, v = rnd(1, (B * S, H * dh)), rnd(2, (B * S, Hkv * dh)), rnd(3, (B * S, Hkv * dh))
    want = _per_row(q, k, v, B, S, H, Hkv, dh, W)
    G = H // Hkv
    got, _ = WO.attention_core_forward(q, GO.repeat_kv(k, Hkv, G, dh), GO.repeat_kv(v, Hkv, G, dh), H, B, 0.0, np.ones((B * H, S, S)), W)
    assert np.all(np.isfinite(got)) and np.abs(got - want).max() <= 1e-12


def test_the_band_is_the_causal_triangle_for_wide_windows():
    B, S, H, dh = 2, 10, 2, 6
    q, k, v = (rnd(s, (B * S, H * dh)) for s in (1, 2, 3))
    noise = np.ones((B * H, S, S))
    want, _ = CO.attention_core_forward(q, k, v, H, B, 0.0, noise)
    for W in (S, S + 1, 1000):
        assert np.array_equal(WO.band_mask(S, W, np.float64), CO.causal_mask(S, np.float64))
        got, _ = WO.attention_core_forward(q, k, v, H, B, 0.0, noise, W)
        assert np.array_equal(got, want)
    m = WO.band_mask(5, 2, np.float32)
    assert m.dtype == np.float32 and np.all(np.diag(m) == 0) and np.all(np.diag(m, -1) == 0) and np.all(np.isinf(np.diag(m, -2)))
    assert np.all(np.isinf(m[np.triu_indices(5, 1)]))


@pytest.mark.parametrize("ring", [False, True], ids=["linear", "ring"])
@pytest.mark.parametrize("W", [1, 3, 6, 40])
@pytest.mark.parametrize("slices", ["tokens", "prefill+tokens", "3"])
def test_stepping_equals_the_banded_forward(W, ring, slices):
    """Stepping a (grouped) layer token by token and in slices reproduces the rows of the banded core; on a ring of the smallest
    legal capacity W + Tmax - 1, whose slots are overwritten many times over."""
    B, S, H, Hkv, dh = 2, 17, 4, 2, 5
    G = H // Hkv
    q, k, v = rnd(1, (B * S, H * dh)), rnd(2, (B * S, Hkv * dh)), rnd(3, (B * S, Hkv * dh))
    want, _ = WO.attention_core_forward(q, GO.repeat_kv(k, Hkv, G, dh), GO.repeat_kv(v, Hkv, G, dh), H, B, 0.0, np.ones((B * H, S, S)), W)
    sizes = {"tokens": [1] * S, "prefill+tokens": [4] + [1] * (S - 4), "3": [3] * (S // 3) + [S % 3]}[slices]
    cap = min(W, S) + max(sizes) - 1 if ring else S
    kc, vc = DO.new_cache(B, Hkv, cap, dh, np.float64, fill=np.nan)
    start, got = np.zeros(B, dtype=np.int64), np.zeros_like(want)
    for T in sizes:
        lo = int(start[0])
        WO.append(kc, vc, _rows(k, B, S, lo, lo + T), _rows(v, B, S, lo, lo + T), start, T, ring)
        ctx = WO.decode_forward(_rows(q, B, S, lo, lo + T), kc, vc, start, T, min(W, S), ring, H=H)
        for b in range(B):
            got[b * S + lo:b * S + lo + T] = ctx[b * T:(b + 1) * T]
        start = start + T
    assert np.all(np.isfinite(got)) and np.abs(got - want).max() <= 1e-12


def test_wide_window_decode_is_the_decode_oracle():
    B, H, dh, cap, T = 3, 2, 6, 20, 2
    start = np.array([7, 0, 15])
    kc, vc = rnd(4, (B, H, cap, dh)), rnd(5, (B, H, cap, dh))
    q = rnd(6, (B * T, H * dh))
    want = DO.decode_forward(q, kc, vc, start, T)
    for W in (17, 20, 99):
        assert np.array_equal(WO.decode_forward(q, kc, vc, start, T, W), want)
    # a linear cache clips n to cap, as tests/decode_oracle.py does
    assert np.array_equal(WO.decode_forward(q, kc, vc, [19, 25, 3], T, 99), DO.decode_forward(q, kc, vc, [19, 25, 3], T))
    # grouped: tests/gqa_oracle.py's repeat
    q4 = rnd(7, (B * T, 4 * dh))
    assert np.array_equal(WO.decode_forward(q4, kc, vc, start, T, 99, H=4), GO.decode_forward_gqa(q4, kc, vc, start, T, 4))


def test_ring_storage_equals_linear_storage():
    """The same positions' contents in a ring (two capacities, ragged starts far past the capacity) and in a linear cache: the
    same bits - the oracle gathers the window's rows in position order either way."""
    B, Hkv, H, dh, T, W = 3, 2, 4, 4, 3, 5
    start = np.array([40, 2, 23])
    n_max = int(start.max()) + T
    kl, vl = rnd(1, (B, Hkv, n_max, dh)), rnd(2, (B, Hkv, n_max, dh))
    q = rnd(3, (B * T, H * dh))
    want = WO.decode_forward(q, kl, vl, start, T, W, H=H)
    for cap in (W + T - 1, W + T + 6):
        kr, vr = WO.ring_image(kl, start + T, cap), WO.ring_image(vl, start + T, cap)
        got = WO.decode_forward(q, kr, vr, start, T, W, ring=True, H=H)
        assert np.array_equal(got, want), cap
    # the ring append writes the step's rows where the image has them
    cap = W + T - 1
    k, v = rnd(4, (B * T, Hkv * dh)), rnd(5, (B * T, Hkv * dh))
    DO.append(kl, vl, k, v, start, T)
    kr, vr = WO.ring_image(kl, start, cap), WO.ring_image(vl, start, cap)
    WO.append(kr, vr, k, v, start, T, ring=True)
    assert np.array_equal(kr, WO.ring_image(kl, start + T, cap), equal_nan=True)
    assert np.array_equal(vr, WO.ring_image(vl, start + T, cap), equal_nan=True)


def test_a_negative_start_gives_a_zero_row_and_nothing_is_appended():
    B, H, dh, cap, T, W = 2, 1, 3, 6, 2, 3
    kc, vc = DO.new_cache(B, H, cap, dh, np.float64, fill=7.0)
    k, v, q = rnd(1, (B * T, dh)), rnd(2, (B * T, dh)), rnd(3, (B * T, dh))
    WO.append(kc, vc, k, v, [-5, 1], T, ring=True)
    assert np.all(kc[0] == 7.0) and np.array_equal(kc[1, 0, 1:3], k[2:4])
    out = WO.decode_forward(q, kc, vc, [-5, 1], T, W, ring=True)
    assert np.all(out[:T] == 0) and np.all(np.isfinite(out[T:]))


# torch runs in a child process: a process that has loaded the HIP library must not import torch as well (a second HIP runtime in
# one address space aborts at exit; tests/test_oracle_layernorm.py)
_TORCH_CHECK = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import rope_oracle as RO
import window_oracle as WO

def rnd(seed, shape, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).random(shape) * (hi - lo) + lo

B, S, d, H = 2, 9, 16, 4
dh = d // H
n = 0
for Hkv in (4, 2, 1):
    for use_rope in (False, True):
        for W in (1, 3, 8, 9):
            dkv, G = dh * Hkv, H // Hkv
            x, g = rnd(0, (B * S, d)), rnd(9, (B * S, d))
            ws = [rnd(1, (d, d)), rnd(2, (dkv, d)), rnd(3, (dkv, d)), rnd(4, (d, d))]
            bs = [rnd(5, (d,)), rnd(6, (dkv,)), rnd(7, (dkv,)), rnd(8, (d,))]
            ro = RO.make(32, dh) if use_rope else None
            out, grads = WO.mha_forward_backward(x, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], ws[3], bs[3], H, Hkv, B, 0.0,
                                                 np.ones((B * H, S, S)), g, W, rope=ro)
            assert np.abs(out - WO.mha_forward(x, ws, bs, H, Hkv, B, W, rope=ro)).max() <= 1e-12
            tx = torch.tensor(x, requires_grad=True)
            tw = [torch.tensor(w, requires_grad=True) for w in ws]
            tb = [torch.tensor(b, requires_grad=True) for b in bs]

            def rot(t, nh):                                              # (B*S, nh*dh), pairs (j, j + dh/2), position = row % S
                if ro is None:
                    return t
                tab = torch.tensor(ro.table[:S]).repeat(B, 1, 1)         # (B*S, dh/2, 2)
                c, s = tab[:, None, :, 0], tab[:, None, :, 1]
                th = t.reshape(B * S, nh, dh)
                x1, x2 = th[:, :, :dh // 2], th[:, :, dh // 2:]
                return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=2).reshape(B * S, nh * dh)

            q, k, v = (tx @ tw[i].T + tb[i] for i in range(3))
            qh = rot(q, H).reshape(B, S, H, dh).permute(0, 2, 1, 3)
            kh = rot(k, Hkv).reshape(B, S, Hkv, dh).permute(0, 2, 1, 3).repeat_interleave(G, dim=1)
            vh = v.reshape(B, S, Hkv, dh).permute(0, 2, 1, 3).repeat_interleave(G, dim=1)
            r, c = torch.arange(S)[:, None], torch.arange(S)[None, :]
            band = torch.where((c <= r) & (c > r - W), 0.0, -np.inf).to(torch.float64)     # its own statement of the band
            sc = qh @ kh.transpose(2, 3) / np.sqrt(dh) + band
            ctx = (torch.softmax(sc, dim=3) @ vh).permute(0, 2, 1, 3).reshape(B * S, d)
            y = ctx @ tw[3].T + tb[3]
            y.backward(torch.tensor(g))
            assert np.abs(out - y.detach().numpy()).max() <= 1e-9
            assert np.abs(grads["x"] - tx.grad.numpy()).max() <= 1e-9
            for i, nme in enumerate("qkvo"):
                assert np.abs(grads["w" + nme] - tw[i].grad.numpy()).max() <= 1e-9, (Hkv, use_rope, W, nme)
                assert np.abs(grads["b" + nme] - tb[i].grad.numpy()).max() <= 1e-9, (Hkv, use_rope, W, nme)
            n += 1
print("cases", n)
"""


def test_torch_autograd_pins_the_banded_module():
    """B = 2, S = 9, dh = 4 in f64; Hkv in (4, 2, 1) of 4 heads, rope on and off, W in (1, 3, 8, 9): the output, dx and all eight
    parameter gradients against torch autograd of the same composition, to 1e-9"""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _TORCH_CHECK, tests, os.path.dirname(tests)], capture_output=True, text=True)
    assert r.returncode == 0 and "cases 24" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("C", [1, 2, 3, 8, 128, 256, 512])
def test_the_workspace_bound_is_the_most_chunks_a_window_touches(C):
    """Chunk c covers positions [cC, cC + C).  Over every lo and every window length 1 .. W, the count of chunks touched never
    exceeds (W + C - 2) / C + 1, and some lo reaches it."""
    for W in sorted({1, 2, 3, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 3, 3 * C + 1} - {0, -1}):
        bound = WO.chunk_bound(W, C)
        worst = 0
        for lo in range(0, 2 * C + 1):
            for length in {1, W // 2 or 1, W}:
                n = lo + length
                touched = len({p // C for p in range(lo, n)})
                assert touched == (n - 1) // C - lo // C + 1 <= bound, (W, C, lo, length)
                worst = max(worst, touched)
        assert worst == bound, (W, C, worst, bound)

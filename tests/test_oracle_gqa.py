"""The grouped-query oracle (tests/gqa_oracle.py) pinned without a GPU: the repeat form against a direct `h // G` loop; kv_heads == heads
equals the multi-head oracle exactly; torch's f64 autograd with `repeat_interleave` pins the module's forward and every parameter
gradient to 1e-9; stepping token by token reproduces the rows of the full causal oracle; the f32 ordered sum is the device's order."""
import numpy as np
import pytest

import decode_oracle as DO
import gqa_oracle as GO
import rope_oracle as RO


def rnd(seed, shape, lo=-1.0, hi=1.0):
    a = np.random.default_rng(seed).random(shape, dtype=np.float32)
    return np.asarray(a * np.float32(hi - lo) + np.float32(lo), dtype=np.float32)


def _weights(seed, d, dkv, dt=np.float64):
    outs = (d, dkv, dkv, d)
    W = [(rnd(seed + i, (outs[i], d)) / np.float32(np.sqrt(d))).astype(dt) for i in range(4)]
    Bs = [rnd(seed + 10 + i, (outs[i],)).astype(dt) for i in range(4)]
    return W, Bs


def test_repeat_kv_and_its_backward():
    rows, Hkv, G, dh = 3, 2, 3, 4
    x = rnd(1, (rows, Hkv * dh))
    y = GO.repeat_kv(x, Hkv, G, dh)
    for k in range(Hkv):
        for j in range(G):
            assert np.array_equal(y[:, (k * G + j) * dh:(k * G + j + 1) * dh], x[:, k * dh:(k + 1) * dh])
    g = rnd(2, (rows, Hkv * G * dh))
    s64, s32 = GO.repeat_kv_backward(g.astype(np.float64), Hkv, G, dh), GO.repeat_kv_backward_f32(g, Hkv, G, dh)
    for k in range(Hkv):
        want = sum(g[:, (k * G + j) * dh:(k * G + j + 1) * dh].astype(np.float64) for j in range(G))
        assert np.abs(s64[:, k * dh:(k + 1) * dh] - want).max() <= 1e-15
        acc = g[:, k * G * dh:(k * G + 1) * dh].copy()                   # ((g_0 + g_1) + g_2), every addition rounded to f32
        for j in range(1, G):
            acc = (acc + g[:, (k * G + j) * dh:(k * G + j + 1) * dh]).astype(np.float32)
        assert np.array_equal(s32[:, k * dh:(k + 1) * dh], acc)
    assert s32.dtype == np.float32 and np.abs(s32 - s64).max() <= G * G * 2.0 ** -24   # G - 1 roundings of partial sums below G
    assert np.array_equal(GO.repeat_kv(x, Hkv, 1, dh), x) and np.array_equal(GO.repeat_kv_backward_f32(x, Hkv, 1, dh), x)
    # <repeat(x), g> == <x, backward(g)>: the two are adjoint
    assert abs(np.sum(y.astype(np.float64) * g) - np.sum(x.astype(np.float64) * s64)) <= 1e-12


@pytest.mark.parametrize("B,T,H,Hkv,dh", [(2, 1, 4, 2, 8), (1, 3, 6, 1, 5), (2, 2, 3, 3, 4)])
def test_decode_repeat_form_equals_the_direct_loop(B, T, H, Hkv, dh):
    cap, G = 13, H // Hkv
    start = np.array([9, 4][:B])
    kc, vc = (rnd(s, (B, Hkv, cap, dh)).astype(np.float64) for s in (1, 2))
    kc[:, :, 12:], vc[:, :, 12:] = np.nan, np.nan                        # past every length: never read
    q = rnd(3, (B * T, H * dh)).astype(np.float64)
    got = GO.decode_forward_gqa(q, kc, vc, start, T, H)
    want = np.zeros_like(got)
    scale = 1.0 / np.sqrt(dh)
    for b in range(B):
        for t in range(T):
            n = min(int(start[b]) + t + 1, cap)
            for h in range(H):
                s = kc[b, h // G, :n] @ q[b * T + t, h * dh:(h + 1) * dh] * scale
                p = np.exp(s - s.max())
                want[b * T + t, h * dh:(h + 1) * dh] = (p / p.sum()) @ vc[b, h // G, :n]
    assert np.all(np.isfinite(got)) and np.abs(got - want).max() <= 2e-15
    if Hkv == H:
        assert np.array_equal(got, DO.decode_forward(q, kc, vc, start, T))


@pytest.mark.parametrize("use_rope", [False, True])
def test_kv_heads_equal_to_heads_is_the_multi_head_oracle(use_rope):
    B, S, H, dh = 2, 9, 3, 4
    d = H * dh
    W, Bs = _weights(1, d, d)
    x, g = rnd(2, (B * S, d)).astype(np.float64), rnd(3, (B * S, d)).astype(np.float64)
    rope = RO.make(16, dh) if use_rope else None
    noise = np.ones((B * H, S, S))
    a = GO.mha_forward_backward(x, W[0], Bs[0], W[1], Bs[1], W[2], Bs[2], W[3], Bs[3], H, H, B, 0.0, noise, g, causal=True, rope=rope)
    b = RO.mha_forward_backward(x, W[0], Bs[0], W[1], Bs[1], W[2], Bs[2], W[3], Bs[3], H, B, 0.0, noise, g, causal=True, rope=rope)
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in b[1])


# torch runs in a child process: a process that has loaded the HIP library must not import torch as well (a second HIP runtime in
# one address space aborts at exit; tests/test_oracle_layernorm.py)
_TORCH_CHECK = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import gqa_oracle as GO
import rope_oracle as RO

def rnd(seed, shape, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).random(shape) * (hi - lo) + lo

B, S, dh = 2, 7, 4
n = 0
for H, Hkv in ((4, 2), (4, 1), (6, 3)):
    for use_rope in (False, True):
        for causal in (True, False):
            d, dkv, G = H * dh, Hkv * dh, H // Hkv
            outs = (d, dkv, dkv, d)
            W = [rnd(4 + i, (outs[i], d)) / np.sqrt(d) for i in range(4)]
            Bs = [rnd(14 + i, (outs[i],)) for i in range(4)]
            x, g = rnd(5, (B * S, d)), rnd(6, (B * S, d))
            rope = RO.make(16, dh) if use_rope else None
            out, grads = GO.mha_forward_backward(x, W[0], Bs[0], W[1], Bs[1], W[2], Bs[2], W[3], Bs[3], H, Hkv, B, 0.0,
                                                 np.ones((B * H, S, S)), g, causal=causal, rope=rope)
            tx = torch.tensor(x, requires_grad=True)
            tW = [torch.tensor(w, requires_grad=True) for w in W]
            tB = [torch.tensor(b, requires_grad=True) for b in Bs]

            def rot(t, nh):                                              # (B*S, nh*dh), pairs (j, j + dh/2), position = row % S
                if rope is None:
                    return t
                tab = torch.tensor(rope.table[:S]).repeat(B, 1, 1)       # (B*S, dh/2, 2)
                c, s = tab[:, None, :, 0], tab[:, None, :, 1]
                th = t.reshape(B * S, nh, dh)
                x1, x2 = th[..., :dh // 2], th[..., dh // 2:]
                return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).reshape(B * S, nh * dh)

            q = rot(tx @ tW[0].T + tB[0], H).reshape(B, S, H, dh).transpose(1, 2)
            k = rot(tx @ tW[1].T + tB[1], Hkv).reshape(B, S, Hkv, dh).transpose(1, 2).repeat_interleave(G, dim=1)
            v = (tx @ tW[2].T + tB[2]).reshape(B, S, Hkv, dh).transpose(1, 2).repeat_interleave(G, dim=1)
            sc = q @ k.transpose(-1, -2) / np.sqrt(dh)
            if causal:
                sc = sc + torch.triu(torch.full((S, S), -np.inf, dtype=torch.float64), 1)
            o = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B * S, d)
            y = o @ tW[3].T + tB[3]
            y.backward(torch.tensor(g))
            assert np.abs(out - y.detach().numpy()).max() <= 1e-9
            assert np.abs(grads["x"] - tx.grad.numpy()).max() <= 1e-9
            for i, nme in enumerate("qkvo"):
                assert np.abs(grads["w" + nme] - tW[i].grad.numpy()).max() <= 1e-9, (H, Hkv, use_rope, causal, nme)
                assert np.abs(grads["b" + nme] - tB[i].grad.numpy()).max() <= 1e-9, (H, Hkv, use_rope, causal, nme)
            n += 1
print("cases", n)
"""


def test_torch_autograd_pins_the_module():
    """B = 2, S = 7, dh = 4 in f64; (H, Hkv) in (4, 2), (4, 1), (6, 3), rope on and off, causal and not: the output, dx and all
    eight parameter gradients against torch autograd with `repeat_interleave` to 1e-9"""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _TORCH_CHECK, tests, os.path.dirname(tests)], capture_output=True, text=True)
    assert r.returncode == 0 and "cases 12" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("use_rope", [False, True])
@pytest.mark.parametrize("slices", [[1] * 11, [5, 3, 1, 1, 1], [11]])
def test_stepping_reproduces_the_full_causal_oracle(slices, use_rope):
    B, S, H, Hkv, dh = 2, 11, 4, 2, 6
    d, dkv = H * dh, Hkv * dh
    W, Bs = _weights(7, d, dkv)
    x = rnd(8, (B * S, d)).astype(np.float64)
    rope = RO.make(16, dh) if use_rope else None
    want = GO.mha_forward(x, W, Bs, H, Hkv, B, causal=True, rope=rope)
    kc, vc = DO.new_cache(B, Hkv, S, dh, np.float64, fill=np.nan)
    start, got = np.zeros(B, dtype=np.int64), np.zeros_like(want)
    for T in slices:
        lo = int(start[0])
        rows = np.concatenate([x[b * S + lo:b * S + lo + T] for b in range(B)])
        out, start = GO.mha_step(rows, W, Bs, H, Hkv, kc, vc, start, T, rope=rope)
        for b in range(B):
            got[b * S + lo:b * S + lo + T] = out[b * T:(b + 1) * T]
    assert np.all(start == S) and np.all(np.isfinite(got))
    assert np.abs(got - want).max() <= 1e-12

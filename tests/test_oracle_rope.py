"""The rotary oracle (tests/rope_oracle.py) pinned without a GPU, in f64: it is the complex multiplication (x1 + i x2) exp(i p theta_j)
to 1e-12; orthogonal; the identity at position 0; the attention output of the decode oracle depends on position differences only
(1e-10); the module backward agrees with torch autograd to 1e-9; stepping token by token reproduces the rows of the full causal
forward."""
import numpy as np
import pytest

import decode_oracle as DO
import rope_oracle as RO


def rnd(seed, shape, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).random(shape) * (hi - lo) + lo


CASES = [(8, 8, False), (8, 8, True), (6, 6, False), (10, 4, True), (5, 4, False), (2, 2, False), (64, 32, False)]


@pytest.mark.parametrize("dh,rot,il", CASES)
def test_it_is_a_complex_multiplication(dh, rot, il):
    B, T, H, base, max_pos = 3, 5, 2, 10000.0, 200
    start = np.array([0, 9, 130])
    x = rnd(1, (B * T, H * dh + 3))                                      # three columns past the heads: never touched
    got = RO.rope(x, start, T, H, dh, rot, il, RO.table(max_pos, rot, base))
    want = x.copy()
    for b in range(B):
        for t in range(T):
            p = int(start[b]) + t
            for h in range(H):
                for j in range(rot // 2):
                    c1, c2 = (2 * j, 2 * j + 1) if il else (j, j + rot // 2)
                    z = complex(x[b * T + t, h * dh + c1], x[b * T + t, h * dh + c2]) * np.exp(1j * p * base ** (-2.0 * j / rot))
                    want[b * T + t, h * dh + c1], want[b * T + t, h * dh + c2] = z.real, z.imag
    assert np.abs(got - want).max() <= 1e-12
    assert np.array_equal(got[:, H * dh:], x[:, H * dh:])
    for h in range(H):
        assert np.array_equal(got[:, h * dh + rot:(h + 1) * dh], x[:, h * dh + rot:(h + 1) * dh])      # pass-through columns


@pytest.mark.parametrize("dh,rot,il", CASES)
def test_orthogonal_and_identity_at_position_zero(dh, rot, il):
    B, T, H = 2, 7, 3
    tab = RO.table(64, rot)
    x = rnd(2, (B * T, H * dh))
    y = RO.rope(x, [3, 40], T, H, dh, rot, il, tab)
    assert np.abs(RO.rope(y, [3, 40], T, H, dh, rot, il, tab, inverse=True) - x).max() <= 1e-12
    assert np.abs(np.linalg.norm(y.reshape(-1, dh), axis=1) - np.linalg.norm(x.reshape(-1, dh), axis=1)).max() <= 1e-12
    one = RO.rope(x[:B], None, 1, H, dh, rot, il, tab)                   # T = 1, start NULL: every row at position 0
    assert np.array_equal(one, x[:B])
    # <R g, x> == <g, R^T x>: `inverse` is the transpose
    g = rnd(3, x.shape)
    assert abs(np.sum(RO.rope(x, [3, 40], T, H, dh, rot, il, tab) * g) - np.sum(x * RO.rope(g, [3, 40], T, H, dh, rot, il, tab, inverse=True))) <= 1e-12


def test_positions_are_clamped_and_the_dtype_is_the_callers():
    tab = RO.table(16, 4)
    x = rnd(4, (4, 4))
    lo = RO.rope(x[:2], [-5], 2, 1, 4, 4, False, tab)                    # positions -5, -4 -> 0, 0
    assert np.array_equal(lo, x[:2])
    hi = RO.rope(x[:2], [15], 2, 1, 4, 4, False, tab)                    # positions 15, 16 -> 15, 15
    assert np.array_equal(hi[1], RO.rope(x[1:2], [15], 1, 1, 4, 4, False, tab)[0])
    assert RO.rope(x.astype(np.float32), None, 4, 1, 4, 4, False, tab).dtype == np.float32
    assert list(RO.positions([0, 9, 130], 3, 2, 131)) == [0, 1, 9, 10, 130, 130]


def _module(seed, B, S, d):
    x = rnd(seed, (B * S, d))
    W = [rnd(seed + 1 + i, (d, d), -0.5, 0.5) for i in range(4)]
    Bs = [rnd(seed + 5 + i, (d,), -0.5, 0.5) for i in range(4)]
    return x, W, Bs


@pytest.mark.parametrize("il", [False, True])
def test_relative_position_property(il):
    """Adding a constant to every start leaves the attention output unchanged: scores depend on position differences only."""
    B, H, dh, cap, T = 2, 2, 8, 64, 3
    d = H * dh
    r = RO.make(cap, dh, dh, il)
    _, W, Bs = _module(99, B, T, d)
    outs = []
    for shift in (0, 17):
        # the cache itself starts at 0 in both runs; only the POSITIONS the rows are rotated at move by `shift`
        kc, vc = DO.new_cache(B, H, cap, dh, np.float64, fill=np.nan)
        held, got = np.array([0, 0]), []
        for step in range(4):
            x = rnd(10 + step, (B * T, d))
            q, k, v = (RO.O.linear_forward(x, W[i], Bs[i]) for i in range(3))
            q, k = (RO.rope(t, held + shift, T, H, dh, r.rot, r.interleaved, r.table) for t in (q, k))
            ctx, held = DO.step(q, k, v, kc, vc, held, T)
            got.append(ctx)
        outs.append(np.concatenate(got))
    assert np.all(np.isfinite(outs[0]))
    assert np.abs(outs[0] - outs[1]).max() <= 1e-10


# torch runs in a child process: a process that has loaded the HIP library must not import torch as well (a second HIP runtime in
# one address space aborts at exit; tests/test_oracle_layernorm.py)
_TORCH_CHECK = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import rope_oracle as RO

def rnd(seed, shape, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).random(shape) * (hi - lo) + lo

B, S, d, H = 2, 7, 16, 2
dh = d // H
n = 0
for causal in (True, False):
    for rot, il in ((8, False), (8, True), (4, False)):
        x = rnd(20, (B * S, d))
        W = [rnd(21 + i, (d, d), -0.5, 0.5) for i in range(4)]
        Bs = [rnd(25 + i, (d,), -0.5, 0.5) for i in range(4)]
        g = rnd(30, (B * S, d))
        r = RO.make(S, dh, rot, il)
        out, grads = RO.mha_forward_backward(x, W[0], Bs[0], W[1], Bs[1], W[2], Bs[2], W[3], Bs[3], H, B, 0.0, np.ones((B * H, S, S)), g,
                                             causal=causal, rope=r)
        tx = torch.tensor(x, requires_grad=True)
        tW = [torch.tensor(w, requires_grad=True) for w in W]
        tB = [torch.tensor(b, requires_grad=True) for b in Bs]
        cos, sin = torch.tensor(r.table[:S, :, 0]), torch.tensor(r.table[:S, :, 1])        # (S, rot/2)

        def rotate(t):                                                   # (B, S, H, dh), written independently of the oracle
            head, tail = t[..., :rot], t[..., rot:]
            a, b = (head[..., 0::2], head[..., 1::2]) if il else (head[..., :rot // 2], head[..., rot // 2:])
            c, s = cos[None, :, None, :], sin[None, :, None, :]
            ya, yb = a * c - b * s, b * c + a * s
            yh = torch.stack([ya, yb], dim=-1).flatten(-2) if il else torch.cat([ya, yb], dim=-1)
            return torch.cat([yh, tail], dim=-1)

        q, k, v = ((tx @ tW[i].T + tB[i]).reshape(B, S, H, dh) for i in range(3))
        q, k = rotate(q), rotate(k)
        sc = torch.einsum("bqhd,bkhd->bhqk", q, k) / np.sqrt(dh)
        if causal:
            sc = sc + torch.triu(torch.full((S, S), -np.inf, dtype=torch.float64), 1)
        ctx = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(sc, dim=-1), v).reshape(B * S, d)
        tout = ctx @ tW[3].T + tB[3]
        tout.backward(torch.tensor(g))
        assert np.abs(out - tout.detach().numpy()).max() <= 1e-9
        want = dict(x=tx.grad, wq=tW[0].grad, wk=tW[1].grad, wv=tW[2].grad, wo=tW[3].grad, bq=tB[0].grad, bk=tB[1].grad, bv=tB[2].grad,
                    bo=tB[3].grad)
        for name, t in want.items():
            assert np.abs(grads[name] - t.numpy()).max() <= 1e-9, (causal, rot, il, name)
        n += 1
print("cases", n)
"""


def test_module_backward_against_torch_autograd():
    """B = 2, S = 7, d = 16, H = 2 in f64, causal and not, both pairings and a partial rotation: output and all nine gradients to 1e-9"""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _TORCH_CHECK, tests, os.path.dirname(tests)], capture_output=True, text=True)
    assert r.returncode == 0 and "cases 6" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("il", [False, True])
@pytest.mark.parametrize("slices", ["tokens", "prefill+tokens"])
def test_stepping_reproduces_the_full_causal_forward(il, slices):
    B, S, d, H = 2, 9, 16, 2
    dh = d // H
    x, W, Bs = _module(40, B, S, d)
    r = RO.make(S, dh, dh, il)
    want, _ = RO.mha_forward_backward(x, W[0], Bs[0], W[1], Bs[1], W[2], Bs[2], W[3], Bs[3], H, B, 0.0, np.ones((B * H, S, S)),
                                      np.zeros((B * S, d)), causal=True, rope=r)
    kc, vc = DO.new_cache(B, H, S, dh, np.float64, fill=np.nan)
    sizes = [1] * S if slices == "tokens" else [4] + [1] * (S - 4)
    start, got = np.zeros(B, dtype=np.int64), np.zeros_like(want)
    for T in sizes:
        lo = int(start[0])
        xs = np.concatenate([x[b * S + lo:b * S + lo + T] for b in range(B)])
        y, start = RO.mha_step(xs, W, Bs, H, kc, vc, start, T, rope=r)
        for b in range(B):
            got[b * S + lo:b * S + lo + T] = y[b * T:(b + 1) * T]
    assert np.abs(got - want).max() <= 1e-12
    # without a rotary description both are the functions they wrap
    y0, _ = RO.mha_step(x[:B], W, Bs, H, *DO.new_cache(B, H, S, dh, np.float64), np.zeros(B, dtype=np.int64), 1)
    y1, _ = DO.mha_step(x[:B], W, Bs, H, *DO.new_cache(B, H, S, dh, np.float64), np.zeros(B, dtype=np.int64), 1)
    assert np.array_equal(y0, y1)

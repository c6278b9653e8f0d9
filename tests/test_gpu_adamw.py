"""nk_adamw_step_multi / nk_adamw_step / nk_clip_grad_norm_multi through the C ABI: a size and alignment grid (lengths 0, 1, 3, 4095,
4096, 4097, 1 Mi + 5; pointers on a 16-byte boundary and one float past it), more parameters than one launch's table holds, values
against tests/adamw_oracle.py inside the bound of optim_trajectory.check, the norm against the f64 norm at ELEMENTWISE_RTOL, the
status codes, non-finite gradients, and capture.  Bit-identity is asserted between device runs only: one call against one call per
parameter, aligned against offset buffers, a run against its rerun, a replay against the eager call."""
import ctypes

import numpy as np
import pytest

import adamw_oracle as A
import optim_trajectory as T
from oracle import neuronika_oracle as O
from tolerance import ELEMENTWISE_RTOL

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = (0, 1, 3, 4095, 4096, 4097, (1 << 20) + 5)
GUARD, SENTINEL = 8, 0x7FC0BEEF
# 7 sizes of the grid + 33 short ones: 39 non-empty entries, more than the 32 of one launch's table
LIST = SIZES + tuple(5 + 37 * k for k in range(33))
HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1)


def capi():
    from neuronika_amd import capi as c
    return c


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Buf:
    """`n` floats holding `init`, `off` floats past a 16-byte boundary, between two sentinel runs; n == 0 keeps a valid pointer"""

    def __init__(self, dev, init, off=0):
        init = np.ascontiguousarray(init, f32).reshape(-1)
        self.n, self.first = init.size, GUARD + off
        host = np.full(self.first + self.n + GUARD, SENTINEL, np.uint32)
        host[self.first:self.first + self.n] = bits(init)
        self.base = dev.array(host.view(f32))
        self.v = self.base.view_offset(self.first)
        self.v.shape, self.v.size = (self.n,), self.n

    def read(self):
        host = bits(self.base.numpy())
        assert (host[:self.first] == SENTINEL).all(), "cells BEFORE the buffer were written"
        assert (host[self.first + self.n:] == SENTINEL).all(), "cells AFTER the buffer were written"
        return host[self.first:self.first + self.n].view(f32).copy()


def host_state(sizes, seed=0):
    """per parameter (w, g, m, v, vmax): weights and gradients in [-1, 1), m small, v and vmax positive"""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        w, g = (rng.random(n, dtype=f32) * f32(2) - f32(1) for _ in range(2))
        m = (rng.random(n, dtype=f32) - f32(0.5)) * f32(0.2)
        v, vmax = rng.random(n, dtype=f32) * f32(0.1), rng.random(n, dtype=f32) * f32(0.1)
        out.append((w, g, m, v, vmax))
    return out


def upload(dev, host, off):
    return [tuple(Buf(dev, a, off) for a in p) for p in host]


def steps_of(sizes):
    return [1 + (3 * k) % 7 for k in range(len(sizes))]                       # the step number differs inside one launch


def run_multi(dev, bufs, amsgrad, steps, **kw):
    c = capi()
    c.adamw_step_multi(dev, [p[0].v for p in bufs], [p[1].v for p in bufs], [p[2].v for p in bufs], [p[3].v for p in bufs],
                       [p[4].v for p in bufs] if amsgrad else None, steps=steps, **kw)


def run_each(dev, bufs, amsgrad, steps, **kw):
    c = capi()
    for p, k in zip(bufs, steps):
        c.adamw_step(dev, p[0].v, p[1].v, p[2].v, p[3].v, p[4].v if amsgrad else None, step=k, **kw)


def read_all(bufs):
    return [tuple(b.read() for b in p) for p in bufs]


@pytest.mark.parametrize("amsgrad", [False, True], ids=["adamw", "amsgrad"])
def test_adamw_grid(dev, amsgrad):
    host, steps = host_state(LIST), steps_of(LIST)
    runs = {}
    for name, launch, off in (("multi", run_multi, 0), ("multi_offset", run_multi, 1), ("each", run_each, 0), ("each_offset", run_each, 1),
                              ("rerun", run_multi, 0)):
        bufs = upload(dev, host, off)
        launch(dev, bufs, amsgrad, steps, **HYPER)
        runs[name] = read_all(bufs)
    worst = 0.0
    for k, (n, h) in enumerate(zip(LIST, host)):
        ref = []
        for dt in (f32, np.float64):
            w, g, m, v, vmax = (a.astype(dt) for a in h)
            if n:
                A.adamw_step(w, g, m, v, HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], steps[k], HYPER["weight_decay"],
                             vmax if amsgrad else None)
            ref.append((w, g, m, v, vmax))
        got = runs["multi"][k]
        for j, what in enumerate(("w", "g", "m", "v", "vmax")):
            for other in ("multi_offset", "each", "each_offset", "rerun"):
                assert same_bits(got[j], runs[other][k][j]), (n, what, other)
            if n:
                worst = max(worst, T.check(f"adamw_grid/{what}", got[j], ref[0][j], ref[1][j]))
        assert same_bits(got[1], h[1])                                            # the gradient is read, never written
        if not amsgrad:
            assert same_bits(got[4], h[4])
    print(f"adamw grid (amsgrad={amsgrad}): worst err / bound = {worst:.3f}")


def test_weight_decay_zero_is_adam(dev):
    """weight_decay = 0 against nk_adam_step without a penalty: both inside the oracle's bound; whether the bits agree is reported"""
    c = capi()
    sizes = (3, 4096, 4097, 70001)
    host = host_state(sizes, 3)
    kw = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)
    for amsgrad in (False, True):
        a, b = upload(dev, host, 0), upload(dev, host, 0)
        run_multi(dev, a, amsgrad, [4] * len(sizes), weight_decay=0.0, **kw)
        for p in b:
            c.adam_step(dev, p[0].v, p[1].v, p[2].v, p[3].v, p[4].v if amsgrad else None, step=4, **kw)
        equal = True
        for h, pa, pb in zip(host, read_all(a), read_all(b)):
            ref = []
            for dt in (f32, np.float64):
                w, g, m, v, vmax = (x.astype(dt) for x in h)
                O.adam_step(w, g, m, v, kw["lr"], kw["beta1"], kw["beta2"], kw["eps"], 4, vmax if amsgrad else None)
                ref.append((w, g, m, v, vmax))
            for j in (0, 2, 3, 4):
                T.check("adamw_decay0/adamw", pa[j], ref[0][j], ref[1][j])
                T.check("adamw_decay0/adam", pb[j], ref[0][j], ref[1][j])
                equal = equal and same_bits(pa[j], pb[j])
        print(f"weight_decay = 0 against nk_adam_step (amsgrad={amsgrad}): bits {'agree' if equal else 'differ'}")


def clip_call(dev, grads_host, max_norm, off):
    c = capi()
    bufs = [Buf(dev, g, off) for g in grads_host]
    out = Buf(dev, np.full(2, 7.0, f32))
    c.clip_grad_norm_multi(dev, [b.v for b in bufs], max_norm, out.v)
    return [b.read() for b in bufs], out.read()


@pytest.mark.parametrize("scale,max_norm", [(1.0, 20.0), (1.0, 1e6), (1.0, float("inf")), (1e-3, 0.25)],
                         ids=["clipped", "unclipped", "measure_only", "small_clipped"])
def test_clip_grid(dev, scale, max_norm):
    rng = np.random.default_rng(5)
    grads = [(rng.standard_normal(n, dtype=f32) * f32(scale)).astype(f32) for n in LIST]
    got, out = clip_call(dev, grads, max_norm, 0)
    for off, what in ((1, "offset"), (0, "rerun")):
        got2, out2 = clip_call(dev, grads, max_norm, off)
        assert same_bits(out, out2), what
        assert all(same_bits(a, b) for a, b in zip(got, got2)), what
    g32, g64 = [g.copy() for g in grads], [g.astype(np.float64) for g in grads]
    norm32, coef32 = A.clip_grad_norm(g32, max_norm)
    A.clip_grad_norm(g64, max_norm)
    norm64 = np.sqrt(sum(float(np.dot(g.astype(np.float64), g.astype(np.float64))) for g in grads))
    print(f"total_norm: device {out[0]!r}, f64 {norm64!r}; coef: device {out[1]!r}, oracle {coef32!r}")
    assert abs(float(out[0]) - norm64) <= ELEMENTWISE_RTOL * norm64
    assert abs(float(out[1]) - float(coef32)) <= ELEMENTWISE_RTOL * float(coef32)
    assert (out[1] < 1) == (norm64 > max_norm)
    if out[1] == 1:
        assert all(same_bits(a, b) for a, b in zip(got, grads))                  # coef == 1: the bits are untouched
    else:
        worst = max(T.check("clip_grid/grad", a, b, c) for a, b, c, n in zip(got, g32, g64, LIST) if n)
        print(f"scaled gradients: worst err / bound = {worst:.3f}")


def test_clip_leaves_special_bit_patterns_alone_when_nothing_is_clipped(dev):
    g = np.array([0.0, -0.0, 1e-40, -1e-40, 1.5, -2.5], f32)                      # zeros of both signs, subnormals
    got, out = clip_call(dev, [g, np.tile(g, 1000)], 1e3, 0)
    assert out[1] == 1 and same_bits(got[0], g) and same_bits(got[1], np.tile(g, 1000))


def _raises_invalid(fn):
    c = capi()
    with pytest.raises(c.NeuronikaHipError) as e:
        fn()
    assert e.value.code == 1, e.value                                            # NK_ERR_INVALID


def test_status_codes(dev):
    c = capi()
    L = c.lib
    host = host_state((5, 4097, 0, 9))
    bufs = upload(dev, host, 0)
    out = Buf(dev, np.full(2, 7.0, f32))
    # nothing to do: count == 0 (null tables allowed), all lengths 0
    c.check(L.nk_adamw_step_multi(dev.h, 0, None, None, None, None, None, None, None, 0.1, 0.9, 0.999, 1e-8, 0.0))
    c.check(L.nk_clip_grad_norm_multi(dev.h, 0, None, None, 1.0, out.v.p))
    assert out.read().tolist() == [0.0, 1.0]
    empty = [Buf(dev, np.zeros(0, f32)) for _ in range(3)]
    out = Buf(dev, np.full(2, 7.0, f32))
    c.clip_grad_norm_multi(dev, [b.v for b in empty], 2.0, out.v)
    assert out.read().tolist() == [0.0, 1.0]
    # refusals
    _raises_invalid(lambda: c.check(L.nk_adamw_step_multi(dev.h, 2, None, None, None, None, None, None, None, 0.1, 0.9, 0.999, 1e-8, 0.0)))
    _raises_invalid(lambda: c.check(L.nk_clip_grad_norm_multi(dev.h, 2, None, None, 1.0, out.v.p)))
    _raises_invalid(lambda: c.check(L.nk_clip_grad_norm_multi(dev.h, 0, None, None, 1.0, None)))
    _raises_invalid(lambda: run_multi(dev, bufs, True, [1, 0, 1, 1], **HYPER))                   # step < 1
    _raises_invalid(lambda: run_multi(dev, bufs + [bufs[1]], True, [1] * 5, **HYPER))            # the same w twice
    for bad in (float("nan"), 0.0, -1.0, float("-inf")):
        _raises_invalid(lambda: c.clip_grad_norm_multi(dev, [p[1].v for p in bufs], bad, out.v))
    _raises_invalid(lambda: c.clip_grad_norm_multi(dev, [p[1].v for p in bufs] + [bufs[0][1].v], 1.0, out.v))   # the same grad twice
    # a refused call wrote nothing
    for h, p in zip(host, read_all(bufs)):
        assert all(same_bits(a, b) for a, b in zip(h, p))
    assert out.read().tolist() == [0.0, 1.0]


def test_nan_gradient_poisons_norm_coefficient_and_gradients(dev):
    rng = np.random.default_rng(6)
    grads = [rng.standard_normal(n, dtype=f32) for n in (7, 4096, 5000, 3)]
    grads[2][4321] = np.nan
    got, out = clip_call(dev, grads, 1.0, 0)
    assert np.isnan(out).all()
    assert all(np.isnan(g).all() for g in got)


def test_adamw_refuses_capture_and_a_captured_clip_replays_the_eager_bits(dev):
    c = capi()
    rng = np.random.default_rng(8)
    grads = [rng.standard_normal(n, dtype=f32) for n in LIST]
    eager, eager_out = clip_call(dev, grads, 20.0, 0)                             # (also the eager call that sizes the workspace)
    bufs = [Buf(dev, g) for g in grads]
    out = Buf(dev, np.full(2, 7.0, f32))
    host = host_state((5, 4097))
    params = upload(dev, host, 0)
    gh = ctypes.c_void_p()
    dev.sync()
    c.check(c.lib.nk_graph_begin(dev.h))
    try:
        c.clip_grad_norm_multi(dev, [b.v for b in bufs], 20.0, out.v)
        with pytest.raises(c.NeuronikaHipError, match="captured") as e:
            run_multi(dev, params, False, [1, 1], **HYPER)
        assert e.value.code == 1
        with pytest.raises(c.NeuronikaHipError, match="captured"):
            c.adamw_step(dev, params[0][0].v, params[0][1].v, params[0][2].v, params[0][3].v, None, step=1, **HYPER)
    finally:
        c.check(c.lib.nk_graph_end(dev.h, ctypes.byref(gh)))
    dev.sync()
    assert all(same_bits(b.read(), g) for b, g in zip(bufs, grads))               # recorded, not run
    c.check(c.lib.nk_graph_launch(gh)); dev.sync()
    replayed, replayed_out = [b.read() for b in bufs], out.read()
    c.check(c.lib.nk_graph_destroy(gh))
    assert same_bits(replayed_out, eager_out) and replayed_out[1] < 1
    assert all(same_bits(a, b) for a, b in zip(replayed, eager))
    for h, p in zip(host, read_all(params)):                                      # the refused steps wrote nothing
        assert all(same_bits(a, b) for a, b in zip(h, p))

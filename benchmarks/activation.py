"""Activation kernels, HIP events on the compute stream (warm-up, windows of at least 25 ms, the best of three), per kernel
    the time and algorithmic bytes / time,
    the ratio to `nk_copy` of the same byte count timed in the same process, alternating,
    the ratio to the SAME FUNCTION COMPOSED from the nodes the tape had before (through `_tape`, forward() and backward(1.0)):
        silu         x * x.sigmoid()
        gelu_tanh    x * 0.5 * ((x + x.pow(3) * 0.044715) * sqrt(2 / pi)).tanh() + 1)
        glu / swiglu chunks of the two halves, sigmoid, * (SwiGLU: b * b.sigmoid() for the gate)
      against the one-node form through the same tape calls, so both sides carry the same seed fill and call overhead
      (erfc GELU has no composed form: the tape has no erf node),
at
    pointwise  (65536, 4096)    1 GiB per tensor
               (8192, 4096)     the hidden tensor of a d = 1024 block at 8 x 1024 tokens, 134 MB: cache-assisted
    gated      rows 12192, H 11008   1 GiB of input
               rows 8192, H 11008    a 4096 -> 11008 SwiGLU feed-forward at 8 x 1024 tokens
    python benchmarks/activation.py [min_ms]
One JSON line per (shape, kernel).  Algorithmic bytes: forward 8 n, backward 12 n (assign) / 16 n (+=); gated forward 12 rows H,
backward 20 rows H (assign) / 28 rows H (+=).  Every shape runs in a fresh child process under its own time limit; the parent touches
no GPU and stops at the first child that fails."""
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("pointwise", 65536, 4096), ("pointwise", 8192, 4096), ("gated", 12192, 11008), ("gated", 8192, 11008)]
CHILD_LIMIT_S = 400


def child(kind, rows, cols, min_ms):
    import neuronika_amd
    from neuronika_amd import capi as c
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/activation.py needs a GPU")
    t = neuronika_amd.tape
    tdev = t.Device(0)
    dev = c.Device(handle=tdev.raw())

    def window(fn):
        e0, e1 = dev.event(), dev.event()
        e0.record(); calls = 0
        while True:
            fn(); fn(); calls += 2
            e1.record(); e1.sync()
            if e0.elapsed_ms(e1) >= min_ms:
                break
        iters = max(4, int(min_ms / max(e0.elapsed_ms(e1) / calls, 1e-3)) + 1)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); e1.sync()
        return e0.elapsed_ms(e1) / iters

    def best(fn):
        return min(window(fn) for _ in range(3))

    rng = np.random.default_rng(0)
    gated = kind == "gated"
    H = cols
    in_shape, out_shape = ((rows, 2 * H), (rows, H)) if gated else ((rows, cols), (rows, cols))
    n_in, n_out = int(np.prod(in_shape)), int(np.prod(out_shape))
    x = rng.standard_normal(in_shape, dtype=np.float32)
    x *= np.float32(2.0)
    X, DX = dev.array(x), dev.zeros(in_shape)
    g = rng.random(out_shape, dtype=np.float32)
    G, Y = dev.array(g), dev.zeros(out_shape)
    SRC, DST = dev.zeros(max(n_in, n_out) * 2), dev.zeros(max(n_in, n_out) * 2)          # the copy's operands
    shape = [rows, 2 * H] if gated else [rows, cols]

    def report(name, fn, nbytes, extra=None):
        m = nbytes // 8                                              # a copy of m floats reads and writes nbytes in all
        copy = lambda: c.check(c.lib.nk_copy(dev.h, DST.p, SRC.p, m))
        ms_k, ms_c = [], []
        for _ in range(3):
            ms_c.append(window(copy))
            ms_k.append(window(fn))
        k, cp = min(ms_k), min(ms_c)
        rate, copy_rate = nbytes / (k * 1e-3), 8 * m / (cp * 1e-3)
        row = {"bench": "activation", "shape": shape, "kernel": name, "algorithmic_bytes": nbytes, "ms": round(k, 4),
               "ms_windows": [round(v, 4) for v in ms_k], "GBps": round(rate / 1e9, 1), "copy_ms": round(cp, 4),
               "copy_GBps": round(copy_rate / 1e9, 1), "ratio_to_copy": round(rate / copy_rate, 3)}
        row.update(extra or {})
        print(json.dumps(row), flush=True)

    # ---- the same function through the tape: one node against the composition of the older nodes
    Act = t.Activation
    k_tanh = math.sqrt(2.0 / math.pi)

    # builders take the leaf and K, which records every differentiable node so that each timed backward starts from pending zero
    # fills (the first-writer forms), as a training step does
    def glu_composed(v, K, swish):
        a, b = (K(h) for h in v.chunks([rows, H]))
        s = K(b.sigmoid())
        return K(a * (K(b * s) if swish else s))

    def tanh_composed(v, K):
        u = K(K(v + K(K(v.pow(3)) * 0.044715)) * k_tanh)
        return K(K(v * 0.5) * K(K(u.tanh()) + 1.0))

    if gated:
        tape_forms = {"sigmoid": (lambda v, K: K(v.glu()), lambda v, K: glu_composed(v, K, False)),
                      "silu": (lambda v, K: K(v.glu(Act.Silu)), lambda v, K: glu_composed(v, K, True))}
    else:
        tape_forms = {"silu": (lambda v, K: K(v.silu()), lambda v, K: K(v * K(v.sigmoid()))),
                      "gelu_tanh": (lambda v, K: K(v.gelu(True)), tanh_composed)}
    composed = {}
    for act, (one, many) in tape_forms.items():
        times = {}
        for label, build in (("one_node", one), ("composed", many)):
            leaf = t.from_ndarray(tdev, x).requires_grad()
            kept = [leaf]
            out = build(leaf, lambda v: (kept.append(v), v)[1])

            def backward():
                for v in kept:
                    v.zero_grad()
                out.backward(1.0)

            out.forward(); backward()
            times[label] = (best(out.forward), best(backward), out.history_len())
            del out, leaf, kept
        composed[act] = times

    for act in ("gelu", "gelu_tanh", "silu", "sigmoid"):
        if gated:
            cases = [("glu_fwd", lambda: c.glu_fwd(dev, act, X, Y, rows, H), 12 * n_out, 0),
                     ("glu_bwd_assign", lambda: c.glu_bwd(dev, act, DX, G, X, rows, H, assign=True), 20 * n_out, 1),
                     ("glu_bwd", lambda: c.glu_bwd(dev, act, DX, G, X, rows, H), 28 * n_out, None)]
        else:
            cases = [("activation_fwd", lambda: c.activation_fwd(dev, act, X, Y), 8 * n_in, 0),
                     ("activation_bwd_assign", lambda: c.activation_bwd(dev, act, DX, G, X, assign=True), 12 * n_in, 1),
                     ("activation_bwd", lambda: c.activation_bwd(dev, act, DX, G, X), 16 * n_in, None)]
        for name, fn, nbytes, which in cases:
            extra = None
            if which is not None and act in composed:
                one, many = composed[act]["one_node"], composed[act]["composed"]
                extra = {"tape_one_node_ms": round(one[which], 4), "tape_composed_ms": round(many[which], 4),
                         "composed_nodes": many[2], "composed_over_one_node": round(many[which] / one[which], 2)}
            report("%s[%s]" % (name, act), fn, nbytes, extra)
    dev.sync()


def main():
    args = sys.argv[1:]
    if args and args[0] == "--shape":
        return child(args[1], int(args[2]), int(args[3]), float(args[4]))
    min_ms = float(args[0]) if args else 25.0
    for kind, rows, cols in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", kind, str(rows), str(cols), str(min_ms)], timeout=CHILD_LIMIT_S)
        if r.returncode != 0:
            raise SystemExit("benchmarks/activation.py: shape %s %d x %d failed with status %d; nothing further is started" % (kind, rows, cols, r.returncode))


if __name__ == "__main__":
    main()

"""Cross-entropy kernels, HIP events on the compute stream (warm-up, windows of at least 25 ms, the best of three): the fused forward
(`nk_cross_entropy_fwd`: the logits read once, loss sum and active count included) and the fused backward in the assign form
(`nk_cross_entropy_bwd_assign`: count, logits read, gradient written) against the COMPOSED path the tape ran before
(forward `nk_log_softmax_fwd` + `nk_nll_fwd`; backward `nk_fill(0)` of the log-probabilities' gradient + `nk_nll_bwd` +
`nk_log_softmax_bwd_assign`) and against `nk_copy` of the same byte count, all timed in the same process, alternating, at
    (8192, 50257)       GPT-2's head, 8 x 1024 tokens: 1.6 GB of logits, odd C (three rows in four off a 16-byte boundary)
    (16384, 32000)      2.1 GB
    (65536, 1000)       262 MB: the row-in-registers family, cache-assisted
    (4096, 128256)      2.1 GB, the widest blocks
    (64, 131072)        34 MB in 64 rows: one block per row under-fills the chip (splitting a row is future work; recorded as it is)
    (16, 150, 128, 128) the strided (generic) kernels
    python benchmarks/cross_entropy.py [min_ms]
One JSON line per (shape, kernel): ms, algorithmic bytes / time (forward 4 N C: the logits read; backward 8 N C: the logits read, the
gradient written), the copy's rate and the ratio to it.  Every shape runs in a fresh child process under its own time limit; the
parent touches no GPU and stops at the first child that fails."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8192, 50257), (16384, 32000), (65536, 1000), (4096, 128256), (64, 131072), (16, 150, 128, 128)]
CHILD_LIMIT_S = 240


def child(shape, min_ms):
    from neuronika_amd import capi as c
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/cross_entropy.py needs a GPU")
    dev = c.Device(0)

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

    rng = np.random.default_rng(0)
    N, C = shape[0], shape[1]
    tshape = (N,) + tuple(shape[2:])
    numel = int(np.prod(shape))
    x = rng.standard_normal(shape, dtype=np.float32)
    x *= np.float32(2.0)
    XS, T = dev.array(x), dev.array(rng.integers(0, C, tshape).astype(np.float32))
    del x
    Y, GY, DX = dev.zeros(shape), dev.zeros(shape), dev.zeros(shape)
    LSE, OUT, G = dev.zeros(tshape), dev.zeros(1), dev.array(np.ones(1, np.float32))

    def composed_fwd():
        c.log_softmax_fwd(dev, XS, Y, 1)
        c.nll_fwd(dev, Y, T, OUT, "mean")

    def composed_bwd():
        GY.fill(0.0)
        c.nll_bwd(dev, GY, G, T, "mean")
        c.log_softmax_bwd(dev, DX, GY, Y, 1, assign=True)

    composed_fwd()                                                   # Y holds the log-probabilities the composed backward reads
    cases = [("cross_entropy_fwd", lambda: c.cross_entropy_fwd(dev, XS, T, LSE, OUT, shape, "mean"), 4 * numel),
             ("log_softmax_fwd + nll_fwd", composed_fwd, 4 * numel),
             ("cross_entropy_bwd_assign", lambda: c.cross_entropy_bwd(dev, DX, G, XS, T, LSE, shape, "mean", assign=True), 8 * numel),
             ("fill + nll_bwd + log_softmax_bwd_assign", composed_bwd, 8 * numel)]
    for name, fn, nbytes in cases:
        m = nbytes // 8                                              # a copy of m floats reads and writes nbytes in all
        copy = lambda: c.check(c.lib.nk_copy(dev.h, GY.p, XS.p, m))
        ms_k, ms_c = [], []
        for _ in range(3):
            ms_c.append(window(copy))
            ms_k.append(window(fn))
        k, cp = min(ms_k), min(ms_c)
        rate, copy_rate = nbytes / (k * 1e-3), 8 * m / (cp * 1e-3)
        print(json.dumps({"bench": "cross_entropy", "shape": list(shape), "kernel": name, "algorithmic_bytes": nbytes, "ms": round(k, 4),
                          "ms_windows": [round(v, 4) for v in ms_k], "GBps": round(rate / 1e9, 1), "copy_ms": round(cp, 4),
                          "copy_GBps": round(copy_rate / 1e9, 1), "ratio_to_copy": round(rate / copy_rate, 3)}), flush=True)
    dev.sync()


def main():
    args = sys.argv[1:]
    if args and args[0] == "--shape":
        return child(tuple(int(v) for v in args[1].split("x")), float(args[2]))
    min_ms = float(args[0]) if args else 25.0
    for shape in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", "x".join(str(v) for v in shape), str(min_ms)], timeout=CHILD_LIMIT_S)
        if r.returncode != 0:
            raise SystemExit("benchmarks/cross_entropy.py: shape %s failed with status %d; nothing further is started" % (shape, r.returncode))


if __name__ == "__main__":
    main()

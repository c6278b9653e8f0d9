"""Batch normalisation kernels, HIP events on the compute stream as bench.py's `measure_hbm_kernels` times its rows (warm-up,
windows of at least 25 ms): training forward (statistics, running update, normalisation), the backward sums and dx (assign form) at
    (128, 128, 56, 56)  C3's output, 205 MB per tensor: labelled cache-assisted (the 256 MB Infinity Cache holds most of it)
    (128, 512, 64, 64)  1 GiB per tensor, the plane class: the judged row
    (1048576, 256)      1 GiB per tensor, the column class: the judged row
    (128, 512, 7, 7)    12.8 MB per tensor, the generic class (scalar kernels, no speed claim)
    python benchmarks/batchnorm.py [min_ms]
One JSON line per (shape, kernel): ms, algorithmic bytes / time, and the ratio to `nk_copy` timed in the same process, alternating
with the kernel (copy, kernel, copy, kernel, ...: the best window of each).  Algorithmic bytes (4 B x elements read + written; the
per-channel vectors and the partial results are left out, under 1 %): forward 12 n (x read twice, y written), backward sums 8 n
(g, x read), dx in the assign form 12 n (g, x read; dx written)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuronika_amd import capi as c  # noqa: E402

SHAPES = [((128, 128, 56, 56), "planes, cache-assisted (205 MB per tensor)"), ((128, 512, 64, 64), "planes, 1 GiB per tensor"),
          ((1048576, 256), "columns, 1 GiB per tensor"), ((128, 512, 7, 7), "generic (12.8 MB per tensor)")]


def main():
    min_ms = float(sys.argv[1]) if len(sys.argv) > 1 else 25.0
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/batchnorm.py needs a GPU")
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

    for shape, label in SHAPES:
        N, C = shape[:2]
        L = int(np.prod(shape[2:]))
        n = N * C * L
        rng = np.random.default_rng(0)
        X = dev.array(rng.standard_normal(n, dtype=np.float32))
        G = dev.array(rng.standard_normal(n, dtype=np.float32))
        W, B = dev.array(rng.standard_normal(C, dtype=np.float32)), dev.array(rng.standard_normal(C, dtype=np.float32))
        RM, RV = dev.zeros((C,)), dev.full((C,), 1.0)
        Y, S, SUMS = dev.zeros((n,)), dev.zeros((C, 2)), dev.zeros((C, 2))
        c.batch_norm_fwd(dev, X, W, B, Y, S, RM, RV, N, C, L, 1e-5, 0.1)
        c.batch_norm_bwd_sums(dev, SUMS, G, X, S, N, C, L)
        cases = [("batch_norm_fwd (training)", lambda: c.batch_norm_fwd(dev, X, W, B, Y, S, RM, RV, N, C, L, 1e-5, 0.1), 12 * n),
                 ("batch_norm_bwd_sums", lambda: c.batch_norm_bwd_sums(dev, SUMS, G, X, S, N, C, L), 8 * n),
                 ("batch_norm_bwd_assign (dx)", lambda: c.batch_norm_bwd(dev, Y, G, X, W, S, SUMS, N, C, L, assign=True), 12 * n)]
        # the copy moves n floats, 8 n bytes, out of / into the same buffers: its RATE stands in for the 12 n rows (a copy's rate does
        # not depend on the count at these sizes)
        copy = lambda: c.check(c.lib.nk_copy(dev.h, Y.p, X.p, n))
        for name, fn, nbytes in cases:
            ms_k, ms_c = [], []
            for _ in range(3):
                ms_c.append(window(copy))
                ms_k.append(window(fn))
            k, cp = min(ms_k), min(ms_c)
            rate, copy_rate = nbytes / (k * 1e-3), 8 * n / (cp * 1e-3)
            print(json.dumps({"bench": "batchnorm", "shape": list(shape), "size": label, "kernel": name, "algorithmic_bytes": nbytes,
                              "ms": round(k, 4), "ms_windows": [round(v, 4) for v in ms_k], "TBps": round(rate / 1e12, 3),
                              "copy_bytes": 8 * n, "copy_ms": round(cp, 4), "copy_TBps": round(copy_rate / 1e12, 3),
                              "ratio_to_copy": round(rate / copy_rate, 3)}), flush=True)
        del X, G, Y
    dev.sync()


if __name__ == "__main__":
    main()

"""Layer normalisation kernels, HIP events on the compute stream as bench.py's `measure_hbm_kernels` times its rows (warm-up,
windows of at least 25 ms): forward (with statistics), dx (assign form) and the parameter gradients (assign form) at
    (32768, 1024)   C5's activation, 128 MB per tensor: labelled cache-assisted (the 256 MB Infinity Cache holds most of it)
    (262144, 1024)  1 GiB per tensor: the judged row
    (32768, 8192)   1 GiB per tensor, the block-per-row kernels
    python benchmarks/layernorm.py [min_ms]
One JSON line per (shape, kernel): ms, algorithmic bytes / time, and the ratio to `nk_copy` of the SAME byte count timed in the
same process, alternating with the kernel (copy, kernel, copy, kernel, ...: the best window of each).  Algorithmic bytes (4 B x
elements read + written; gamma, beta, stats and the partial sums are left out, under 1 %): forward 8 n (x read, y written), dx in the
assign form timed here 12 n (g, x read; dx written; the `+=` form reads dx as well, 16 n), parameter gradients 8 n (g, x read)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuronika_amd import capi as c  # noqa: E402

SHAPES = [(32768, 1024, "cache-assisted (128 MB per tensor)"), (262144, 1024, "1 GiB per tensor"), (32768, 8192, "1 GiB per tensor")]


def main():
    min_ms = float(sys.argv[1]) if len(sys.argv) > 1 else 25.0
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/layernorm.py needs a GPU")
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

    for rows, D, label in SHAPES:
        n = rows * D
        rng = np.random.default_rng(0)
        X = dev.array(rng.standard_normal((rows, D), dtype=np.float32))
        G = dev.array(rng.standard_normal((rows, D), dtype=np.float32))
        W, B = dev.array(rng.standard_normal(D, dtype=np.float32)), dev.array(rng.standard_normal(D, dtype=np.float32))
        Y, S, DG, DB = dev.zeros((rows, D)), dev.zeros((rows, 2)), dev.zeros((D,)), dev.zeros((D,))
        c.layer_norm_fwd(dev, X, W, B, Y, S, rows, D, 1e-5)
        # a copy of `nbytes` algorithmic bytes moves nbytes / 8 floats (one read + one write each), out of / into the same buffers
        cases = [("layer_norm_fwd", lambda: c.layer_norm_fwd(dev, X, W, B, Y, S, rows, D, 1e-5), 8 * n),
                 ("layer_norm_bwd_assign (dx)", lambda: c.layer_norm_bwd(dev, Y, G, X, W, S, rows, D, assign=True), 12 * n),
                 ("layer_norm_bwd_params_assign (dgamma, dbeta)", lambda: c.layer_norm_bwd_params(dev, DG, DB, G, X, S, rows, D, assign=True), 8 * n)]
        for name, fn, nbytes in cases:
            m = nbytes // 8
            # 12 n bytes as a copy need 1.5 n floats of source and destination: two tensors side by side do not exist here, so the
            # copy of the dx row moves n floats and its RATE stands in (a copy's rate does not depend on the count at this size)
            m = min(m, n)
            copy = lambda: c.check(c.lib.nk_copy(dev.h, Y.p, X.p, m))
            ms_k, ms_c = [], []
            for _ in range(3):
                ms_c.append(window(copy))
                ms_k.append(window(fn))
            k, cp = min(ms_k), min(ms_c)
            rate, copy_rate = nbytes / (k * 1e-3), 8 * m / (cp * 1e-3)
            print(json.dumps({"bench": "layernorm", "shape": [rows, D], "size": label, "kernel": name, "algorithmic_bytes": nbytes,
                              "ms": round(k, 4), "ms_windows": [round(v, 4) for v in ms_k], "TBps": round(rate / 1e12, 3),
                              "copy_bytes": 8 * m, "copy_ms": round(cp, 4), "copy_TBps": round(copy_rate / 1e12, 3),
                              "ratio_to_copy": round(rate / copy_rate, 3)}), flush=True)
        del X, G, Y
    dev.sync()


if __name__ == "__main__":
    main()

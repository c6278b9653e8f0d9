"""Pooling kernels, HIP events on the compute stream as bench.py's `measure_hbm_kernels` times its rows (warm-up, windows of at
least 25 ms, the best of three): max forward (y and idx), average forward, max backward in the assign and the `+=` form, average
backward in the assign form, per kernel class at about 1 GiB of input and at the two pooling layers of a ResNet:
    windowed  (128, 128, 128, 128) through 2/2/0, 3/2/1, 3/2/0 (scalar stores: out_W is odd) and 3/1/1
              (128, 64, 112, 112) through 3/2/1: the stem pool, 411 MB in, cache-assisted in part
    plane     (65536, 84, 7, 7), (65536, 64, 8, 8), (128, 672, 56, 56), (64, 64, 256, 256): L = 49, 64, 3136, 65536, about 1 GiB
              (128, 512, 7, 7): the global average of a ResNet, 12.8 MB: cache-assisted
    generic   (128, 128, 126, 130) through 3/2/1 (in_W % 4 != 0)
    python benchmarks/pooling.py [min_ms]
One JSON line per (shape, kernel): microseconds, algorithmic bytes / time, and the ratio to `nk_copy` timed in the same process,
alternating with the kernel.  Algorithmic bytes (4 B per element): max forward x + y + idx, average forward x + y, max backward
g + idx + dx (assign) or g + idx + 2 dx (`+=`), average backward g + dx."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuronika_amd import capi as c  # noqa: E402

G1 = "about 1 GiB of input"
CASES = [
    ("windowed 2/2/0", (128, 128, 128, 128), (2, 2), (2, 2), (0, 0), G1),
    ("windowed 3/2/1", (128, 128, 128, 128), (3, 3), (2, 2), (1, 1), G1),
    ("windowed 3/2/0 (scalar stores)", (128, 128, 128, 128), (3, 3), (2, 2), (0, 0), G1),
    ("windowed 3/1/1", (128, 128, 128, 128), (3, 3), (1, 1), (1, 1), G1),
    ("windowed 3/2/1", (128, 64, 112, 112), (3, 3), (2, 2), (1, 1), "ResNet stem pool, 411 MB in: cache-assisted in part"),
    ("plane L = 49", (65536, 84, 7, 7), (7, 7), (7, 7), (0, 0), G1),
    ("plane L = 64", (65536, 64, 8, 8), (8, 8), (8, 8), (0, 0), G1),
    ("plane L = 3136", (128, 672, 56, 56), (56, 56), (56, 56), (0, 0), G1),
    ("plane L = 65536", (64, 64, 256, 256), (256, 256), (256, 256), (0, 0), G1),
    ("plane L = 49", (128, 512, 7, 7), (7, 7), (7, 7), (0, 0), "ResNet global average, 12.8 MB in: cache-assisted"),
    ("generic 3/2/1, in_W % 4 != 0", (128, 128, 126, 130), (3, 3), (2, 2), (1, 1), G1),
]


def main():
    min_ms = float(sys.argv[1]) if len(sys.argv) > 1 else 25.0
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/pooling.py needs a GPU")
    dev = c.Device(0)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None

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

    host = np.random.default_rng(0).standard_normal(max(int(np.prod(case[1])) for case in CASES), dtype=np.float32)
    for name, shape, k, s, p, label in CASES:
        oshape = c.pool_out_shape(shape, k, s, p)
        n, m = int(np.prod(shape)), int(np.prod(oshape))
        X, G = dev.array(host[:n]), dev.array(host[:m])
        assert X.size == n and G.size == m
        Y, I, DX = dev.zeros((m,)), dev.int_zeros((m,)), dev.zeros((n,))
        c.max_pool_fwd(dev, X, shape, Y, I, k, s, p)
        cases = [("max_pool_fwd", lambda: c.max_pool_fwd(dev, X, shape, Y, I, k, s, p), 4 * (n + 2 * m)),
                 ("avg_pool_fwd", lambda: c.avg_pool_fwd(dev, X, shape, Y, k, s, p), 4 * (n + m)),
                 ("max_pool_bwd_assign", lambda: c.max_pool_bwd(dev, DX, shape, G, I, k, s, p, assign=True), 4 * (n + 2 * m)),
                 ("max_pool_bwd", lambda: c.max_pool_bwd(dev, DX, shape, G, I, k, s, p), 4 * (2 * n + 2 * m)),
                 ("avg_pool_bwd_assign", lambda: c.avg_pool_bwd(dev, DX, shape, G, k, s, p, assign=True), 4 * (n + m))]
        copy = lambda: c.check(c.lib.nk_copy(dev.h, DX.p, X.p, n))          # n floats read, n written
        for kernel, fn, nbytes in cases:
            ms_k, ms_c = [], []
            for _ in range(3):
                ms_c.append(window(copy))
                ms_k.append(window(fn))
            kk, cp = min(ms_k), min(ms_c)
            rate, copy_rate = nbytes / (kk * 1e-3), 8 * n / (cp * 1e-3)
            print(json.dumps({"bench": "pooling", "commit": commit, "class": name, "shape": list(shape), "kernel_size": list(k), "stride": list(s),
                              "padding": list(p), "size": label, "kernel": kernel, "algorithmic_bytes": nbytes, "us": round(kk * 1e3, 2),
                              "us_windows": [round(v * 1e3, 2) for v in ms_k], "TBps": round(rate / 1e12, 3), "copy_bytes": 8 * n,
                              "copy_us": round(cp * 1e3, 2), "copy_TBps": round(copy_rate / 1e12, 3), "ratio_to_copy": round(rate / copy_rate, 3)}),
                  flush=True)
        del X, G, Y, I, DX
    dev.sync()


if __name__ == "__main__":
    main()

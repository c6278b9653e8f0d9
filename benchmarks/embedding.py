"""Embedding kernels, HIP events on the compute stream (warm-up, windows of at least 25 ms, the best of three): forward (row gather),
backward in the `+=` form and in the assign form (each call builds the inverted index and runs the ordered sum), for uniform and
Zipf-distributed ids at
    V = 50257, D = 768,  n = 8192     GPT-2 small's table, 8 x 1024 tokens (154 MB table, 25 MB of rows: cache-assisted)
    V = 50257, D = 768,  n = 65536    the same table, 64 x 1024 tokens
    V = 32000, D = 4096, n = 16384    524 MB table, 268 MB of rows
    V = 131072, D = 1024, n = 262144  537 MB table, 1 GiB of rows: past the Infinity Cache
    python benchmarks/embedding.py [min_ms]
One JSON line per (shape, ids, kernel): ms, algorithmic bytes / time, and the ratio to `nk_copy` of the SAME byte count timed in the
same process, alternating with the kernel.  Algorithmic bytes (4 B x floats read + written; ids and index are left out): forward
8 n D; assign form 4 n D (g read) + 4 V D (the whole table written); `+=` form 4 n D + 8 r D with r the rows some token selected
(read and written).  `max_row` is the longest row's token count (rows beyond 128 tokens are summed in chunks by separate owners),
`index_ms` the two index launches alone (from a backward with D = 1, whose sum pass is negligible)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuronika_amd import capi as c  # noqa: E402

SHAPES = [(50257, 768, 8192), (50257, 768, 65536), (32000, 4096, 16384), (131072, 1024, 262144)]


def uniform_ids(rng, n, V):
    return rng.integers(0, V, n).astype(np.float32)


def zipf_ids(rng, n, V):
    p = 1.0 / np.arange(1, V + 1)
    return rng.permutation(V)[rng.choice(V, size=n, p=p / p.sum())].astype(np.float32)


def main():
    min_ms = float(sys.argv[1]) if len(sys.argv) > 1 else 25.0
    if c.device_count() < 1:
        raise RuntimeError("benchmarks/embedding.py needs a GPU")
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

    for V, D, n in SHAPES:
        rng = np.random.default_rng(0)
        W = dev.array(rng.standard_normal((V, D), dtype=np.float32))
        G = dev.array(rng.standard_normal((n, D), dtype=np.float32))
        OUT, DW = dev.zeros((n, D)), dev.zeros((V, D))
        big = max(n, V) * D
        SRC, DST = dev.zeros(big), dev.zeros(big)
        G1, DW1 = dev.zeros(n), dev.zeros(V)
        for dist, make in (("uniform", uniform_ids), ("zipf", zipf_ids)):
            idx = make(rng, n, V)
            counts = np.bincount(idx.astype(np.int64), minlength=V)
            r = int((counts > 0).sum())
            I = dev.array(idx)
            index_ms = min(window(lambda: c.embedding_bwd(dev, DW1, G1, I, n, V, 1, assign=False)) for _ in range(3))
            cases = [("embedding_fwd", lambda: c.embedding_fwd(dev, W, I, OUT, n, V, D), 8 * n * D),
                     ("embedding_bwd (+=)", lambda: c.embedding_bwd(dev, DW, G, I, n, V, D), 4 * n * D + 8 * r * D),
                     ("embedding_bwd_assign", lambda: c.embedding_bwd(dev, DW, G, I, n, V, D, assign=True), 4 * n * D + 4 * V * D)]
            for name, fn, nbytes in cases:
                m = min(nbytes // 8, big)
                copy = lambda: c.check(c.lib.nk_copy(dev.h, DST.p, SRC.p, m))
                ms_k, ms_c = [], []
                for _ in range(3):
                    ms_c.append(window(copy))
                    ms_k.append(window(fn))
                k, cp = min(ms_k), min(ms_c)
                rate, copy_rate = nbytes / (k * 1e-3), 8 * m / (cp * 1e-3)
                print(json.dumps({"bench": "embedding", "V": V, "D": D, "n": n, "ids": dist, "rows_selected": r, "max_row": int(counts.max()),
                                  "kernel": name, "algorithmic_bytes": nbytes, "ms": round(k, 4), "ms_windows": [round(v, 4) for v in ms_k],
                                  "TBps": round(rate / 1e12, 3), "copy_bytes": 8 * m, "copy_ms": round(cp, 4),
                                  "copy_TBps": round(copy_rate / 1e12, 3), "ratio_to_copy": round(rate / copy_rate, 3),
                                  "index_ms": round(index_ms, 4)}), flush=True)
            del I
        del W, G, OUT, DW, SRC, DST
    dev.sync()


if __name__ == "__main__":
    main()
